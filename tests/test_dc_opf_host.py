"""CPU checks of the DC optimal power flow (include/gns_powerflow.h, "DC optimal power flow") that need no device: the float64
reference (``dc_opf_reference``) against SciPy's HiGHS on the linear programs, its KKT certificate on every set, its prices against
central differences of its own optimal cost, two closed forms, the problem sets' own promises (``dc_opf_cases``), the exports, the
refusals of the C entry points and of the Python call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_opf_cases as cases
import dc_opf_reference as ref
import pf_topologies as pt

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
TOL = ref.DEFAULT_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference and the sets

@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_reference_converges_at_the_default_tolerance(name):
    for r in cases.optimum(name):
        assert r['converged'] and 0 < r['iterations'] <= ref.DEFAULT_MAX_ITER
        assert all(np.all(np.isfinite(r[k])) for k in ('pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin'))


def test_default_tolerance_is_the_probes_and_the_products():
    import inspect
    assert ref.probe_default_tol() == ref.DEFAULT_TOL == 1e-8
    sig = inspect.signature(powerflow.dc_optimal_power_flow)
    assert sig.parameters['tol'].default == ref.DEFAULT_TOL and sig.parameters['max_iter'].default == ref.DEFAULT_MAX_ITER == 150


def test_sets_are_feasible_and_limits_bind():
    cases.check_active()
    assert set(cases.ACTIVE_SETS) | set(cases.INACTIVE_SETS) == set(cases.SETS)
    for name in cases.SETS:
        for p, r in zip(cases.problems(name), cases.optimum(name)):
            assert np.all(p[2][:, 2] < p[2][:, 1])                      # Pmin < Pmax
            assert np.all(p[2][:, 6] == 7.5)                            # the listed Pg, which nothing reads
    # the forms of cost and rating the sets cover
    assert cases.batch('case14_qp').cost.dim() == 3 and cases.batch('case14_qp').rating.dim() == 2
    assert cases.batch('case14_lp').cost.dim() == 2 and cases.batch('case14_lp').rating.dim() == 1
    assert cases.batch('case14_no_rating').rating is None
    assert cases.batch('one_unit').gens.shape[1] == 1 and cases.batch('hub150_qp').gens.shape[1] == 70
    assert [cases.batch(n).lines.shape[1] for n in ('path64', 'path65', 'path66_pv')] == [63, 64, 65]
    b = cases.batch('slack_unit')
    assert b.slack in b.gens[0, :, 0].long().tolist()
    g = cases.batch('stacked_units').gens[0, :, 0].long().tolist()
    assert g.count(4) == 4 and g.count(1) == 2


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_reference_kkt_certificate(name):
    """The three termination figures, the dual signs and the primal feasibility, recomputed from the returned values alone."""
    for p, r in zip(cases.problems(name), cases.optimum(name)):
        k = ref.kkt_residuals(r, p)
        bar = TOL + 1e-12 * k['scale']
        assert k['feas'] <= bar and k['grad'] <= bar and k['comp'] <= bar, k
        assert k['min_mu'] >= 0.0 and k['mu_off'] <= bar, k
        assert k['max_h'] <= bar * k['feas_scale'] and k['max_g'] <= bar * k['feas_scale'], k


@pytest.mark.parametrize('name', cases.LP_SETS)
def test_reference_against_highs(name):
    """Every LP set against scipy.optimize.linprog(method='highs') in the (theta_r, p) variables: the objective, and the dispatch
    where the optimum is unique (distinct c1 make it so on these sets; HiGHS's own tolerances are 1e-7)."""
    so = pytest.importorskip('scipy.optimize')
    for p, r in zip(cases.problems(name), cases.optimum(name)):
        m = ref._model(*(np.asarray(x, dtype=np.float64) for x in p[:3]), p[3], p[4], p[5])
        nth, Gn, nl = m['nth'], m['Gn'], m['lim'].size
        c = np.concatenate([np.zeros(nth), m['c1']])
        res = so.linprog(c, A_ub=m['A'][:2 * nl], b_ub=m['ub'][:2 * nl], A_eq=m['G'], b_eq=m['load'],
                         bounds=[(None, None)] * nth + list(zip(m['pmin'], m['pmax'])), method='highs')
        assert res.status == 0, res.message
        assert abs(r['objective'] - res.fun) <= 1e-7 * max(1.0, abs(res.fun))
        assert np.abs(r['pg'] - res.x[nth:]).max() <= 1e-6 * max(1.0, np.abs(res.x).max())


@pytest.mark.parametrize('name', ('three_bus', 'case14_qp', 'case14_lp', 'stacked_units'))
def test_reference_lmp_is_the_derivative_of_the_optimal_cost(name):
    """lmp against central differences of the reference's own optimal cost in Pd, at three buses of the first grid.  The step 1e-4
    keeps the active set (no limit is within 1e-4 of changing on these grids); the bar is the differences' own error: the cost is
    solved to about 1e-11 relative, so (cost error) / step ~ 1e-11 * cost / 1e-4, plus the second-order term of a quadratic cost."""
    p, r = cases.problems(name)[0], cases.optimum(name)[0]
    step = 1e-4
    for bus in (0, p[0].shape[0] // 2, p[0].shape[0] - 1):
        vals = []
        for s in (+step, -step):
            buses = p[0].copy()
            buses[bus, 2] += s
            vals.append(ref.optimal_cost(buses, *p[1:]))
        fd = (vals[0] - vals[1]) / (2 * step)
        bar = 1e-10 * max(1.0, abs(r['objective'])) / step + 1e-5 * max(1.0, abs(r['lmp'][bus]))
        assert abs(fd - r['lmp'][bus]) <= bar, (bus, fd, r['lmp'][bus])


def test_closed_form_three_bus():
    """The dispatch and the prices written out by hand in ``dc_opf_cases.three_bus``: p = (0.5, 0.5), lmp = (10, 30, 50), mu = 60."""
    r = cases.optimum('three_bus')[0]
    assert np.abs(r['pg'] - np.array(cases.THREE_BUS_PG)).max() <= 1e-7
    assert np.abs(r['lmp'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5
    assert abs(r['mu_line'][1] - cases.THREE_BUS_MU) <= 1e-5 and r['mu_line'][0] == 0.0 and r['mu_line'][2] == 0.0
    assert abs(r['line_flow'][1] - 0.5) <= 1e-7 and abs(r['objective'] - 20.0) <= 1e-6


def test_closed_form_equal_incremental_cost():
    """No line limit and quadratic costs: the units strictly inside their bounds share one incremental cost, the price at every bus."""
    inside_seen = 0
    for p, r in zip(cases.problems('case14_no_rating'), cases.optimum('case14_no_rating')):
        c2, c1, pmax, pmin = p[3][:, 0], p[3][:, 1], p[2][:, 1], p[2][:, 2]
        inc = 2 * c2 * r['pg'] + c1
        inside = (r['pg'] > pmin + 1e-4 * (pmax - pmin)) & (r['pg'] < pmax - 1e-4 * (pmax - pmin))
        inside_seen += int(inside.sum())
        assert inside.any()
        assert np.abs(inc[inside] - inc[inside][0]).max() <= 1e-5 * np.abs(inc).max()
        assert np.abs(r['lmp'] - inc[inside][0]).max() <= 1e-5 * np.abs(inc).max()
        assert np.all(r['mu_line'] == 0.0)
    assert inside_seen >= 3


# ---- the exports and the C entry points' refusals

def test_exports_are_there_typed_and_declared():
    lib = amd.load_library()
    assert _lib.DCOPF_EXPORTS == ('gns_dcopf_lds_bytes', 'gns_dcopf_workspace_bytes', 'gns_dcopf_solve')
    header = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    assert 'DC optimal power flow' in header
    for f in _lib.DCOPF_EXPORTS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype is ctypes.c_int and getattr(lib, f).argtypes
        assert re.search(r'\bint ' + f + r'\(', header), f
    assert len(lib.gns_dcopf_solve.argtypes) == 24
    assert callable(powerflow.dc_optimal_power_flow)
    assert powerflow.DcOpfResult._fields == ('pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective',
                                             'converged', 'iterations')


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _solve(lib, cfg, host, Bt=2, ws_bytes=1 << 40, null=(), cost_per_grid=0, rating_per_grid=0, cfg_null=False, host_null=False):
    """gns_dcopf_solve with placeholder device pointers (every refusal comes before a launch, so nothing dereferences them); the
    0-based positions ``null`` of its pointer arguments after Bt are NULL."""
    p = 0x1000
    ptrs = [p] * 12                    # cost, rating, pg, theta, line_flow, lmp, mu_line, mu_pmax, mu_pmin, objective, converged, iterations
    for i in null:
        ptrs[i] = None
    return lib.gns_dcopf_solve(None if cfg_null else ctypes.byref(cfg), None if host_null else host.ctypes.data, p, p, p, p, Bt,
                               ptrs[0], cost_per_grid, ptrs[1], rating_per_grid, *ptrs[2:], p, ws_bytes, None)


def test_c_entry_points_refuse_before_any_launch():
    lib = amd.load_library()
    tp = pt.path(9, pv=(5,))
    fd = _fd(tp)
    cfg = PfConfig(tp.n, tp.f.size, tp.g.size, 150, 1e-8)
    nbytes, lds, lanes = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int32()
    # the queries
    assert lib.gns_dcopf_lds_bytes(None, ctypes.byref(lds), None) == EINVAL
    assert lib.gns_dcopf_lds_bytes(fd.host.ctypes.data, None, None) == EINVAL
    assert lib.gns_dcopf_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(lanes)) == 0
    i = fd.info
    factor = 8 * (i['nnz_lu_p'] + i['dim_p'] + i['n_bus'] + 3 * i['n_line'] + i['dim_p'] * (lanes.value + 1)) + 32 * i['n_gen']
    ipm = 8 * (i['n_gen'] * (i['n_gen'] + 1) // 2 + 14 * i['n_gen'] + 10 * i['n_line'])
    assert lanes.value == 64 and lds.value == max(factor, ipm)
    assert lib.gns_dcopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, ctypes.byref(nbytes)) == 0
    E, Gn = tp.f.size, tp.g.size
    assert nbytes.value == (8 * 3 * (E * Gn + E + Gn + 3) + 255) // 256 * 256
    assert lib.gns_dcopf_workspace_bytes(None, fd.host.ctypes.data, 3, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_workspace_bytes(ctypes.byref(cfg), None, 3, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 0, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, None) == EINVAL
    # null pointers: every input and output but the rating
    for k in (0, *range(2, 12)):
        assert _solve(lib, cfg, fd.host, null=(k,)) == EINVAL, k
    assert _solve(lib, cfg, fd.host, cfg_null=True) == EINVAL and _solve(lib, cfg, fd.host, host_null=True) == EINVAL
    for Bt in (0, -1, 1 << 31):
        assert _solve(lib, cfg, fd.host, Bt=Bt) == EINVAL
    assert _solve(lib, cfg, fd.host, cost_per_grid=2) == EINVAL and _solve(lib, cfg, fd.host, rating_per_grid=-1) == EINVAL
    # a wrong magic, another shape, a Newton-Raphson blob, no unit
    bad = fd.host.copy()
    bad[0] ^= 1
    assert _solve(lib, cfg, bad) == EINVAL
    assert lib.gns_dcopf_lds_bytes(bad.ctypes.data, ctypes.byref(lds), None) == EINVAL
    assert _solve(lib, PfConfig(tp.n, tp.f.size, tp.g.size + 1, 150, 1e-8), fd.host) == EINVAL
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _solve(lib, cfg, nr.host) == EINVAL
    none = pt.Topo('no_unit', 4, *pt._ids([1, 2, 3], [2, 3, 4], []), 1)
    assert _solve(lib, PfConfig(4, 3, 0, 150, 1e-8), _fd(none).host) == EINVAL
    assert _solve(lib, PfConfig(tp.n, tp.f.size, tp.g.size, -1, 1e-8), fd.host) == EINVAL
    assert _solve(lib, PfConfig(tp.n, tp.f.size, tp.g.size, 150, -1.0), fd.host) == EINVAL
    # a short workspace
    assert _solve(lib, cfg, fd.host, Bt=3, ws_bytes=nbytes.value - 1) == ESIZE


def _over_the_limit():
    """A star whose 251 units make the interior point's packed normal matrix alone 253 008 B."""
    return pt.star(251, 'pv')


def test_lds_refusal_needs_no_device():
    lib = amd.load_library()
    tp = _over_the_limit()
    fd = _fd(tp)
    Gn, E = tp.g.size, tp.f.size
    lds = ctypes.c_int64()
    assert lib.gns_dcopf_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), None) == 0
    assert lds.value == 8 * (Gn * (Gn + 1) // 2 + 14 * Gn + 10 * E) > pt.LDS_LIMIT
    cfg = PfConfig(tp.n, E, Gn, 150, 1e-8)
    assert _solve(lib, cfg, fd.host) == EUNSUPPORTED
    assert _solve(lib, cfg, fd.host, ws_bytes=0) == ESIZE                     # a short workspace is named first
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcopf_solve', lds.value, powerflow._DCOPF.formula)
    assert str(lds.value) in str(e.value) and 'Gn (Gn + 1) / 2' in str(e.value)


# ---- the Python refusals, raised before a device is needed

def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E, Gn = lines.shape[1], gens.shape[1]
    cost = torch.ones(Gn, 2, dtype=torch.float64)

    def opf(**kw):
        kw.setdefault('cost', cost)
        return powerflow.dc_optimal_power_flow(buses, lines, gens, slack_bus=1, **kw)

    with pytest.raises(TypeError):
        powerflow.dc_optimal_power_flow(buses, lines, gens, slack_bus=1)                # cost is required
    with pytest.raises(ValueError, match='cost is required'):
        opf(cost=None)
    for bad in (torch.ones(Gn, 2), torch.ones(Gn, 2, dtype=torch.int64), np.ones((Gn, 2), dtype=np.float32)):
        with pytest.raises(ValueError, match='cost must be float64'):
            opf(cost=bad)
    for bad in (torch.ones(Gn, dtype=torch.float64), torch.ones(Gn, 3, dtype=torch.float64), torch.ones(2, Gn, 2, dtype=torch.float64),
                torch.ones(Gn + 1, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match='cost must be'):
            opf(cost=bad)
    for v in (float('nan'), float('inf')):
        bad = cost.clone()
        bad[1, 1] = v
        with pytest.raises(ValueError, match='cost must be finite'):
            opf(cost=bad)
    bad = cost.clone()
    bad[2, 0] = -1e-30
    with pytest.raises(ValueError, match='c2 .* must be >= 0'):
        opf(cost=bad)
    for bad in (torch.zeros(E, dtype=torch.float64), -torch.ones(E, dtype=torch.float64),
                torch.full((3, E), float('nan'), dtype=torch.float64)):
        with pytest.raises(ValueError, match='rating must be positive'):
            opf(rating=bad)
    for bad in (torch.ones(E - 1, dtype=torch.float64), torch.ones(2, E, dtype=torch.float64)):
        with pytest.raises(ValueError, match='rating must be'):
            opf(rating=bad)
    with pytest.raises(ValueError, match='rating must be float64'):
        opf(rating=torch.ones(E))
    for bad in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='tol must be >= 0'):
            opf(tol=bad)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match='max_iter must be a non-negative integer'):
            opf(max_iter=bad)
    with pytest.raises(ValueError, match='float32'):
        powerflow.dc_optimal_power_flow(buses.double(), lines, gens, slack_bus=1, cost=cost)
    with pytest.raises(ValueError, match='at least one generator'):
        powerflow.dc_optimal_power_flow(buses, lines, gens[:, :0], slack_bus=1, cost=torch.ones(0, 2, dtype=torch.float64))
    # +inf is a rating: the line has no limit; the existing screens' check still refuses it
    r = torch.full((E,), float('inf'), dtype=torch.float64)
    assert powerflow._dcopf_rating(r, 3, E, False) is r and powerflow._dcopf_rating(None, 3, E, False) is None
    with pytest.raises(ValueError, match='rating must be positive and finite'):
        powerflow._rating(r, 3, E, False)
    assert powerflow._dcopf_cost(torch.zeros(1, Gn, 2, dtype=torch.float64), 1, Gn, True).shape == (Gn, 2)
    assert powerflow._DCOPF.prefix == 'gns_dcopf' and powerflow._DCOPF.formula == powerflow._DCOPF_LDS_FORMULA
