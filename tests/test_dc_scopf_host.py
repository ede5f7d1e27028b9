"""CPU checks of the security-constrained DC optimal power flow (include/gns_powerflow.h, "Security-constrained DC optimal power
flow") that need no device: the refusals of the C entry points in their order, the size queries against their formulas, the
exports, the Python calls' refusals, the problem sets' own promises (``dc_scopf_cases.check``), the float64 reference
(``dc_scopf_reference``) against the three-bus closed form, against central differences of its own optimal cost and its two
formulations against each other."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd import _lib
from opf_graph_neural_solver_amd._lib import PfConfig
import dc_scopf_cases as cases
import dc_scopf_reference as ref
import pf_topologies as pt

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the exports and the C entry points

def test_exports_are_there_typed_declared_and_apart():
    lib = amd.load_library()
    assert _lib.DCSCOPF_EXPORTS == ('gns_dcscopf_lds_bytes', 'gns_dcscopf_workspace_bytes', 'gns_dcscopf_solve')
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('EXPORTS') and n != 'DCSCOPF_EXPORTS']
    assert len(others) >= 17 and _lib.DCOPF_EXPORTS in others
    header = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    assert 'Security-constrained DC optimal power flow' in header
    for f in _lib.DCSCOPF_EXPORTS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype is ctypes.c_int and getattr(lib, f).argtypes
        assert re.search(r'\bint ' + f + r'\(', header), f
        assert all(f not in o for o in others), f
    assert len(lib.gns_dcscopf_solve.argtypes) == 32
    assert powerflow.DcScopfResult._fields == powerflow.DcOpfResult._fields + ('mu_row', 'row_flow')
    assert powerflow.DcSecureDispatch._fields == ('result', 'rows', 'worst_loading', 'secure')
    assert callable(powerflow.dc_security_constrained_opf) and callable(powerflow.dc_secure_dispatch)


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _solve(lib, cfg, host, Bt=2, n_row=5, ws_bytes=1 << 40, null=(), flags=(0, 0, 0, 0), cfg_null=False, host_null=False):
    """gns_dcscopf_solve with placeholder device pointers (every refusal comes before a launch, so nothing dereferences them); the
    0-based positions ``null`` of its pointer arguments after Bt are NULL: cost, rating, rows, rating_c, bridge, then the twelve
    outputs.  ``flags``: cost_per_grid, rating_per_grid, rows_per_grid, rating_c_per_grid."""
    p = 0x1000
    ptrs = [p] * 17
    for i in null:
        ptrs[i] = None
    return lib.gns_dcscopf_solve(None if cfg_null else ctypes.byref(cfg), None if host_null else host.ctypes.data, p, p, p, p, Bt,
                                 ptrs[0], flags[0], ptrs[1], flags[1], ptrs[2], flags[2], n_row, ptrs[3], flags[3], ptrs[4], *ptrs[5:],
                                 p, ws_bytes, None)


def test_c_entry_points_refuse_before_any_launch_in_order():
    lib = amd.load_library()
    tp = pt.path(9, pv=(5,))
    fd = _fd(tp)
    E, Gn = tp.f.size, tp.g.size
    cfg = PfConfig(tp.n, E, Gn, 150, 1e-8)
    nbytes, base_bytes, lds, lanes = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int32()
    # the queries against their formulas
    assert lib.gns_dcscopf_lds_bytes(None, 5, ctypes.byref(lds), None) == EINVAL
    assert lib.gns_dcscopf_lds_bytes(fd.host.ctypes.data, 5, None, None) == EINVAL
    assert lib.gns_dcscopf_lds_bytes(fd.host.ctypes.data, 0, ctypes.byref(lds), None) == EINVAL
    i = fd.info
    for R in (1, 5, 64, 1000):
        assert lib.gns_dcscopf_lds_bytes(fd.host.ctypes.data, R, ctypes.byref(lds), ctypes.byref(lanes)) == 0
        factor = 8 * (i['nnz_lu_p'] + i['dim_p'] + i['n_bus'] + 3 * i['n_line'] + i['dim_p'] * (lanes.value + 1)) + 32 * i['n_gen']
        ipm = 8 * (Gn * (Gn + 1) // 2 + 14 * Gn + 10 * E + 10 * R + (E + 1) // 2)
        assert lanes.value == 64 and lds.value == max(factor, ipm), R
    assert lib.gns_dcopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, ctypes.byref(base_bytes)) == 0
    assert lib.gns_dcscopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, 5, ctypes.byref(nbytes)) == 0
    assert nbytes.value == base_bytes.value + (8 * 3 * (2 * 5 + E) + 255) // 256 * 256
    assert lib.gns_dcscopf_workspace_bytes(None, fd.host.ctypes.data, 3, 5, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcscopf_workspace_bytes(ctypes.byref(cfg), None, 3, 5, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcscopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 0, 5, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcscopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, 0, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcscopf_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, 5, None) == EINVAL
    # null pointers: every input and output but the two ratings
    assert _solve(lib, cfg, fd.host, Bt=3, ws_bytes=nbytes.value - 1) == ESIZE          # (the placeholders alone pass the checks)
    for k in (0, 2, *range(4, 17)):
        assert _solve(lib, cfg, fd.host, null=(k,)) == EINVAL, k
    assert _solve(lib, cfg, fd.host, Bt=3, null=(1, 3), ws_bytes=nbytes.value - 1) == ESIZE
    assert _solve(lib, cfg, fd.host, cfg_null=True) == EINVAL and _solve(lib, cfg, fd.host, host_null=True) == EINVAL
    for Bt in (0, -1, 1 << 31):
        assert _solve(lib, cfg, fd.host, Bt=Bt) == EINVAL
    for n_row in (0, -3):
        assert _solve(lib, cfg, fd.host, n_row=n_row) == EINVAL
    for at in range(4):
        for v in (2, -1):
            flags = [0, 0, 0, 0]
            flags[at] = v
            assert _solve(lib, cfg, fd.host, flags=tuple(flags)) == EINVAL, flags
    assert _solve(lib, cfg, fd.host, Bt=3, flags=(1, 1, 1, 1), ws_bytes=nbytes.value - 1) == ESIZE
    # a wrong magic, another shape, a Newton-Raphson blob, no unit
    bad = fd.host.copy()
    bad[0] ^= 1
    assert _solve(lib, cfg, bad) == EINVAL
    assert lib.gns_dcscopf_lds_bytes(bad.ctypes.data, 5, ctypes.byref(lds), None) == EINVAL
    assert _solve(lib, PfConfig(tp.n, E, Gn + 1, 150, 1e-8), fd.host) == EINVAL
    assert _solve(lib, cfg, powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).host) == EINVAL
    none = pt.Topo('no_unit', 4, *pt._ids([1, 2, 3], [2, 3, 4], []), 1)
    assert _solve(lib, PfConfig(4, 3, 0, 150, 1e-8), _fd(none).host) == EINVAL
    assert _solve(lib, PfConfig(tp.n, E, Gn, -1, 1e-8), fd.host) == EINVAL
    # more workgroups than a launch takes: the row chunks of 2^31 - 1 grids with 65 slots; EINVAL wins over the short workspace
    assert _solve(lib, cfg, fd.host, Bt=(1 << 31) - 1, n_row=65, ws_bytes=0) == EINVAL
    # then the short workspace, then the image above the limit
    assert _solve(lib, cfg, fd.host, Bt=3, ws_bytes=nbytes.value - 1) == ESIZE
    big = (pt.LDS_LIMIT // 80) + 1                                   # ten doubles per slot alone pass the limit
    assert lib.gns_dcscopf_lds_bytes(fd.host.ctypes.data, big, ctypes.byref(lds), None) == 0 and lds.value > pt.LDS_LIMIT
    assert _solve(lib, cfg, fd.host, n_row=big) == EUNSUPPORTED
    assert _solve(lib, cfg, fd.host, n_row=big, ws_bytes=0) == ESIZE


# ---- the Python refusals, raised before a device is needed

def test_python_argument_checks():
    buses, lines, gens = synth.synth_grids(14, 3)
    E, Gn = lines.shape[1], gens.shape[1]
    cost = torch.ones(Gn, 2, dtype=torch.float64)
    ok = torch.tensor([[1, 0], [-1, -1]])

    def scopf(**kw):
        kw.setdefault('cost', cost)
        kw.setdefault('rows', ok)
        return powerflow.dc_security_constrained_opf(buses, lines, gens, slack_bus=1, **kw)

    with pytest.raises(TypeError):
        powerflow.dc_security_constrained_opf(buses, lines, gens, slack_bus=1, cost=cost)           # rows is required
    with pytest.raises(ValueError, match='rows is required'):
        scopf(rows=None)
    with pytest.raises(ValueError, match='cost is required'):
        scopf(cost=None)
    for bad in (torch.ones(2, 2), np.ones((2, 2)), torch.ones(2, 2, dtype=torch.bool)):
        with pytest.raises(ValueError, match='rows must hold integers'):
            scopf(rows=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64),
                torch.zeros(2, 4, 2, dtype=torch.int32), torch.zeros(1, 3, 4, 2, dtype=torch.int32)):
        with pytest.raises(ValueError, match='rows must be'):
            scopf(rows=bad)
    # the rows against the topology, on the host's own bridge flags (the public call makes this pass once the topology is known)
    none = np.zeros(E, dtype=bool)

    def check(rows, Bt=1, single=False, bridges=none, n_line=E):
        r = powerflow._dcscopf_rows(rows, Bt, n_line, single)
        powerflow._dcscopf_check_rows(r, n_line, bridges)
        return r

    with pytest.raises(ValueError, match=r'rows\[1\] = \(20, 0\): both must lie in 0..19'):
        check([[1, 0], [E, 0]])
    with pytest.raises(ValueError, match=r'rows\[0\] = \(-1, 3\): both must lie'):
        check(np.array([[-1, 3]]))
    with pytest.raises(ValueError, match=r'rows\[2, 1\] = \(4, 4\): the monitored line is the outaged line'):
        check(torch.tensor([[[1, 0], [-1, -1]]] * 2 + [[[1, 0], [4, 4]]]), Bt=3)
    tp = pt.path(5)                                                       # a path's lines are all bridges
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    assert bridges.all()
    with pytest.raises(ValueError, match=r'rows\[1\] = \(0, 2\): the outage of line 2 disconnects the grid'):
        check([[-1, -1], [0, 2]], bridges=bridges, n_line=4)
    with pytest.raises(ValueError, match=r'rows\[0\] = \(1, 1\): the monitored line is the outaged line'):
        check([[1, 1], [0, 2]], bridges=bridges, n_line=4)                # the first bad row is the one named
    r = check(np.array([[[0, 2], [-1, -1]]]), single=True, n_line=4)
    assert tuple(r.shape) == (2, 2)
    for bad in (torch.zeros(E, dtype=torch.float64), torch.full((3, E), float('nan'), dtype=torch.float64)):
        with pytest.raises(ValueError, match='rating must be positive'):
            scopf(contingency_rating=bad)
    with pytest.raises(ValueError, match='rating must be float64'):
        scopf(contingency_rating=torch.ones(E))
    with pytest.raises(ValueError, match='tol must be >= 0'):
        scopf(tol=-1.0)
    with pytest.raises(ValueError, match='at least one generator'):
        powerflow.dc_security_constrained_opf(buses, lines, gens[:, :0], slack_bus=1, cost=torch.ones(0, 2, dtype=torch.float64), rows=ok)
    # the driver's own
    for kw in (dict(rounds=0), dict(rounds=1.5), dict(rows_per_round=0), dict(rows_per_round=None)):
        with pytest.raises(ValueError, match='must be a positive integer'):
            powerflow.dc_secure_dispatch(buses, lines, gens, slack_bus=1, cost=cost, rating=torch.ones(E, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match='violation_tol must be >= 0'):
        powerflow.dc_secure_dispatch(buses, lines, gens, slack_bus=1, cost=cost, rating=torch.ones(E, dtype=torch.float64), violation_tol=-1)


# ---- the sets and the reference

def test_sets_keep_their_promises():
    cases.check()
    assert cases.case('case14_qp').rows.dim() == 3 and cases.case('case14_qp').batch.buses.shape[0] == 3
    assert cases.case('case14_lp').rows.dim() == 2 and cases.case('case14_lp').rating_c.dim() == 1
    assert [cases.case(n).rows.shape[-2] for n in ('wheel_qp_r63', 'wheel_qp_r64', 'wheel_lp_r65')] == [63, 64, 65]
    w = cases.case('wheel_qp_r64')
    assert w.batch.gens.shape[1] == 66 and w.batch.lines.shape[1] == 140
    for name in cases.SETS:
        rows = cases.case(name).rows.reshape(-1, cases.case(name).rows.shape[-2], 2)
        empty = (rows == -1).all(dim=-1)
        assert empty[:, -1].all(), name                                     # empty slots at the end of every list
        if rows.shape[1] > 6:
            assert empty[:, 4].all() and (~empty[:, 5:]).any(), name          # and in the middle, rows behind it
    f, t = cases.case('meshed14').batch.lines[0, :, 0], cases.case('meshed14').batch.lines[0, :, 1]
    assert (f == t).any()                                                   # the self-loop


def test_reference_three_bus_closed_form():
    """No base rating, line 1-3 may carry 0.6 after an outage, the row (1, 0): p = (0.6, 0.4), cost 18, mu_row 20, lmp (10, 30, 30);
    the lmp also against central differences of the reference's own optimal cost."""
    (p, rc), r = cases.problems('three_bus')[0], cases.optimum('three_bus')[0]
    rows = cases.rows_of('three_bus', 0)
    assert r['converged']
    assert np.abs(r['pg'] - np.array(cases.THREE_BUS_PG)).max() <= 1e-7 and abs(r['objective'] - cases.THREE_BUS_OBJECTIVE) <= 1e-6
    live = np.flatnonzero(rows[:, 0] >= 0)
    assert live.size == 1 and abs(r['mu_row'][live[0]] - cases.THREE_BUS_MU_ROW) <= 1e-5 and abs(r['row_flow'][live[0]] - 0.6) <= 1e-7
    assert np.abs(r['lmp'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5
    assert np.all(r['mu_row'][rows[:, 0] < 0] == 0.0) and np.all(np.isnan(r['row_flow'][rows[:, 0] < 0]))
    step = 1e-4
    for bus in range(3):
        vals = []
        for s in (+step, -step):
            buses = p[0].copy()
            buses[bus, 2] += s
            vals.append(ref.solve(buses, *p[1:], rows, rc, tol=1e-11, max_iter=60, best=True)['objective'])
        assert abs((vals[0] - vals[1]) / (2 * step) - cases.THREE_BUS_LMP[bus]) <= 1e-5


@pytest.mark.parametrize('name', ('three_bus', 'case14_qp'))
def test_the_two_formulations_agree(name):
    """The reduced formulation (rows of the rebuilt networks' shift factors) against the full one (an angle vector per network): the
    dispatch, the cost, the rows' multipliers and the lmp as the sum of the balance multipliers over all networks.  Both stop inside
    the same tolerance ball, so they agree to what ``bars`` allows for that."""
    (p, rc), r = cases.problems(name)[0], cases.optimum(name)[0]
    f = ref.solve_full(*p, cases.rows_of(name, 0), rc)
    bar = cases.bars(name)
    assert f['converged'] and r['converged']
    assert abs(f['objective'] - r['objective']) <= bar['objective'] * max(1.0, abs(r['objective']))
    assert np.abs(f['pg'] - r['pg']).max() <= bar['pg']
    assert np.abs(f['lmp'] - r['lmp']).max() <= bar['lmp']
    assert np.abs(f['mu_row'] - r['mu_row']).max() <= bar['lmp']


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_reference_kkt_certificate(name):
    for g, ((p, rc), r) in enumerate(zip(cases.problems(name), cases.optimum(name))):
        k = ref.kkt_residuals(r, p, cases.rows_of(name, g), rc)
        bar = ref.DEFAULT_TOL + 1e-12 * k['scale']
        assert k['grad'] <= bar and k['comp'] <= bar and k['lmp_def'] <= bar and k['min_mu'] >= 0.0, k
        assert k['max_h'] <= bar * k['feas_scale'], k


def test_generated_rows_reach_the_optimum_with_every_row():
    """The reference's constraint generation (every pair overloaded by more than 1e-9 listed) against its optimum with every row
    listed, on the driver's small sets: the same dispatch, within the sets' bars."""
    for name in ('case14_qp', 'lattice5'):
        want, bar = cases.secure_optimum(name), cases.bars(name)
        for g, (p, rc) in enumerate(cases.problems(name)):
            res, rows, _ = ref.generate(*p, rc, cases.case(name).outages, 8, 1e-9)
            print(name, g, len(rows), np.abs(res['pg'] - want[g]['pg']).max(), bar['pg'])
            assert np.abs(res['pg'] - want[g]['pg']).max() <= bar['pg']
