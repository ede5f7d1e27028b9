"""CPU checks of the DC optimal power flow's gradient (include/gns_powerflow.h, "DC optimal power flow: adjoint") that need no
device: the float64 reference (``dc_opf_grad_reference``: the active-set adjoint in the full ``(theta_r, p)`` formulation) against
central differences of ``dc_opf_reference.solve`` on every grid of every set of ``dc_opf_cases`` that has a derivative, the count of
the grids that do not, the exports, the refusals of the C entry points and of the Python call.

The differences are of the reference solved to 1e-11 with step 1e-5, two entries of each input (the first and the last; of the
rating, the first and the last line with a limit); the bar is 1e-6 of the gradient's scale ``max(1, max|ref grad|)`` over the grid.
Measured: 1.7e-7 at worst (hub150_lp), the differences' own noise.  A grid is left out when its margin ``min_i max(z_i, mu_i)`` is
below 1e-4: ``stacked_units`` grid 0 alone (7e-6; the next smallest margin is 6.6e-4)."""
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
import dc_opf_grad_reference as gref
import pf_topologies as pt

EINVAL, EUNSUPPORTED, ESIZE = 1, 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BAR, FD_STEP = 1e-6, 1e-5


@pytest.mark.parametrize('name', sorted(cases.SETS))
def test_reference_against_central_differences(name):
    kept, margins = gref.kept_grids(name)
    weights = gref.set_weights(name)
    for g in kept:
        p = cases.problems(name)[g]
        res = ref.solve(*p, tol=1e-11, max_iter=60, best=True)
        grads = gref.gradients(p, res, weights[g])
        assert grads['margin'] == margins[g] >= gref.MARGIN_MIN
        scale = max(1.0, max(np.abs(grads[k]).max() for k in gref.INPUTS))
        worst = 0.0
        for k in gref.INPUTS:
            idx = np.flatnonzero(np.isfinite(p[4])) if k == 'rating' else np.arange(grads[k].size)
            for i in sorted({int(j) for j in idx[[0, -1]]} if idx.size else ()):
                fd = gref.central_difference(p, weights[g], k, i, FD_STEP)
                worst = max(worst, abs(fd - grads[k][i]) / scale)
                assert abs(fd - grads[k][i]) <= FD_BAR * scale, (name, g, k, i, fd, grads[k][i], scale)
        print(f'{name}[{g}] margin {margins[g]:.2e} scale {scale:.2e} worst |fd - ref| / scale {worst:.2e}')


def test_the_exclusion_is_a_condition_and_excludes_one_grid():
    out = [(name, g) for name in cases.SETS for g, x in enumerate(gref.kept_grids(name)[1]) if x < gref.MARGIN_MIN]
    total = sum(len(gref.kept_grids(name)[1]) for name in cases.SETS)
    assert total == 28 and len(out) <= 1, out
    assert out == [('stacked_units', 0)]
    assert gref.MARGIN_MIN == 1e-4


def test_reference_gradient_of_the_objective_is_the_prices():
    """The envelope identities on the reference itself, at the closed-form grid: d objective / d Pd = lmp, / d rating = -|mu_line|."""
    p, r = cases.problems('three_bus')[0], cases.optimum('three_bus')[0]
    g = gref.gradients(p, r, dict(objective=1.0))
    assert np.abs(g['Pd'] - np.array(cases.THREE_BUS_LMP)).max() <= 1e-5
    assert abs(g['rating'][1] + cases.THREE_BUS_MU) <= 1e-5 and g['rating'][0] == 0.0 and g['rating'][2] == 0.0
    d = gref.gradients(p, r, dict(pg=np.array([1.0, 0.0])))['Pd'][2], gref.gradients(p, r, dict(pg=np.array([0.0, 1.0])))['Pd'][2]
    assert abs(d[0] + 1.0) <= 1e-9 and abs(d[1] - 2.0) <= 1e-9


# ---- the exports and the C entry points' refusals

def test_exports_are_there_typed_and_declared():
    lib = amd.load_library()
    assert _lib.DCOPF_GRAD_EXPORTS == ('gns_dcopf_adjoint_lds_bytes', 'gns_dcopf_adjoint_workspace_bytes', 'gns_dcopf_adjoint')
    assert _lib.DCOPF_EXPORTS == ('gns_dcopf_lds_bytes', 'gns_dcopf_workspace_bytes', 'gns_dcopf_solve')
    header = open(os.path.join(ROOT, 'include', 'gns_powerflow.h')).read()
    assert 'DC optimal power flow: adjoint' in header
    for f in _lib.DCOPF_GRAD_EXPORTS:
        assert hasattr(lib, f), f
        assert getattr(lib, f).restype is ctypes.c_int and getattr(lib, f).argtypes
        assert re.search(r'\bint ' + f + r'\(', header), f
    assert len(lib.gns_dcopf_adjoint.argtypes) == 36
    assert callable(powerflow.dc_optimal_power_flow_differentiable)
    assert 'dc_optimal_power_flow_differentiable' in powerflow.dc_optimal_power_flow.__doc__
    assert 'Not differentiable' not in powerflow.dc_optimal_power_flow.__doc__


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _adjoint(lib, cfg, host, Bt=2, ws_bytes=1 << 40, null=(), cost_per_grid=0, rating_per_grid=0, cfg_null=False, host_null=False,
             no_outputs=False):
    """gns_dcopf_adjoint with placeholder device pointers (every refusal comes before a launch, so nothing dereferences them); the
    0-based positions ``null`` of its pointer arguments after Bt are NULL: cost, rating, the ten forward outputs, the eight incoming
    gradients, the four gradient outputs."""
    p = 0x1000
    ptrs = [p] * 24
    for i in null:
        ptrs[i] = None
    if no_outputs:
        ptrs[20:24] = [None] * 4
    return lib.gns_dcopf_adjoint(None if cfg_null else ctypes.byref(cfg), None if host_null else host.ctypes.data, p, p, p, p, Bt,
                                 ptrs[0], cost_per_grid, ptrs[1], rating_per_grid, *ptrs[2:], p, ws_bytes, None)


def test_c_entry_points_refuse_before_any_launch():
    lib = amd.load_library()
    tp = pt.path(9, pv=(5,))
    fd = _fd(tp)
    E, Gn = tp.f.size, tp.g.size
    cfg = PfConfig(tp.n, E, Gn, 150, 1e-8)
    nbytes, lds, order = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int32()
    # the queries
    assert lib.gns_dcopf_adjoint_lds_bytes(None, ctypes.byref(lds), None) == EINVAL
    assert lib.gns_dcopf_adjoint_lds_bytes(fd.host.ctypes.data, None, None) == EINVAL
    assert lib.gns_dcopf_adjoint_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(order)) == 0
    i = fd.info
    n = 2 * Gn
    network = 8 * (i['nnz_lu_p'] + i['dim_p'] + i['n_bus'] + 3 * E + 2 * i['dim_p']) + 32 * Gn
    assert order.value == n and lds.value == network + 8 * (3 * Gn + E + (2 * Gn + E + 1) // 2 + n * ((n + 1) | 1))
    assert lib.gns_dcopf_adjoint_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, ctypes.byref(nbytes)) == 0
    assert nbytes.value == (8 * 3 * (E * Gn + E + Gn + 3) + 255) // 256 * 256
    assert lib.gns_dcopf_adjoint_workspace_bytes(None, fd.host.ctypes.data, 3, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_adjoint_workspace_bytes(ctypes.byref(cfg), None, 3, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_adjoint_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 0, ctypes.byref(nbytes)) == EINVAL
    assert lib.gns_dcopf_adjoint_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, 3, None) == EINVAL
    # null pointers: the cost and every forward output are needed; the rating, the incoming gradients and the outputs are not
    for k in (0, *range(2, 12)):
        assert _adjoint(lib, cfg, fd.host, null=(k,)) == EINVAL, k
    assert _adjoint(lib, cfg, fd.host, cfg_null=True) == EINVAL and _adjoint(lib, cfg, fd.host, host_null=True) == EINVAL
    for Bt in (0, -1, 1 << 31):
        assert _adjoint(lib, cfg, fd.host, Bt=Bt) == EINVAL
    assert _adjoint(lib, cfg, fd.host, cost_per_grid=2) == EINVAL and _adjoint(lib, cfg, fd.host, rating_per_grid=-1) == EINVAL
    # a wrong magic, another shape, a Newton-Raphson blob, no unit, a bad configuration
    bad = fd.host.copy()
    bad[0] ^= 1
    assert _adjoint(lib, cfg, bad) == EINVAL
    assert lib.gns_dcopf_adjoint_lds_bytes(bad.ctypes.data, ctypes.byref(lds), None) == EINVAL
    assert _adjoint(lib, PfConfig(tp.n, E, Gn + 1, 150, 1e-8), fd.host) == EINVAL
    nr = powerflow.analyse_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    assert _adjoint(lib, cfg, nr.host) == EINVAL
    none = pt.Topo('no_unit', 4, *pt._ids([1, 2, 3], [2, 3, 4], []), 1)
    assert _adjoint(lib, PfConfig(4, 3, 0, 150, 1e-8), _fd(none).host) == EINVAL
    assert _adjoint(lib, PfConfig(tp.n, E, Gn, -1, 1e-8), fd.host) == EINVAL
    # a short workspace, before anything else the blob decides; no gradient output: nothing to do, after every check
    assert _adjoint(lib, cfg, fd.host, Bt=3, ws_bytes=nbytes.value - 1) == ESIZE
    assert _adjoint(lib, cfg, fd.host, Bt=3, ws_bytes=nbytes.value - 1, no_outputs=True) == ESIZE
    assert _adjoint(lib, cfg, fd.host, no_outputs=True) == 0
    assert _adjoint(lib, cfg, fd.host, null=(1, *range(12, 20)), no_outputs=True) == 0


def test_the_order_is_capped_by_the_lds_limit_and_the_refusal_names_the_formula():
    """250 units on a star: the worst-case KKT order 2 Gn = 500 would take 2 MB; the image is cut to the limit and holds a smaller
    order, which a grid may still exceed (it then gets NaN rows); the call itself is not refused."""
    lib = amd.load_library()
    tp = pt.star(251, 'pv')
    fd = _fd(tp)
    E, Gn = tp.f.size, tp.g.size
    lds, order = ctypes.c_int64(), ctypes.c_int32()
    assert lib.gns_dcopf_adjoint_lds_bytes(fd.host.ctypes.data, ctypes.byref(lds), ctypes.byref(order)) == 0
    n = order.value
    i = fd.info
    fixed = 8 * (i['nnz_lu_p'] + i['dim_p'] + i['n_bus'] + 3 * E + 2 * i['dim_p']) + 32 * Gn + 8 * (3 * Gn + E + (2 * Gn + E + 1) // 2)
    assert 0 < n < 2 * Gn and lds.value == fixed + 8 * n * ((n + 1) | 1) <= pt.LDS_LIMIT
    assert fixed + 8 * (n + 1) * ((n + 2) | 1) > pt.LDS_LIMIT
    assert _adjoint(lib, PfConfig(tp.n, E, Gn, 150, 1e-8), fd.host, ws_bytes=0) == ESIZE          # (not GNS_EUNSUPPORTED)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow._check(EUNSUPPORTED, 'gns_dcopf_adjoint', lds.value, powerflow._DCOPF_ADJOINT_LDS_FORMULA)
    assert 'n ((n + 1) | 1)' in str(e.value)


# ---- the Python refusals, raised before a device is needed

def test_lines_that_require_grad_are_refused():
    buses, lines, gens = synth.synth_grids(14, 2)
    cost = torch.ones(gens.shape[1], 2, dtype=torch.float64)
    with pytest.raises(ValueError, match='does not differentiate with respect to lines'):
        powerflow.dc_optimal_power_flow_differentiable(buses, lines.clone().requires_grad_(), gens, cost=cost, slack_bus=1)
    # the twin takes the plain call's arguments and refuses what it refuses
    with pytest.raises(ValueError, match='cost is required'):
        powerflow.dc_optimal_power_flow_differentiable(buses, lines, gens, cost=None, slack_bus=1)
    with pytest.raises(ValueError, match='rating must be positive'):
        powerflow.dc_optimal_power_flow_differentiable(buses, lines, gens, cost=cost, slack_bus=1,
                                                       rating=torch.zeros(lines.shape[1], dtype=torch.float64))
    import inspect
    assert inspect.signature(powerflow.dc_optimal_power_flow_differentiable) == inspect.signature(powerflow.dc_optimal_power_flow)
