"""Newton-Raphson power flow on the MI355X (include/gns_powerflow.h): manufactured solutions, the test-side reference NR,
an independent residual, per-grid failure, bitwise reproducibility, warm starts, slack selection and the raw C-ABI."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig
from helpers import load_golden
import nr_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the exact solution of the float32 inputs lies within this of the chosen point (test_powerflow_host.TRUTH_TOL)
TRUTH_TOL = 5e-7
ODD = ['odd_chain_one_way_b2_K2_d20_single', 'odd_hub_all_gens_b2_K4_d10_single', 'odd_pair_b3_K3_d20_multi',
       'odd_random_33_many_gens_b2_K4_d20_single']


def _manufacture(buses, lines, gens, slack, spread, seed):
    """(v, theta) chosen like synth.solvable_grids, made a solution by synth.manufacture_solution."""
    bt, n = buses.shape[0], buses.shape[1]
    theta = (synth.counter_uniform(seed, 301, 0, bt, n, buses.device).double() * 2 - 1) * spread
    theta[:, slack - 1] = 0.0
    v = synth.counter_uniform(seed, 302, 0, bt, n, buses.device).double() * 0.1 + 0.95
    gb = gens[..., 0].long() - 1
    for j in range(gens.shape[1] - 1, -1, -1):           # the first generator listed on a bus sets its |V|
        v.scatter_(1, gb[:, j:j + 1], gens[:, j:j + 1, 4].double())
    b, g = synth.manufacture_solution(buses, lines, gens, slack, v, theta)
    return b, lines, g, slack, v, theta


def _odd(name, seed=0, spread=0.1):
    gd = load_golden(name)
    buses, lines, gens = (torch.as_tensor(gd[k]).float().to(DEV) for k in ('buses', 'lines', 'generators'))
    return _manufacture(buses, lines, gens, int(gd['generators'][0, 0, 0]), spread, seed)


def _dupgen14(batch=16, seed=3):
    """case14 with generator 3 moved onto generator 2's bus (a PV bus) under another vg: the first one's vg holds, the Pg add."""
    buses, lines, gens = synth.synth_grids(14, batch, seed=seed, device=DEV)
    gens[:, 2, 0] = gens[:, 1, 0]
    gens[:, 2, 4] = 1.3
    return _manufacture(buses, lines, gens, 1, 0.1, seed)


def _sets():
    out = {f'case{c}': synth.solvable_grids(c, b, seed=7, device=DEV) for c, b in ((14, 64), (30, 32), (118, 16), (300, 8))}
    for name in ODD:
        out[name] = _odd(name, seed=2)            # (seed 0 puts a chain grid where flat-start NR reaches another solution)
    out['case14_dupgen'] = _dupgen14()
    return out


@pytest.fixture(scope='module')
def grid_sets():
    return _sets()


def _solve(s, **kw):
    buses, lines, gens, slack = s[:4]
    return powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, **kw)


def test_manufactured_solutions_are_recovered(grid_sets):
    for name, s in grid_sets.items():
        res = _solve(s)
        assert res.v.dtype == torch.float64 and res.converged.dtype == torch.bool and res.iterations.dtype == torch.int32
        assert bool(res.converged.all()), (name, res.converged, res.mismatch)
        assert float((res.mismatch < 1e-8).all()), name
        assert float((res.v - s[4]).abs().max()) <= TRUTH_TOL, name
        assert float((res.theta - s[5]).abs().max()) <= TRUTH_TOL, name
        assert float(res.theta[:, s[3] - 1].abs().max()) == 0.0


def test_against_reference_nr(grid_sets):
    n_it, n_same = 0, 0
    for name, s in grid_sets.items():
        res = _solve(s)
        buses, lines, gens = (t.cpu() for t in s[:3])
        for i in range(buses.shape[0]):
            vm, va, conv, it, _ = ref.newton_raphson(buses[i], lines[i], gens[i], s[3])
            assert conv
            assert np.max(np.abs(res.v[i].cpu().numpy() - vm)) <= 1e-9, (name, i)
            assert np.max(np.abs(res.theta[i].cpu().numpy() - va)) <= 1e-9, (name, i)
            d = abs(int(res.iterations[i]) - it)
            assert d <= 1, (name, i, int(res.iterations[i]), it)
            n_it += 1
            n_same += d == 0
    assert n_same >= 0.99 * n_it, (n_same, n_it)


@pytest.mark.parametrize('spread', [0.1, 0.3])
def test_independent_residual(spread):
    sets = [synth.solvable_grids(c, 16, seed=11, angle_spread=spread, device=DEV) for c in (14, 30, 118)]
    sets += [_odd(n, seed=5, spread=spread) for n in ODD]
    n_conv = 0
    for s in sets:
        res = _solve(s)
        buses, lines, gens = (t.cpu() for t in s[:3])
        for i in np.flatnonzero(res.converged.cpu().numpy()):
            assert ref.mismatch(buses[i], lines[i], gens[i], s[3], res.v[i].cpu(), res.theta[i].cpu()) <= 1e-7
            n_conv += 1
    assert n_conv > 0


def test_bad_grids_fail_alone():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(30, 8, seed=4, device=DEV)
    lines[2, 3, 2] = float('nan')               # NaN in a line
    lines[4, 5, 2] = 0.0                        # r = x = 0: infinite admittance
    lines[4, 5, 3] = 0.0
    buses[6, :, 2:4] *= 100.0                   # far past what the grid can carry
    res = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    bad = [2, 4, 6]
    good = [0, 1, 3, 5, 7]
    assert not bool(res.converged[bad].any())
    assert bool(torch.isfinite(res.v[bad]).all()) and bool(torch.isfinite(res.theta[bad]).all())
    assert bool(res.converged[good].all())
    alone = powerflow.newton_raphson(buses[good], lines[good], gens[good], slack_bus=slack)
    for k in ('v', 'theta', 'iterations', 'mismatch', 'converged'):
        assert torch.equal(getattr(res, k)[good], getattr(alone, k)), k
    for j, i in enumerate(good):
        one = powerflow.newton_raphson(buses[i], lines[i], gens[i], slack_bus=slack)
        assert torch.equal(one.v, res.v[i]) and torch.equal(one.theta, res.theta[i])


def test_bitwise_reproducible_and_batch_size_independent():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 1000, seed=9, device=DEV)
    a = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    b = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for bt in (1, 63, 64, 65):
        p = powerflow.newton_raphson(buses[:bt], lines[:bt], gens[:bt], slack_bus=slack)
        assert torch.equal(p.v, a.v[:bt]) and torch.equal(p.theta, a.theta[:bt])
        assert torch.equal(p.iterations, a.iterations[:bt]) and torch.equal(p.mismatch, a.mismatch[:bt])


def test_warm_start():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(118, 32, seed=6, device=DEV)
    cold = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    hot = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, v0=cold.v, theta0=cold.theta + 0.25)
    assert bool((hot.iterations == 0).all()) and bool(hot.converged.all())
    assert float((hot.theta - cold.theta).abs().max()) <= 1e-12
    torch.manual_seed(0)
    model = amd.GNS(latent_dim=20, hidden_dim=10, K=4, gamma=0.9, multiple_phi=True).to(DEV)
    with torch.no_grad():
        gv, gth, _, _ = model(buses, lines, gens, *amd.get_BLG())
    warm = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, v0=gv, theta0=gth)
    ok = np.flatnonzero(warm.converged.cpu().numpy())
    assert ok.size >= 16                        # an untrained model's prediction is a poor start for some grids ...
    b, l, g = (t.cpu() for t in (buses, lines, gens))
    for i in ok:                                # ... and from it NR can reach another valid solution of the same grid
        assert ref.mismatch(b[i], l[i], g[i], slack, warm.v[i].cpu(), warm.theta[i].cpu()) <= 1e-7


def test_slack_from_type_column_and_errors():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 8, seed=2, device=DEV)
    explicit = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    with pytest.raises(ValueError, match='slack_bus'):
        powerflow.newton_raphson(buses, lines, gens)
    typed = buses.clone()
    typed[:, slack - 1, 1] = 3.0
    by_type = powerflow.newton_raphson(typed, lines, gens)
    assert torch.equal(by_type.v, explicit.v) and torch.equal(by_type.theta, explicit.theta)
    mixed = lines.clone()
    mixed[3, 0, 1] = 6.0
    with pytest.raises(ValueError, match='differ across the batch'):
        powerflow.newton_raphson(buses, mixed, gens, slack_bus=slack)
    with pytest.raises(ValueError, match='float32'):
        powerflow.newton_raphson(buses.double(), lines, gens, slack_bus=slack)
    single = powerflow.newton_raphson(buses[0], lines[0], gens[0], slack_bus=slack)
    assert single.v.shape == (14,) and torch.equal(single.v, explicit.v[0])


def test_c_abi_errors_and_poisoned_workspace():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 70, seed=8, device=DEV)
    ref_res = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    old = gns_mod.POISON_WORKSPACES
    gns_mod.POISON_WORKSPACES = True
    try:
        poisoned = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    finally:
        gns_mod.POISON_WORKSPACES = old
    for k in ref_res._fields:
        assert torch.equal(getattr(ref_res, k), getattr(poisoned, k)), k
    lib = amd.load_library()
    topo = powerflow._topology(buses, lines, gens, slack)
    Bt, N = buses.shape[0], buses.shape[1]
    cfg = PfConfig(N, lines.shape[1], gens.shape[1], 10, 1e-8)
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    v = torch.empty(Bt, N, dtype=torch.float64, device=DEV)
    th = torch.empty_like(v)
    conv = torch.empty(Bt, dtype=torch.uint8, device=DEV)
    it = torch.empty(Bt, dtype=torch.int32, device=DEV)
    mis = torch.empty(Bt, dtype=torch.float64, device=DEV)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes=need.value, buses_p=buses.data_ptr(), v_p=v.data_ptr(), cfg_=cfg):
        return lib.gns_pf_solve(ctypes.byref(cfg_), topo.host.ctypes.data, topo.blob.data_ptr(), buses_p, lines.data_ptr(),
                                gens.data_ptr(), Bt, None, None, v_p, th.data_ptr(), conv.data_ptr(), it.data_ptr(),
                                mis.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert call(ws_bytes=need.value - 1) == 4                 # GNS_ESIZE
    assert call(buses_p=None) == 1                            # GNS_EINVAL
    assert call(v_p=None) == 1
    assert call(cfg_=PfConfig(N + 1, lines.shape[1], gens.shape[1], 10, 1e-8)) == 1
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(v, ref_res.v) and torch.equal(it, ref_res.iterations)
