"""Newton-Raphson power flow on batches that mix topologies (``newton_raphson(..., mixed_topologies=True)``, ``gns_pf_solve_set``)
on the MI355X: bit-identity with per-topology plain calls, manufactured truth, islands, launch-order independence, uniform
batches, caching, poisoned workspaces, the C-ABI's errors and one full-size N-1 set."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig
import nr_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TRUTH_TOL = 5e-7                      # test_powerflow_host.TRUTH_TOL
FIELDS = ('v', 'theta', 'converged', 'iterations', 'mismatch')
C30_OUTAGES = [0, 3, 7, 12, 15, 20, 22, 25, 29, 33, 38, 40]


def _islanding(case, slack, outages):
    f, t, _ = synth.case_topology(case)
    n, e, _ = synth.CASE_SHAPES[case]
    out = set()
    for j in outages:
        keep = np.arange(e) != j
        if powerflow._islanded(n, (f[keep] - 1).astype(np.int64), (t[keep] - 1).astype(np.int64), slack - 1).size:
            out.add(int(j))
    return out


@pytest.fixture(scope='module')
def mixed_sets():
    return {14: synth.solvable_contingency_grids(14, 120, range(20), seed=3, device=DEV, shuffle=True),
            30: synth.solvable_contingency_grids(30, 96, C30_OUTAGES, seed=4, device=DEV, shuffle=True)}


def _mixed(s, **kw):
    buses, lines, gens, slack = s[:4]
    return powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, mixed_topologies=True, **kw)


def _warm(s):
    v, theta = s[4], s[5]
    return v * (1.0 + 0.01 * torch.cos(torch.arange(v.numel(), device=v.device, dtype=v.dtype)).reshape(v.shape)), theta + 0.02


def _same(a, b):
    """Bit-identical, NaN rows (grids not solved) included."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def _assert_rows(res, idx, other, what=''):
    for k in FIELDS:
        assert _same(getattr(res, k)[idx], getattr(other, k)), (what, k)


def _assert_not_solved(res, idx):
    assert not bool(res.converged[idx].any())
    assert bool((res.iterations[idx] == -1).all())
    assert bool(res.v[idx].isnan().all()) and bool(res.theta[idx].isnan().all()) and bool(res.mismatch[idx].isnan().all())


def test_bit_identical_to_per_topology_plain_calls(mixed_sets):
    for case, s in mixed_sets.items():
        buses, lines, gens, slack, v, theta, outage = s
        isl = _islanding(case, slack, outage.unique().tolist())
        assert isl and len(isl) < outage.unique().numel()
        for warm in (False, True):
            v0, th0 = _warm(s) if warm else (None, None)
            res = _mixed(s, v0=v0, theta0=th0)
            assert res.v.dtype == torch.float64 and res.converged.dtype == torch.bool and res.iterations.dtype == torch.int32
            for j in outage.unique().tolist():
                idx = torch.nonzero(outage == j).flatten()
                if j in isl:
                    _assert_not_solved(res, idx)
                    continue
                kw = dict(v0=v0[idx], theta0=th0[idx]) if warm else {}
                plain = powerflow.newton_raphson(buses[idx], lines[idx], gens[idx], slack_bus=slack, **kw)
                _assert_rows(res, idx, plain, (case, j, warm))


def test_truth_and_reference_nr(mixed_sets):
    n_conv, n_ref = 0, 0
    for case, s in mixed_sets.items():
        buses, lines, gens, slack, v, theta, outage = s
        isl = _islanding(case, slack, outage.unique().tolist())
        res = _mixed(s)
        solved = np.array([int(o) not in isl for o in outage.tolist()])
        conv = res.converged.cpu().numpy()
        assert conv[solved].mean() >= 0.9, (case, conv[solved].mean())
        ok = np.flatnonzero(conv & solved)
        n_conv += ok.size
        assert float((res.v[ok] - v[ok]).abs().max()) <= TRUTH_TOL
        assert float((res.theta[ok] - theta[ok]).abs().max()) <= TRUTH_TOL
        assert float(res.mismatch[ok].max()) < 1e-8
        b, l, g = (t.cpu() for t in (buses, lines, gens))
        for i in ok[::7]:
            vm, va, c, it, _ = ref.newton_raphson(b[i], l[i], g[i], slack)
            assert c
            assert np.max(np.abs(res.v[i].cpu().numpy() - vm)) <= 1e-9, (case, i)
            assert np.max(np.abs(res.theta[i].cpu().numpy() - va)) <= 1e-9, (case, i)
            assert abs(int(res.iterations[i]) - it) <= 1
            n_ref += 1
    assert n_conv > 150 and n_ref > 20


def test_islands_are_per_grid(mixed_sets):
    buses, lines, gens, slack, v, theta, outage = mixed_sets[30]
    isl = _islanding(30, slack, C30_OUTAGES)
    res = _mixed(mixed_sets[30])
    bad = torch.as_tensor([int(o) in isl for o in outage.tolist()], device=DEV)
    assert 0 < int(bad.sum()) < bad.numel()
    _assert_not_solved(res, bad)
    keep = torch.nonzero(~bad).flatten()
    without = powerflow.newton_raphson(buses[keep], lines[keep], gens[keep], slack_bus=slack, mixed_topologies=True)
    _assert_rows(res, keep, without, 'neighbours')
    # one islanding topology alone: not solved under mixed_topologies, refused by name without it
    one = torch.nonzero(outage == min(isl & set(outage.tolist()))).flatten()[:3]
    alone = powerflow.newton_raphson(buses[one], lines[one], gens[one], slack_bus=slack, mixed_topologies=True)
    _assert_not_solved(alone, torch.arange(one.numel(), device=DEV))
    with pytest.raises(ValueError, match='have no path of lines to slack_bus'):
        powerflow.newton_raphson(buses[one], lines[one], gens[one], slack_bus=slack)


def test_uniform_batches_match_the_plain_call():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(118, 70, seed=5, device=DEV)
    plain = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    mixed = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, mixed_topologies=True)
    _assert_rows(mixed, slice(None), plain, 'uniform')
    typed = buses.clone()
    typed[:, slack - 1, 1] = 3.0
    _assert_rows(powerflow.newton_raphson(typed, lines, gens, mixed_topologies=True), slice(None), plain, 'slack from type')
    one = powerflow.newton_raphson(buses[3], lines[3], gens[3], slack_bus=slack, mixed_topologies=True)
    assert one.v.shape == (118,) and torch.equal(one.v, plain.v[3]) and torch.equal(one.iterations, plain.iterations[3])
    cpu = powerflow.newton_raphson(buses.cpu(), lines.cpu(), gens.cpu(), slack_bus=slack, mixed_topologies=True)
    assert cpu.v.device.type == 'cpu' and torch.equal(cpu.v, plain.v.cpu())


def _raw(plan, s, order, grid_off=None, ws_delta=0, cfg=None, null=None):
    """One gns_pf_solve_set call on plan's set; returns (rc, outputs)."""
    lib = amd.load_library()
    buses, lines, gens = s[:3]
    Bt, N = buses.shape[0], buses.shape[1]
    cfg = cfg or PfConfig(N, lines.shape[1], gens.shape[1], 10, 1e-8)
    ts, members = plan.topo_set, plan.member_off
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes_set(ctypes.byref(PfConfig(N, lines.shape[1], gens.shape[1], 10, 1e-8)), ts.host.ctypes.data,
                                          ts.words, members.ctypes.data, members.size, Bt, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    out = [torch.full((Bt, N), 7.0, dtype=torch.float64, device=DEV), torch.full((Bt, N), 7.0, dtype=torch.float64, device=DEV),
           torch.full((Bt,), 7, dtype=torch.uint8, device=DEV), torch.full((Bt,), 7, dtype=torch.int32, device=DEV),
           torch.full((Bt,), 7.0, dtype=torch.float64, device=DEV)]
    ptr = dict(set_dev=ts.blob.data_ptr(), grid_off=(plan.grid_off if grid_off is None else grid_off).data_ptr(),
               buses=buses.data_ptr(), v=out[0].data_ptr(), ws=ws.data_ptr())
    if null:
        ptr[null] = None
    rc = lib.gns_pf_solve_set(ctypes.byref(cfg), ts.host.ctypes.data, ptr['set_dev'], ts.words, members.ctypes.data, members.size,
                              ptr['grid_off'], order, ptr['buses'], lines.data_ptr(), gens.data_ptr(), Bt, None, None, ptr['v'],
                              out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), ptr['ws'],
                              need.value + ws_delta, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_order_independence_and_c_abi_errors(mixed_sets):
    s = mixed_sets[14]
    buses, lines, gens, slack = s[:4]
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    res = _mixed(s)
    rc, sorted_out = _raw(plan, s, plan.order.data_ptr())
    assert rc == 0
    rc, input_out = _raw(plan, s, None)
    assert rc == 0
    rev = torch.flip(plan.order, [0]).contiguous()
    rc, rev_out = _raw(plan, s, rev.data_ptr())
    assert rc == 0
    for k, a, b, c in zip(FIELDS, sorted_out, input_out, rev_out):
        assert _same(a, b) and _same(a, c), k
        assert _same(a.bool() if k == 'converged' else a, getattr(res, k)), k
    assert _raw(plan, s, None, ws_delta=-1)[0] == 4                       # GNS_ESIZE
    for null in ('set_dev', 'grid_off', 'buses', 'v', 'ws'):
        assert _raw(plan, s, None, null=null)[0] == 1, null               # GNS_EINVAL
    N, E, Gn = buses.shape[1], lines.shape[1], gens.shape[1]
    assert _raw(plan, s, None, cfg=PfConfig(N + 1, E, Gn, 10, 1e-8))[0] == 1
    assert _raw(plan, s, None, cfg=PfConfig(N, E, Gn + 1, 10, 1e-8))[0] == 1
    # offsets that are not at a blob of this set: those grids come back not solved, the others as before
    go = plan.grid_off.clone()
    solved = torch.nonzero(go >= 0).flatten()
    hit = solved[[0, 1, 2, 3]]
    go[hit[0]] = go[hit[0]] + 16                                          # aligned, inside a blob
    go[hit[1]] = go[hit[1]] + 2                                           # misaligned
    go[hit[2]] = plan.topo_set.words                                      # past the set
    go[hit[3]] = 1 << 30
    rc, out = _raw(plan, s, plan.order.data_ptr(), grid_off=go)
    assert rc == 0
    r = powerflow.PowerFlowResult(out[0], out[1], out[2].bool(), out[3], out[4])
    _assert_not_solved(r, hit)
    rest = torch.ones(buses.shape[0], dtype=torch.bool, device=DEV)
    rest[hit] = False
    for k, a in zip(FIELDS, out):
        want = getattr(res, k)
        assert _same(a[rest].bool() if k == 'converged' else a[rest], want[rest]), k


def test_caching_and_poisoned_workspace(mixed_sets, monkeypatch):
    monkeypatch.setattr(powerflow, '_TOPO_CACHE', {})
    monkeypatch.setattr(powerflow, '_ISLANDED', set())
    monkeypatch.setattr(powerflow, '_SET_CACHE', {})
    calls = []
    real = powerflow.analyse_topology
    monkeypatch.setattr(powerflow, 'analyse_topology', lambda *a, **k: calls.append(a[1:4]) or real(*a, **k))
    s = mixed_sets[30]
    first = _mixed(s)
    assert len(calls) == s[6].unique().numel()
    (ts,) = powerflow._SET_CACHE.values()
    words, blob = ts.words, ts.blob
    calls.clear()
    again = _mixed(s)
    assert calls == [] and ts.words == words and ts.blob is blob
    _assert_rows(again, slice(None), first, 'repeat')
    sub = torch.arange(0, 40, device=DEV)                                 # a subset of the topologies: still nothing new
    _mixed(tuple(t[sub] if torch.is_tensor(t) else t for t in s))
    assert calls == [] and ts.blob is blob
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)
    poisoned = _mixed(s, v0=s[4], theta0=s[5])
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', False)
    clean = _mixed(s, v0=s[4], theta0=s[5])
    _assert_rows(poisoned, slice(None), clean, 'poisoned')
    _assert_rows(_mixed(s), slice(None), first, 'after poison')


def test_full_size_case118_n_minus_1_and_case300():
    bt = 16384
    e = synth.CASE_SHAPES[118][1]
    buses, lines, gens, slack, v, theta, outage = synth.solvable_contingency_grids(118, bt, range(e), seed=8, device=DEV,
                                                                                   shuffle=True)
    res = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack, mixed_topologies=True)
    isl = _islanding(118, slack, range(e))
    assert len(isl) == 20
    bad = torch.as_tensor([int(o) in isl for o in outage.tolist()], device=DEV)
    assert int((res.iterations == -1).sum()) == int(bad.sum())
    _assert_not_solved(res, bad)
    rng = np.random.default_rng(0)
    ok_outages = sorted(set(range(e)) - isl)
    n_conv_plain, n_conv_mixed = 0, 0
    for j in rng.choice(ok_outages, size=12, replace=False).tolist():
        idx = torch.nonzero(outage == j).flatten()
        plain = powerflow.newton_raphson(buses[idx], lines[idx], gens[idx], slack_bus=slack)
        _assert_rows(res, idx, plain, j)
        n_conv_plain += int(plain.converged.sum())
        n_conv_mixed += int(res.converged[idx].sum())
    assert n_conv_plain == n_conv_mixed
    assert res.converged.cpu().numpy()[~bad.cpu().numpy()].mean() >= 0.9
    # case300: a 93 KB LDS image per grid
    outs = [0, 5, 60, 200, 400]
    b3, l3, g3, s3, v3, t3, o3 = synth.solvable_contingency_grids(300, 40, outs, seed=2, device=DEV)
    r3 = powerflow.newton_raphson(b3, l3, g3, slack_bus=s3, mixed_topologies=True)
    isl3 = _islanding(300, s3, outs)
    for j in outs:
        idx = torch.nonzero(o3 == j).flatten()
        if j in isl3:
            _assert_not_solved(r3, idx)
        else:
            _assert_rows(r3, idx, powerflow.newton_raphson(b3[idx], l3[idx], g3[idx], slack_bus=s3), (300, j))
    assert len(isl3) < len(outs) and bool(r3.converged.any())
