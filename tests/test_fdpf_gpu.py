"""Fast-decoupled power flow on the MI355X (``powerflow.fast_decoupled``, include/gns_powerflow.h "Fast-decoupled"): both variants
per grid against the float64 oracle (``fd_reference``), manufactured solutions, an independent NR residual, bitwise
reproducibility, warm starts, per-grid failure, n_pq = 0, mixed batches, gradients through the NR adjoint and the LDS refusal."""
import ctypes

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig, load_library
import fd_reference as fref
import nr_reference as ref
import pf_topologies as pt
from test_powerflow_gpu import TRUTH_TOL, _odd, _sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VARIANTS = ('XB', 'BX')
FIELDS = ('v', 'theta', 'converged', 'iterations', 'mismatch')


@pytest.fixture(scope='module')
def grid_sets():
    return _sets()


def _fd(s, variant, **kw):
    buses, lines, gens, slack = s[:4]
    return powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant, **kw)


def _same(a, b):
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


@pytest.mark.parametrize('variant', VARIANTS)
def test_against_the_oracle(grid_sets, variant):
    n_conv, n_same, n_all = 0, 0, 0
    for name, s in grid_sets.items():
        res = _fd(s, variant)
        assert res.v.dtype == torch.float64 and res.converged.dtype == torch.bool and res.iterations.dtype == torch.int32
        buses, lines, gens = (t.cpu() for t in s[:3])
        for i in range(buses.shape[0]):
            vm, va, conv, it, mis = fref.fast_decoupled(buses[i], lines[i], gens[i], s[3], variant)
            n_all += 1
            assert bool(res.converged[i]) == conv, (name, i, float(res.mismatch[i]), mis)
            if not conv:
                continue
            n_conv += 1
            assert np.max(np.abs(res.v[i].cpu().numpy() - vm)) <= 1e-9, (name, i)
            assert np.max(np.abs(res.theta[i].cpu().numpy() - va)) <= 1e-9, (name, i)
            d = abs(int(res.iterations[i]) - it)
            assert d <= 1, (name, i, int(res.iterations[i]), it)
            n_same += d == 0
            assert float(res.mismatch[i]) < 1e-8
    assert n_conv >= 0.4 * n_all and n_same >= 0.99 * n_conv, (n_conv, n_same, n_all)


@pytest.mark.parametrize('variant', VARIANTS)
def test_manufactured_solutions_and_independent_residual(grid_sets, variant):
    for name, s in grid_sets.items():
        res = _fd(s, variant)
        ok = res.converged
        if name == 'case14':
            assert bool(ok.all()) and bool((res.iterations > 0).all())
        assert float(res.theta[:, s[3] - 1].abs().max()) == 0.0
        if not bool(ok.any()):
            continue
        assert float((res.v[ok] - s[4][ok]).abs().max()) <= TRUTH_TOL, name
        assert float((res.theta[ok] - s[5][ok]).abs().max()) <= TRUTH_TOL, name
        buses, lines, gens = (t.cpu() for t in s[:3])
        for i in np.flatnonzero(ok.cpu().numpy()):
            assert ref.mismatch(buses[i], lines[i], gens[i], s[3], res.v[i].cpu(), res.theta[i].cpu()) <= 1e-7, (name, i)


def test_bitwise_reproducible_alone_batched_reordered():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 300, seed=9, device=DEV)
    for variant in VARIANTS:
        a = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant)
        b = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant)
        for k in FIELDS:
            assert _same(getattr(a, k), getattr(b, k)), k
        for bt in (1, 63, 64, 65):
            p = powerflow.fast_decoupled(buses[:bt], lines[:bt], gens[:bt], slack_bus=slack, variant=variant)
            for k in FIELDS:
                assert _same(getattr(p, k), getattr(a, k)[:bt]), (bt, k)
        perm = torch.randperm(buses.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
        r = powerflow.fast_decoupled(buses[perm], lines[perm], gens[perm], slack_bus=slack, variant=variant)
        for k in FIELDS:
            assert _same(getattr(r, k), getattr(a, k)[perm]), k
        one = powerflow.fast_decoupled(buses[5], lines[5], gens[5], slack_bus=slack, variant=variant)
        assert one.v.shape == (118,) and torch.equal(one.v, a.v[5]) and torch.equal(one.iterations, a.iterations[5])
    xb = powerflow.fast_decoupled(buses[:16], lines[:16], gens[:16], slack_bus=slack, variant='XB')
    bx = powerflow.fast_decoupled(buses[:16], lines[:16], gens[:16], slack_bus=slack, variant='BX')
    assert not torch.equal(xb.iterations, bx.iterations) or not torch.equal(xb.v, bx.v)


def test_warm_start_and_defaults():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(14, 32, seed=6, device=DEV)
    cold = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='XB')
    assert bool(cold.converged.all())
    hot = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='XB', v0=cold.v, theta0=cold.theta + 0.25)
    assert bool((hot.iterations == 0).all()) and bool(hot.converged.all())
    assert float((hot.theta - cold.theta).abs().max()) <= 1e-12
    near = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='BX', v0=v + 0.01, theta0=theta)
    b, l, g = (t.cpu() for t in (buses, lines, gens))
    for i in range(4):
        want = fref.fast_decoupled(b[i], l[i], g[i], slack, 'BX', v0=(v + 0.01)[i].cpu().numpy(), theta0=theta[i].cpu().numpy())
        assert bool(near.converged[i]) == want[2] and abs(int(near.iterations[i]) - want[3]) <= 1
        assert np.max(np.abs(near.v[i].cpu().numpy() - want[0])) <= 1e-9
    capped = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='XB', max_iter=2)
    assert bool((capped.iterations <= 2).all()) and not bool(capped.converged.any())
    with pytest.raises(ValueError, match='variant'):
        powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='XX')
    with pytest.raises(TypeError):
        powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack)


def test_bad_grids_fail_alone_and_n_pq_zero():
    buses, lines, gens, slack, v, theta = synth.solvable_grids(14, 8, seed=4, device=DEV)
    lines[2, 3, 2] = float('nan')
    buses[6, :, 2:4] *= 100.0
    for variant in VARIANTS:
        res = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant)
        good = [0, 1, 3, 4, 5, 7]
        assert not bool(res.converged[[2, 6]].any()) and bool(res.converged[good].all())
        assert int(res.iterations[2]) == 0 and bool(res.mismatch[2].isnan())
        assert bool(torch.isfinite(res.v[2]).all()) and bool(torch.isfinite(res.theta[6]).all())
        alone = powerflow.fast_decoupled(buses[good], lines[good], gens[good], slack_bus=slack, variant=variant)
        for k in FIELDS:
            assert _same(getattr(res, k)[good], getattr(alone, k)), k
    name = 'odd_hub_all_gens_b2_K4_d10_single'
    s = _odd(name, seed=2)
    f = s[1][0, :, :2].cpu().numpy()
    assert powerflow.analyse_fd_topology(s[0].shape[1], f[:, 0], f[:, 1], s[2][0, :, 0].cpu().numpy(), s[3]).info['dim_pp'] == 0
    buses, lines, gens = (t.cpu() for t in s[:3])
    for variant in VARIANTS:
        res = _fd(s, variant)
        ok = res.converged
        assert bool(ok[0])                          # (grid 1 needs more than 30 iterations: the oracle agrees)
        assert float((res.v[ok] - s[4][ok]).abs().max()) <= TRUTH_TOL and float((res.theta[ok] - s[5][ok]).abs().max()) <= TRUTH_TOL
        for i in range(buses.shape[0]):
            vm, va, conv, it, _ = fref.fast_decoupled(buses[i], lines[i], gens[i], s[3], variant)
            assert bool(ok[i]) == conv and abs(int(res.iterations[i]) - it) <= 1
            assert np.max(np.abs(res.v[i].cpu().numpy() - vm)) <= 1e-9 and np.max(np.abs(res.theta[i].cpu().numpy() - va)) <= 1e-9


def test_mixed_batches_match_plain_calls():
    s = synth.solvable_contingency_grids(14, 120, range(20), seed=3, device=DEV, shuffle=True)
    buses, lines, gens, slack, v, theta, outage = s
    for variant in VARIANTS:
        res = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant, mixed_topologies=True)
        n_isl = 0
        for j in outage.unique().tolist():
            idx = torch.nonzero(outage == j).flatten()
            try:
                plain = powerflow.fast_decoupled(buses[idx], lines[idx], gens[idx], slack_bus=slack, variant=variant)
            except powerflow.IslandedTopology:
                n_isl += 1
                assert not bool(res.converged[idx].any()) and bool((res.iterations[idx] == -1).all())
                assert bool(res.v[idx].isnan().all()) and bool(res.mismatch[idx].isnan().all())
                continue
            for k in FIELDS:
                assert _same(getattr(res, k)[idx], getattr(plain, k)), (variant, j, k)
        assert n_isl >= 1
        again = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant=variant, mixed_topologies=True)
        for k in FIELDS:
            assert _same(getattr(again, k), getattr(res, k)), k


def _loss_grads(solver, buses, lines, gens, slack, a, b, **kw):
    bu, li, ge = (t.clone().requires_grad_(True) for t in (buses, lines, gens))
    res = solver(bu, li, ge, slack_bus=slack, **kw)
    (torch.where(res.converged[:, None], res.v * a + res.theta * b, 0.0).sum()).backward()
    return res, bu.grad, li.grad, ge.grad


def test_gradients_are_the_nr_adjoint_at_the_fd_solution():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 16, seed=5, device=DEV)
    g = torch.Generator().manual_seed(0)
    a = torch.randn(buses.shape[:2], generator=g, dtype=torch.float64).to(DEV)
    b = torch.randn(buses.shape[:2], generator=g, dtype=torch.float64).to(DEV)
    fd, gb, gl, gg = _loss_grads(powerflow.fast_decoupled, buses, lines, gens, slack, a, b, variant='BX')
    nofd = powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='BX')
    for k in FIELDS:
        assert _same(getattr(fd, k), getattr(nofd, k)), k
    # bit-identical to one direct gns_pf_adjoint call at FD's outputs
    lib = load_library()
    topo = powerflow._topology(buses, lines, gens, slack)
    Bt, N = buses.shape[0], buses.shape[1]
    cfg = PfConfig(N, lines.shape[1], gens.shape[1], 30, 1e-8)
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    conv = fd.converged.to(torch.uint8)
    gv = torch.where(fd.converged[:, None], a, 0.0).contiguous()
    gth = torch.where(fd.converged[:, None], b, 0.0).contiguous()
    ob, ol, og = torch.empty_like(buses), torch.empty_like(lines), torch.empty_like(gens)
    assert lib.gns_pf_adjoint(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), buses.data_ptr(), lines.data_ptr(),
                              gens.data_ptr(), Bt, fd.v.data_ptr(), fd.theta.data_ptr(), conv.data_ptr(), gv.data_ptr(),
                              gth.data_ptr(), ob.data_ptr(), ol.data_ptr(), og.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _same(gb, ob) and _same(gl, ol) and _same(gg, og)
    # within 1e-5 relative of newton_raphson's gradients where both converged
    nr, nb, nl, ng = _loss_grads(powerflow.newton_raphson, buses, lines, gens, slack, a, b)
    both = (fd.converged & nr.converged).cpu()
    assert int(both.sum()) >= 12
    for x, y in ((gb, nb), (gl, nl), (gg, ng)):
        x, y = x.cpu()[both].double(), y.cpu()[both].double()
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
    # a grid that did not converge gets NaN rows (with a non-zero incoming gradient)
    bu = buses.clone().requires_grad_(True)
    capped = powerflow.fast_decoupled(bu, lines, gens, slack_bus=slack, variant='XB', max_iter=3)
    (capped.v * a).sum().backward()
    assert not bool(capped.converged.any()) and bool(bu.grad.isnan().all())


def test_mixed_gradients_reuse_one_classification():
    s = synth.solvable_contingency_grids(14, 40, range(20), seed=3, device=DEV, shuffle=True)
    buses, lines, gens, slack = s[:4]
    a = torch.ones(buses.shape[:2], dtype=torch.float64, device=DEV)
    calls = []
    orig = gns_mod._classify_ids

    def counting(*args, **kw):
        calls.append(1)
        return orig(*args, **kw)

    gns_mod._classify_ids = counting
    try:
        res, gb, gl, gg = _loss_grads(powerflow.fast_decoupled, buses, lines, gens, slack, a, a, variant='XB', mixed_topologies=True)
    finally:
        gns_mod._classify_ids = orig
    assert len(calls) == 1
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    N = buses.shape[1]
    gv = torch.where(res.converged[:, None], a, 0.0).contiguous()
    want = powerflow._adjoint_mixed(load_library(), PfConfig(N, lines.shape[1], gens.shape[1], 30, 1e-8), plan,
                                    (plan.topo_set.host, plan.topo_set.blob), buses, lines, gens, res.v, res.theta, res.converged,
                                    gv, gv, (True, True, True))
    assert _same(gb, want[0]) and _same(gl, want[1]) and _same(gg, want[2])


def test_lds_refusal_names_the_image():
    tp = pt.path(1500)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    info = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack).info
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.fast_decoupled(buses, lines, gens, slack_bus=tp.slack, variant='XB')
    assert str(info['lds_bytes']) in str(e.value)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE):
        powerflow.fast_decoupled(buses, lines, gens, slack_bus=tp.slack, variant='BX', mixed_topologies=True)
