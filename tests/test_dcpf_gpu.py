"""DC power flow on the MI355X (``powerflow.dc_power_flow``, include/gns_powerflow.h "DC power flow"): every grid against the
float64 reference (``dc_reference``), power balance, bitwise reproducibility, mixed batches, per-grid failure, gradients against the
reference's autograd, the reuse of the fast-decoupled analysis and the LDS refusal.

The bar of every comparison with the reference is relative, per grid and per output: max|out - ref| <= 1e-9 max(1, max|ref|).  On
the case grids the scale is 1 to 10; on path(1500) the reduced Bbus has a condition number of 2e7 and angles up to 1.2e4 rad, where
two float64 reference solves differ by 2.5e-9 absolute (2e-13 relative) themselves."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import metrics, powerflow, synth
import dc_reference as dref
import pf_topologies as pt
from test_powerflow_gpu import _sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9
FIELDS = ('v', 'theta', 'line_flow', 'slack_p', 'converged')
OUTPUTS = ('theta', 'line_flow', 'slack_p')
NAMES = ('buses', 'lines', 'generators')
CONTRACT = {'buses': [2, 4], 'lines': [3, 5, 6], 'generators': [6]}


def _perturbed(lines, seed):
    """``lines`` with shifts of order +-0.1 rad on a third of the lines and the taps of another third redrawn in [0.85, 1.15]."""
    g = torch.Generator().manual_seed(seed)
    shape = lines.shape[:2]
    draw = [torch.rand(shape, generator=g).to(lines.device) for _ in range(4)]
    lines = lines.clone()
    lines[..., 6] = torch.where(draw[0] < 1 / 3, (draw[1] - 0.5) * 0.4, lines[..., 6])
    lines[..., 5] = torch.where(draw[2] < 1 / 3, 0.85 + 0.3 * draw[3], lines[..., 5])
    return lines


def _all_sets():
    """name -> (buses, lines, generators, slack): the sets of the Newton-Raphson tests and two grids on every generated topology,
    all with shifts and taps that matter."""
    out = {}
    for k, (name, s) in enumerate(_sets().items()):
        out[name] = (s[0], _perturbed(s[1], k), s[2], s[3])
    for k, (name, tp) in enumerate(sorted(pt.families().items())):
        buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
        out[name] = (buses, _perturbed(lines, 100 + k), gens, tp.slack)
    return out


@pytest.fixture(scope='module')
def grid_sets():
    return _all_sets()


def _dc(s, **kw):
    return powerflow.dc_power_flow(s[0], s[1], s[2], slack_bus=s[3], **kw)


def _same(a, b):
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def _check_against_reference(res, s, name):
    buses, lines, gens = (t.cpu() for t in s[:3])
    assert bool(res.converged.all()), name
    for i in range(buses.shape[0]):
        want = dref.dc_power_flow(buses[i], lines[i], gens[i], s[3])
        for k, w in zip(OUTPUTS, want):
            got = getattr(res, k)[i].cpu()
            err, scale = float((got - w).abs().max()), max(1.0, float(w.abs().max()))
            print(f'{name}[{i}] {k}: err {err:.3e} scale {scale:.3e}')
            assert err <= TOL * scale, (name, i, k, err, scale)


def test_against_the_reference(grid_sets):
    for name, s in grid_sets.items():
        res = _dc(s)
        Bt, N, E = s[0].shape[0], s[0].shape[1], s[1].shape[1]
        assert res.v.shape == res.theta.shape == (Bt, N) and res.line_flow.shape == (Bt, E) and res.slack_p.shape == (Bt,)
        assert all(getattr(res, k).dtype == torch.float64 for k in FIELDS[:4]) and res.converged.dtype == torch.bool
        assert res.theta.device == s[0].device
        _check_against_reference(res, s, name)


def test_properties(grid_sets):
    for name, s in grid_sets.items():
        buses, lines, gens, slack = s
        res = _dc(s)
        assert bool((res.theta[:, slack - 1] == 0).all()) and bool((res.v == 1).all()), name
        Bt, N = buses.shape[:2]
        f, t = lines[..., 0].long() - 1, lines[..., 1].long() - 1
        out = torch.zeros(Bt, N, dtype=torch.float64, device=DEV).scatter_add(1, f, res.line_flow).scatter_add(1, t, -res.line_flow)
        pg = torch.zeros(Bt, N, dtype=torch.float64, device=DEV).scatter_add(1, gens[..., 0].long() - 1, gens[..., 6].double())
        net = pg - buses[..., 2].double() - buses[..., 4].double()
        total = -net.sum(dim=1)                                        # sum(Pd + Gs) - sum Pg
        net[:, slack - 1] += res.slack_p
        scale = res.line_flow.abs().amax(dim=1).clamp(min=1.0)
        assert bool(((out - net).abs().amax(dim=1) <= TOL * scale).all()), name
        assert bool(((res.slack_p - total).abs() <= TOL * total.abs().clamp(min=1.0)).all()), name
    # without shifts and taps the flows are active_line_flow with sin replaced by its argument
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 8, seed=2, device=DEV)
    lines[..., 5], lines[..., 6] = 1.0, 0.0
    res = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    f, t = lines[..., 0].long() - 1, lines[..., 1].long() - 1
    d = torch.gather(res.theta, 1, f) - torch.gather(res.theta, 1, t)
    want = d / lines[..., 3].double()
    assert float((res.line_flow - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))
    small = 1e-6 * res.theta                                           # where sin(x) = x to 1e-12 relative
    flow = metrics.active_line_flow(res.v, small, lines[..., 3].double(), lines[0, :, 0], lines[0, :, 1])
    assert float((flow - 1e-6 * want).abs().max()) <= TOL * 1e-6 * max(1.0, float(want.abs().max()))


def test_bitwise_reproducible_alone_batched_reordered():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 300, seed=9, device=DEV)
    lines = _perturbed(lines, 5)
    a = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    b = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    assert bool(a.converged.all())
    for k in FIELDS:
        assert _same(getattr(a, k), getattr(b, k)), k
    for bt in (1, 63, 64, 65):
        p = powerflow.dc_power_flow(buses[:bt], lines[:bt], gens[:bt], slack_bus=slack)
        for k in FIELDS:
            assert _same(getattr(p, k), getattr(a, k)[:bt]), (bt, k)
    perm = torch.randperm(buses.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    r = powerflow.dc_power_flow(buses[perm], lines[perm], gens[perm], slack_bus=slack)
    for k in FIELDS:
        assert _same(getattr(r, k), getattr(a, k)[perm]), k
    one = powerflow.dc_power_flow(buses[5], lines[5], gens[5], slack_bus=slack)
    assert one.theta.shape == (118,) and one.line_flow.shape == (lines.shape[1],) and one.slack_p.shape == ()
    for k in FIELDS:
        assert _same(getattr(one, k), getattr(a, k)[5]), k
    cpu = powerflow.dc_power_flow(buses[:4].cpu(), lines[:4].cpu(), gens[:4].cpu(), slack_bus=slack)
    assert cpu.theta.device.type == 'cpu' and torch.equal(cpu.line_flow, a.line_flow[:4].cpu())


def test_mixed_batches_match_plain_calls():
    s = synth.solvable_contingency_grids(14, 120, range(20), seed=3, device=DEV, shuffle=True)
    buses, lines, gens, slack, _, _, outage = s
    lines = _perturbed(lines, 6)
    res = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack, mixed_topologies=True)
    n_isl = 0
    for j in outage.unique().tolist():
        idx = torch.nonzero(outage == j).flatten()
        try:
            plain = powerflow.dc_power_flow(buses[idx], lines[idx], gens[idx], slack_bus=slack)
        except powerflow.IslandedTopology:
            n_isl += 1
            assert not bool(res.converged[idx].any()) and bool((res.v[idx] == 1).all())
            assert bool(res.theta[idx].isnan().all()) and bool(res.line_flow[idx].isnan().all()) and bool(res.slack_p[idx].isnan().all())
            continue
        assert bool(plain.converged.all())
        for k in FIELDS:
            assert _same(getattr(res, k)[idx], getattr(plain, k)), (j, k)
    assert n_isl >= 1
    again = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack, mixed_topologies=True)
    for k in FIELDS:
        assert _same(getattr(again, k), getattr(res, k)), k
    ok = torch.nonzero(res.converged).flatten()[:6]
    sub = type(res)(*(getattr(res, k)[ok] for k in FIELDS))
    _check_against_reference(sub, (buses[ok], lines[ok], gens[ok], slack), 'case14 N-1')
    with pytest.raises(ValueError, match='dc_power_flow solves one topology'):
        powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    isl = torch.nonzero(~res.converged).flatten()[:3]
    none = powerflow.dc_power_flow(buses[isl], lines[isl], gens[isl], slack_bus=slack, mixed_topologies=True)
    assert not bool(none.converged.any()) and bool(none.theta.isnan().all()) and bool((none.v == 1).all())


def test_bad_grids_fail_alone():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 8, seed=4, device=DEV)
    lines[2, 3, 3] = float('nan')
    lines[5, 7, 3] = 0.0
    res = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    good = [0, 1, 3, 4, 6, 7]
    assert not bool(res.converged[[2, 5]].any()) and bool(res.converged[good].all())
    for k in OUTPUTS:
        assert bool(getattr(res, k)[[2, 5]].isnan().all()) and bool(torch.isfinite(getattr(res, k)[good]).all()), k
    assert bool((res.v == 1).all())
    alone = powerflow.dc_power_flow(buses[good], lines[good], gens[good], slack_bus=slack)
    for k in FIELDS:
        assert _same(getattr(res, k)[good], getattr(alone, k)), k


def _weights(bt, n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV) for shape in ((bt, n), (bt, e), (bt,)))


def _grads(buses, lines, gens, slack, weights, **kw):
    """(result, d(sum of the weighted outputs) / d(buses, lines, generators)); a weight that is None leaves its output out."""
    ins = [t.detach().clone().requires_grad_(True) for t in (buses, lines, gens)]
    res = powerflow.dc_power_flow(*ins, slack_bus=slack, **kw)
    loss = sum((w * getattr(res, k)).sum() for w, k in zip(weights, OUTPUTS) if w is not None)
    return res, torch.autograd.grad(loss, ins)


def _check_gradients(grads, buses, lines, gens, slack, weights, grids, name):
    for i in grids:
        want = dref.gradients(buses[i].cpu(), lines[i].cpu(), gens[i].cpu(), slack, *(None if w is None else w[i].cpu() for w in weights))
        for k, what in enumerate(NAMES):
            assert grads[k].dtype == torch.float32
            got, ref = grads[k][i].double().cpu().numpy(), want[k].numpy()
            for c in range(ref.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(got[:, c] == 0), (name, i, what, c)
                    continue
                err, scale = np.max(np.abs(got[:, c] - ref[:, c])), np.max(np.abs(ref[:, c]))
                print(f'{name}[{i}] d/d{what}[{c}]: err {err:.3e} scale {scale:.3e}')
                assert err <= 1e-5 * scale + 1e-7, (name, i, what, c, err, scale)


@pytest.mark.parametrize('case,batch', [(14, 16), (118, 6)])
def test_gradients_match_the_reference_autograd(case, batch):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=5, device=DEV)
    lines = _perturbed(lines, case)
    weights = _weights(batch, buses.shape[1], lines.shape[1], 1)
    res, grads = _grads(buses, lines, gens, slack, weights)
    assert bool(res.converged.all())
    _check_gradients(grads, buses, lines, gens, slack, weights, range(min(4, batch)), f'case{case}')
    # the forward is bit-identical with and without gradients
    plain = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    assert res.theta.grad_fn is not None and res.line_flow.grad_fn is not None and res.slack_p.grad_fn is not None
    assert not res.converged.requires_grad and not res.v.requires_grad
    for k in FIELDS:
        assert _same(getattr(plain, k), getattr(res, k).detach()), k
    # each incoming gradient alone
    for only in range(3):
        part = tuple(w if j == only else None for j, w in enumerate(weights))
        _, g = _grads(buses, lines, gens, slack, part)
        _check_gradients(g, buses, lines, gens, slack, part, range(2), f'case{case} only {OUTPUTS[only]}')
    # bit-identical alone and in another batch
    _, sub = _grads(buses[1:3], lines[1:3], gens[1:3], slack, tuple(w[1:3] for w in weights))
    for x, y in zip(sub, grads):
        assert torch.equal(x, y[1:3])
    # only the lines require grad
    li = lines.detach().clone().requires_grad_(True)
    r = powerflow.dc_power_flow(buses, li, gens, slack_bus=slack)
    (gl,) = torch.autograd.grad(sum((w * getattr(r, k)).sum() for w, k in zip(weights, OUTPUTS)), [li])
    assert torch.equal(gl, grads[1])


def test_mixed_gradients_one_classification_and_failed_grids():
    s = synth.solvable_contingency_grids(14, 40, range(20), seed=3, device=DEV, shuffle=True)
    buses, lines, gens, slack = s[:4]
    lines = _perturbed(lines, 8)
    weights = _weights(40, 14, lines.shape[1], 2)
    calls = []
    orig = gns_mod._classify_ids

    def counting(*args, **kw):
        calls.append(1)
        return orig(*args, **kw)

    gns_mod._classify_ids = counting
    try:
        res, grads = _grads(buses, lines, gens, slack, weights, mixed_topologies=True)
    finally:
        gns_mod._classify_ids = orig
    assert len(calls) == 1
    ok, isl = torch.nonzero(res.converged).flatten().tolist(), torch.nonzero(~res.converged).flatten()
    assert len(ok) >= 20 and isl.numel() >= 1
    _check_gradients(grads, buses, lines, gens, slack, weights, ok[:4], 'case14 N-1')
    for g in grads:
        assert bool(g[isl].isnan().all()) and bool(torch.isfinite(g[ok]).all())
    # per topology, the plain call gives the same bits
    outage = s[6]
    j = int(outage[ok[0]])
    idx = torch.nonzero(outage == j).flatten()
    _, plain = _grads(buses[idx], lines[idx], gens[idx], slack, tuple(w[idx] for w in weights))
    for g, h in zip(grads, plain):
        assert _same(g[idx], h)
    # zero incoming gradients give zero rows, solved or not; a batch whose grids all island gives NaN rows
    mask = torch.ones(40, dtype=torch.float64, device=DEV)
    mask[isl] = 0.0
    mask[ok[0]] = 0.0
    masked = tuple(w * (mask[:, None] if w.dim() == 2 else mask) for w in weights)
    _, gm = _grads(buses, lines, gens, slack, masked, mixed_topologies=True)
    for g, h in zip(gm, grads):
        assert bool((g[isl] == 0).all()) and bool((g[ok[0]] == 0).all()) and torch.equal(g[ok[1:]], h[ok[1:]])
    _, only = _grads(buses[isl], lines[isl], gens[isl], slack, tuple(w[isl] for w in weights), mixed_topologies=True)
    assert all(bool(g.isnan().all()) for g in only)
    # a plain call: a grid that fails gets NaN rows with a non-zero incoming gradient, zero rows with a zero one
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 6, seed=4, device=DEV)
    lines[2, 3, 3] = float('nan')
    weights = _weights(6, 30, lines.shape[1], 3)
    res, grads = _grads(buses, lines, gens, slack, weights)
    assert res.converged.tolist() == [True, True, False, True, True, True]
    for g in grads:
        assert bool(g[2].isnan().all()) and bool(torch.isfinite(g[[0, 1, 3, 4, 5]]).all())
    mask = torch.ones(6, dtype=torch.float64, device=DEV)
    mask[2] = 0.0
    _, gz = _grads(buses, lines, gens, slack, tuple(w * (mask[:, None] if w.dim() == 2 else mask) for w in weights))
    for g, h in zip(gz, grads):
        assert bool((g[2] == 0).all()) and torch.equal(g[[0, 1, 3, 4, 5]], h[[0, 1, 3, 4, 5]])


def test_the_fast_decoupled_analysis_is_reused():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 4, seed=11, device=DEV)
    powerflow.fast_decoupled(buses, lines, gens, slack_bus=slack, variant='XB')
    n_topo, n_nr = len(powerflow._FD_TOPO_CACHE), len(powerflow._TOPO_CACHE)
    res = powerflow.dc_power_flow(buses, lines, gens, slack_bus=slack)
    assert bool(res.converged.all())
    assert len(powerflow._FD_TOPO_CACHE) == n_topo and len(powerflow._TOPO_CACHE) == n_nr
    s = synth.solvable_contingency_grids(14, 30, range(6), seed=1, device=DEV, shuffle=True)
    powerflow.fast_decoupled(s[0], s[1], s[2], slack_bus=s[3], variant='BX', mixed_topologies=True)
    n_topo, n_set = len(powerflow._FD_TOPO_CACHE), len(powerflow._FD_SET_CACHE)
    powerflow.dc_power_flow(s[0], s[1], s[2], slack_bus=s[3], mixed_topologies=True)
    assert len(powerflow._FD_TOPO_CACHE) == n_topo and len(powerflow._FD_SET_CACHE) == n_set


def test_lds_refusal_names_dcs_image_and_larger_chains_than_fd_are_solved():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000)
    for kw in ({}, {'mixed_topologies': True}):
        with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
            powerflow.dc_power_flow(buses, lines, gens, slack_bus=tp.slack, **kw)
        assert str(want) in str(e.value) and 'nnz_lu_p + dim_p + N' in str(e.value), kw
    tp = pt.path(1500)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE):
        powerflow.fast_decoupled(buses, lines, gens, slack_bus=tp.slack, variant='XB')
    s = (buses, lines, gens, tp.slack)
    _check_against_reference(_dc(s), s, 'path1500')
    mixed = _dc(s, mixed_topologies=True)
    for k in FIELDS:
        assert _same(getattr(mixed, k), getattr(_dc(s), k)), k
