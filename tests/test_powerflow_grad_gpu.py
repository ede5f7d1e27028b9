"""Gradients through the Newton-Raphson power flow on the MI355X (``gns_pf_adjoint`` / ``gns_pf_adjoint_set`` behind
``powerflow.newton_raphson``): the float64 implicit-gradient oracle, structural zeros, per-grid failure and masked losses,
bitwise reproducibility, mixed N-1 sets, column maps / single grids / CPU inputs, unchanged forward outputs and the raw C-ABI."""
import ctypes

import numpy as np
import pytest
import torch

import opf_graph_neural_solver_amd as amd
from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig
import nr_grad_reference as gref
from test_powerflow_gpu import _sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('buses', 'lines', 'generators')


@pytest.fixture(scope='module')
def grid_sets():
    return _sets()


def _loss_weights(bt, n, seed, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(bt, n, generator=g, dtype=torch.float64).to(dev), torch.randn(bt, n, generator=g, dtype=torch.float64).to(dev))


def _grads(buses, lines, gens, slack, a, b, **kw):
    """(result, d(sum(a v + b theta))/d(buses, lines, generators))."""
    ins = [t.detach().clone().requires_grad_(True) for t in (buses, lines, gens)]
    res = powerflow.newton_raphson(*ins, slack_bus=slack, **kw)
    return res, torch.autograd.grad((a * res.v + b * res.theta).sum(), ins)


def _same(a, b):
    """Bit-identical, NaN included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0.0, a), torch.where(b.isnan(), 0.0, b))


def test_gradients_match_the_float64_oracle(grid_sets):
    for name, s in grid_sets.items():
        buses, lines, gens, slack = s[:4]
        a, b = _loss_weights(buses.shape[0], buses.shape[1], 1)
        res, grads = _grads(buses, lines, gens, slack, a, b)
        assert bool(res.converged.all()), name
        for i in range(min(3, buses.shape[0])):
            want = gref.implicit_gradient(buses[i].double().cpu(), lines[i].double().cpu(), gens[i].double().cpu(), slack,
                                          res.v[i].cpu(), res.theta[i].cpu(), a[i].cpu(), b[i].cpu())
            for k in range(3):
                got = grads[k][i].double().cpu().numpy()
                assert grads[k].dtype == torch.float32
                err, scale = np.max(np.abs(got - want[k])), np.max(np.abs(want[k]))
                assert err <= 1e-5 * scale + 1e-7, (name, i, NAMES[k], err, scale)


def test_structural_zeros(grid_sets):
    for name, s in grid_sets.items():
        buses, lines, gens, slack = s[:4]
        a, b = _loss_weights(buses.shape[0], buses.shape[1], 2)
        _, (gb, gl, gg) = _grads(buses, lines, gens, slack, a, b)
        gbus = gens[0, :, 0].long().cpu().numpy() - 1
        n = buses.shape[1]
        is_gen = np.zeros(n, dtype=bool)
        is_gen[gbus] = True
        assert bool((gb[..., 0:2] == 0).all()) and bool((gb[:, slack - 1, :] == 0).all()), name
        pv = torch.as_tensor(is_gen, device=DEV)
        pv[slack - 1] = False
        assert bool((gb[:, pv][..., [3, 5]] == 0).all()), name            # Qd, Bs at PV buses
        assert bool((gl[..., 0:2] == 0).all()), name
        assert bool((gg[..., [0, 1, 2, 3, 5]] == 0).all()), name
        first = {}
        for j, bb in enumerate(gbus.tolist()):
            first.setdefault(bb, j)
        not_first = [j for j in range(gbus.size) if first[gbus[j]] != j]
        if name == 'case14_dupgen':
            assert not_first
        if not_first:
            assert bool((gg[:, not_first, 4] == 0).all()), name
        at_slack = [j for j in range(gbus.size) if gbus[j] == slack - 1]
        assert bool((gg[:, at_slack, 6] == 0).all()), name
        assert bool(gg[:, first[slack - 1], 4].ne(0).any()), name        # the slack's vg does move the loss


def test_bad_grids_give_nan_rows_and_zero_gradients_give_zero_rows():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 8, seed=4, device=DEV)
    lines[2, 3, 2] = float('nan')               # test_bad_grids_fail_alone's recipe
    lines[4, 5, 2] = 0.0
    lines[4, 5, 3] = 0.0
    buses[6, :, 2:4] *= 100.0
    bad, good = [2, 4, 6], [0, 1, 3, 5, 7]
    a, b = _loss_weights(8, 30, 3)
    res, grads = _grads(buses, lines, gens, slack, a, b)
    assert not bool(res.converged[bad].any()) and bool(res.converged[good].all())
    for g in grads:
        assert bool(g[bad].isnan().all())
        assert bool(torch.isfinite(g[good]).all())
    _, alone = _grads(buses[good], lines[good], gens[good], slack, a[good], b[good])
    for g, h in zip(grads, alone):
        assert torch.equal(g[good], h)
    # a masked loss: zero incoming gradient rows give zero rows, converged or not
    mask = torch.ones(8, 1, dtype=torch.float64, device=DEV)
    mask[[1, 2, 4]] = 0.0
    _, masked = _grads(buses, lines, gens, slack, a * mask, b * mask)
    for g, h in zip(masked, grads):
        assert bool((g[[1, 2, 4]] == 0).all())
        assert bool(g[6].isnan().all())
        assert torch.equal(g[[0, 3, 5, 7]], h[[0, 3, 5, 7]])
    # only theta in the loss, only v in the loss
    for wa, wb in ((a * 0, b), (a, b * 0)):
        _, part = _grads(buses[good], lines[good], gens[good], slack, wa[good], wb[good])
        assert all(bool(torch.isfinite(g).all()) for g in part)


def test_bitwise_reproducible_alone_and_in_any_batch():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 130, seed=9, device=DEV)
    a, b = _loss_weights(130, 118, 4)
    _, g1 = _grads(buses, lines, gens, slack, a, b)
    _, g2 = _grads(buses, lines, gens, slack, a, b)
    for x, y in zip(g1, g2):
        assert torch.equal(x, y)
    for bt in (1, 63, 65):
        _, p = _grads(buses[:bt], lines[:bt], gens[:bt], slack, a[:bt], b[:bt])
        for x, y in zip(p, g1):
            assert torch.equal(x, y[:bt])
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(0)).to(DEV)
    _, q = _grads(buses[perm], lines[perm], gens[perm], slack, a[perm], b[perm])
    for x, y in zip(q, g1):
        assert torch.equal(x, y[perm])
    for i in (0, 77):
        _, one = _grads(buses[i], lines[i], gens[i], slack, a[i], b[i])
        for x, y in zip(one, g1):
            assert torch.equal(x, y[i])


def test_mixed_set_matches_per_topology_plain_calls():
    buses, lines, gens, slack, _, _, outage = synth.solvable_contingency_grids(14, 120, range(20), seed=3, device=DEV, shuffle=True)
    a, b = _loss_weights(120, 14, 5)
    res, grads = _grads(buses, lines, gens, slack, a, b, mixed_topologies=True)
    n_isl = 0
    for j in outage.unique().tolist():
        idx = torch.nonzero(outage == j).flatten()
        if bool((res.iterations[idx] == -1).all()):            # an islanding outage: not solved, NaN rows
            n_isl += 1
            for g in grads:
                assert bool(g[idx].isnan().all())
            continue
        _, plain = _grads(buses[idx], lines[idx], gens[idx], slack, a[idx], b[idx])
        for g, h in zip(grads, plain):
            assert _same(g[idx], h), j
    assert n_isl > 0
    # the same grids by the oracle for two of them
    ok = torch.nonzero(res.converged).flatten()[:2].tolist()
    for i in ok:
        want = gref.implicit_gradient(buses[i].double().cpu(), lines[i].double().cpu(), gens[i].double().cpu(), slack,
                                      res.v[i].cpu(), res.theta[i].cpu(), a[i].cpu(), b[i].cpu())
        for k in range(3):
            err, scale = np.max(np.abs(grads[k][i].double().cpu().numpy() - want[k])), np.max(np.abs(want[k]))
            assert err <= 1e-5 * scale + 1e-7, (i, NAMES[k], err, scale)
    # a masked loss zeroes the rows of islanded grids too; a batch whose grids all island gives NaN rows
    _, zero = _grads(buses, lines, gens, slack, a * 0, b * 0, mixed_topologies=True)
    assert all(bool((g == 0).all()) for g in zero)
    isl = torch.nonzero(res.iterations == -1).flatten()[:3]
    _, only = _grads(buses[isl], lines[isl], gens[isl], slack, a[isl], b[isl], mixed_topologies=True)
    assert all(bool(g.isnan().all()) for g in only)


def test_column_maps_single_grids_and_cpu_inputs():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 6, seed=8, device=DEV)
    a, b = _loss_weights(6, 14, 6)
    _, ref_g = _grads(buses, lines, gens, slack, a, b)
    B0, L0, G0 = amd.get_BLG()
    pb, pl, pg = [5, 0, 3, 1, 4, 2], [6, 2, 0, 5, 1, 4, 3], [3, 6, 0, 4, 1, 5, 2]   # stored column c holds canonical pb[c]

    def cols(m, perm):
        inv = {canon: stored for stored, canon in enumerate(perm)}
        return {k: inv[v] for k, v in m.items()}

    ins = [t[..., p].detach().clone().requires_grad_(True) for t, p in zip((buses, lines, gens), (pb, pl, pg))]
    res = powerflow.newton_raphson(*ins, cols(B0, pb), cols(L0, pl), cols(G0, pg), slack_bus=slack)
    got = torch.autograd.grad((a * res.v + b * res.theta).sum(), ins)
    for g, h, p in zip(got, ref_g, (pb, pl, pg)):
        assert torch.equal(g, h[..., p])
    one = [t[2].detach().clone().requires_grad_(True) for t in (buses, lines, gens)]
    r1 = powerflow.newton_raphson(*one, slack_bus=slack)
    g1 = torch.autograd.grad((a[2] * r1.v + b[2] * r1.theta).sum(), one)
    for g, h in zip(g1, ref_g):
        assert g.shape == h[2].shape and torch.equal(g, h[2])
    cpu = [t.detach().cpu().requires_grad_(True) for t in (buses, lines, gens)]
    rc = powerflow.newton_raphson(*cpu, slack_bus=slack)
    assert rc.v.device.type == 'cpu'
    gc = torch.autograd.grad((a.cpu() * rc.v + b.cpu() * rc.theta).sum(), cpu)
    for g, h in zip(gc, ref_g):
        assert g.device.type == 'cpu' and torch.equal(g, h.cpu())
    # only the generators require grad: the others get none
    gen_only = gens.detach().clone().requires_grad_(True)
    rg = powerflow.newton_raphson(buses, lines, gen_only, slack_bus=slack)
    (gg,) = torch.autograd.grad((a * rg.v + b * rg.theta).sum(), [gen_only])
    assert torch.equal(gg, ref_g[2])


def test_forward_outputs_do_not_depend_on_requires_grad(grid_sets):
    for name, s in grid_sets.items():
        buses, lines, gens, slack = s[:4]
        plain = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
        ins = [t.detach().clone().requires_grad_(True) for t in (buses, lines, gens)]
        tracked = powerflow.newton_raphson(*ins, slack_bus=slack)
        assert tracked.v.grad_fn is not None and tracked.theta.grad_fn is not None
        assert not tracked.converged.requires_grad and not tracked.iterations.requires_grad and not tracked.mismatch.requires_grad
        for k in plain._fields:
            assert torch.equal(getattr(plain, k), getattr(tracked, k).detach()), (name, k)
        with torch.no_grad():
            off = powerflow.newton_raphson(*ins, slack_bus=slack)
        assert off.v.grad_fn is None and torch.equal(off.v, plain.v)


def test_c_abi_errors_and_poisoned_workspace():
    buses, lines, gens, slack, _, _ = synth.solvable_grids(30, 70, seed=8, device=DEV)
    a, b = _loss_weights(70, 30, 7)
    _, want = _grads(buses, lines, gens, slack, a, b)
    old = gns_mod.POISON_WORKSPACES
    gns_mod.POISON_WORKSPACES = True
    try:
        _, poisoned = _grads(buses, lines, gens, slack, a, b)
    finally:
        gns_mod.POISON_WORKSPACES = old
    for x, y in zip(want, poisoned):
        assert torch.equal(x, y)
    lib = amd.load_library()
    res = powerflow.newton_raphson(buses, lines, gens, slack_bus=slack)
    topo = powerflow._topology(buses, lines, gens, slack)
    Bt, N = buses.shape[0], buses.shape[1]
    cfg = PfConfig(N, lines.shape[1], gens.shape[1], 10, 1e-8)
    need = ctypes.c_size_t()
    assert lib.gns_pf_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=DEV)
    outs = [torch.full_like(t, float('nan')) for t in (buses, lines, gens)]
    conv = res.converged.to(torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes=need.value, buses_p=buses.data_ptr(), v_p=res.v.data_ptr(), conv_p=conv.data_ptr(), cfg_=cfg):
        return lib.gns_pf_adjoint(ctypes.byref(cfg_), topo.host.ctypes.data, topo.blob.data_ptr(), buses_p, lines.data_ptr(),
                                  gens.data_ptr(), Bt, v_p, res.theta.data_ptr(), conv_p, a.data_ptr(), b.data_ptr(),
                                  outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert call(ws_bytes=need.value - 1) == 4                 # GNS_ESIZE
    assert call(buses_p=None) == 1                            # GNS_EINVAL
    assert call(v_p=None) == 1
    assert call(conv_p=None) == 1
    assert call(cfg_=PfConfig(N + 1, lines.shape[1], gens.shape[1], 10, 1e-8)) == 1
    assert call() == 0
    torch.cuda.synchronize()
    for x, y in zip(outs, want):                              # every element written, over NaN-filled outputs
        assert torch.equal(x, y)
    # the set entry on a one-member set: the same bits
    plan = powerflow._plan_mixed(buses, lines, gens, slack)
    ts = plan.topo_set
    need_s = ctypes.c_size_t()
    m = plan.member_off
    assert lib.gns_pf_workspace_bytes_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.words, m.ctypes.data, m.size, Bt,
                                          ctypes.byref(need_s)) == 0
    ws_s = torch.full((need_s.value,), 0xFF, dtype=torch.uint8, device=DEV)
    outs_s = [torch.full_like(t, float('nan')) for t in (buses, lines, gens)]

    def call_set(ws_bytes=need_s.value, grid_off=plan.grid_off.data_ptr()):
        return lib.gns_pf_adjoint_set(ctypes.byref(cfg), ts.host.ctypes.data, ts.blob.data_ptr(), ts.words, m.ctypes.data, m.size,
                                      grid_off, None, buses.data_ptr(), lines.data_ptr(), gens.data_ptr(), Bt, res.v.data_ptr(),
                                      res.theta.data_ptr(), conv.data_ptr(), a.data_ptr(), b.data_ptr(), outs_s[0].data_ptr(),
                                      outs_s[1].data_ptr(), outs_s[2].data_ptr(), ws_s.data_ptr(), ws_bytes, stream)

    assert call_set(ws_bytes=need_s.value - 1) == 4
    assert call_set(grid_off=None) == 1
    assert call_set() == 0
    torch.cuda.synchronize()
    for x, y in zip(outs_s, want):
        assert torch.equal(x, y)
