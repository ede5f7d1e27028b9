"""Gradients of the DC contingency screen on the MI355X (``powerflow.dc_contingency_screen(differentiable=True)``,
include/gns_powerflow.h "DC contingency screening", gradients): against the float64 autograd reference
(``dc_contingency_grad_reference``: the line removed, the smaller grid solved densely), against the product's other routes
(``dc_power_flow``'s adjoint for ``base.*``; the sum over copies of ``dc_power_flow(mixed_topologies=True)`` on the expanded
batch), the properties of the contract, bitwise reproducibility, per-row and per-grid failure and the LDS refusal.

The bar is the project's DC gradient bar per column per grid, as ``test_dcpf_gpu._check_gradients``: the outputs are float32, so
max|out - ref| <= 1e-5 max|ref| + 1e-7; every column outside the contract is exactly 0.  A loss reads the rows of ``~islanding``
only unless a test says otherwise, so islanding rows get an incoming gradient of exactly zero."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_contingency_grad_reference as gref
import pf_topologies as pt
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('buses', 'lines', 'generators')
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}
FAMILIES = ('random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8')


def _case(case, batch, seed):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    return buses, _perturbed(lines, case), gens, slack


def _weights(bt, k, e, seed, flow=True, worst=True):
    g = torch.Generator().manual_seed(seed)
    wf, ww = torch.randn(bt, k, e, generator=g, dtype=torch.float64).to(DEV), torch.randn(bt, k, generator=g, dtype=torch.float64).to(DEV)
    return (wf if flow else None, ww if worst else None)


def _rating(e, seed, bt=None):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 2.0 * torch.rand((e,) if bt is None else (bt, e), generator=g, dtype=torch.float64)).to(DEV)


def _loss(res, weights, rows=None):
    """sum of the weighted line_flow and worst_loading over the rows of ``rows`` (default: the outages that do not island)."""
    rows = ~res.islanding if rows is None else rows
    loss = 0.0
    if weights[0] is not None:
        loss = loss + (weights[0][..., rows, :] * res.line_flow[..., rows, :]).sum()
    if weights[1] is not None:
        loss = loss + (weights[1][..., rows] * res.worst_loading[..., rows]).sum()
    return loss


def _grads(s, weights, outages=None, rating=None, flows=True, req=(True, True, True), rows=None):
    """(result, gradients of the inputs that require grad) of the weighted loss through the differentiable screen."""
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip(s[:3], req)]
    res = powerflow.dc_contingency_screen(*ins, slack_bus=s[3], outages=outages, rating=rating, flows=flows, differentiable=True)
    return res, torch.autograd.grad(_loss(res, weights, rows), [t for t in ins if t.requires_grad])


def _check(grads, res, s, weights, rating, grids, name):
    buses, lines, gens = (t.cpu() for t in s[:3])
    outages = res.outages.tolist()
    worst = 0.0
    for i in grids:
        r = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu()
        want, flows = gref.gradients(buses[i], lines[i], gens[i], s[3], outages, *(None if w is None else w[i].cpu() for w in weights),
                                     rating=r)
        assert torch.equal(flows.isnan().all(dim=1), res.islanding.cpu()), (name, i)
        for k, what in enumerate(NAMES):
            assert grads[k].dtype == torch.float32 and grads[k].shape == s[k].shape
            got, ref = grads[k][i].double().cpu().numpy(), want[k].numpy()
            for c in range(ref.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(got[:, c] == 0), (name, i, what, c)
                    continue
                err, scale = np.max(np.abs(got[:, c] - ref[:, c])), np.max(np.abs(ref[:, c]))
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                print(f'{name}[{i}] d/d{what}[{c}]: err {err:.3e} scale {scale:.3e}')
                assert err <= 1e-5 * scale + 1e-7, (name, i, what, c, err, scale)
    print(f'{name}: worst error / bar {worst:.3f}')


def _equal(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def test_case14_every_outage_against_the_reference_autograd():
    s = _case(14, 16, seed=5)
    E = s[1].shape[1]
    weights = _weights(16, E, E, 1)
    for rating in (None, _rating(E, 2), _rating(E, 3, bt=16)):
        res, grads = _grads(s, weights, rating=rating)
        assert bool(res.converged.all()) and int(res.islanding.sum()) == 1
        assert res.line_flow.grad_fn is not None and res.worst_loading.grad_fn is not None
        assert not res.worst_line.requires_grad and not res.converged.requires_grad and not res.islanding.requires_grad
        _check(grads, res, s, weights, rating, range(16), f'case14 rating {None if rating is None else tuple(rating.shape)}')
    # the forward is bit-identical with and without gradients
    plain = powerflow.dc_contingency_screen(*s[:3], slack_bus=s[3], rating=rating)
    for k in ('line_flow', 'worst_loading', 'worst_line', 'islanding', 'converged', 'outages'):
        assert _same(getattr(plain, k), getattr(res, k).detach()), k
    for k in plain.base._fields:
        assert _same(getattr(plain.base, k), getattr(res.base, k).detach()), k
    # each incoming gradient alone; flows=False, where worst_loading alone has a gradient, gives those bits
    rating = _rating(E, 2)
    for flow, worst in ((True, False), (False, True)):
        part = _weights(16, E, E, 1, flow=flow, worst=worst)
        res, g = _grads(s, part, rating=rating)
        _check(g, res, s, part, rating, range(4), f'case14 flow={flow} worst={worst}')
    slim, gs = _grads(s, part, rating=rating, flows=False)
    assert slim.line_flow is None and _equal(gs, g) and _same(slim.worst_loading.detach(), res.worst_loading.detach())
    # only the lines requiring grad: the same bits as all three
    _, g_all = _grads(s, weights, rating=rating)
    for k in range(3):
        _, g_one = _grads(s, weights, rating=rating, req=tuple(j == k for j in range(3)))
        assert len(g_one) == 1 and _same(g_one[0], g_all[k]), NAMES[k]


def test_case118_every_outage_against_the_reference_autograd():
    s = _case(118, 6, seed=7)
    E = s[1].shape[1]
    weights, rating = _weights(6, E, E, 4), _rating(E, 5)
    res, grads = _grads(s, weights, rating=rating)
    assert bool(res.converged.all()) and int(res.islanding.sum()) == 20
    _check(grads, res, s, weights, rating, range(4), 'case118')
    res, grads = _grads(s, weights)
    _check(grads, res, s, weights, None, range(2), 'case118 no rating')


def test_case300_a_list_over_several_chunks_against_the_reference_autograd():
    """The adjoint takes 16 outages side by side at case300: 41 outages are three chunks, the last one short."""
    s = _case(300, 3, seed=300)
    E = s[1].shape[1]
    fd = powerflow._analysed(powerflow._FD, *powerflow._topology_key(*s, 'dc_contingency_screen'), torch.device(DEV))
    assert powerflow._dcn1_adjoint_lds_bytes(fd.host)[1] == 16
    outages = list(range(0, 410, 10))
    weights, rating = _weights(3, len(outages), E, 6), _rating(E, 7)
    res, grads = _grads(s, weights, outages=outages, rating=rating)
    assert bool(res.converged.all()) and 0 < int(res.islanding.sum()) < len(outages) - 17
    _check(grads, res, s, weights, rating, range(2), 'case300')


@pytest.mark.parametrize('name', FAMILIES)
def test_generated_families_against_the_reference_autograd(name):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E = tp.f.size
    weights, rating = _weights(2, E, E, len(name)), _rating(E, 8)
    res, grads = _grads(s, weights, rating=rating)
    _check(grads, res, s, weights, rating, range(2), name)


def test_base_gradients_are_dc_power_flows_bit_for_bit():
    s = _case(30, 5, seed=3)
    g = torch.Generator().manual_seed(9)
    wt, wf, ws = (torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV) for shape in ((5, 30), (5, s[1].shape[1]), (5,)))
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res = powerflow.dc_contingency_screen(*ins, slack_bus=s[3], outages=[0, 4], differentiable=True)
    got = torch.autograd.grad((wt * res.base.theta).sum() + (wf * res.base.line_flow).sum() + (ws * res.base.slack_p).sum(), ins)
    ins2 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    dc = powerflow.dc_power_flow(*ins2, slack_bus=s[3])
    want = torch.autograd.grad((wt * dc.theta).sum() + (wf * dc.line_flow).sum() + (ws * dc.slack_p).sum(), ins2)
    assert _equal(got, want) and not res.base.v.requires_grad
    # both parts in one loss: the sum of the two gradients, to float32 rounding of the sum
    weights = _weights(5, 2, s[1].shape[1], 10)
    ins3 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res3 = powerflow.dc_contingency_screen(*ins3, slack_bus=s[3], outages=[0, 4], differentiable=True)
    both = torch.autograd.grad(_loss(res3, weights) + (wt * res3.base.theta).sum(), ins3)
    _, screen_only = _grads(s, weights, outages=[0, 4])
    ins4 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    base_only = torch.autograd.grad((wt * powerflow.dc_power_flow(*ins4, slack_bus=s[3]).theta).sum(), ins4)
    for b, x, y in zip(both, screen_only, base_only):
        assert torch.equal(b, x + y)


def test_agrees_with_the_sum_over_copies_of_the_mixed_route():
    """The route the adjoint replaces: one grid per (grid, outage) with the line deleted, ``dc_power_flow(mixed_topologies=True)``
    with requires_grad, autograd summing over the copies."""
    bt = 4
    s = _case(14, bt, seed=8)
    E = s[1].shape[1]
    f, t, _ = synth.case_topology(14)
    outages = np.flatnonzero(~powerflow._bridges(14, f - 1, t - 1))
    K = outages.size
    weights, rating = _weights(bt, K, E, 11), _rating(E, 12)
    res, grads = _grads(s, weights, outages=outages.tolist(), rating=rating)
    assert not bool(res.islanding.any())
    ins = [x.detach().clone().requires_grad_(True) for x in s[:3]]
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device=DEV)                # [K, E-1]
    xl = ins[1][:, keep].reshape(bt * K, E - 1, 7)
    xb, xg = ins[0].repeat_interleave(K, dim=0), ins[2].repeat_interleave(K, dim=0)
    mixed = powerflow.dc_power_flow(xb, xl, xg, slack_bus=s[3], mixed_topologies=True)
    assert bool(mixed.converged.all())
    flow = mixed.line_flow.reshape(bt, K, E - 1)
    wf = torch.gather(weights[0], 2, keep.unsqueeze(0).expand(bt, K, E - 1))
    load = (flow.abs() / rating[keep].unsqueeze(0)).amax(dim=2)
    want = torch.autograd.grad((wf * flow).sum() + (weights[1] * load).sum(), ins)
    for k, what in enumerate(NAMES):
        for i in range(bt):
            for c in CONTRACT[what]:
                a, b = grads[k][i, :, c].double(), want[k][i, :, c].double()
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                print(f'mixed route [{i}] d/d{what}[{c}]: err {err:.3e} scale {scale:.3e}')
                # both sides are float32 results of float64 arithmetic: each is within the bar of the exact value
                assert err <= 1e-5 * scale + 1e-7, (what, i, c, err, scale)


def test_properties_of_the_contract():
    s = _case(30, 4, seed=6)
    E = s[1].shape[1]
    f, t, _ = synth.case_topology(30)
    free = np.flatnonzero(~powerflow._bridges(30, f - 1, t - 1))
    rating = _rating(E, 13)
    for k in free[[0, 7, -1]].tolist():
        # row k alone: exactly 0 in line k's own columns, whatever the weights
        w1 = _weights(4, 1, E, k)
        res, g1 = _grads(s, w1, outages=[k], rating=rating)
        assert bool((g1[1][:, k, :] == 0).all()) and bool((g1[1] != 0).any()) and bool(torch.isfinite(g1[1]).all())
        # a duplicated outage contributes twice (twice a float64 sum, rounded once: exactly twice the float32 value)
        w2 = tuple(torch.cat([w, w], dim=1) for w in w1)
        _, g2 = _grads(s, w2, outages=[k, k], rating=rating)
        for a, b in zip(g2, g1):
            assert torch.equal(a, 2 * b)
    # a row with a zero incoming gradient adds nothing: the list with the row, weights zero there, gives the bits without it
    ks = free[:5].tolist()
    w = _weights(4, 5, E, 14)
    w[0][:, 2] = 0
    w[1][:, 2] = 0
    _, ga = _grads(s, w, outages=ks, rating=rating)
    _, gb = _grads(s, tuple(x[:, [0, 1, 3, 4]] for x in w), outages=[ks[0], ks[1], ks[3], ks[4]], rating=rating)
    assert _equal(ga, gb)


def test_reproducible_bit_for_bit_and_other_input_forms():
    s = _case(118, 9, seed=9)
    buses, lines, gens, slack = s
    E = lines.shape[1]
    outages = list(range(0, E, 2)) + [5, 5]                            # 95 outages: two chunks
    weights, rating = _weights(9, len(outages), E, 15), _rating(E, 16)
    res, a = _grads(s, weights, outages=outages, rating=rating)
    _, b = _grads(s, weights, outages=outages, rating=rating)          # from run to run
    assert _equal(a, b) and all(bool(torch.isfinite(x).all()) for x in a)
    for sel in ([4], [2, 3, 4], [8, 0]):                               # alone and in a sub-batch
        sub = tuple(x[sel] for x in s[:3]) + (slack,)
        _, p = _grads(sub, tuple(w[sel] for w in weights), outages=outages, rating=rating)
        assert _equal(p, [x[sel] for x in a]), sel
    # a 2-D single grid
    ins = [x[4].detach().clone().requires_grad_(True) for x in s[:3]]
    one = powerflow.dc_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating, differentiable=True)
    assert one.line_flow.shape == (len(outages), E) and one.worst_loading.shape == (len(outages),)
    g = torch.autograd.grad(_loss(one, tuple(w[4] for w in weights)), ins)
    assert all(x.shape == y.shape for x, y in zip(g, ins)) and _equal(g, [x[4] for x in a])
    # CPU tensors in: CPU outputs, CPU gradients, the same bits
    ins = [x[:3].cpu().clone().requires_grad_(True) for x in s[:3]]
    cpu = powerflow.dc_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating.cpu(), differentiable=True)
    assert cpu.line_flow.device.type == 'cpu' and cpu.worst_loading.requires_grad
    g = torch.autograd.grad(_loss(cpu, tuple(w[:3].cpu() for w in weights)), ins)
    assert all(x.device.type == 'cpu' for x in g) and _equal(g, [x[:3].cpu() for x in a])
    # no grad asked for, or grad mode off: plain tensors
    with torch.no_grad():
        off = powerflow.dc_contingency_screen(*ins, slack_bus=slack, outages=[0], differentiable=True)
    assert not off.worst_loading.requires_grad and not off.base.theta.requires_grad
    off = powerflow.dc_contingency_screen(*s[:3], slack_bus=slack, outages=[0], differentiable=True)
    assert not off.worst_loading.requires_grad
    on = powerflow.dc_contingency_screen(lines=lines.clone().requires_grad_(True), buses=buses, generators=gens, slack_bus=slack,
                                         outages=[0])
    assert not on.worst_loading.requires_grad and not on.line_flow.requires_grad            # the default stays as it was


def test_islanding_rows_and_failure_per_grid():
    s = _case(30, 6, seed=4)
    E = s[1].shape[1]
    weights = _weights(6, E, E, 17)
    res, good = _grads(s, weights)
    isl = res.islanding
    assert int(isl.sum()) == 5 and all(bool(torch.isfinite(x).all()) for x in good)
    # a non-zero incoming gradient on an islanding row of grid 2 (the loss reads every row): NaN rows for that grid only
    everything = torch.ones_like(isl)
    wf, wl = weights[0].clone(), weights[1].clone()
    wf[:, isl] = 0
    wl[:, isl] = 0
    wl[2, int(torch.nonzero(isl)[0])] = 1.5
    _, g = _grads(s, (wf, wl), rows=everything)
    for x, y in zip(g, good):
        assert bool(x[2].isnan().all()) and _same(x[[0, 1, 3, 4, 5]], y[[0, 1, 3, 4, 5]])
    wl[2] = torch.where(isl, 0.0, wl[2])
    wf[4, int(torch.nonzero(isl)[-1]), 7] = -2.0
    _, g = _grads(s, (wf, wl), rows=everything)
    for x, y in zip(g, good):
        assert bool(x[4].isnan().all()) and _same(x[[0, 1, 2, 3, 5]], y[[0, 1, 2, 3, 5]])
    # weights that are exactly zero on the islanding rows, read through the NaN rows: as the indexed loss, bit for bit
    wf[4] = torch.where(isl.unsqueeze(1), 0.0, wf[4])
    _, g = _grads(s, (wf, wl), rows=everything)
    assert _equal(g, good)
    # a grid with a line that cannot be solved: converged False and NaN rows, the others unchanged bit for bit
    lines = s[1].clone()
    lines[3, 7, 3] = float('nan')
    bad = (s[0], lines, s[2], s[3])
    res, g = _grads(bad, weights)
    assert res.converged.tolist() == [True, True, True, False, True, True] and bool(res.worst_loading[3].isnan().all())
    for x, y in zip(g, good):
        assert bool(x[3].isnan().all()) and _same(x[[0, 1, 2, 4, 5]], y[[0, 1, 2, 4, 5]])
    zero = tuple(w.clone() for w in weights)
    zero[0][3] = 0
    zero[1][3] = 0
    res, g = _grads(bad, zero)
    for x, y in zip(g, good):
        assert bool((x[3] == 0).all()) and _same(x[[0, 1, 2, 4, 5]], y[[0, 1, 2, 4, 5]])


def test_lds_refusal_names_the_adjoints_image():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 2 * 5999 * 2 + 3)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_contingency_screen(buses, lines.requires_grad_(True), gens, slack_bus=tp.slack, outages=[0], differentiable=True)
    assert str(want) in str(e.value) and '2 dim_p (W + 1) + 3 W' in str(e.value)


def test_column_maps_route_the_gradients_back():
    """Inputs with permuted (and one more) columns and the maps B, L, G that name them, as ``dc_power_flow`` takes them: the
    gradients come back in the caller's columns, with the bits of the plain call; a column no map names gets 0."""
    s = _case(14, 3, seed=12)
    E = s[1].shape[1]
    weights, rating = _weights(3, E, E, 18), _rating(E, 19)
    _, want = _grads(s, weights, rating=rating)
    g = torch.Generator().manual_seed(20)
    perms = [torch.randperm(n + 1, generator=g) for n in (6, 7, 7)]                     # canonical column c sits at perms[k][c]
    wide = []
    for t, p in zip(s[:3], perms):
        x = torch.full((*t.shape[:2], t.shape[2] + 1), 7.5, device=DEV)
        x[..., p[:t.shape[2]].to(DEV)] = t
        wide.append(x.requires_grad_(True))
    maps = [{name: int(p[c]) for name, c in default.items()} for p, default in zip(perms, (gns_mod._B0, gns_mod._L0, gns_mod._G0))]
    assert all(sorted(d.values()) == list(range(n)) for d, n in zip((gns_mod._B0, gns_mod._L0, gns_mod._G0), (6, 7, 7)))
    res = powerflow.dc_contingency_screen(*wide, B=maps[0], L=maps[1], G=maps[2], slack_bus=s[3], rating=rating, differentiable=True)
    got = torch.autograd.grad(_loss(res, weights), wide)
    for x, y, p, n in zip(got, want, perms, (6, 7, 7)):
        assert x.shape[2] == n + 1 and _same(x[..., p[:n].to(DEV)], y) and bool((x[..., int(p[n])] == 0).all())
