"""Gradients of the AC contingency screen on the MI355X (``powerflow.ac_contingency_screen(differentiable=True)``,
include/gns_powerflow.h "AC contingency screening", gradients): against the float64 reference (``ac_contingency_grad_reference``:
the line's row deleted, the reference's own Newton from the base, autograd's dense Jacobian and the implicit function theorem),
against the product's other route (the sum over copies of ``newton_raphson(mixed_topologies=True)`` on the expanded batch), the
properties of the contract, bitwise reproducibility, per-row and per-grid failure and the LDS refusal.

The bar is the project's gradient bar per column per grid (test_powerflow_grad_gpu, test_dc_contingency_grad_gpu): the outputs are
float32, so max|out - ref| <= 1e-5 max|ref| + 1e-7; every column outside the contract is exactly 0.  A loss reads only the rows
where both the product and the reference converged (indexed, so every other row's incoming gradient is exactly zero); each test
asserts that those rows are enough of the pairs whose outage does not island the grid."""
import functools

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import ac_contingency_grad_reference as gref
import pf_topologies as pt

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('buses', 'lines', 'generators')
CONTRACT = gref.DIFF_COLS
OUT = gref.OUTPUTS
SUMMARIES = ('worst_loading', 'v_min', 'v_max')


@functools.lru_cache(maxsize=None)
def _case(case, batch, seed=0):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    return buses, lines, gens, slack


@functools.lru_cache(maxsize=None)
def _family(name, batch):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', batch, 0, device=DEV)
    return buses, lines, gens, tp.slack


@functools.lru_cache(maxsize=None)
def _ref_rows(key, outages):
    """The reference's rows of every grid of a cached case for a tuple of outages: solved once."""
    s = key[0](*key[1:])
    return [gref.solve_rows(s[0][i].cpu(), s[1][i].cpu(), s[2][i].cpu(), s[3], list(outages)) for i in range(s[0].shape[0])]


def _ref_mask(rows):
    return torch.tensor([[r is not None and r.converged for r in grid] for grid in rows], device=DEV)


def _weights(bt, k, n, e, seed, only=OUT):
    g = torch.Generator().manual_seed(seed)
    shapes = dict(v=(bt, k, n), theta=(bt, k, n), p_from=(bt, k, e), q_from=(bt, k, e), p_to=(bt, k, e), q_to=(bt, k, e),
                  worst_loading=(bt, k), v_min=(bt, k), v_max=(bt, k))
    w = {name: torch.randn(*shapes[name], generator=g, dtype=torch.float64).to(DEV) for name in OUT}       # the same draws for any `only`
    return {name: (w[name] if name in only else None) for name in OUT}


def _rating(e, seed, bt=None):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 2.0 * torch.rand((e,) if bt is None else (bt, e), generator=g, dtype=torch.float64)).to(DEV)


def _loss(res, w, mask):
    """The weighted sum of the outputs over the rows of ``mask`` (bool, the outputs' leading shape), by indexing."""
    loss = 0.0
    for name in OUT:
        out = getattr(res, name)
        if w[name] is not None and out is not None:
            loss = loss + (w[name].to(out.device)[mask.to(out.device)] * out[mask.to(out.device)]).sum()
    return loss


def _grads(s, w, mask=None, req=(True, True, True), **kw):
    """(result, the rows of the loss, gradients of the inputs that require grad).  ``mask``: None (the converged rows), a bool
    tensor that is and-ed with them, or a callable of the result."""
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip(s[:3], req)]
    res = powerflow.ac_contingency_screen(*ins, slack_bus=s[3], differentiable=True, **kw)
    rows = mask(res) if callable(mask) else res.converged if mask is None else res.converged & mask
    return res, rows, torch.autograd.grad(_loss(res, w, rows), [t for t in ins if t.requires_grad])


def _equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _check(grads, s, res, w, rows, refrows, rating, grids, name):
    """Every contract column of every grid of ``grids`` to the bar; returns the worst error / bar."""
    outages = res.outages.tolist()
    worst = (0.0, None)
    for i in grids:
        r = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu().numpy()
        want, cond = gref.gradients(s[0][i].cpu(), s[1][i].cpu(), s[2][i].cpu(), s[3], outages, refrows[i], rows[i].tolist(),
                                    {n: None if w[n] is None else w[n][i].cpu() for n in OUT}, r)
        for k, what in enumerate(NAMES):
            assert grads[k].dtype == torch.float32 and grads[k].shape == s[k].shape
            got = grads[k][i].double().cpu().numpy()
            for c in range(got.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(got[:, c] == 0), (name, i, what, c)
                    continue
                err, scale = np.max(np.abs(got[:, c] - want[k][:, c])), np.max(np.abs(want[k][:, c]))
                ratio = err / (1e-5 * scale + 1e-7)
                worst = max(worst, (ratio, (i, what, c)))
                print(f'{name}[{i}] d/d{what}[{c}]: err {err:.3e} scale {scale:.3e} ratio {ratio:.3f} (cond <= {cond:.1f})')
        print(f'{name}[{i}]: {int(rows[i].sum())} rows in the loss')
    print(f'{name}: worst error / bar {worst[0]:.3f} at {worst[1]}')
    assert worst[0] <= 1.0, (name, worst)
    return worst[0]


@pytest.mark.parametrize('rated', ['none', 'per_line', 'per_grid'])
def test_case14_every_line_against_the_reference(rated):
    s = _case(14, 3)
    E, N = 20, 14
    rating = {'none': None, 'per_line': _rating(E, 21), 'per_grid': _rating(E, 22, 3)}[rated]
    refrows = _ref_rows((_case, 14, 3), tuple(range(E)))
    w = _weights(3, E, N, E, 23)
    res, rows, grads = _grads(s, w, _ref_mask(refrows), rating=rating)
    n_pairs = 3 * int((~res.islanding).sum())
    print(f'case14 {rated}: {int(rows.sum())} of {n_pairs} non-bridge pairs in the loss')
    assert n_pairs == 57 and int(rows.sum()) >= 0.8 * n_pairs
    assert res.v.requires_grad and res.q_to.requires_grad and res.worst_loading.requires_grad and res.v_min.requires_grad
    assert not res.converged.requires_grad and not res.worst_line.requires_grad and not res.mismatch.requires_grad
    _check(grads, s, res, w, rows, refrows, rating, range(3), f'case14 {rated}')


@functools.lru_cache(maxsize=None)
def _case118_list():
    f, t, _ = synth.case_topology(118)
    bridges = powerflow._bridges(118, f - 1, t - 1)
    free = np.flatnonzero(~bridges)
    picked = free[::10][:14].tolist()
    return tuple([int(np.flatnonzero(bridges)[0])] + picked + [picked[1]])       # a bridge, fourteen lines, a duplicate: 16 chunks


def test_case118_a_list_with_a_bridge_and_a_duplicate_against_the_reference():
    s = _case(118, 1)
    outages = _case118_list()
    assert len(outages) == 16
    refrows = _ref_rows((_case, 118, 1), outages)
    w = _weights(1, 16, 118, s[1].shape[1], 24)
    rating = _rating(s[1].shape[1], 25)
    res, rows, grads = _grads(s, w, _ref_mask(refrows), outages=list(outages), rating=rating)
    n_pairs = int((~res.islanding).sum())
    print(f'case118: {int(rows.sum())} of {n_pairs} listed non-bridge pairs in the loss')
    assert bool(res.islanding[0]) and n_pairs == 15 and int(rows.sum()) >= 0.85 * n_pairs
    _check(grads, s, res, w, rows, refrows, rating, range(1), 'case118')


def test_generated_family_with_parallel_lines_and_a_self_loop_against_the_reference():
    name = 'random40_parallel_selfloop'
    s = _family(name, 2)
    E, N = s[1].shape[1], s[0].shape[1]
    refrows = _ref_rows((_family, name, 2), tuple(range(E)))
    w = _weights(2, E, N, E, 26)
    rating = _rating(E, 27)
    res, rows, grads = _grads(s, w, _ref_mask(refrows), rating=rating)
    n_pairs = 2 * int((~res.islanding).sum())
    print(f'{name}: {int(rows.sum())} of {n_pairs} non-bridge pairs in the loss')
    assert int(rows.sum()) >= 0.8 * n_pairs
    _check(grads, s, res, w, rows, refrows, rating, range(2), name)


def test_case300_a_list_over_several_chunks_three_rows_against_the_reference():
    s = _case(300, 1)
    outages = tuple(range(0, 411, 7))                                             # 59 outages: chunks of two rows
    plain = powerflow.ac_contingency_screen(*s[:3], slack_bus=s[3], outages=list(outages))
    cand = torch.nonzero(plain.converged[0]).flatten().tolist()
    pick = [cand[0], cand[len(cand) // 2], cand[-1]]                              # rows of three different chunks
    assert len({j // 2 for j in pick}) == 3
    bus, ln, gen = (t[0].cpu() for t in s[:3])
    part = gref.solve_rows(bus, ln, gen, s[3], [outages[j] for j in pick])
    refrows = [[part[pick.index(j)] if j in pick else None for j in range(len(outages))]]
    mask = _ref_mask(refrows)
    assert int(mask.sum()) == 3
    w = _weights(1, len(outages), 300, 411, 28)
    res, rows, grads = _grads(s, w, mask, outages=list(outages))
    assert int(rows.sum()) == 3
    _check(grads, s, res, w, rows, refrows, None, range(1), 'case300')
    # every converged row of the list: finite, and the same bits from run to run
    _, all_rows, a = _grads(s, w, outages=list(outages))
    _, _, b = _grads(s, w, outages=list(outages))
    assert int(all_rows.sum()) > 30 and _equal(a, b) and all(bool(torch.isfinite(x).all()) for x in a)


def test_each_incoming_gradient_alone_and_the_slim_calls():
    s = _case(14, 3)
    E, N = 20, 14
    refrows = _ref_rows((_case, 14, 3), tuple(range(E)))
    mask = _ref_mask(refrows)
    rating = _rating(E, 21)
    for name in OUT:
        w = _weights(3, E, N, E, 29, only=(name,))
        res, rows, grads = _grads(s, w, mask, rating=rating)
        _check(grads, s, res, w, rows, refrows, rating, [1], f'case14 {name} alone')
    # flows=False, states=False: the summaries' gradients with the same bits, the tensors not returned
    w = _weights(3, E, N, E, 30, only=SUMMARIES)
    _, _, full = _grads(s, w, mask, rating=rating)
    for kw in (dict(flows=False), dict(states=False), dict(flows=False, states=False)):
        res, _, slim = _grads(s, w, mask, rating=rating, **kw)
        assert _equal(slim, full), kw
        assert (res.v is None) == ('states' in kw) and (res.p_from is None) == ('flows' in kw)
    # a subset of the inputs requires grad: the bits of all three
    w = _weights(3, E, N, E, 23)
    _, _, full = _grads(s, w, mask, rating=rating)
    for req in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        _, _, part = _grads(s, w, mask, req=req, rating=rating)
        assert _equal(part, [g for g, r in zip(full, req) if r]), req


def test_base_gradients_are_newton_raphsons_and_the_forward_is_unchanged():
    s = _case(14, 3)
    g = torch.Generator().manual_seed(31)
    wv, wt = (torch.randn(3, 14, generator=g, dtype=torch.float64).to(DEV) for _ in range(2))
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res = powerflow.ac_contingency_screen(*ins, slack_bus=s[3], outages=[0, 4], differentiable=True)
    got = torch.autograd.grad((wv * res.base.v).sum() + (wt * res.base.theta).sum(), ins)
    ins2 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    nr = powerflow.newton_raphson(*ins2, slack_bus=s[3])
    want = torch.autograd.grad((wv * nr.v).sum() + (wt * nr.theta).sum(), ins2)
    assert _equal(got, want)
    # the forward: the same bits with and without gradients, in every field
    plain = powerflow.ac_contingency_screen(*s[:3], slack_bus=s[3])
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    diff = powerflow.ac_contingency_screen(*ins, slack_bus=s[3], differentiable=True)
    for k in powerflow.AcContingencyResult._fields[1:]:
        a, b = getattr(plain, k), getattr(diff, k).detach()
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int64 if a.element_size() == 8 else torch.int32),
                                                  b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int64 if b.element_size() == 8 else torch.int32)), k
    for a, b in zip(plain.base, diff.base):
        assert torch.equal(a, b.detach())
    # no grad asked for, or grad mode off, or the default: plain tensors
    with torch.no_grad():
        off = powerflow.ac_contingency_screen(*ins, slack_bus=s[3], outages=[0], differentiable=True)
    assert not off.worst_loading.requires_grad and not off.base.v.requires_grad
    off = powerflow.ac_contingency_screen(*s[:3], slack_bus=s[3], outages=[0], differentiable=True)
    assert not off.worst_loading.requires_grad
    on = powerflow.ac_contingency_screen(*ins, slack_bus=s[3], outages=[0])
    assert not on.worst_loading.requires_grad and not on.v.requires_grad and not on.base.v.requires_grad


def test_agrees_with_the_sum_over_copies_of_the_expanded_route():
    """The route the adjoint replaces: one grid per (grid, outage) with the line's row deleted, ``newton_raphson(mixed_topologies=True)``
    with requires_grad warm-started from the base, autograd summing over the copies.  The loss reads v and theta (what that route
    returns) on the rows both routes converged on."""
    s = _case(14, 3)
    E, N = 20, 14
    f, t, _ = synth.case_topology(14)
    outages = np.flatnonzero(~powerflow._bridges(14, f - 1, t - 1))
    K = outages.size
    w = _weights(3, K, N, E, 32, only=('v', 'theta'))
    res, rows, grads = _grads(s, w, outages=outages.tolist())
    ins = [x.detach().clone().requires_grad_(True) for x in s[:3]]
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device=DEV)                # [K, E-1]
    xl = ins[1][:, keep].reshape(3 * K, E - 1, 7)
    xb, xg = ins[0].repeat_interleave(K, dim=0), ins[2].repeat_interleave(K, dim=0)
    v0, th0 = res.base.v.detach().repeat_interleave(K, dim=0), res.base.theta.detach().repeat_interleave(K, dim=0)
    mixed = powerflow.newton_raphson(xb, xl, xg, slack_bus=s[3], mixed_topologies=True, v0=v0, theta0=th0)
    assert torch.equal(mixed.converged.reshape(3, K), res.converged) and int(rows.sum()) >= 0.8 * 57
    mv, mth = mixed.v.reshape(3, K, N), mixed.theta.reshape(3, K, N)
    want = torch.autograd.grad((w['v'][rows] * mv[rows]).sum() + (w['theta'][rows] * mth[rows]).sum(), ins)
    worst = 0.0
    for k, what in enumerate(NAMES):
        for i in range(3):
            for c in CONTRACT[what]:
                a, b = grads[k][i, :, c].double(), want[k][i, :, c].double()
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                # both sides are float32 results of float64 arithmetic: each is within the bar of the exact value
                assert err <= 1e-5 * scale + 1e-7, (what, i, c, err, scale)
    print(f'expanded route: worst error / bar {worst:.3f}')


def test_reproducible_bit_for_bit_and_other_input_forms():
    s = _case(14, 3)
    buses, lines, gens, slack = s
    E, N = 20, 14
    outages = list(range(E)) + [3, 3, 7] + list(range(0, E, 2))                   # 33 outages: chunks of two rows
    w, rating = _weights(3, len(outages), N, E, 33), _rating(E, 34)
    res, rows, a = _grads(s, w, outages=outages, rating=rating)
    _, _, b = _grads(s, w, outages=outages, rating=rating)                          # from run to run
    assert _equal(a, b) and all(bool(torch.isfinite(x).all()) for x in a)
    for sel in ([1], [2, 0]):                                                       # alone and in another batch
        sub = tuple(x[sel] for x in s[:3]) + (slack,)
        _, _, p = _grads(sub, {n: x[sel] for n, x in w.items()}, outages=outages, rating=rating)
        assert _equal(p, [x[sel] for x in a]), sel
    # a 2-D single grid
    ins = [x[1].detach().clone().requires_grad_(True) for x in s[:3]]
    one = powerflow.ac_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating, differentiable=True)
    assert one.v.shape == (len(outages), N) and one.worst_loading.shape == (len(outages),)
    g = torch.autograd.grad(_loss(one, {n: x[1] for n, x in w.items()}, one.converged), ins)
    assert all(x.shape == y.shape for x, y in zip(g, ins)) and _equal(g, [x[1] for x in a])
    # CPU tensors in: CPU outputs, CPU gradients, the same bits
    ins = [x.cpu().clone().requires_grad_(True) for x in s[:3]]
    cpu = powerflow.ac_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating.cpu(), differentiable=True)
    assert cpu.v.device.type == 'cpu' and cpu.worst_loading.requires_grad
    g = torch.autograd.grad(_loss(cpu, w, cpu.converged), ins)
    assert all(x.device.type == 'cpu' for x in g) and _equal(g, [x.cpu() for x in a])
    # column maps: the gradients come back in the caller's columns with the bits of the plain call; an unnamed column gets 0
    gen = torch.Generator().manual_seed(35)
    perms = [torch.randperm(n + 1, generator=gen) for n in (6, 7, 7)]
    wide = []
    for t, p in zip(s[:3], perms):
        x = torch.full((*t.shape[:2], t.shape[2] + 1), 7.5, device=DEV)
        x[..., p[:t.shape[2]].to(DEV)] = t
        wide.append(x.requires_grad_(True))
    maps = [{name: int(p[c]) for name, c in default.items()} for p, default in zip(perms, (gns_mod._B0, gns_mod._L0, gns_mod._G0))]
    mapped = powerflow.ac_contingency_screen(*wide, B=maps[0], L=maps[1], G=maps[2], slack_bus=slack, outages=outages, rating=rating,
                                             differentiable=True)
    got = torch.autograd.grad(_loss(mapped, w, mapped.converged), wide)
    for x, y, p, n in zip(got, a, perms, (6, 7, 7)):
        assert x.shape[2] == n + 1 and _equal([x[..., p[:n].to(DEV)].contiguous()], [y]) and bool((x[..., int(p[n])] == 0).all())


def test_properties_of_the_contract_and_failure_per_row_and_per_grid():
    s = _case(14, 3)
    E, N = 20, 14
    w = _weights(3, E, N, E, 36)
    res, rows, good = _grads(s, w)
    assert all(bool(torch.isfinite(x).all()) for x in good)
    conv, isl = res.converged, res.islanding
    # row k alone: exactly 0 in line k's own columns; a duplicated outage contributes exactly twice
    for k in (0, 9, 19):
        assert bool(conv[:, k].all())
        w1 = {n: x[:, [k]] for n, x in w.items()}
        _, _, g1 = _grads(s, w1, outages=[k])
        assert bool((g1[1][:, k, :] == 0).all()) and bool((g1[1] != 0).any()) and bool(torch.isfinite(g1[1]).all())
        _, _, g2 = _grads(s, {n: torch.cat([x, x], dim=1) for n, x in w1.items()}, outages=[k, k])
        for a, b in zip(g2, g1):
            assert torch.equal(a, 2 * b)
    # islanding and non-converged rows masked by indexing contribute nothing: the list without them gives the same bits when the
    # chunks are the same (a wave per row up to 32 outages)
    stopped = ~conv & ~isl.unsqueeze(0)
    assert int(isl.sum()) == 1 and bool(stopped.any())
    keep = torch.nonzero(conv.all(dim=0)).flatten().tolist()
    _, _, part = _grads(s, {n: x[:, keep] for n, x in w.items()}, outages=keep)
    _, _, same = _grads(s, w, mask=conv.all(dim=0).unsqueeze(0).expand(3, E))
    assert _equal(part, same)
    # zero weights on those rows, the loss reading every row's finite outputs: still skipped (never multiplied by zero)
    everything = lambda r: torch.ones_like(r.converged)                            # noqa: E731
    wz = {n: torch.where(conv.reshape(3, E, *[1] * (x.dim() - 2)), x, torch.zeros_like(x)) for n, x in w.items()}
    wz_sum = {n: (x if n in SUMMARIES[1:] else None) for n, x in wz.items()}       # v_min, v_max: finite wherever a row was iterated
    _, _, a = _grads(s, wz_sum, mask=lambda r: ~r.islanding.unsqueeze(0).expand(3, E))
    _, _, b = _grads(s, wz_sum)
    assert _equal(a, b)
    # a non-zero cotangent into a non-converged row: NaN rows for that grid, the others bit for bit
    gi, ji = (int(x) for x in torch.nonzero(stopped)[0])
    _, _, bad = _grads(s, w, mask=lambda r: r.converged | (torch.arange(3, device=DEV).unsqueeze(1) == gi) & (torch.arange(E, device=DEV) == ji))
    others = [i for i in range(3) if i != gi]
    for x, y in zip(bad, good):
        assert bool(x[gi].isnan().all()) and _equal([x[others]], [y[others]])
    # ... and into an islanding row (NaN outputs, a weight on v_max alone)
    jb = int(torch.nonzero(isl)[0])
    wi = dict(w)
    _, _, bad = _grads(s, wi, mask=lambda r: r.converged | (torch.arange(3, device=DEV).unsqueeze(1) == 2) & (torch.arange(E, device=DEV) == jb))
    for x, y in zip(bad, good):
        assert bool(x[2].isnan().all()) and _equal([x[[0, 1]]], [y[[0, 1]]])
    # a grid without a base solution: NaN rows with a non-zero incoming gradient, zero rows without; the others bit for bit
    buses = s[0].clone()
    buses[1, :, 2:4] *= 40.0                                                       # loads no network of this size can serve
    sb = (buses, s[1], s[2], s[3])
    res_b, _, g = _grads(sb, w, mask=everything)
    assert res_b.base.converged.tolist() == [True, False, True] and not bool(res_b.converged[1].any())
    for x, y in zip(g, good):
        assert bool(x[1].isnan().all())
    _, _, g0 = _grads(sb, w)                                                       # the converged rows: none of grid 1
    for x, y in zip(g0, good):
        assert bool((x[1] == 0).all()) and _equal([x[[0, 2]]], [y[[0, 2]]])


def test_a_tie_in_the_worst_loading_follows_worst_line():
    """Two identical lines between the same buses in the same direction have bit-identical flows: with the lowest rating they tie
    for the worst loading, worst_line is the lower of them, and the whole gradient of worst_loading is that of that line's loading."""
    tp = pt.Topo('ring5_twin', 5, np.array([1, 2, 3, 4, 5, 1]), np.array([2, 3, 4, 5, 1, 2]), np.array([1, 3]), 1)
    buses, lines, gens, v, theta = pt.grids(tp, 'reference', 2, 0, device=DEV)
    lines = lines.clone()
    lines[:, 5, 2:] = lines[:, 0, 2:]
    buses, gens = synth.manufacture_solution(buses, lines, gens, tp.slack, v, theta)     # solvable again with the twin
    s = (buses, lines, gens, tp.slack)
    rating = torch.tensor([0.05, 1.0, 1.0, 1.0, 1.0, 0.05], dtype=torch.float64, device=DEV)
    outages = [2, 3]
    w = _weights(2, 2, 5, 6, 37, only=('worst_loading',))
    res, rows, got = _grads(s, w, outages=outages, rating=rating)
    assert int(rows.sum()) >= 2 and bool((res.worst_line[rows] == 0).all())           # the loss reads the converged rows
    assert torch.equal(res.p_from[..., 0], res.p_from[..., 5]) and torch.equal(res.q_to[..., 0], res.q_to[..., 5])
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    r2 = powerflow.ac_contingency_screen(*ins, slack_bus=tp.slack, outages=outages, rating=rating, differentiable=True)
    sf = torch.sqrt(r2.p_from[..., 0] ** 2 + r2.q_from[..., 0] ** 2)
    st = torch.sqrt(r2.p_to[..., 0] ** 2 + r2.q_to[..., 0] ** 2)
    want = torch.autograd.grad((w['worst_loading'] * torch.where(sf >= st, sf, st) / rating[0])[rows].sum(), ins)
    for k, what in enumerate(NAMES):
        for c in CONTRACT[what]:
            a, b = got[k][..., c].double(), want[k][..., c].double()
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            assert err <= 1e-5 * scale + 1e-7, (what, c, err, scale)
    # line 0's own r gets the direct term, its twin's does not: they differ although the lines are identical
    assert bool((got[1][:, 0, 2] != got[1][:, 5, 2]).all())


def test_an_oversize_image_is_refused_by_name_before_any_launch(monkeypatch):
    tp = pt.path(4096)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 1, 0, device=DEV)
    launched = []
    monkeypatch.setattr(powerflow, '_solve', lambda *a, **k: launched.append('solve'))
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.ac_contingency_screen(buses, lines.requires_grad_(True), gens, slack_bus=tp.slack, outages=[0], differentiable=True)
    assert 'gns_acn1_adjoint_workspace_bytes' in str(e.value) and 'nnz(L+U) + dim + 8 N' in str(e.value) and not launched
