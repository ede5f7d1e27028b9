"""Gradients of the DC N-2 contingency screen on the MI355X (``powerflow.dc_n2_contingency_screen(differentiable=True)``,
include/gns_powerflow.h "DC N-2 contingency screening", gradients): against the float64 autograd reference
(``dc_n2_grad_reference``: both lines removed, the smaller grid solved densely), against the product's other routes
(``dc_power_flow``'s adjoint for ``base.*``; the sum over copies of ``dc_power_flow(mixed_topologies=True)`` on the expanded batch),
the properties of the contract, bitwise reproducibility, per-row and per-grid failure and the LDS refusal.

The bar is the project's DC gradient bar per contract column per grid, as ``test_dc_contingency_grad_gpu._check`` applies it: the
outputs are float32, so max|out - ref| <= 1e-5 max|ref| + 1e-7; every column outside the contract is exactly 0.  A loss reads the
rows of ``~islanding`` only unless a test says otherwise, so islanding rows get an incoming gradient of exactly zero.

Generated families (``dc_n2_grad_cases.FAMILIES``, two 'reference' grids with ``_perturbed`` lines, the at most 120 non-islanding
pairs of ``family_pairs``): a family is held to the bar only if the reference's two float64 methods (``method='remove'`` and
``method='rank2'``) agree per contract column to 1e-8 max|ref| + 1e-10 on those pairs on the CPU.  Worst difference / that bar and
smallest |det| of a 2x2 system, both outputs in the loss and a rating:
  random40_parallel_selfloop 1.6e-6, 7.0e-3 (with the parallel pair (0, 59) and the self-loop pair (62, 0));
  random24_stacked_gens 1.6e-6, 1.7e-2 (with the parallel pair (4, 35));  ring30_slack_no_gen 4.8e-2, 9.8e-5;
  lattice8x8 4.0e-6, 1.6e-2.
No family failed the probe; none is dropped.

``test_row_jk_gives_zeros_to_its_own_lines`` asks for exact zeros as the contract states them: a pair alone, and two pairs that
share a line (that line alone is held by every row)."""
import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import dc_n2_grad_reference as gref
from dc_n2_grad_cases import FAMILIES, case300_pairs, family_pairs, special_pairs
import pf_topologies as pt
from test_dcpf_gpu import _perturbed, _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('buses', 'lines', 'generators')
CONTRACT = {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}


def _case(case, batch, seed):
    buses, lines, gens, slack, _, _ = synth.solvable_grids(case, batch, seed=seed, device=DEV)
    return buses, _perturbed(lines, case), gens, slack


def _weights(bt, p, e, seed, flow=True, worst=True):
    g = torch.Generator().manual_seed(seed)
    wf, ww = torch.randn(bt, p, e, generator=g, dtype=torch.float64).to(DEV), torch.randn(bt, p, generator=g, dtype=torch.float64).to(DEV)
    return (wf if flow else None, ww if worst else None)


def _rating(e, seed, bt=None):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + 2.0 * torch.rand((e,) if bt is None else (bt, e), generator=g, dtype=torch.float64)).to(DEV)


def _loss(res, weights, rows=None):
    """sum of the weighted line_flow and worst_loading over the rows of ``rows`` (default: the pairs that do not island)."""
    rows = ~res.islanding if rows is None else rows
    loss = 0.0
    if weights[0] is not None:
        loss = loss + (weights[0][..., rows, :] * res.line_flow[..., rows, :]).sum()
    if weights[1] is not None:
        loss = loss + (weights[1][..., rows] * res.worst_loading[..., rows]).sum()
    return loss


def _grads(s, weights, pairs=None, rating=None, flows=True, req=(True, True, True), rows=None):
    """(result, gradients of the inputs that require grad) of the weighted loss through the differentiable screen."""
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip(s[:3], req)]
    res = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=pairs, rating=rating, flows=flows, differentiable=True)
    return res, torch.autograd.grad(_loss(res, weights, rows), [t for t in ins if t.requires_grad])


def _reference(s, pairs, weights, rating, grids, rows=None):
    """The reference gradients of the grids, on the rows of ``rows`` (positions in ``pairs``; default all, islanding ones skipped)."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    rows = list(range(len(pairs))) if rows is None else rows
    out = {}
    for i in grids:
        r = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu()
        out[i] = gref.gradients(buses[i], lines[i], gens[i], s[3], [pairs[p] for p in rows],
                                *(None if w is None else w[i].cpu()[rows] for w in weights), rating=r)
    return out


def _check(grads, s, want, name):
    worst = 0.0
    for i, (ref_grads, _) in want.items():
        for k, what in enumerate(NAMES):
            assert grads[k].dtype == torch.float32 and grads[k].shape == s[k].shape
            got, ref = grads[k][i].double().cpu().numpy(), ref_grads[k].numpy()
            for c in range(ref.shape[1]):
                if c not in CONTRACT[what]:
                    assert np.all(got[:, c] == 0), (name, i, what, c)
                    continue
                err, scale = np.max(np.abs(got[:, c] - ref[:, c])), np.max(np.abs(ref[:, c]))
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                assert err <= 1e-5 * scale + 1e-7, (name, i, what, c, err, scale)
    print(f'{name}: worst error / bar {worst:.3f}')


def _equal(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def case14():
    """case14, 3 grids, every pair: 190 pairs, 20 candidates in one ragged chunk, 24 pair chunks of 8 with the last one short."""
    s = _case(14, 3, seed=2)
    E = s[1].shape[1]
    pairs = powerflow._pair_list(None, E).tolist()
    assert len(pairs) == 190 and E == 20
    return s, E, pairs, _weights(3, 190, E, 5)


@pytest.mark.parametrize('rating_kind', ['none', 'per_line', 'per_grid'])
def test_case14_every_pair_against_the_reference_autograd(case14, rating_kind):
    s, E, pairs, weights = case14
    rating = {'none': None, 'per_line': _rating(E, 6), 'per_grid': _rating(E, 7, 3)}[rating_kind]
    res, grads = _grads(s, weights, rating=rating)
    assert int((~res.islanding).sum()) == 163
    want = _reference(s, pairs, weights, rating, range(3))
    for i, (_, flows) in want.items():
        assert torch.equal(flows.isnan().all(dim=1), res.islanding.cpu())
    _check(grads, s, want, f'case14 {rating_kind}')
    # the forward outputs and base.* are the non-differentiable call's, bit for bit
    plain = powerflow.dc_n2_contingency_screen(*s[:3], slack_bus=s[3], rating=rating, flows=True)
    assert not plain.worst_loading.requires_grad and res.worst_loading.requires_grad and res.line_flow.requires_grad
    for a, b in ((res.line_flow, plain.line_flow), (res.worst_loading, plain.worst_loading), (res.worst_line, plain.worst_line),
                 (res.base.theta, plain.base.theta), (res.base.line_flow, plain.base.line_flow), (res.base.slack_p, plain.base.slack_p)):
        assert _same(a.detach(), b)


def test_case14_each_incoming_gradient_alone_and_each_input_alone(case14):
    s, E, pairs, weights = case14
    rating = _rating(E, 6)
    _, both = _grads(s, weights, rating=rating)
    for name, w in (('line_flow', (weights[0], None)), ('worst_loading', (None, weights[1]))):
        _, g = _grads(s, w, rating=rating)
        _check(g, s, _reference(s, pairs, w, rating, range(3)), f'case14 {name} alone')
    # flows=False: the bits of the worst-only gradient taken with flows=True
    _, worst_only = _grads(s, (None, weights[1]), rating=rating)
    res, g = _grads(s, (None, weights[1]), rating=rating, flows=False)
    assert res.line_flow is None and _equal(g, worst_only)
    # each input requiring grad alone: the bits of all three
    for k in range(3):
        _, g = _grads(s, weights, rating=rating, req=tuple(j == k for j in range(3)))
        assert len(g) == 1 and _same(g[0], both[k]), k


def test_base_gradients_are_dc_power_flows_bit_for_bit(case14):
    s, E, pairs, _ = case14
    g = torch.Generator().manual_seed(9)
    wt, wf, ws = (torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV) for shape in ((3, 14), (3, E), (3,)))
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=[[0, 4], [3, 9]], differentiable=True)
    got = torch.autograd.grad((wt * res.base.theta).sum() + (wf * res.base.line_flow).sum() + (ws * res.base.slack_p).sum(), ins)
    ins2 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    dc = powerflow.dc_power_flow(*ins2, slack_bus=s[3])
    want = torch.autograd.grad((wt * dc.theta).sum() + (wf * dc.line_flow).sum() + (ws * dc.slack_p).sum(), ins2)
    assert _equal(got, want) and not res.base.v.requires_grad


def test_case118_a_sample_and_the_full_list():
    """E = 186: three passes of the line-per-lane loops, the last ragged; candidates in one pair and in many.  Then the full list
    (17 205 pairs, chunks of 32) with a loss that reads the sampled rows only, held to the same reference."""
    s = _case(118, 2, seed=3)
    E = s[1].shape[1]
    every = powerflow._pair_list(None, E)
    assert E == 186 and every.shape[0] == 17205
    rng = np.random.default_rng(118)
    at = np.sort(rng.choice(every.shape[0], 150, replace=False))
    pairs = every[at].tolist()
    weights, rating = _weights(2, len(pairs), E, 21), _rating(E, 22)
    res, grads = _grads(s, weights, pairs=pairs, rating=rating)
    count = np.bincount(np.asarray(pairs).ravel(), minlength=E)
    assert (count == 1).any() and count.max() > 3
    _check(grads, s, _reference(s, pairs, weights, rating, range(2)), 'case118 sample')
    # the full list, summaries alone: one backward
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    full = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], rating=rating, differentiable=True)
    live = torch.from_numpy(at).to(DEV)[~res.islanding]
    g = torch.autograd.grad((weights[1][:, ~res.islanding] * full.worst_loading[:, live]).sum(), ins)
    _check(g, s, _reference(s, pairs, (None, weights[1]), rating, range(2)), 'case118 full list, sampled rows')


def test_row_jk_gives_zeros_to_its_own_lines():
    s = _case(30, 2, seed=6)
    E = s[1].shape[1]
    rating = _rating(E, 13)
    every = powerflow._pair_list(None, E)
    f, t, _ = synth.case_topology(30)
    live = every[~powerflow._pair_islanding(30, f - 1, t - 1, every)]
    for j, k in live[[0, 77, -1]].tolist():
        w = _weights(2, 1, E, j + k)
        _, g = _grads(s, w, pairs=[[j, k]], rating=rating)
        own = g[1][:, [j, k], :]
        print(f'pair ({j}, {k}): largest own-line entry {float(own.abs().max()):.3e} of {float(g[1].abs().max()):.3e}')
        assert bool(torch.isfinite(g[1]).all()) and bool((g[1] != 0).any())
        assert bool((own == 0).all()), (j, k)
    # two rows that share line j: exact zeros at j, which both hold; k and k2 get the other row's contribution
    (j, k), (j2, k2) = live[0].tolist(), live[1].tolist()
    assert j == j2 and k != k2
    _, g = _grads(s, _weights(2, 2, E, 3), pairs=[[j, k], [k2, j]], rating=rating)
    assert bool((g[1][:, j, :] == 0).all()) and bool((g[1][:, [k, k2]][..., [3, 5, 6]] != 0).all())


def test_properties_of_the_contract():
    s = _case(30, 3, seed=6)
    E = s[1].shape[1]
    rating = _rating(E, 13)
    every = powerflow._pair_list(None, E)
    f, t, _ = synth.case_topology(30)
    live = every[~powerflow._pair_islanding(30, f - 1, t - 1, every)]
    pairs = live[[0, 40, 77, 200, 400, 611, 77]].tolist()                  # lines in one pair and in several, one pair twice
    weights = _weights(3, len(pairs), E, 23)
    res, a = _grads(s, weights, pairs=pairs, rating=rating)
    assert not bool(res.islanding.any()) and all(bool(torch.isfinite(x).all()) for x in a)
    # (k, j) in place of (j, k): the same bits
    _, b = _grads(s, weights, pairs=[[q, p] if i % 2 else [p, q] for i, (p, q) in enumerate(pairs)], rating=rating)
    assert _equal(a, b)
    # from run to run, alone and in a sub-batch
    _, b = _grads(s, weights, pairs=pairs, rating=rating)
    assert _equal(a, b)
    for sel in ([1], [2, 0]):
        sub = tuple(x[sel] for x in s[:3]) + (s[3],)
        _, p = _grads(sub, tuple(w[sel] for w in weights), pairs=pairs, rating=rating)
        assert _equal(p, [x[sel] for x in a]), sel
    # a duplicated pair gives twice the gradient, at the bar
    w1 = _weights(3, 1, E, 24)
    _, g1 = _grads(s, w1, pairs=[pairs[2]], rating=rating)
    _, g2 = _grads(s, tuple(torch.cat([w, w], dim=1) for w in w1), pairs=[pairs[2], pairs[2][::-1]], rating=rating)
    for x, y in zip(g2, g1):
        err, scale = float((x.double() - 2 * y.double()).abs().max()), float(2 * y.double().abs().max())
        assert err <= 1e-5 * scale + 1e-7
    # a 2-D single grid and CPU tensors in: the same bits
    ins = [x[1].detach().clone().requires_grad_(True) for x in s[:3]]
    one = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=pairs, rating=rating, flows=True, differentiable=True)
    assert one.line_flow.shape == (len(pairs), E) and one.worst_loading.shape == (len(pairs),)
    g = torch.autograd.grad(_loss(one, tuple(w[1] for w in weights)), ins)
    assert all(x.shape == y.shape for x, y in zip(g, ins)) and _equal(g, [x[1] for x in a])
    ins = [x.cpu().clone().requires_grad_(True) for x in s[:3]]
    cpu = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=pairs, rating=rating.cpu(), flows=True, differentiable=True)
    assert cpu.line_flow.device.type == 'cpu' and cpu.worst_loading.requires_grad
    g = torch.autograd.grad(_loss(cpu, tuple(w.cpu() for w in weights)), ins)
    assert all(x.device.type == 'cpu' for x in g) and _equal(g, [x.cpu() for x in a])
    # no grad asked for, grad mode off, or the default: plain tensors
    with torch.no_grad():
        off = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=pairs, differentiable=True)
    assert not off.worst_loading.requires_grad and not off.base.theta.requires_grad
    on = powerflow.dc_n2_contingency_screen(*ins, slack_bus=s[3], pairs=pairs)
    assert not on.worst_loading.requires_grad


def test_a_tie_in_the_worst_loading_follows_worst_line():
    s = _case(14, 2, seed=4)
    E = s[1].shape[1]
    pairs = [[0, 5], [3, 9]]
    plain = powerflow.dc_n2_contingency_screen(*s[:3], slack_bus=s[3], pairs=pairs, flows=True)
    # a rating per grid that makes lines 2 and 7 carry exactly the same loading, the largest of the row
    flow = plain.line_flow.abs()
    rating = (flow.amax(dim=1) * 4 + 1.0)
    rating[:, 2] = flow[:, 0, 2]
    rating[:, 7] = flow[:, 0, 7]
    res, g = _grads(s, (None, torch.ones(2, 2, dtype=torch.float64, device=DEV)), pairs=pairs, rating=rating, flows=False)
    assert res.worst_line[:, 0].tolist() == [2, 2] and res.worst_loading[:, 0].tolist() == [1.0, 1.0]
    # the tie holds in the device's bits only (the reference's flows differ in the last ones), so the reference is told the line:
    # the same loss written on line_flow, sign(F'_w) / rating_w at w = worst_line
    wf = torch.zeros(2, 2, E, dtype=torch.float64)
    for i in range(2):
        for p in range(2):
            w = int(res.worst_line[i, p])
            wf[i, p, w] = float(torch.sign(plain.line_flow[i, p, w]) / rating[i, w])
    _check(g, s, _reference(s, pairs, (wf, None), None, range(2)), 'case14 tie')
    # and line 7, which ties, gets nothing of it: with the rating of line 2 a hair larger the gradient moves to line 7
    rating[:, 2] *= 1.0 + 1e-12
    res7, g7 = _grads(s, (None, torch.ones(2, 2, dtype=torch.float64, device=DEV)), pairs=pairs, rating=rating, flows=False)
    assert res7.worst_line[:, 0].tolist() == [7, 7] and not _equal(g, g7)


def test_islanding_rows_and_failure_per_grid():
    s = _case(14, 4, seed=4)
    E = s[1].shape[1]
    pairs = powerflow._pair_list(None, E).tolist()
    weights = _weights(4, len(pairs), E, 17)
    res, good = _grads(s, weights)
    isl = res.islanding
    assert int(isl.sum()) == 27 and all(bool(torch.isfinite(x).all()) for x in good)
    # a non-zero incoming gradient on an islanding row of grid 2 (the loss reads every row): NaN rows for that grid only
    everything = torch.ones_like(isl)
    wf, wl = weights[0].clone(), weights[1].clone()
    wf[:, isl] = 0
    wl[:, isl] = 0
    wl[2, int(torch.nonzero(isl)[0])] = 1.5
    _, g = _grads(s, (wf, wl), rows=everything)
    for x, y in zip(g, good):
        assert bool(x[2].isnan().all()) and _same(x[[0, 1, 3]], y[[0, 1, 3]])
    wl[2] = torch.where(isl, 0.0, wl[2])
    wf[1, int(torch.nonzero(isl)[-1]), 7] = -2.0
    _, g = _grads(s, (wf, wl), rows=everything)
    for x, y in zip(g, good):
        assert bool(x[1].isnan().all()) and _same(x[[0, 2, 3]], y[[0, 2, 3]])
    # weights that are exactly zero on the islanding rows, read through the NaN rows: as the indexed loss, bit for bit
    wf[1] = torch.where(isl.unsqueeze(1), 0.0, wf[1])
    _, g = _grads(s, (wf, wl), rows=everything)
    assert _equal(g, good)
    # a grid with a line that cannot be solved: converged False and NaN rows, the others unchanged bit for bit
    lines = s[1].clone()
    lines[3, 7, 3] = float('nan')
    bad = (s[0], lines, s[2], s[3])
    res, g = _grads(bad, weights)
    assert res.converged.tolist() == [True, True, True, False] and bool(res.worst_loading[3].isnan().all())
    for x, y in zip(g, good):
        assert bool(x[3].isnan().all()) and _same(x[:3], y[:3])
    zero = tuple(w.clone() for w in weights)
    zero[0][3] = 0
    zero[1][3] = 0
    res, g = _grads(bad, zero)
    for x, y in zip(g, good):
        assert bool((x[3] == 0).all()) and _same(x[:3], y[:3])
    # a batch that mixes topologies is refused
    mixed = s[1].clone()
    mixed[1, 0, 1] = mixed[1, 5, 1]
    with pytest.raises((ValueError, gns_mod.GNSError)):
        powerflow.dc_n2_contingency_screen(s[0], mixed.requires_grad_(True), s[2], slack_bus=s[3], pairs=[[0, 1]], differentiable=True)


def test_lds_refusal_names_the_adjoints_image():
    tp = pt.path(6000)
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    want = 8 * (23994 + 6000 + 3 * 5999 + 2 * 5999 * 2 + 3)
    with pytest.raises(gns_mod.GNSError, match=pt.LDS_MESSAGE) as e:
        powerflow.dc_n2_contingency_screen(buses, lines.requires_grad_(True), gens, slack_bus=tp.slack, pairs=[[0, 1]],
                                           differentiable=True)
    assert str(want) in str(e.value) and '2 dim_p (W + 1) + 3 W' in str(e.value)


def test_agrees_with_the_sum_over_copies_of_the_mixed_route():
    """The route the adjoint replaces: one grid per (grid, pair) with both lines deleted, ``dc_power_flow(mixed_topologies=True)``
    with requires_grad, autograd summing over the copies."""
    bt = 2
    s = _case(14, bt, seed=8)
    E = s[1].shape[1]
    every = powerflow._pair_list(None, E)
    f, t, _ = synth.case_topology(14)
    pairs = every[~powerflow._pair_islanding(14, f - 1, t - 1, every)][::16]
    P = pairs.shape[0]
    weights, rating = _weights(bt, P, E, 11), _rating(E, 12)
    res, grads = _grads(s, weights, pairs=pairs.tolist(), rating=rating)
    assert P >= 10 and not bool(res.islanding.any())
    ins = [x.detach().clone().requires_grad_(True) for x in s[:3]]
    keep = torch.tensor(np.array([np.delete(np.arange(E), p) for p in pairs]), device=DEV)                   # [P, E-2]
    xl = ins[1][:, keep].reshape(bt * P, E - 2, 7)
    xb, xg = ins[0].repeat_interleave(P, dim=0), ins[2].repeat_interleave(P, dim=0)
    mixed = powerflow.dc_power_flow(xb, xl, xg, slack_bus=s[3], mixed_topologies=True)
    assert bool(mixed.converged.all())
    flow = mixed.line_flow.reshape(bt, P, E - 2)
    wf = torch.gather(weights[0], 2, keep.unsqueeze(0).expand(bt, P, E - 2))
    load = (flow.abs() / rating[keep].unsqueeze(0)).amax(dim=2)
    want = torch.autograd.grad((wf * flow).sum() + (weights[1] * load).sum(), ins)
    worst = 0.0
    for k, what in enumerate(NAMES):
        for i in range(bt):
            for c in CONTRACT[what]:
                a, b = grads[k][i, :, c].double(), want[k][i, :, c].double()
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                worst = max(worst, err / (1e-5 * scale + 1e-7))
                # both sides are float32 results of float64 arithmetic: each is within the bar of the exact value
                assert err <= 1e-5 * scale + 1e-7, (what, i, c, err, scale)
    print(f'expanded route: worst error / bar {worst:.3f}')


@pytest.mark.parametrize('name', FAMILIES)
def test_generated_families_against_the_reference_autograd(name):
    tp = pt.families()[name]
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', 2, 0, device=DEV)
    s = (buses, _perturbed(lines, len(name)), gens, tp.slack)
    E = tp.f.size
    pairs = family_pairs(name, tp)
    assert len(pairs) <= 120 and all(p in pairs for p in special_pairs(tp))
    if name == 'random40_parallel_selfloop':
        loop = int(np.flatnonzero(tp.f == tp.t)[0])
        (a, b), (c, d) = special_pairs(tp)
        assert {tp.f[a], tp.t[a]} == {tp.f[b], tp.t[b]} and c == loop
    weights, rating = _weights(2, len(pairs), E, len(name)), _rating(E, 8)
    res, grads = _grads(s, weights, pairs=pairs, rating=rating)
    assert not bool(res.islanding.any())
    _check(grads, s, _reference(s, pairs, weights, rating, range(2)), name)


def test_case300_a_list_over_three_candidate_chunks():
    """1 grid, 60 pairs over exactly 41 distinct lines: with W = 16 the 42 columns of the solve kernel are three chunks, the last of
    10.  Two pairs island although neither line is a bridge; the last line (a bridge of case300, so its pairs island) is a
    candidate."""
    s = _case(300, 1, seed=5)
    E = s[1].shape[1]
    f, t, g = synth.case_topology(300)
    pairs = case300_pairs(300, f, t)
    fd = powerflow.analyse_fd_topology(300, f, t, g, s[3])
    assert powerflow._dcn2_adjoint_lds_bytes(fd.host)[1] == 16 and np.unique(pairs).size == 41 and len(pairs) == 60
    bridges = powerflow._bridges(300, f - 1, t - 1)
    weights, rating = _weights(1, len(pairs), E, 31), _rating(E, 32)
    res, grads = _grads(s, weights, pairs=pairs, rating=rating)
    isl = res.islanding.cpu().numpy()
    assert isl[:3].all() and not bridges[np.array(pairs[:2])].any() and E - 1 in pairs[2] and 10 < int((~isl).sum())
    _check(grads, s, _reference(s, pairs, weights, rating, range(1)), 'case300')


def test_column_maps_route_the_gradients_back():
    """Inputs with permuted (and one more) columns and the maps B, L, G that name them, as ``dc_power_flow`` takes them: the
    gradients come back in the caller's columns, with the bits of the plain call; a column no map names gets 0."""
    s = _case(14, 3, seed=12)
    E = s[1].shape[1]
    pairs = powerflow._pair_list(None, E)[::3].tolist()
    weights, rating = _weights(3, len(pairs), E, 18), _rating(E, 19)
    _, want = _grads(s, weights, pairs=pairs, rating=rating)
    g = torch.Generator().manual_seed(20)
    perms = [torch.randperm(n + 1, generator=g) for n in (6, 7, 7)]                     # canonical column c sits at perms[k][c]
    wide = []
    for t, p in zip(s[:3], perms):
        x = torch.full((*t.shape[:2], t.shape[2] + 1), 7.5, device=DEV)
        x[..., p[:t.shape[2]].to(DEV)] = t
        wide.append(x.requires_grad_(True))
    maps = [{name: int(p[c]) for name, c in default.items()} for p, default in zip(perms, (gns_mod._B0, gns_mod._L0, gns_mod._G0))]
    res = powerflow.dc_n2_contingency_screen(*wide, B=maps[0], L=maps[1], G=maps[2], slack_bus=s[3], pairs=pairs, rating=rating,
                                             flows=True, differentiable=True)
    got = torch.autograd.grad(_loss(res, weights), wide)
    for x, y, p, n in zip(got, want, perms, (6, 7, 7)):
        assert x.shape[2] == n + 1 and _same(x[..., p[:n].to(DEV)], y) and bool((x[..., int(p[n])] == 0).all())
