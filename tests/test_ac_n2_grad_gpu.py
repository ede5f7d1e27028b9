"""Gradients of the AC N-2 contingency screen on the MI355X (``powerflow.ac_n2_contingency_screen_differentiable``,
include/gns_powerflow.h "Gradients of the AC N-2 screen"): against the float64 reference (``ac_n2_grad_reference``: both line rows
deleted, the reference's own Newton from the base, autograd's dense Jacobian and the implicit function theorem), against the
product's other route (the sum over copies of ``newton_raphson(mixed_topologies=True)`` on the expanded batch), the properties of
the contract, bitwise reproducibility, per-row and per-grid failure and the LDS refusal.

The bar is the project's gradient bar per column per grid (test_ac_contingency_grad_gpu): the outputs are float32, so
max|out - ref| <= 1e-5 max|ref| + 1e-7; every column outside the contract is exactly 0.  A loss reads only the rows where both the
product converged and the reference converged with two iterations to spare (``ac_n2_reference.spare``), by indexing, so every
other row's incoming gradient is exactly zero; each test asserts the share of rows it compares.  The counts stated with the tests
were computed on the CPU from the reference alone."""
import functools

import numpy as np
import pytest
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
import ac_n2_grad_reference as g2ref
import ac_n2_reference as n2ref
from ac_n2_pairs import KINDS, every_pair, pair_kinds, rows_pairs
import pf_topologies as pt
from test_ac_contingency_grad_gpu import CONTRACT, NAMES, OUT, SUMMARIES, _case, _equal, _family, _loss, _rating, _weights
from test_ac_contingency_host import toy
from test_ac_n2_gpu import _reference14

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EVERY14 = tuple(every_pair(20))
SUB14 = EVERY14[::9][:20]          # 20 pairs of case14 spread over the list (positions 0, 9, ..., 171)


@functools.lru_cache(maxsize=None)
def _toy(batch):
    tp = toy()
    buses, lines, gens, _, _ = pt.grids(tp, 'reference', batch, 0, device=DEV)
    return buses, lines, gens, tp.slack


@functools.lru_cache(maxsize=None)
def _ref_rows(key, pairs):
    """The reference's rows of every grid of a cached case for a tuple of pairs: solved once, never changed."""
    s = key[0](*key[1:])
    return [g2ref.solve_rows(s[0][i].cpu(), s[1][i].cpu(), s[2][i].cpu(), s[3], list(pairs)) for i in range(s[0].shape[0])]


def _ref14(pairs):
    """The reference's rows of ``_case(14, 3)`` (test_ac_n2_gpu's grids) for pairs in either order, from test_ac_n2_gpu's cached solve
    of every pair: the 570 reference solves are made once for both modules."""
    rows, _ = _reference14()
    return [[rows[i, min(p), max(p)] for p in pairs] for i in range(3)]


def _spare_mask(rows):
    return torch.tensor([[n2ref.spare(r) for r in grid] for grid in rows], device=DEV)


def _diff(s, ins=None, **kw):
    ins = s[:3] if ins is None else ins
    return powerflow.ac_n2_contingency_screen_differentiable(*ins, slack_bus=s[3], **kw)


def _grads(s, w, mask=None, req=(True, True, True), **kw):
    """(result, the rows of the loss, gradients of the inputs that require grad) of the call with states and flows unless ``kw``
    says otherwise.  ``mask``: None (the converged rows), a bool tensor that is and-ed with them, or a callable of the result."""
    ins = [t.detach().clone().requires_grad_(r) for t, r in zip(s[:3], req)]
    res = _diff(s, ins, **{**dict(flows=True, states=True), **kw})
    rows = mask(res) if callable(mask) else res.converged if mask is None else res.converged & mask
    return res, rows, torch.autograd.grad(_loss(res, w, rows), [t for t in ins if t.requires_grad])


def _check(grads, s, res, w, rows, refrows, rating, grids, name):
    """Every contract column of every grid of ``grids`` to the bar; returns the worst error / bar."""
    pairs = res.pairs.tolist()
    worst = (0.0, None)
    for i in grids:
        r = None if rating is None else (rating if rating.dim() == 1 else rating[i]).cpu().numpy()
        want, cond = g2ref.gradients(s[0][i].cpu(), s[1][i].cpu(), s[2][i].cpu(), s[3], pairs, refrows[i], rows[i].tolist(),
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


def test_case14_every_pair_against_the_reference():
    """570 rows: 81 islanding (27 per grid), 489 not; the reference converges 329 of the 489 with two iterations to spare (counted
    on the CPU from the reference alone), so at least 0.6 x 489 rows must be in the loss, the cap test_ac_n2_gpu uses.  All nine
    outputs are weighted, the rating is per grid.  190 pairs: C = 3, 64 chunks per grid, the last of a single row."""
    s = _case(14, 3)
    E, N, P = 20, 14, 190
    rating = _rating(E, 42, 3)
    refrows = _ref14(EVERY14)
    assert sum(r is not None for g in refrows for r in g) == 489 and int(_spare_mask(refrows).sum()) == 329
    w = _weights(3, P, N, E, 43)
    res, rows, grads = _grads(s, w, _spare_mask(refrows), rating=rating)
    n_pairs = 3 * int((~res.islanding).sum())
    print(f'case14 every pair: {int(rows.sum())} of {n_pairs} non-islanding rows in the loss')
    assert n_pairs == 489 and int(rows.sum()) >= 0.6 * 489
    assert res.v.requires_grad and res.q_to.requires_grad and res.worst_loading.requires_grad and res.v_min.requires_grad
    assert not res.converged.requires_grad and not res.worst_line.requires_grad and not res.mismatch.requires_grad
    _check(grads, s, res, w, rows, refrows, rating, range(3), 'case14 every pair')


@pytest.mark.parametrize('rated', ['none', 'per_line'])
def test_case14_a_sublist_without_a_rating_and_with_one_per_line(rated):
    """20 pairs spread over the list, 3 grids: 60 rows, 15 islanding (5 per grid), 45 not; the reference converges 31 of the 45 with
    two iterations to spare (counted on the CPU from the reference alone): at least 0.6 x 45 rows in the loss."""
    s = _case(14, 3)
    E, N = 20, 14
    rating = {'none': None, 'per_line': _rating(E, 44)}[rated]
    refrows = _ref14(SUB14)
    assert sum(r is not None for g in refrows for r in g) == 45 and int(_spare_mask(refrows).sum()) == 31
    w = _weights(3, len(SUB14), N, E, 45)
    res, rows, grads = _grads(s, w, _spare_mask(refrows), pairs=list(SUB14), rating=rating)
    print(f'case14 sublist {rated}: {int(rows.sum())} of 45 non-islanding rows in the loss')
    assert 3 * int((~res.islanding).sum()) == 45 and int(rows.sum()) >= 0.6 * 45
    _check(grads, s, res, w, rows, refrows, rating, range(3), f'case14 sublist {rated}')


def test_generated_family_with_parallel_lines_and_a_self_loop_against_the_reference():
    """``rows_pairs`` of random40_parallel_selfloop (128 pairs: 1 parallel, 12 shared-bus, 1 loop-at-bus, 6 loop-elsewhere) x 2
    grids: 188 non-islanding rows, of which the reference converges 140 with two iterations to spare (counted on the CPU from the
    reference alone): at least 0.6 x 188 rows in the loss.  At least one pair of each kind the reference converges is among them;
    a kind it converges none of (the loop-at-bus pair islands: the self-loop's bus hangs on a bridge) is covered on the toy grid
    below, where parallel lines are covered again."""
    name = 'random40_parallel_selfloop'
    tp = pt.families()[name]
    s = _family(name, 2)
    E, N = s[1].shape[1], s[0].shape[1]
    pairs = tuple(rows_pairs(tp))
    kinds = pair_kinds(tp)
    listed = [kinds.get(p) for p in pairs]
    assert len(pairs) == 128 and [listed.count(k) for k in KINDS] == [1, 12, 1, 6]
    refrows = _ref_rows((_family, name, 2), pairs)
    spare = _spare_mask(refrows)
    assert sum(r is not None for g in refrows for r in g) == 188 and int(spare.sum()) == 140
    w = _weights(2, len(pairs), N, E, 46)
    rating = _rating(E, 47)
    res, rows, grads = _grads(s, w, spare, pairs=list(pairs), rating=rating)
    print(f'{name}: {int(rows.sum())} of 188 non-islanding rows in the loss')
    assert 2 * int((~res.islanding).sum()) == 188 and int(rows.sum()) >= 0.6 * 188
    in_loss = rows.any(dim=0).tolist()
    for kind in KINDS:
        converged = [p for p in range(128) if listed[p] == kind and bool(spare[:, p].any())]
        covered = [p for p in converged if in_loss[p]]
        print(f'{name}: {kind}: {listed.count(kind)} listed, the reference converges {len(converged)}, in the loss {len(covered)}')
        assert covered or not converged, kind
    _check(grads, s, res, w, rows, refrows, rating, range(2), name)
    # one pair alone in the loss: exactly 0 in the own columns of both of its lines
    for kind in KINDS:
        p = next((p for p in range(128) if listed[p] == kind and bool(rows[:, p].all())), None)
        if p is None:
            continue
        j, k = pairs[p]
        _, r1, g1 = _grads(s, {n: x[:, [p]] for n, x in w.items()}, pairs=[pairs[p]], rating=rating)
        assert bool(r1.all()) and bool((g1[1][:, [j, k], :] == 0).all()) and bool((g1[1] != 0).any()) and bool(torch.isfinite(g1[1]).all())


@pytest.mark.parametrize('pair', [(0, 5), (2, 6), (6, 1), (0, 1)])
def test_toy_grid_parallel_lines_and_the_self_loop_against_the_reference(pair):
    """The toy grid x 2: lines 0 and 5 are parallel and both out (numeric zeros in the pattern), line 6 runs from bus 3 to itself
    (with line 2 at its bus, and, named the other way round, with line 1 at its bus), lines 0 and 1 share bus 2.  The pair alone
    is the list; both grids must be in the loss, and the own columns of both lines are exactly 0."""
    s = _toy(2)
    refrows = _ref_rows((_toy, 2), (pair,))
    assert bool(_spare_mask(refrows).all())
    w = _weights(2, 1, 5, 7, 48)
    rating = _rating(7, 49)
    res, rows, grads = _grads(s, w, _spare_mask(refrows), pairs=[pair], rating=rating)
    assert bool(rows.all()) and res.pairs.tolist() == [list(pair)]
    assert bool((grads[1][:, list(pair), :] == 0).all())
    _check(grads, s, res, w, rows, refrows, rating, range(2), f'toy {pair}')


@functools.lru_cache(maxsize=None)
def _case118_list():
    every = every_pair(186)
    picked = [every[p] for p in np.random.default_rng(118).permutation(len(every))[:24]]
    f, t, _ = synth.case_topology(118)
    bridge = int(np.flatnonzero(powerflow._bridges(118, f - 1, t - 1))[0])
    return tuple(picked + [(bridge, 0 if bridge else 1), picked[1]])              # 24 pairs, a pair with a bridge, a duplicate


def test_case118_a_list_with_a_bridge_pair_and_a_duplicate_against_the_reference():
    """The first 24 entries of ``default_rng(118).permutation`` over every pair: 22 non-islanding, of which the reference converges
    18 with two iterations to spare (counted on the CPU from the reference alone): at least 0.7 x 22 of those rows in the loss."""
    s = _case(118, 1)
    pairs = _case118_list()
    assert len(pairs) == 26
    refrows = _ref_rows((_case, 118, 1), pairs)
    spare = _spare_mask(refrows)
    assert sum(r is not None for r in refrows[0][:24]) == 22 and int(spare[0, :24].sum()) == 18 and refrows[0][24] is None
    w = _weights(1, 26, 118, s[1].shape[1], 50)
    rating = _rating(s[1].shape[1], 51)
    res, rows, grads = _grads(s, w, spare, pairs=list(pairs), rating=rating)
    print(f'case118: {int(rows[0, :24].sum())} of 22 listed non-islanding rows in the loss, {int(rows.sum())} with the duplicate')
    assert bool(res.islanding[24]) and int((~res.islanding[:24]).sum()) == 22 and int(rows[0, :24].sum()) >= 0.7 * 22
    assert bool(rows[0, 25]) == bool(rows[0, 1])
    _check(grads, s, res, w, rows, refrows, rating, range(1), 'case118')


def test_case14_a_list_over_several_rows_per_wave_three_rows_against_the_reference():
    """130 pairs: C = 3, 44 chunks per grid, the last of a single row.  Three rows of different chunks against the reference; every
    converged row: finite, and the same bits from run to run."""
    s3 = _case(14, 3)
    s = tuple(x[:1] for x in s3[:3]) + (s3[3],)                                     # grid 0 alone
    pairs = EVERY14[:130]
    plain = powerflow.ac_n2_contingency_screen(*s[:3], slack_bus=s[3], pairs=list(pairs))
    full = _ref14(EVERY14)[0]
    cand = [p for p in torch.nonzero(plain.converged[0]).flatten().tolist() if n2ref.spare(full[p])]
    pick = [cand[0], cand[len(cand) // 2], cand[-1]]                               # rows of three different chunks, the last one's too
    assert len({p // 3 for p in pick}) == 3 and pick[-1] == 129
    refrows = [[full[p] if p in pick else None for p in range(130)]]
    mask = torch.tensor([[p in pick for p in range(130)]], device=DEV)
    w = _weights(1, 130, 14, 20, 52)
    res, rows, grads = _grads(s, w, mask, pairs=list(pairs))
    assert int(rows.sum()) == 3
    _check(grads, s, res, w, rows, refrows, None, range(1), 'case14 130 pairs')
    _, all_rows, a = _grads(s, w, pairs=list(pairs))
    _, _, b = _grads(s, w, pairs=list(pairs))
    assert int(all_rows.sum()) > 60 and _equal(a, b) and all(bool(torch.isfinite(x).all()) for x in a)


def test_each_incoming_gradient_alone_and_the_slim_calls():
    s = _case(14, 3)
    E, N, P = 20, 14, len(SUB14)
    refrows = _ref14(SUB14)
    mask = _spare_mask(refrows)
    rating = _rating(E, 44)
    for name in OUT:
        w = _weights(3, P, N, E, 53, only=(name,))
        res, rows, grads = _grads(s, w, mask, pairs=list(SUB14), rating=rating)
        _check(grads, s, res, w, rows, refrows, rating, [1], f'case14 {name} alone')
    # flows=False, states=False (the defaults): the summaries' gradients with the same bits, the tensors not returned
    w = _weights(3, P, N, E, 54, only=SUMMARIES)
    _, _, full = _grads(s, w, mask, pairs=list(SUB14), rating=rating)
    for kw in (dict(flows=False), dict(states=False), dict(flows=False, states=False)):
        res, _, slim = _grads(s, w, mask, pairs=list(SUB14), rating=rating, **kw)
        assert _equal(slim, full), kw
        assert (res.v is None) == ('states' in kw) and (res.p_from is None) == ('flows' in kw)
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res = _diff(s, ins, pairs=list(SUB14), rating=rating)                           # the call's own defaults
    assert res.v is None and res.theta is None and res.p_from is None and res.q_to is None and res.worst_loading.requires_grad
    rows = res.converged & mask
    assert _equal(torch.autograd.grad(_loss(res, w, rows), ins), full)
    # a subset of the inputs requires grad: the bits of all three
    w = _weights(3, P, N, E, 45)
    _, _, full = _grads(s, w, mask, pairs=list(SUB14), rating=rating)
    for req in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        _, _, part = _grads(s, w, mask, req=req, pairs=list(SUB14), rating=rating)
        assert _equal(part, [g for g, r in zip(full, req) if r]), req


def _bits(a):
    return a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int64 if a.element_size() == 8 else torch.int32)


def test_base_gradients_are_newton_raphsons_and_the_forward_is_unchanged():
    s = _case(14, 3)
    g = torch.Generator().manual_seed(55)
    wv, wt = (torch.randn(3, 14, generator=g, dtype=torch.float64).to(DEV) for _ in range(2))
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    res = _diff(s, ins, pairs=[(0, 4), (7, 2)])
    got = torch.autograd.grad((wv * res.base.v).sum() + (wt * res.base.theta).sum(), ins)
    ins2 = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    nr = powerflow.newton_raphson(*ins2, slack_bus=s[3])
    want = torch.autograd.grad((wv * nr.v).sum() + (wt * nr.theta).sum(), ins2)
    assert _equal(got, want)
    # the forward: the bits of the plain call in every field, with every choice of flows and states
    for kw in (dict(flows=True, states=True), dict(), dict(flows=True), dict(states=True)):
        plain = powerflow.ac_n2_contingency_screen(*s[:3], slack_bus=s[3], **kw)
        ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
        diff = _diff(s, ins, **kw)
        assert type(diff) is powerflow.AcN2ContingencyResult
        for k in powerflow.AcN2ContingencyResult._fields[1:]:
            a, b = getattr(plain, k), getattr(diff, k)
            assert (a is None) == (b is None), (kw, k)
            if a is not None:
                assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b.detach())), (kw, k)
        for a, b in zip(plain.base, diff.base):
            assert torch.equal(a, b.detach())
    # no grad asked for, or grad mode off: plain tensors
    with torch.no_grad():
        off = _diff(s, ins, pairs=[(0, 1)], states=True)
    assert not off.worst_loading.requires_grad and not off.v.requires_grad and not off.base.v.requires_grad
    off = _diff(s, pairs=[(0, 1)], states=True)
    assert not off.worst_loading.requires_grad and not off.v.requires_grad and not off.base.v.requires_grad


def test_agrees_with_the_sum_over_copies_of_the_expanded_route():
    """The route the adjoint replaces: one grid per (grid, pair) with both line rows deleted, ``newton_raphson(mixed_topologies=True)``
    with requires_grad warm-started from the base, autograd summing over the copies.  The loss reads v and theta (what that route
    returns) on the rows both routes converged on, over every non-islanding pair of case14 x 3."""
    s = _case(14, 3)
    E, N = 20, 14
    f, t, _ = synth.case_topology(14)
    every = np.asarray(EVERY14)
    pairs = every[~powerflow._pair_islanding(14, f - 1, t - 1, every)]
    P = pairs.shape[0]
    assert P == 163
    w = _weights(3, P, N, E, 56, only=('v', 'theta'))
    res, rows, grads = _grads(s, w, pairs=pairs, flows=False)
    ins = [x.detach().clone().requires_grad_(True) for x in s[:3]]
    keep = torch.tensor(np.array([np.delete(np.arange(E), p) for p in pairs]), device=DEV)                  # [P, E-2]
    xl = ins[1][:, keep].reshape(3 * P, E - 2, 7)
    xb, xg = ins[0].repeat_interleave(P, dim=0), ins[2].repeat_interleave(P, dim=0)
    v0, th0 = res.base.v.detach().repeat_interleave(P, dim=0), res.base.theta.detach().repeat_interleave(P, dim=0)
    mixed = powerflow.newton_raphson(xb, xl, xg, slack_bus=s[3], mixed_topologies=True, v0=v0, theta0=th0)
    assert torch.equal(mixed.converged.reshape(3, P), res.converged) and int(rows.sum()) >= 0.6 * 489
    mv, mth = mixed.v.reshape(3, P, N), mixed.theta.reshape(3, P, N)
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
    print(f'expanded route: {int(rows.sum())} rows, worst error / bar {worst:.3f}')


def test_reproducible_bit_for_bit_and_other_input_forms(monkeypatch):
    s = _case(14, 3)
    buses, lines, gens, slack = s
    E, N = 20, 14
    pairs = list(EVERY14[::3]) + [(3, 7), (3, 7), (7, 3)]                            # 67 pairs: C = 2, the last chunk of a single row
    w, rating = _weights(3, len(pairs), N, E, 57), _rating(E, 58)
    res, rows, a = _grads(s, w, pairs=pairs, rating=rating)
    _, _, b = _grads(s, w, pairs=pairs, rating=rating)                              # from run to run
    assert _equal(a, b) and all(bool(torch.isfinite(x).all()) for x in a) and int(rows.sum()) > 60
    for sel in ([1], [2, 0]):                                                       # alone and in another batch
        sub = tuple(x[sel] for x in s[:3]) + (slack,)
        _, _, p = _grads(sub, {n: x[sel] for n, x in w.items()}, pairs=pairs, rating=rating)
        assert _equal(p, [x[sel] for x in a]), sel
    # every pair's two lines swapped: the same rows, the same gradient bits
    swapped, srows, c = _grads(s, w, pairs=[(k, j) for j, k in pairs], rating=rating)
    assert torch.equal(srows, rows) and swapped.pairs.tolist() == [[k, j] for j, k in pairs] and _equal(c, a)
    # a 2-D single grid
    ins = [x[1].detach().clone().requires_grad_(True) for x in s[:3]]
    one = _diff(s, ins, pairs=pairs, rating=rating, flows=True, states=True)
    assert one.v.shape == (len(pairs), N) and one.worst_loading.shape == (len(pairs),)
    g = torch.autograd.grad(_loss(one, {n: x[1] for n, x in w.items()}, one.converged), ins)
    assert all(x.shape == y.shape for x, y in zip(g, ins)) and _equal(g, [x[1] for x in a])
    # CPU tensors in: CPU outputs, CPU gradients, the same bits
    ins = [x.cpu().clone().requires_grad_(True) for x in s[:3]]
    cpu = _diff(s, ins, pairs=pairs, rating=rating.cpu(), flows=True, states=True)
    assert cpu.v.device.type == 'cpu' and cpu.worst_loading.requires_grad
    g = torch.autograd.grad(_loss(cpu, w, cpu.converged), ins)
    assert all(x.device.type == 'cpu' for x in g) and _equal(g, [x.cpu() for x in a])
    # nothing is read that nothing wrote: the same bits from poisoned workspaces
    monkeypatch.setattr(gns_mod, 'POISON_WORKSPACES', True)
    _, _, d = _grads(s, w, pairs=pairs, rating=rating)
    assert _equal(d, a)


def test_properties_of_the_contract_and_failure_per_row_and_per_grid():
    s = _case(14, 3)
    E, N = 20, 14
    pairs = list(SUB14)
    P = len(pairs)
    w = _weights(3, P, N, E, 59)
    res, rows, good = _grads(s, w, pairs=pairs)
    assert all(bool(torch.isfinite(x).all()) for x in good)
    conv, isl = res.converged, res.islanding
    # a pair alone: exactly 0 in both lines' own columns; a duplicated pair, in either order, contributes exactly twice
    for p in torch.nonzero(conv.all(dim=0)).flatten().tolist()[:3]:
        j, k = pairs[p]
        w1 = {n: x[:, [p]] for n, x in w.items()}
        _, _, g1 = _grads(s, w1, pairs=[pairs[p]])
        assert bool((g1[1][:, [j, k], :] == 0).all()) and bool((g1[1] != 0).any()) and bool(torch.isfinite(g1[1]).all())
        _, _, g2 = _grads(s, {n: torch.cat([x, x], dim=1) for n, x in w1.items()}, pairs=[(j, k), (k, j)])
        for a, b in zip(g2, g1):
            assert torch.equal(a, 2 * b)
    # islanding and non-converged rows masked by indexing contribute nothing: the list without them gives the same bits when the
    # chunks are the same (a wave per row up to 64 pairs)
    stopped = ~conv & ~isl.unsqueeze(0)
    assert int(isl.sum()) == 5 and bool(stopped.any())
    keep = torch.nonzero(conv.all(dim=0)).flatten().tolist()
    _, _, part = _grads(s, {n: x[:, keep] for n, x in w.items()}, pairs=[pairs[p] for p in keep])
    _, _, same = _grads(s, w, mask=conv.all(dim=0).unsqueeze(0).expand(3, P), pairs=pairs)
    assert _equal(part, same)
    # zero weights on those rows, the loss reading every row's finite outputs: still skipped (never multiplied by zero)
    wz = {n: torch.where(conv.reshape(3, P, *[1] * (x.dim() - 2)), x, torch.zeros_like(x)) for n, x in w.items()}
    wz_sum = {n: (x if n in SUMMARIES[1:] else None) for n, x in wz.items()}       # v_min, v_max: finite wherever a row was iterated
    _, _, a = _grads(s, wz_sum, mask=lambda r: ~r.islanding.unsqueeze(0).expand(3, P), pairs=pairs)
    _, _, b = _grads(s, wz_sum, pairs=pairs)
    assert _equal(a, b)
    # a non-zero cotangent into a non-converged row: NaN rows for that grid, the others bit for bit
    gi, ji = (int(x) for x in torch.nonzero(stopped)[0])
    also = lambda g, p: (torch.arange(3, device=DEV).unsqueeze(1) == g) & (torch.arange(P, device=DEV) == p)   # noqa: E731
    _, _, bad = _grads(s, w, mask=lambda r: r.converged | also(gi, ji), pairs=pairs)
    others = [i for i in range(3) if i != gi]
    for x, y in zip(bad, good):
        assert bool(x[gi].isnan().all()) and _equal([x[others]], [y[others]])
    # ... and into an islanding row (NaN outputs)
    jb = int(torch.nonzero(isl)[0])
    _, _, bad = _grads(s, w, mask=lambda r: r.converged | also(2, jb), pairs=pairs)
    for x, y in zip(bad, good):
        assert bool(x[2].isnan().all()) and _equal([x[[0, 1]]], [y[[0, 1]]])
    # a grid without a base solution: NaN rows with a non-zero incoming gradient, zero rows without; the others bit for bit
    buses = s[0].clone()
    buses[1, :, 2:4] *= 40.0                                                       # loads no network of this size can serve
    sb = (buses, s[1], s[2], s[3])
    res_b, _, g = _grads(sb, w, mask=lambda r: torch.ones_like(r.converged), pairs=pairs)
    assert res_b.base.converged.tolist() == [True, False, True] and not bool(res_b.converged[1].any())
    for x in g:
        assert bool(x[1].isnan().all())
    _, _, g0 = _grads(sb, w, pairs=pairs)                                          # the converged rows: none of grid 1
    for x, y in zip(g0, good):
        assert bool((x[1] == 0).all()) and _equal([x[[0, 2]]], [y[[0, 2]]])


def test_a_tie_in_the_worst_loading_follows_worst_line():
    """Two identical lines between the same buses in the same direction have bit-identical flows: with the lowest rating they tie
    for the worst loading, worst_line is the lower of them, and the whole gradient of worst_loading is that of that line's loading.
    A second ring (lines 6 to 8) lets two of its lines go out without islanding."""
    tp = pt.Topo('ring5_twin_chords', 5, np.array([1, 2, 3, 4, 5, 1, 1, 2, 3]), np.array([2, 3, 4, 5, 1, 2, 3, 4, 5]), np.array([1, 3]), 1)
    buses, lines, gens, v, theta = pt.grids(tp, 'reference', 2, 0, device=DEV)
    lines = lines.clone()
    lines[:, 5, 2:] = lines[:, 0, 2:]
    buses, gens = synth.manufacture_solution(buses, lines, gens, tp.slack, v, theta)     # solvable again with the twin
    s = (buses, lines, gens, tp.slack)
    rating = torch.tensor([0.05, 1.0, 1.0, 1.0, 1.0, 0.05, 1.0, 1.0, 1.0], dtype=torch.float64, device=DEV)
    pairs = [(2, 3), (7, 3)]
    w = _weights(2, 2, 5, 9, 60, only=('worst_loading',))
    res, rows, got = _grads(s, w, pairs=pairs, rating=rating)
    assert int(rows.sum()) >= 2 and bool((res.worst_line[rows] == 0).all())           # the loss reads the converged rows
    assert torch.equal(res.p_from[..., 0], res.p_from[..., 5]) and torch.equal(res.q_to[..., 0], res.q_to[..., 5])
    ins = [t.detach().clone().requires_grad_(True) for t in s[:3]]
    r2 = _diff(s, ins, pairs=pairs, rating=rating, flows=True)
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
        powerflow.ac_n2_contingency_screen_differentiable(buses, lines.requires_grad_(True), gens, slack_bus=tp.slack, pairs=[(0, 1)])
    assert 'gns_acn2_adjoint_workspace_bytes' in str(e.value) and 'nnz(L+U) + dim + 8 N' in str(e.value) and not launched
