"""The DC family on the MI355X in the 'wide' value regime (``dc_wide_cases``: taps 0.5 .. 1.5, shifts within +-30 degrees, about
one line in eight series-compensated with x in [-0.3, -0.05]): ``dc_power_flow``, ``dc_contingency_screen``,
``dc_n2_contingency_screen`` and ``dc_generator_contingency_screen`` against the direct float64 references, the three adjoints
against the references' autograd, and two constructed grids with an exactly zero pivot and an exactly zero denominator off the
bridges.  With x < 0 a line's b = 1 / (x tau) is negative and Bbus[r, r] is indefinite: denominators 1 - b_k d_k and 2x2
determinants take both signs, and a line that is no bridge can leave a singular network, which only the device's own ``den != 0``
and ``det != 0`` tests catch.  The checks are the existing files' own (``_check_values``, ``_check_summaries``, ``_check``,
``_check_gradients``), imported, at their bars:
  forward, per (grid, row): max|out - ref| <= 1e-9 max(1, max|ref|); no selected row is left out; islanding exactly where the
  reference returns None;  gradients, per column and grid: max|out - ref| <= 1e-5 max|ref| + 1e-7, other columns exactly 0.

Sets: two 'wide' grids per topology as drawn (no ``_perturbed``), seed 0 but for ring30_slack_no_gen (seed 1: a worst line with
b < 0) and pair (seed 3: its one line has x > 0 in grid 0 and x < 0 in grid 1); both seeds chosen on the CPU from float64 factors.
Every topology passes the probe of ``test_dc_wide_host`` (its docstring holds the figures), so none is dropped, and the host's
float64 replay of the blob's own programs meets the bar on every set, so no seed changed for the elimination's sake.

Every test also holds ``res.base`` (or the solve itself) to the reference, so each one fails if a sign of x is lost, whatever
its rows compare (ring30_slack_no_gen without two lines is a tree, whose rows do not depend on x); that the row comparisons notice
it by themselves is shown on the CPU (``test_dc_wide_host.test_the_replay_with_the_sign_of_x_lost_misses_the_rows``).  In the
rated gradient tests the worst line of the coverage is the one of largest |F'| / rating, the one ``sign(F') / rating`` acts on.
Every test with rows that do not island asserts its coverage from the float64 factors, not from the device:
rows whose outaged line has x < 0, rows with den < 0 (det < 0 for pairs), rows whose worst line has b < 0, rows whose worst flow
is negative.  Measured on one MI355X (``profiles/dc_wide/gpu_suite_summary.txt`` holds the run): worst scaled error against the
bar's 1e-9, then of the compared (grid, row)s that do not island the rows with x_k < 0 / den or det < 0 / a worst line with b < 0 / a
negative worst flow:
  dc_power_flow, all eleven sets <= 1.0e-13; its gradients <= 0.006 of the gradient bar.
  N-1, every outage: lattice8x8 3.0e-12 (23 / 26 / 115 / 209 of 224); complete20 4.9e-13 (49 / 68 / 378 / 133 of 380);
    random40_parallel_selfloop 4.9e-15 (13 / 14 / 1 / 1 of 112); random97_parallel_selfloop 8.4e-14 (36 / 33 / 130 / 139 of 254);
    ring30_slack_no_gen 8.9e-15 (13 / 13 / 14 / 46 of 62); random24_stacked_gens 1.3e-14 (11 / 10 / 2 / 46 of 66);
    wheel71 4.4e-13 (37 / 50 / 274 / 137 of 280); pair, path65, star65_pv, hub150_70lines_70gens: islanding rows only.
  N-2: random24_stacked_gens, 703 pairs, 4.0e-14 (317 / 268 / 75 / 757 of 1036); ring30_slack_no_gen, 465 pairs, 2.6e-14
    (193 / 175 / 117 / 331 of 508); lattice8x8, 300 pairs, 4.7e-10 (115 / 145 / 320 / 523 of 600); complete20, 300 pairs, 5.3e-11
    (147 / 184 / 596 / 137 of 600); random40_parallel_selfloop, 300 pairs, 1.1e-14 (110 / 114 / 5 / 8 of 504); wheel71, 300 pairs,
    3.2e-12 (152 / 197 / 576 / 289 of 600).  lattice8x8's figure is pair (19, 45) of grid 0, selected for its determinant of -6.7e-6
    (flows of 2.9e5): the host's float64 replay of the kernels is 5.8e-10 from the direct reference there and 7.2e-11 at its next
    row (``test_dc_wide_host.test_the_fd_blob_serves_the_n2_screen_on_the_selected_pairs_of_lattice8x8``), and the two float64
    references differ by 6.7e-11 on that pair.
  generator rows (pickup None / 'pmax' / random alike to two digits): random24_stacked_gens 1.3e-14 (88 / 80 / 17 / 363 of 544);
    ring30_slack_no_gen 1.2e-14 (39 / 39 / 29 / 145 of 192); random40_parallel_selfloop 1.9e-15 (48 / 54 / 4 / 6 of 348); lattice8x8
    3.0e-12 (43 / 50 / 226 / 393 of 442); hub150_70lines_70gens 1.6e-13 and path65 5.2e-14 (generator-alone rows only).
  gradients of the two screens, every set and rating: <= 0.005 of the bar.
  constructed grids: zero pivot 4.8e-15 on grids 0 and 2; zero denominator 1.1e-15 (N-1), 1.2e-15 (generator), 2.4e-15 (N-2), with
    1, 3 and 6 rows singular without a bridge.
A library built with b = 1 / (|x| tau) passes every other DC test file and fails the tests of this one (the record is in the
profile file)."""
import types

import numpy as np
import pytest
import torch

import dc_contingency_reference as cref
import dc_generator_contingency_reference as gref
import dc_n2_reference as n2ref
import dc_wide_cases as wc
import test_dc_contingency_gpu as n1
import test_dc_contingency_grad_gpu as n1g
import test_dc_generator_contingency_gpu as g1
import test_dc_n2_gpu as n2
import test_dc_n2_grad_gpu as n2g
import test_dcpf_gpu as dcpf
from opf_graph_neural_solver_amd import powerflow
from test_dcpf_gpu import _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-9
ITEMS = ('x_neg', 'den_neg', 'worst_b_neg', 'worst_flow_neg')
N2_NAMES = ('random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8', 'complete20', 'random40_parallel_selfloop', 'wheel71')
G1_NAMES = ('random24_stacked_gens', 'ring30_slack_no_gen', 'random40_parallel_selfloop', 'lattice8x8', 'hub150_70lines_70gens',
            'path65')
RATINGS = ('none', 'per_line', 'per_grid')
ROWS = ('line_flow', 'worst_loading', 'worst_line')
# the seed of the gradient tests' ratings: the first from 8 on with which every rated case keeps its coverage, the worst line being
# the one of largest |F'| / rating (seed 8 leaves random40_parallel_selfloop and random24_stacked_gens without a worst line of b < 0);
# chosen on the CPU from the float64 factors
RATING_SEED = 11


def _base_meets_the_reference(base, s, name):
    assert not bool(base.v.requires_grad)
    dcpf._check_against_reference(type(base)(*(t.detach() for t in base)), s, f'{name} base')


def _covered(cov, name):
    print(f'{name}: coverage {cov}')
    for k in ITEMS:
        assert cov[k] >= 1, (name, k, cov)


def _is_wide(lines, name):
    """The compared lines' x column holds both signs, and tau reaches below 0.6 and above 1.4 (pair has two taps in all)."""
    neg, pos, lo, hi, _ = wc.regime(lines)
    assert neg and pos, name
    assert name == 'pair' or (lo < 0.6 and hi > 1.4), (name, lo, hi)


def _rating(kind, E, seed, bt=2):
    return {'none': None, 'per_line': n1g._rating(E, seed), 'per_grid': n1g._rating(E, seed + 1, bt=bt)}[kind]


# ---- dc_power_flow

@pytest.mark.parametrize('name', wc.NAMES)
def test_dc_power_flow_against_the_reference_and_power_balance(name):
    s = wc.wide_set(name, DEV)
    buses, lines, gens, slack = s
    _is_wide(lines, name)
    res = dcpf._dc(s)
    dcpf._check_against_reference(res, s, name)
    assert bool((res.theta[:, slack - 1] == 0).all()) and bool((res.v == 1).all())
    Bt, N = buses.shape[:2]
    f, t = lines[..., 0].long() - 1, lines[..., 1].long() - 1
    out = torch.zeros(Bt, N, dtype=torch.float64, device=DEV).scatter_add(1, f, res.line_flow).scatter_add(1, t, -res.line_flow)
    pg = torch.zeros(Bt, N, dtype=torch.float64, device=DEV).scatter_add(1, gens[..., 0].long() - 1, gens[..., 6].double())
    net = pg - buses[..., 2].double() - buses[..., 4].double()
    total = -net.sum(dim=1)
    net[:, slack - 1] += res.slack_p
    scale = res.line_flow.abs().amax(dim=1).clamp(min=1.0)
    assert bool(((out - net).abs().amax(dim=1) <= TOL * scale).all()), name
    assert bool(((res.slack_p - total).abs() <= TOL * total.abs().clamp(min=1.0)).all()), name


@pytest.mark.parametrize('name', wc.NAMES)
def test_dc_power_flow_gradients_against_the_reference_autograd(name):
    buses, lines, gens, slack = wc.wide_set(name, DEV)
    _is_wide(lines, name)
    weights = dcpf._weights(2, buses.shape[1], lines.shape[1], len(name))
    res, grads = dcpf._grads(buses, lines, gens, slack, weights)
    assert bool(res.converged.all())
    dcpf._check_gradients(grads, buses, lines, gens, slack, weights, range(2), name)
    for only in range(3):
        part = tuple(w if j == only else None for j, w in enumerate(weights))
        _, g = dcpf._grads(buses, lines, gens, slack, part)
        dcpf._check_gradients(g, buses, lines, gens, slack, part, range(2), f'{name} only {dcpf.OUTPUTS[only]}')


# ---- the N-1 screen

@pytest.mark.parametrize('name', wc.NAMES)
def test_n1_every_outage_against_the_reference(name):
    """Every outage of every wide set; pair, path65, star65_pv and hub150_70lines_70gens are all-bridge: islanding rows only."""
    s = wc.wide_set(name, DEV)
    E = s[1].shape[1]
    res = n1._screen(s)
    _base_meets_the_reference(res.base, s, name)
    n_isl = n1._check_values(res, s, list(range(E)), name)
    n1._check_summaries(s, None, res, name)
    if name in wc.ALL_BRIDGE:
        assert n_isl == E
    else:
        assert n_isl < E
        _covered(wc.n1_coverage(name), name)


@pytest.mark.parametrize('kind', RATINGS)
@pytest.mark.parametrize('name', ['lattice8x8', 'random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen',
                                  'complete20'])
def test_n1_gradients_against_the_reference_autograd(name, kind):
    s = wc.wide_set(name, DEV)
    _is_wide(s[1], name)
    E = s[1].shape[1]
    weights, rating = n1g._weights(2, E, E, len(name)), _rating(kind, E, RATING_SEED)
    res, grads = n1g._grads(s, weights, rating=rating)
    assert bool(res.converged.all()) and not bool(res.islanding.all())
    _base_meets_the_reference(res.base, s, name)
    n1g._check(grads, res, s, weights, rating, range(2), f'{name} rating {kind}')
    _covered(wc.n1_coverage(name, rating=None if rating is None else rating.cpu().numpy()), f'{name} rating {kind}')


# ---- the N-2 screen

@pytest.mark.parametrize('name', N2_NAMES)
def test_n2_pairs_against_the_reference(name):
    """Every pair of random24_stacked_gens and ring30_slack_no_gen; on the others at most 300 pairs (``dc_wide_cases.n2_pairs``):
    the pairs of parallel lines, the self-loop, the pairs whose float64 determinant is smallest and most negative, and a seeded
    sample."""
    s = wc.wide_set(name, DEV)
    tp = wc.topo(name)
    pairs = wc.n2_pairs(name)
    assert pairs.shape[0] <= 300 or name in N2_NAMES[:2]
    listed = {tuple(p) for p in pairs.tolist()}
    assert all(tuple(sorted(p)) in listed for p in wc.parallel_pairs(tp))
    assert all(sum(int(loop) in p for p in listed) >= 8 for loop in np.flatnonzero(tp.f == tp.t))
    res = n2._screen(s, pairs=pairs, flows=True)
    _base_meets_the_reference(res.base, s, name)
    n_isl = n2._check_values(res, s, name)
    assert n_isl < pairs.shape[0]
    n2._check_summaries(s, pairs, res, name)
    _covered(wc.n2_coverage(name, pairs), name)
    full = n2._screen(s)                                     # the whole default list: the same bits at the selected rows
    at = torch.from_numpy(n2._positions(pairs, tp.f.size)).to(DEV)
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)


@pytest.mark.parametrize('kind', RATINGS)
@pytest.mark.parametrize('name', ['random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8'])
def test_n2_gradients_against_the_reference_autograd(name, kind):
    """Every pair of random24_stacked_gens and ring30_slack_no_gen (islanding ones get no incoming gradient); on lattice8x8 at most
    120 live pairs, the ones of smallest and most negative determinant among them."""
    s = wc.wide_set(name, DEV)
    _is_wide(s[1], name)
    E = s[1].shape[1]
    pairs = wc.n2_grad_pairs(name) if name == 'lattice8x8' else powerflow._pair_list(None, E).tolist()
    assert name != 'lattice8x8' or len(pairs) <= 120
    weights, rating = n2g._weights(2, len(pairs), E, len(name)), _rating(kind, E, RATING_SEED)
    res, grads = n2g._grads(s, weights, pairs=pairs, rating=rating)
    assert bool(res.converged.all()) and not bool(res.islanding.all())
    _base_meets_the_reference(res.base, s, name)             # ring30 without two lines is a tree: its rows do not depend on x
    want = n2g._reference(s, pairs, weights, rating, range(2))
    for _, flows in want.values():
        assert torch.equal(flows.isnan().all(dim=1), res.islanding.cpu())
    n2g._check(grads, s, want, f'{name} rating {kind}')
    _covered(wc.n2_coverage(name, pairs, None if rating is None else rating.cpu().numpy()), f'{name} rating {kind}')


# ---- the generator screen

@pytest.mark.parametrize('kind', g1.PICKUPS)
@pytest.mark.parametrize('name', G1_NAMES)
def test_generator_rows_against_the_reference(name, kind):
    s = wc.wide_set(name, DEV)
    tp = wc.topo(name)
    E, Gn = tp.f.size, tp.g.size
    pickup = g1._pickup(kind, 2, Gn)
    rows = g1._family_rows(name, tp)
    assert rows.shape[0] <= 330
    res = g1._screen(s, contingencies=rows, pickup=pickup, flows=True)
    _base_meets_the_reference(res.base, s, name)
    n_isl = g1._check_values(res, s, pickup, f'{name}, pickup {kind}')
    g1._check_summaries(s, rows, pickup, res, name)
    alone = res.contingencies[:, 1] == -1
    assert int(alone.sum()) == Gn and not bool(res.islanding[alone].any())
    if name in wc.ALL_BRIDGE:
        assert n_isl == rows.shape[0] - Gn and torch.equal(res.islanding, ~alone)
    else:
        ws = [gref.weights(pickup, s[2][i].cpu(), i) for i in range(2)]
        _covered(wc.gen_coverage(name, rows, [None if w is None else w.numpy() for w in ws]), f'{name}, pickup {kind}')
    full = g1._screen(s, pickup=pickup)
    at = torch.from_numpy(g1._positions(rows, E)).to(DEV)
    assert _same(full.worst_loading[:, at], res.worst_loading) and torch.equal(full.worst_line[:, at], res.worst_line)


def test_generator_pins_hold_bit_for_bit_against_the_wide_n1_screen():
    """Pg_g exactly 0, or a generator on the slack bus with no pickup: row (g, -1) is the base flow and row (g, k) is row k of
    ``dc_contingency_screen`` on the same wide grids, bit for bit, islanding rows included."""
    name = 'random24_stacked_gens'
    tp = wc.topo(name)
    buses, lines, gens, slack = wc.wide_set(name, DEV)
    gens = gens.clone()
    gens[:, 2, 6] = 0.0
    gens[1, 6, 6] = 0.0
    s = (buses, lines, gens, slack)
    E, Gn = tp.f.size, tp.g.size
    assert tp.g.tolist() == [4, 1, 7, 4, 1, 4, 9, 4] and slack == 1
    screen = n1._screen(s)
    _base_meets_the_reference(screen.base, s, name)
    live = [k for k in range(E) if not bool(screen.islanding[k])][:6]
    n1._check_values(n1._screen(s, outages=live), s, live, f'{name}, Pg of generator 2 zero')
    assert bool(screen.islanding.any()) and not bool(screen.islanding.all())
    for kind, pinned in ((None, {0: (1, 2, 4), 1: (1, 2, 4, 6)}), ('random', {0: (2,), 1: (2, 6)}), ('pmax', {0: (2,), 1: (2, 6)})):
        res = g1._screen(s, pickup=g1._pickup(kind, 2, Gn), flows=True)
        flow = res.line_flow.reshape(2, Gn, E + 1, E)
        wl, wi = res.worst_loading.reshape(2, Gn, E + 1), res.worst_line.reshape(2, Gn, E + 1)
        for i, gs in pinned.items():
            for g in range(Gn):
                same = _same(flow[i, g, 0], res.base.line_flow[i]) and _same(flow[i, g, 1:], screen.line_flow[i])
                assert same == (g in gs), (kind, i, g)
                if g in gs:
                    assert _same(wl[i, g, 1:], screen.worst_loading[i]) and torch.equal(wi[i, g, 1:], screen.worst_line[i])


# ---- bit identity on one wide set

def test_rows_of_the_three_screens_are_bitwise_reproducible_on_a_wide_set():
    name = 'lattice8x8'
    s = wc.wide_set(name, DEV)
    tp = wc.topo(name)
    E, Gn = tp.f.size, tp.g.size
    one = tuple(x[1:2] for x in s[:3]) + (s[3],)
    pairs = wc.n2_pairs(name)[::3]
    rows = g1._family_rows(name, tp)
    pickup = g1._pickup('random', 2, Gn)
    calls = (('N-1', np.arange(E), lambda s_, l, **kw: n1._screen(s_, outages=l, **kw)),
             ('N-2', pairs, lambda s_, l, **kw: n2._screen(s_, pairs=l, flows=True, **kw)),
             ('generator', rows, lambda s_, l, **kw: g1._screen(s_, contingencies=l, flows=True,
                                                                pickup=pickup[1:2] if s_ is one else pickup, **kw)))
    for what, rows_, call in calls:
        a = call(s, rows_)
        _base_meets_the_reference(a.base, s, f'{name} {what}')
        b = call(s, rows_)                                                     # from run to run
        alone = call(one, rows_)                                               # in another batch
        rev = call(s, rows_[::-1].copy())                                      # a reversed list
        sub = [5, 0, 70, 5, 64, 63]
        dup = call(s, rows_[sub])                                              # a list with a duplicate
        row = call(one, rows_[70:71])                                          # a row alone
        for k in ROWS:
            x = getattr(a, k)
            assert _same(x, getattr(b, k)) and _same(x[1:2], getattr(alone, k)) and _same(x.flip(1), getattr(rev, k)), (what, k)
            assert _same(x[:, sub], getattr(dup, k)) and _same(x[1, 70], getattr(row, k)[0, 0]), (what, k)
        assert _same(dup.line_flow[:, 0], dup.line_flow[:, 3]) and bool(torch.isfinite(a.line_flow[:, 70]).all())
    # and the rows themselves are right: a few N-1 rows against the reference
    few = [0, 5, 63, 64, 70, 111]
    n1._check_values(n1._screen(s, outages=few), s, few, f'{name}, six outages')


# ---- constructed grids: an exactly zero pivot

def _grid1_failed(res, rows=True):
    assert res.converged.tolist() == [True, False, True]
    if rows:
        assert torch.equal(res.converged, res.base.converged)
        assert bool(res.line_flow[1].isnan().all()) and bool(res.worst_loading[1].isnan().all()) and bool((res.worst_line[1] == -1).all())
        assert bool(torch.isfinite(res.worst_loading[[0, 2]][:, ~res.islanding]).all())


def test_zero_pivot_fails_one_grid_alone_in_every_entry_point():
    """``dc_wide_cases.zero_pivot_batch``: in grid 1 the leaf's two parallel lines have b = 4 and -4, its Bbus row is exactly zero
    and so is its pivot wherever it is eliminated: ``pf_bad_pivot``'s zero, not the inf / NaN of x = 0."""
    buses, lines, gens, slack = (x.to(DEV) if torch.is_tensor(x) else x for x in wc.zero_pivot_batch())
    s = (buses, lines, gens, slack)
    keep = [0, 2]
    sub = (buses[keep], lines[keep], gens[keep], slack)
    E, Gn = lines.shape[1], gens.shape[1]
    res = dcpf._dc(s)
    assert res.converged.tolist() == [True, False, True] and bool((res.v == 1).all())
    for k in dcpf.OUTPUTS:
        assert bool(getattr(res, k)[1].isnan().all()) and bool(torch.isfinite(getattr(res, k)[keep]).all()), k
    alone = dcpf._dc(sub)
    for k in dcpf.FIELDS:
        assert _same(getattr(res, k)[keep], getattr(alone, k)), k
    dcpf._check_against_reference(alone, sub, 'zero pivot, grids 0 and 2')
    pickup = g1._pickup('random', 3, Gn)
    for what, call, check in (
            ('N-1', lambda s_, p: n1._screen(s_), lambda r: n1._check_values(r, sub, list(range(E)), 'zero pivot N-1')),
            ('N-2', lambda s_, p: n2._screen(s_, flows=True), lambda r: n2._check_values(r, sub, 'zero pivot N-2')),
            ('generator', lambda s_, p: g1._screen(s_, pickup=p, flows=True),
             lambda r: g1._check_values(r, sub, pickup[keep], 'zero pivot generator'))):
        full, part = call(s, pickup), call(sub, pickup[keep])
        _grid1_failed(full)
        for k in ROWS:
            assert _same(getattr(full, k)[keep], getattr(part, k)), (what, k)
        assert torch.equal(full.islanding, part.islanding) and bool(full.islanding.any()) == (what == 'N-2')   # two ring lines
        check(part)


def test_zero_pivot_gradients_nan_or_zero_in_that_grid_alone():
    """The three adjoints: grid 1 gets NaN rows for a non-zero incoming gradient and zero rows for an exactly zero one; grids 0 and
    2 keep the reference values, and their bits."""
    buses, lines, gens, slack = (x.to(DEV) if torch.is_tensor(x) else x for x in wc.zero_pivot_batch())
    s = (buses, lines, gens, slack)
    keep = [0, 2]
    N, E = buses.shape[1], lines.shape[1]

    def zero_grid1(weights):
        out = tuple(w.clone() for w in weights)
        for w in out:
            w[1] = 0.0
        return out

    def held(grads, zeroed):
        for g, z in zip(grads, zeroed):
            assert bool(g[1].isnan().all()) and bool(torch.isfinite(g[keep]).all())
            assert bool((z[1] == 0).all()) and _same(z[keep], g[keep])

    weights = dcpf._weights(3, N, E, 4)
    res, grads = dcpf._grads(buses, lines, gens, slack, weights)
    assert res.converged.tolist() == [True, False, True]
    dcpf._check_gradients(grads, buses, lines, gens, slack, weights, keep, 'zero pivot dc_power_flow')
    held(grads, dcpf._grads(buses, lines, gens, slack, zero_grid1(weights))[1])

    rating = n1g._rating(E, 5)
    weights = n1g._weights(3, E, E, 6)
    res, grads = n1g._grads(s, weights, rating=rating)
    _grid1_failed(res)
    n1g._check(grads, res, s, weights, rating, keep, 'zero pivot N-1')
    held(grads, n1g._grads(s, zero_grid1(weights), rating=rating)[1])

    pairs = powerflow._pair_list(None, E).tolist()
    weights = n2g._weights(3, len(pairs), E, 7)
    res, grads = n2g._grads(s, weights, pairs=pairs, rating=rating)
    _grid1_failed(res)
    n2g._check(grads, s, n2g._reference(s, pairs, weights, rating, keep), 'zero pivot N-2')
    held(grads, n2g._grads(s, zero_grid1(weights), pairs=pairs, rating=rating)[1])


# ---- constructed grids: an exactly zero denominator on a line that is no bridge

def _rows_but_the_singular(res, s, listed, failed, ref, name):
    """Rows ``failed`` (positions): NaN / NaN / -1 although islanding is False.  Every other row against ``ref(i, row)``, which is
    never asked for a failed row (its matrix is singular)."""
    buses, lines, gens = (t.cpu() for t in s[:3])
    assert bool(res.converged.all()), name
    flow, wl, wi, isl = res.line_flow.cpu(), res.worst_loading.cpu(), res.worst_line.cpu(), res.islanding.cpu()
    worst = 0.0
    for i in range(buses.shape[0]):
        for p, row in enumerate(listed):
            if p in failed:
                assert not bool(isl[p]), (name, row)
                assert bool(flow[i, p].isnan().all()) and bool(wl[i, p].isnan()) and int(wi[i, p]) == -1, (name, i, row)
                continue
            want = ref(buses[i], lines[i], gens[i], i, row)
            assert (want is None) == bool(isl[p]), (name, i, row)
            if want is None:
                assert bool(flow[i, p].isnan().all()) and bool(wl[i, p].isnan()) and int(wi[i, p]) == -1, (name, i, row)
                continue
            err, scale = float((flow[i, p] - want).abs().max()), max(1.0, float(want.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i, row, err, scale)
            assert bool(torch.isfinite(wl[i, p])) and int(wi[i, p]) >= 0
    print(f'{name}: {len(listed)} rows ({len(failed)} singular without a bridge), worst scaled error {worst:.3e}')


def test_zero_denominator_off_the_bridges_fails_its_rows_alone():
    """``dc_wide_cases.zero_den_batch``: a leaf on the slack by three parallel lines with b = 2, 4, -4.  The outage of the b = 2
    line leaves b = 0 at the leaf: z = 1/2 and den = 1 - 2 * 1/2 = 0 exactly while no line is a bridge, so the host's islanding flag
    is False and the row falls to the device's ``den != 0.0`` test, in the N-1 screen and in the generator screen's rows with that
    line.  The b = 4 line has den = -1 and the b = -4 line den = 3: ordinary rows.  N-2: the pairs of the b = 2 line with a line of
    the ring have a determinant of exactly 0 in the float64 replay of the row kernel's arithmetic on the host
    (``test_dc_wide_host.test_zero_denominator_grid_is_exact``: m11 = 0 and m12 = m21 = 0), so all of them are included and fail
    alone; its pairs with the b = 4 and b = -4 lines (det -2 and 2) and the pair (b = 4, b = -4), which leaves b = 2, are
    ordinary rows."""
    s = tuple(x.to(DEV) if torch.is_tensor(x) else x for x in wc.zero_den_batch())
    slack = s[3]
    E, Gn = s[1].shape[1], s[2].shape[1]
    A = wc.ZD_B2
    res = n1._screen(s)
    _base_meets_the_reference(res.base, s, 'zero den')
    assert not bool(res.islanding.any())
    asked = []

    def n1_ref(bus, line, gen, i, k):
        asked.append(k)
        return cref.outage_flows(bus, line, gen, slack, k)

    _rows_but_the_singular(res, s, list(range(E)), {A}, n1_ref, 'zero den N-1')
    assert A not in asked and len(asked) == 2 * (E - 1)
    for i in range(2):
        assert cref.dense_lodf(s[0][i].cpu(), s[1][i].cpu(), s[2][i].cpu(), slack, A)[1] == 0.0
    n1._check_summaries(s, None, res, 'zero den N-1')
    # the generator screen: the rows with that line
    for kind in g1.PICKUPS:
        pickup = g1._pickup(kind, 2, Gn)
        rows = powerflow._generator_contingency_list(None, Gn, E)
        res = g1._screen(s, pickup=pickup, flows=True)
        failed = {p for p, (g, k) in enumerate(rows.tolist()) if k == A}
        assert len(failed) == Gn
        _rows_but_the_singular(res, s, rows.tolist(), failed,
                               lambda bus, line, gen, i, row: gref.direct(bus, line, gen, slack, row[0], row[1],
                                                                          gref.weights(pickup, gen, i)), f'zero den generator {kind}')
        g1._check_summaries(s, None, pickup, res, 'zero den generator')
    # the N-2 screen: every pair
    pairs = powerflow._pair_list(None, E)
    failed = set(wc.zero_det_pairs())
    res = n2._screen(s, flows=True)
    assert len(failed) == E - 3 and not bool(res.islanding[sorted(failed)].any())
    _rows_but_the_singular(res, s, pairs.tolist(), failed,
                           lambda bus, line, gen, i, row: n2ref.pair_flows(bus, line, gen, slack, row[0], row[1]), 'zero den N-2')
    at = {tuple(p): i for i, p in enumerate(pairs.tolist())}
    for pair in (sorted((A, wc.ZD_B4)), sorted((A, wc.ZD_BM4)), sorted((wc.ZD_B4, wc.ZD_BM4))):
        assert bool(torch.isfinite(res.worst_loading[:, at[tuple(pair)]]).all())
    n2._check_summaries(s, None, res, 'zero den N-2')


def test_zero_denominator_gradients_skip_or_poison_the_failed_row():
    """A row that is not solved although it does not island: with an exactly zero incoming gradient it is skipped and the gradients
    are the reference's over the other rows; with a non-zero one the grid's three gradient rows are NaN, in that grid alone."""
    s = tuple(x.to(DEV) if torch.is_tensor(x) else x for x in wc.zero_den_batch())
    E = s[1].shape[1]
    A = wc.ZD_B2
    rating = n1g._rating(E, 3)
    # N-1
    kept = [k for k in range(E) if k != A]
    weights = n1g._weights(2, E, E, 9)
    weights[0][:, A] = 0.0
    weights[1][:, A] = 0.0
    everything = torch.ones(E, dtype=torch.bool, device=DEV)
    res, good = n1g._grads(s, weights, rating=rating, rows=everything)
    assert not bool(res.islanding.any()) and bool(res.worst_loading[:, A].isnan().all())
    fake = types.SimpleNamespace(outages=torch.tensor(kept), islanding=torch.zeros(len(kept), dtype=torch.bool))
    n1g._check(good, fake, s, tuple(w[:, kept] for w in weights), rating, range(2), 'zero den N-1 gradients')
    for poison in (0, 1):
        w = tuple(x.clone() for x in weights)
        w[poison][1, A] = 1.5
        _, g = n1g._grads(s, w, rating=rating, rows=everything)
        for x, y in zip(g, good):
            assert bool(x[1].isnan().all()) and _same(x[0], y[0])
    # N-2
    pairs = powerflow._pair_list(None, E).tolist()
    failed = wc.zero_det_pairs()
    live = [p for p in range(len(pairs)) if p not in failed]
    weights = n2g._weights(2, len(pairs), E, 10)
    weights[0][:, failed] = 0.0
    weights[1][:, failed] = 0.0
    res, good = n2g._grads(s, weights, pairs=pairs, rating=rating)                # reads ~islanding: the failed rows among them
    assert not bool(res.islanding[failed].any()) and bool(res.worst_loading[:, failed].isnan().all())
    n2g._check(good, s, n2g._reference(s, pairs, weights, rating, range(2), rows=live), 'zero den N-2 gradients')
    for poison in (0, 1):
        w = tuple(x.clone() for x in weights)
        w[poison][0, failed[2]] = -2.0
        _, g = n2g._grads(s, w, pairs=pairs, rating=rating)
        for x, y in zip(g, good):
            assert bool(x[0].isnan().all()) and _same(x[1], y[1])
