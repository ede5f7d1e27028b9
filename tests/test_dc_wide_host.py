"""CPU part of the DC family's tests in the 'wide' value regime (``dc_wide_cases``: taps 0.5 .. 1.5, shifts within +-30 degrees, one
line in eight with x < 0, so Bbus[r, r] is indefinite and denominators and 2x2 determinants take both signs): the probe of the two
float64 references on every wide set, the coverage the GPU tests rely on (from float64 factors, no device), the exactness claims of
the two constructed grids in numpy, and the kernels' algorithms replayed in numpy on the fast-decoupled blob (the blob's own factor
and solve programs, so the no-pivot elimination in the product's minimum-degree order) on wide sets and on the constructed grids.

Probe (``dense_lodf`` against ``outage_flows`` on every outage of both grids; ``dense_rank2`` against ``pair_flows`` on 60 seeded
pairs of grid 0), worst scaled difference, smallest |den| off the bridges, largest |flow|, islanding outages:
  complete20 1.1e-12 / 1.3e-13, 1.2e-2, 3.0e4, 0/190;      lattice8x8 4.7e-13 / 1.6e-13, 5.6e-4, 1.0e4, 0/112;
  random40_parallel_selfloop 2.5e-15 / 5.7e-15, 5.7e-2, 25, 7/63;  random97_parallel_selfloop 3.5e-14 / 2.5e-14, 3.6e-2, 95, 21/148;
  ring30_slack_no_gen (seed 1) 7.5e-15 / 2.0e-14, 1.2e-2, 11, 0/31;    random24_stacked_gens 5.3e-15 / 4.4e-15, 6.6e-2, 22, 5/38;
  wheel71 2.3e-13 / 7.7e-13, 3.5e-3, 1.8e3, 0/140;  pair, path65, star65_pv and hub150_70lines_70gens: every line is a bridge.
Every topology passes the 1e-10 probe; none is dropped.  On the N-2 lists the GPU test samples, which hold the pairs of smallest
and most negative determinant on purpose, the two references differ by at most 6.7e-11 (lattice8x8, pair (19, 45) of grid 0, det
-6.7e-6), 2.8e-11 (complete20), 2.1e-12 (wheel71).

Replay of the blob's programs in float64 against the direct references, worst scaled error: the base solve on all eleven sets
<= 1.0e-13 (hub150), its adjoint <= 5.6e-12; every N-1 outage of lattice8x8 and random24_stacked_gens 3.2e-12 and 1.3e-14; the N-2
and generator rows of random24_stacked_gens 2.4e-14 and 1.2e-14; the N-1 and N-2 adjoints of random24_stacked_gens within 1e-11 of
the references' autograd; the N-2 rows of the 300 pairs the GPU test samples on lattice8x8 5.8e-10 at pair (19, 45) of grid 0 and
7.2e-11 at the next row.  On the two constructed grids (both grids of the zero-denominator batch, grids 0 and 2 of the zero-pivot
batch) the replays of all three screens and of both screens' adjoints meet the bar on every row the references can be asked for,
and the rows with the singular line have a denominator or determinant of exactly 0.  The minimum-degree order without pivoting
keeps the digits on these indefinite matrices: no seed had to change on that ground.

``test_the_replay_with_the_sign_of_x_lost_misses_the_rows`` replays N-1 rows with b = 1 / (|x| tau): each of the first twelve rows
that do not island, on grid 0 of every set with such rows, leaves the bar, so the row comparisons notice a lost sign by themselves."""
import itertools

import numpy as np
import pytest
import torch

import dc_contingency_reference as cref
import dc_generator_contingency_reference as gref
import dc_n2_reference as n2ref
import dc_reference as dref
import dc_wide_cases as wc
from opf_graph_neural_solver_amd import powerflow
import dc_contingency_grad_reference as n1gref
import dc_n2_grad_reference as n2gref
import test_dc_contingency_host as n1h
import test_dcpf_host as dch
from test_dc_contingency_grad_host import _replay as _replay_n1_adjoint, emulate_screen_adjoint
from test_dc_contingency_host import _replay as _replay_n1, emulate_screen
from test_dc_n2_grad_host import _replay as _replay_n2_adjoint, emulate_n2_adjoint
from test_dc_generator_contingency_gpu import _family_rows, _pickup
from test_dc_generator_contingency_host import emulate_factor as gen_factor, emulate_row as gen_row
from test_dc_n2_host import emulate_factor, emulate_pair
from test_dcpf_host import _factor, emulate_adjoint, emulate_solve
from test_fdpf_host import FH, _arr

TOL = 1e-9
LIVE = tuple(n for n in wc.NAMES if n not in wc.ALL_BRIDGE)
ITEMS = ('x_neg', 'den_neg', 'worst_b_neg', 'worst_flow_neg')


def _fd(tp):
    return powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)


def _numpy(s, i):
    return tuple(x[i].double().numpy() for x in s[:3])


@pytest.mark.parametrize('name', wc.NAMES)
def test_the_two_references_agree_on_every_wide_set(name):
    worst, min_den, top, n_isl = wc.probe_n1(name)
    worst2 = wc.probe_n2(name)
    E = wc.topo(name).f.size
    print(f'{name}: N-1 {worst:.1e}, N-2 {worst2:.1e}, smallest |den| {min_den:.1e}, largest |flow| {top:.1e}, islanding {n_isl}/{E}')
    assert worst <= wc.PROBE_TOL and worst2 <= wc.PROBE_TOL
    assert (n_isl == E) == (name in wc.ALL_BRIDGE)


@pytest.mark.parametrize('name', ['lattice8x8', 'complete20', 'random40_parallel_selfloop', 'wheel71'])
def test_the_two_references_agree_on_the_selected_pairs(name):
    """The sampled N-2 lists hold the pairs of smallest and most negative determinant on purpose: the probe on exactly those rows."""
    buses, lines, gens, slack = wc.wide_set(name)
    worst, at = 0.0, None
    for i in range(2):
        for j, k in wc.n2_pairs(name).tolist():
            want = n2ref.pair_flows(buses[i], lines[i], gens[i], slack, j, k)
            if want is None:
                continue
            got, det = n2ref.dense_rank2(buses[i], lines[i], gens[i], slack, j, k)
            d = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
            if d > worst:
                worst, at = d, (i, j, k, det)
    print(f'{name}: worst scaled difference {worst:.1e} at (grid, j, k, det) {at}')
    assert worst <= wc.PROBE_TOL


@pytest.mark.parametrize('name', wc.NAMES)
def test_the_sets_are_wide(name):
    lines = wc.wide_set(name)[1]
    neg, pos, lo, hi, shift = wc.regime(lines)
    assert 0.5 <= lo and hi <= 1.5 and shift <= 30.0 and bool((lines[..., 3].abs() >= 0.04).all())
    assert neg and pos
    if name != 'pair':                                       # one line in two grids: two taps and two shifts in all
        assert lo < 0.6 and hi > 1.4 and shift > 20.0
    assert wc.SEEDS.get(name, 0) == {'pair': 3, 'ring30_slack_no_gen': 1}.get(name, 0)


@pytest.mark.parametrize('name', LIVE)
def test_coverage_of_the_compared_rows(name):
    """What the GPU tests assert again on their own rows: outaged lines with x < 0, negative denominators and determinants, a worst
    line with b < 0 and a negative worst flow, all from the float64 factors."""
    n1 = wc.n1_coverage(name)
    pairs = wc.n2_pairs(name)
    n2 = wc.n2_coverage(name, pairs)
    print(f'{name}: N-1 {n1}; N-2 {len(pairs)} pairs {n2}')
    assert len(pairs) <= 300 or name in ('random24_stacked_gens', 'ring30_slack_no_gen')
    for k in ITEMS:
        assert n1[k] >= 1 and n2[k] >= 1, (name, k)
    tp = wc.topo(name)
    listed = {tuple(p) for p in pairs.tolist()}
    assert all(tuple(sorted(p)) in listed for p in wc.parallel_pairs(tp))
    for loop in np.flatnonzero(tp.f == tp.t).tolist():
        assert sum(loop in p for p in listed) >= 8


@pytest.mark.parametrize('name', ['random24_stacked_gens', 'ring30_slack_no_gen', 'random40_parallel_selfloop', 'lattice8x8'])
def test_coverage_of_the_generator_rows(name):
    tp = wc.topo(name)
    s = wc.wide_set(name)
    rows = _family_rows(name, tp)
    for kind in (None, 'pmax', 'random'):
        pickup = _pickup(kind, 2, tp.g.size)
        ws = [gref.weights(pickup, s[2][i], i) for i in range(2)]
        cov = wc.gen_coverage(name, rows, [None if w is None else w.numpy() for w in ws])
        print(f'{name}, pickup {kind}: {cov}')
        for k in ITEMS:
            assert cov[k] >= 1, (name, kind, k)


# ---- the blob's own programs in float64 on the wide sets

@pytest.mark.parametrize('name', wc.NAMES)
def test_the_fd_blob_serves_the_dc_solve_and_its_adjoint_on_every_wide_set(name):
    tp = wc.topo(name)
    w = _fd(tp).host
    s = wc.wide_set(name)
    rng = np.random.default_rng(len(name))
    worst, worst_g = 0.0, 0.0
    for i in range(2):
        bus, line, gen = _numpy(s, i)
        got = emulate_solve(w, bus, line, gen)
        want = dref.dc_power_flow(bus, line, gen, tp.slack)
        for x, y in zip(got, want):
            y = np.asarray(y)
            err, scale = float(np.max(np.abs(x - y))), max(1.0, float(np.max(np.abs(y))))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (name, i)
        gth, gfl, gsp = rng.standard_normal(tp.n), rng.standard_normal(tp.f.size), float(rng.standard_normal())
        ga = emulate_adjoint(w, bus, line, gen, got[0], gth, gfl, gsp)
        gr = dref.gradients(bus, line, gen, tp.slack, gth, gfl, gsp)
        for x, y in zip(ga, gr):
            y = y.numpy()
            err, scale = float(np.max(np.abs(x - y))), max(1.0, float(np.max(np.abs(y))))
            worst_g = max(worst_g, err / scale)
            assert err <= TOL * scale, (name, i)
    print(f'{name}: base solve {worst:.1e}, adjoint {worst_g:.1e}')


@pytest.mark.parametrize('name', ['lattice8x8', 'random24_stacked_gens'])
def test_the_fd_blob_serves_the_n1_screen_on_wide_sets(name):
    tp = wc.topo(name)
    s = wc.wide_set(name)
    _replay_n1(tp, *s[:3], list(range(tp.f.size)), name)


def test_the_fd_blob_serves_the_n1_adjoint_on_a_wide_set():
    tp = wc.topo('random24_stacked_gens')
    s = wc.wide_set('random24_stacked_gens')
    _replay_n1_adjoint(tp, *s[:3], 'random24_stacked_gens wide')


def test_the_fd_blob_serves_the_n2_adjoint_on_a_wide_set():
    """Every non-islanding pair of random24_stacked_gens wide (518 of 703), a rating, both incoming gradients."""
    tp = wc.topo('random24_stacked_gens')
    s = wc.wide_set('random24_stacked_gens')
    _replay_n2_adjoint(tp, s[0][:1], s[1][:1], s[2][:1], 'random24_stacked_gens wide')


def test_the_fd_blob_serves_the_n2_screen_on_the_selected_pairs_of_lattice8x8():
    """The pair kernel's arithmetic on the 300 pairs the GPU test samples, the ones of smallest and most negative determinant among
    them: pair (19, 45) of grid 0 (det -6.7e-6, flows of 2.9e5) is the tightest row of the whole file, 5.8e-10 here and 4.7e-10 on
    the device against the bar's 1e-9; the next row is 7.2e-11."""
    name = 'lattice8x8'
    tp = wc.topo(name)
    s = wc.wide_set(name)
    E = tp.f.size
    w = _fd(tp).host
    pairs = wc.n2_pairs(name)
    assert [19, 45] in pairs.tolist() and not powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs).any()
    errs = []
    for i in range(2):
        bus, line, gen = _numpy(s, i)
        H, F, b = emulate_factor(w, bus, line, gen, list(range(E)))
        for j, k in pairs.tolist():
            want = n2ref.pair_flows(bus, line, gen, tp.slack, j, k).numpy()
            got, det = emulate_pair(H, F, b, np.arange(E), j, k)
            err, scale = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
            errs.append((err / scale, i, j, k, det))
            assert err <= TOL * scale, (i, j, k, err, scale, det)
    errs.sort(reverse=True)
    print(f'{name}: {len(errs)} rows, the two worst (scaled error, grid, j, k, det): {errs[0]}, {errs[1]}')
    assert errs[0][1:4] == (0, 19, 45) and errs[0][4] < 0 and abs(errs[0][4]) < 1e-5


@pytest.mark.parametrize('name', LIVE)
def test_the_replay_with_the_sign_of_x_lost_misses_the_rows(name, monkeypatch):
    """The row comparison notices a lost sign by itself, not only through the base case: the N-1 replay with b = 1 / (|x| tau) in
    place of ``_line_b`` is off the bar on every set with rows to compare, in rows whose base flows are not looked at."""
    def abs_b(line):
        return 1.0 / (np.abs(line[:, 3]) * line[:, 5])

    tp = wc.topo(name)
    s = wc.wide_set(name)
    w = _fd(tp).host
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    outages = np.flatnonzero(~bridges)[:12].tolist()
    bus, line, gen = _numpy(s, 0)
    right = emulate_screen(w, bus, line, gen, outages, bridges)
    monkeypatch.setattr(dch, '_line_b', abs_b)
    monkeypatch.setattr(n1h, '_line_b', abs_b)
    wrong = emulate_screen(w, bus, line, gen, outages, bridges)
    missed = 0
    for j, k in enumerate(outages):
        want = cref.outage_flows(bus, line, gen, tp.slack, k).numpy()
        scale = max(1.0, float(np.max(np.abs(want))))
        assert np.max(np.abs(right[j] - want)) <= TOL * scale
        missed += bool(np.max(np.abs(wrong[j] - want)) > TOL * scale)
    assert missed == len(outages), (name, missed)


def test_the_fd_blob_serves_the_n2_and_generator_screens_on_a_wide_set():
    name = 'random24_stacked_gens'
    tp = wc.topo(name)
    s = wc.wide_set(name)
    E, Gn = tp.f.size, tp.g.size
    w = _fd(tp).host
    pairs = powerflow._pair_list(None, E)[::3]
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    rows = powerflow._generator_contingency_list(None, Gn, E)[::2]
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    worst2, worstg, neg = 0.0, 0.0, 0
    for i in range(2):
        bus, line, gen = _numpy(s, i)
        H, F, b = emulate_factor(w, bus, line, gen, list(range(E)))
        for p, (j, k) in enumerate(pairs.tolist()):
            want = n2ref.pair_flows(bus, line, gen, tp.slack, j, k)
            assert (want is None) == bool(isl[p])
            if want is None:
                continue
            got, det = emulate_pair(H, F, b, np.arange(E), j, k)
            neg += det < 0
            err, scale = float(np.max(np.abs(got - want.numpy()))), max(1.0, float(want.abs().max()))
            worst2 = max(worst2, err / scale)
            assert err <= TOL * scale, (i, j, k, err, scale)
        wi = gref.weights('pmax', gen)
        H, D, F, b = gen_factor(w, bus, line, gen, list(range(E)), list(range(Gn)), wi.numpy())
        for g, k in rows.tolist():
            want = gref.direct(bus, line, gen, tp.slack, g, k, wi)
            assert (want is None) == (k >= 0 and bool(bridges[k]))
            if want is None:
                continue
            got, _ = gen_row(H, D, F, b, list(range(E)), g, k)
            err, scale = float(np.max(np.abs(got - want.numpy()))), max(1.0, float(want.abs().max()))
            worstg = max(worstg, err / scale)
            assert err <= TOL * scale, (i, g, k, err, scale)
    print(f'{name}: N-2 {worst2:.1e} ({neg} rows with det < 0), generator rows {worstg:.1e}')
    assert neg >= 1


# ---- the constructed grids: exact zeros

def _bbus(line, n):
    return dref.make_bdc(torch.as_tensor(line, dtype=torch.float64), n)[0].numpy()


@pytest.mark.filterwarnings('ignore::RuntimeWarning')         # 0 / 0 in the replayed factor program is the point
def test_zero_pivot_grid_is_exact():
    tp = wc.ZP_TOPO
    buses, lines, gens, slack = wc.zero_pivot_batch()
    assert lines[:, wc.ZP_PAIR[1], 3].tolist() == [0.25, -0.25, 0.5] and lines[:, wc.ZP_PAIR[0], 3].tolist() == [0.25] * 3
    assert not powerflow._bridges(tp.n, tp.f - 1, tp.t - 1).any()            # the graph is connected whatever the values
    w = _fd(tp).host
    piv = _arr(w, 'PIVOT1', w[FH['DIM1']])
    leaf = wc.ZP_LEAF - 1
    for i in range(3):
        bus, line, gen = _numpy((buses, lines, gens), i)
        B = _bbus(line, tp.n)
        b = 1.0 / (line[:, 3] * line[:, 5])
        assert all(float(v).is_integer() and abs(v) <= 8 for v in b)         # small integers: every sum below is exact
        F, nnz1 = _factor(w, line)
        if i != 1:
            assert np.all(np.isfinite(F[piv])) and np.all(F[piv] != 0.0)
            assert B[leaf, leaf] == {0: 8.0, 2: 6.0}[i]
            continue
        assert np.all(B[leaf] == 0.0) and np.all(B[:, leaf] == 0.0)          # 4 - 4 and -4 + 4, in either order
        assert b[wc.ZP_PAIR[0]] + b[wc.ZP_PAIR[1]] == 0.0 == b[wc.ZP_PAIR[1]] + b[wc.ZP_PAIR[0]]
        assert int(np.sum(F[piv] == 0.0)) == 1                               # the blob's own factor program: one pivot, exactly 0
        # and a dense elimination without pivoting in any order of the five non-slack buses meets an exact zero at the leaf
        keep = [k for k in range(tp.n) if k != slack - 1]
        for order in itertools.permutations(keep):
            A = B[np.ix_(order, order)].copy()
            at = order.index(leaf)
            for k in range(at):
                A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / A[k, k]
            assert A[at, at] == 0.0, order


@pytest.mark.filterwarnings('ignore::RuntimeWarning')         # x / 0 in the replayed pair arithmetic is the point
def test_zero_denominator_grid_is_exact():
    tp = wc.ZD_TOPO
    buses, lines, gens, slack = wc.zero_den_batch()
    E = tp.f.size
    A_, B_, C_ = wc.ZD_B2, wc.ZD_B4, wc.ZD_BM4
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    assert not bridges.any()                                                 # islanding is False for every outage
    assert {tp.f[e] + tp.t[e] for e in (A_, B_, C_)} == {wc.ZD_LEAF + slack} and len({(tp.f[e], tp.t[e]) for e in (A_, B_, C_)}) == 2
    w = _fd(tp).host
    leaf = wc.ZD_LEAF - 1
    every = powerflow._pair_list(None, E)
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, every)
    zero_det = []
    for i in range(2):
        bus, line, gen = _numpy((buses, lines, gens), i)
        b = 1.0 / (line[:, 3] * line[:, 5])
        assert (b[A_], b[B_], b[C_]) == (2.0, 4.0, -4.0)
        for order in itertools.permutations((A_, B_, C_)):                   # the leaf's block of B' is [2] in any order of the sum
            assert sum(b[e] for e in order) == 2.0
        Bm = _bbus(line, tp.n)
        assert Bm[leaf, leaf] == 2.0 and np.count_nonzero(np.delete(Bm[leaf], [leaf, slack - 1])) == 0
        H, F, _ = emulate_factor(w, bus, line, gen, list(range(E)))          # the blob's solve program, a lane per line
        den = 1.0 - b * np.diag(H)
        assert H[A_, A_] == 0.5 and den[A_] == 0.0 and den[B_] == -1.0 and den[C_] == 3.0
        assert F[A_] != 0.0                                                  # alpha = F_k / 0 is +-inf, not 0 / 0
        assert cref.dense_lodf(bus, line, gen, slack, A_)[1] == 0.0          # the second reference sees the exact zero too
        for k in range(E):
            if k == A_:
                continue                                                     # the direct reference is not asked: its matrix is singular
            want = cref.outage_flows(bus, line, gen, slack, k).numpy()
            got = F + b * H[k] * (F[k] / den[k])
            got[k] = 0.0
            assert np.max(np.abs(got - want)) <= TOL * max(1.0, np.max(np.abs(want))), (i, k)
        dets = np.array([emulate_pair(H, F, b, np.arange(E), j, k)[1] if A_ in (j, k) else np.nan for j, k in every.tolist()])
        zero_det.append(set(np.flatnonzero(dets == 0.0).tolist()))
        for other, want in ((B_, -2.0), (C_, 2.0)):
            assert emulate_pair(H, F, b, np.arange(E), A_, other)[1] == want
        assert emulate_pair(H, F, b, np.arange(E), B_, C_)[1] == 1.0         # the pair that leaves b = 2: an ordinary row
    # the pairs of the b = 2 line with a line of the ring: not islanding, determinant exactly 0 in the row kernel's arithmetic
    ring = [p for p, (j, k) in enumerate(every.tolist()) if A_ in (j, k) and not {j, k} & {B_, C_}]
    assert zero_det[0] == zero_det[1] == set(ring) == set(wc.zero_det_pairs()) and len(ring) == E - 3 and not isl[ring].any()


# ---- the screens' and adjoints' replays on the constructed grids

def _close_columns(got, want, what):
    for x, y, name in zip(got, want, ('buses', 'lines', 'generators')):
        y = y.numpy()
        for c in range(y.shape[1]):
            if c not in {'buses': (2, 4), 'lines': (3, 5, 6), 'generators': (6,)}[name]:
                assert np.all(x[:, c] == 0.0) and np.all(y[:, c] == 0.0), (what, name, c)
                continue
            err, scale = float(np.max(np.abs(x[:, c] - y[:, c]))), max(1.0, float(np.max(np.abs(y[:, c]))))
            assert err <= TOL * scale, (what, name, c, err, scale)


def _replay_everything(tp, s, grids, singular, name):
    """The replays of the N-1 screen, the N-2 screen, the generator screen and the two screens' adjoints on the grids ``grids`` of
    ``s``, every row but the ones that hold the line ``singular`` (None: every row) against the direct references; the rows with
    that line have a denominator or determinant of exactly 0 in the replay and the references are not asked for them."""
    E, Gn = tp.f.size, tp.g.size
    w = _fd(tp).host
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    outages = [k for k in range(E) if k != singular]
    every = powerflow._pair_list(None, E)
    dead = set(wc.zero_det_pairs()) if singular is not None else set()
    pairs = every[[p for p in range(every.shape[0]) if p not in dead]]
    isl = powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    rows = powerflow._generator_contingency_list(None, Gn, E)
    sub = tuple(x[grids] for x in s[:3])
    _replay_n1(tp, *sub, outages, name)                                       # emulate_screen against outage_flows
    rng = np.random.default_rng(E)
    for i in grids:
        bus, line, gen = _numpy(s, i)
        if singular is not None:
            assert not np.isfinite(np.delete(emulate_screen(w, bus, line, gen, [singular], bridges)[0], singular)).any()
        H, F, b = emulate_factor(w, bus, line, gen, list(range(E)))
        for p, (j, k) in enumerate(pairs.tolist()):
            want = n2ref.pair_flows(bus, line, gen, tp.slack, j, k)
            assert (want is None) == bool(isl[p]), (name, i, j, k)
            if want is not None:
                got, det = emulate_pair(H, F, b, np.arange(E), j, k)
                assert det != 0.0 and np.max(np.abs(got - want.numpy())) <= TOL * max(1.0, float(want.abs().max())), (name, i, j, k)
        for kind in (None, 'pmax'):
            wi = gref.weights(kind, gen)
            H, D, F, b = gen_factor(w, bus, line, gen, list(range(E)), list(range(Gn)), None if wi is None else wi.numpy())
            for g, k in rows.tolist():
                got, den = gen_row(H, D, F, b, list(range(E)), g, k)
                if k == singular:
                    assert den == 0.0 and not np.isfinite(np.delete(got, k)).any(), (name, i, g, k)
                    continue
                want = gref.direct(bus, line, gen, tp.slack, g, k, wi).numpy()
                assert den != 0.0 and np.max(np.abs(got - want)) <= TOL * max(1.0, np.max(np.abs(want))), (name, i, g, k)
        rating = 0.5 + 2.0 * rng.random(E)
        w_flow, w_worst = rng.standard_normal((len(outages), E)), rng.standard_normal(len(outages))
        got = emulate_screen_adjoint(w, bus, line, gen, outages, bridges, w_flow, w_worst, rating)
        want, flows = n1gref.gradients(bus, line, gen, tp.slack, outages, w_flow, w_worst, rating)
        assert not np.isnan(flows.numpy()).any()
        _close_columns(got, want, (name, i, 'N-1 adjoint'))
        w_flow, w_worst = rng.standard_normal((pairs.shape[0], E)), rng.standard_normal(pairs.shape[0])
        got = emulate_n2_adjoint(w, bus, line, gen, pairs, isl, w_flow, w_worst, rating)
        want, flows = n2gref.gradients(bus, line, gen, tp.slack, pairs.tolist(), w_flow, w_worst, rating)
        assert np.array_equal(np.isnan(flows.numpy()).all(axis=1), isl)
        _close_columns(got, want, (name, i, 'N-2 adjoint'))


@pytest.mark.filterwarnings('ignore::RuntimeWarning')         # x / 0 in the singular rows is the point
def test_the_fd_blob_serves_every_screen_and_adjoint_on_the_zero_denominator_grid():
    _replay_everything(wc.ZD_TOPO, wc.zero_den_batch(), [0, 1], wc.ZD_B2, 'zero denominator grid')


def test_the_fd_blob_serves_every_screen_and_adjoint_on_grids_0_and_2_of_the_zero_pivot_batch():
    _replay_everything(wc.ZP_TOPO, wc.zero_pivot_batch(), [0, 2], None, 'zero pivot batch, grids 0 and 2')
