"""What the host and GPU tests of the DC family in the 'wide' value regime share (no device needed): the wide sets, the float64
factors every coverage count and row selection is taken from, the probe of the two references, and two constructed grids whose
small-integer susceptances make a pivot and a denominator exactly zero in any elimination order.

Wide sets: ``pf_topologies.grids(tp, 'wide', 2, seed)`` as drawn, with no ``_perturbed`` on top (it would redraw taps into
[0.85, 1.15]): taps 0.5 .. 1.5, shifts within +-30 degrees, about one line in eight with x in [-0.3, -0.05].  Every topology uses
seed 0 but two.  pair uses seed 3, the first whose one line has x > 0 in one grid and x < 0 in the other (seed 0: 0.14 and 0.06, so
nothing on it would tell x from |x|).  ring30_slack_no_gen uses seed 1: on its seed-0 grids no compared row of the N-1, N-2 or generator screen has
its worst line on a line with b < 0 (0 of 62, 508 and 192 rows; seed 1: 14, 117 and 47).  Both seeds were chosen on the CPU from the
float64 ``Factors`` below, before any device run."""
import functools

import numpy as np
import torch

import dc_contingency_reference as cref
import dc_n2_reference as n2ref
import dc_reference as dref
import pf_topologies as pt
from opf_graph_neural_solver_amd import powerflow

NAMES = ('pair', 'path65', 'star65_pv', 'lattice8x8', 'complete20', 'random40_parallel_selfloop', 'random97_parallel_selfloop',
         'ring30_slack_no_gen', 'random24_stacked_gens', 'hub150_70lines_70gens', 'wheel71')
ALL_BRIDGE = ('pair', 'path65', 'star65_pv', 'hub150_70lines_70gens')
SEEDS = {'pair': 3, 'ring30_slack_no_gen': 1}       # name -> seed where seed 0 lacks a coverage item (see above)
PROBE_TOL = 1e-10


def topo(name):
    return pt.wheel(71) if name == 'wheel71' else pt.families()[name]


@functools.lru_cache(maxsize=None)
def _cpu_set(name):
    tp = topo(name)
    buses, lines, gens, _, _ = pt.grids(tp, 'wide', 2, SEEDS.get(name, 0))
    return buses, lines, gens, tp.slack


def wide_set(name, device='cpu'):
    """(buses, lines, generators, slack) float32: two 'wide' grids on the topology, as drawn."""
    s = _cpu_set(name)
    return tuple(t.to(device) for t in s[:3]) + (s[3],)


def regime(lines):
    """(x < 0 somewhere, x > 0 somewhere, smallest tau, largest tau, largest |shift| in degrees) of a line tensor."""
    x, tau, sh = lines[..., 3], lines[..., 5], lines[..., 6]
    return bool((x < 0).any()), bool((x > 0).any()), float(tau.min()), float(tau.max()), float(sh.abs().max()) * 180 / np.pi


# ---- float64 factors of one grid: the dense inverse of Bbus[r, r] and everything the rank-1 and rank-2 formulas need

class Factors:
    """b [E], base flow F [E], H [E,E] with H[c, l] = z_c[f_l] - z_c[t_l] (A z_c = m_c, dense float64), den [E] = 1 - b_k H[k,k]."""

    def __init__(self, bus, line, gen, slack):
        bus, line, gen = (torch.as_tensor(x, dtype=torch.float64) for x in (bus, line, gen))
        n, E = bus.shape[0], line.shape[0]
        keep = [i for i in range(n) if i != slack - 1]
        Bbus, b, _, _ = dref.make_bdc(line, n)
        _, flow, _ = dref.dc_power_flow(bus, line, gen, slack)
        f, t = line[:, 0].long().numpy() - 1, line[:, 1].long().numpy() - 1
        M = np.zeros((n, E))
        M[f, np.arange(E)] += 1.0
        M[t, np.arange(E)] -= 1.0
        self.Ainv = np.zeros((n, n))                               # the inverse of Bbus[r, r], zero in the slack's row and column
        if keep:
            self.Ainv[np.ix_(keep, keep)] = np.linalg.inv(Bbus.numpy()[np.ix_(keep, keep)])
        self.M, self.gen_bus, self.pg, self.pmax = M, gen[:, 0].long().numpy() - 1, gen[:, 6].numpy(), gen[:, 1].numpy()
        self.b, self.F, self.x = b.numpy(), flow.numpy(), line[:, 3].numpy()
        self.H = M.T @ self.Ainv @ M                               # H[c, l], symmetric
        self.den = 1.0 - self.b * np.diag(self.H)

    def n1_rows(self, outages):
        """Post-outage flows [K, E] by the rank-1 formula (rows of a zero denominator are inf / NaN)."""
        k = np.asarray(outages)
        with np.errstate(divide='ignore', invalid='ignore'):
            out = self.F + self.b * self.H[k] * (self.F[k] / self.den[k])[:, None]
        out[np.arange(k.size), k] = 0.0
        return out

    def gen_rows(self, rows, w=None):
        """Post-outage flows [R, E] of the rows (generator, line or -1) with pickup weights ``w`` [Gn] or None, and den [R] (1
        without a line): the generator's Pg shared out, then the rank-1 formula."""
        rows = np.asarray(rows)
        out, den = np.zeros((rows.shape[0], self.b.size)), np.ones(rows.shape[0])
        for r, (g, k) in enumerate(rows.tolist()):
            dP = np.zeros(self.Ainv.shape[0])
            dP[self.gen_bus[g]] -= self.pg[g]
            if w is not None:
                others = [h for h in range(self.pg.size) if h != g]
                total = float(sum(w[h] for h in others))
                if total > 0.0:
                    for h in others:
                        dP[self.gen_bus[h]] += self.pg[g] * (w[h] / total)
            fg = self.F + self.b * (self.M.T @ (self.Ainv @ dP))
            if k >= 0:
                den[r] = self.den[k]
                with np.errstate(divide='ignore', invalid='ignore'):
                    fg = fg + self.b * self.H[k] * (fg[k] / self.den[k])
                fg[k] = 0.0
            out[r] = fg
        return out, den

    def det(self, pairs):
        j, k = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
        m11, m12 = 1.0 - self.b[j] * self.H[j, j], -self.b[j] * self.H[k, j]
        m21, m22 = -self.b[k] * self.H[j, k], 1.0 - self.b[k] * self.H[k, k]
        return m11 * m22 - m12 * m21

    def n2_rows(self, pairs):
        """Post-outage flows [P, E] by the rank-2 formulas of include/gns_powerflow.h."""
        j, k = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
        m11, m12 = 1.0 - self.b[j] * self.H[j, j], -self.b[j] * self.H[k, j]
        m21, m22 = -self.b[k] * self.H[j, k], 1.0 - self.b[k] * self.H[k, k]
        det = m11 * m22 - m12 * m21
        with np.errstate(divide='ignore', invalid='ignore'):
            aj, ak = (self.F[j] * m22 - m12 * self.F[k]) / det, (m11 * self.F[k] - m21 * self.F[j]) / det
            out = self.F + self.b * (self.H[j] * aj[:, None] + self.H[k] * ak[:, None])
        out[np.arange(j.size), j] = 0.0
        out[np.arange(j.size), k] = 0.0
        return out


@functools.lru_cache(maxsize=None)
def factors(name):
    """The two grids' ``Factors`` of a wide set."""
    buses, lines, gens, slack = _cpu_set(name)
    return tuple(Factors(buses[i], lines[i], gens[i], slack) for i in range(buses.shape[0]))


def row_coverage(fac, flows, outaged, live, den=None, rating=None):
    """Counts over the compared (grid, row)s, from float64 factors alone: rows with an outaged line of x < 0, rows with a negative
    denominator (``den`` [Bt, R]: den of N-1, det of N-2), rows whose worst line has b < 0, rows whose worst flow is negative.
    ``flows`` [Bt, R, E] float64 reference rows, ``outaged`` [R, 1 or 2] line indices (-1: none), ``live`` bool [R].  The worst
    line is the one of largest |flow| / rating (``rating`` None, [E] or [Bt, E]): the line ``sign(F') / rating`` acts on."""
    rating = None if rating is None else np.asarray(rating, dtype=np.float64)
    out = {'x_neg': 0, 'den_neg': 0, 'worst_b_neg': 0, 'worst_flow_neg': 0, 'rows': 0}
    outaged = np.asarray(outaged).reshape(len(live), -1)
    for i, fc in enumerate(fac):
        for r in np.flatnonzero(live):
            ks = [k for k in outaged[r] if k >= 0]
            row = flows[i][r]
            at = int(np.argmax(np.abs(row) if rating is None else np.abs(row) / (rating if rating.ndim == 1 else rating[i])))
            out['rows'] += 1
            out['x_neg'] += int(any(fc.x[k] < 0 for k in ks))
            out['den_neg'] += int(den is not None and den[i][r] < 0)
            out['worst_b_neg'] += int(fc.b[at] < 0)
            out['worst_flow_neg'] += int(row[at] < 0)
    return out


def n1_coverage(name, outages=None, rating=None):
    tp = topo(name)
    fac = factors(name)
    outages = list(range(tp.f.size)) if outages is None else list(outages)
    live = ~powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)[outages]
    return row_coverage(fac, [fc.n1_rows(outages) for fc in fac], np.asarray(outages), live, [fc.den[outages] for fc in fac], rating)


def n2_coverage(name, pairs, rating=None):
    tp = topo(name)
    fac = factors(name)
    pairs = np.asarray(pairs)
    live = ~powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, pairs)
    return row_coverage(fac, [fc.n2_rows(pairs) for fc in fac], pairs, live, [fc.det(pairs) for fc in fac], rating)


def gen_coverage(name, rows, weights):
    """``row_coverage`` of generator rows [R,2]; ``weights``: per grid, the float64 pickup weights [Gn] or None."""
    tp = topo(name)
    fac = factors(name)
    rows = np.asarray(rows)
    live = ~powerflow._generator_islanding(powerflow._bridges(tp.n, tp.f - 1, tp.t - 1), rows)
    got = [fc.gen_rows(rows[live], w) for fc, w in zip(fac, weights)]
    flows, den = [], []
    for fl, dn in got:
        full, dfull = np.zeros((rows.shape[0], tp.f.size)), np.ones(rows.shape[0])
        full[live], dfull[live] = fl, dn
        flows.append(full), den.append(dfull)
    return row_coverage(fac, flows, rows[:, 1:], live, den)


def parallel_pairs(tp):
    """Every pair of lines that join the same two buses."""
    ends = {}
    for e, (a, b) in enumerate(zip(tp.f.tolist(), tp.t.tolist())):
        if a != b:
            ends.setdefault((min(a, b), max(a, b)), []).append(e)
    return [[v[i], v[j]] for v in ends.values() for i in range(len(v)) for j in range(i + 1, len(v))]


def n2_pairs(name, most=300, extreme=12, loops=8):
    """The pairs of a wide set that go to the reference, in the default list's order: every pair when there are at most ``most``
    (and on the two families whose every pair the tests ask for), else a seeded sample filled up to ``most`` after the pairs that
    must be there: the pairs of parallel lines, the self-loop with the first ``loops`` lines that are not bridges, and the
    ``extreme`` live pairs of smallest |det| and of most negative det (the float64 ``Factors``, the smaller over the two grids)."""
    tp = topo(name)
    E = tp.f.size
    every = powerflow._pair_list(None, E)
    if every.shape[0] <= most or name in ('random24_stacked_gens', 'ring30_slack_no_gen'):
        return every
    live = ~powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, every)
    det = np.stack([fc.det(every) for fc in factors(name)])
    must = {tuple(sorted(p)) for p in parallel_pairs(tp)}
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    for loop in np.flatnonzero(tp.f == tp.t).tolist():
        must |= {tuple(sorted((loop, e))) for e in [e for e in range(E) if e != loop and not bridges[e]][:loops]}
    at = np.flatnonzero(live)
    must |= {tuple(every[p]) for p in at[np.argsort(np.abs(det[:, at]).min(axis=0))[:extreme]]}
    must |= {tuple(every[p]) for p in at[np.argsort(det[:, at].min(axis=0))[:extreme]]}
    pos = {tuple(p): i for i, p in enumerate(every.tolist())}
    pick = {pos[p] for p in must}
    rest = [i for i in np.random.default_rng(len(name)).permutation(every.shape[0]).tolist() if i not in pick]
    pick |= set(rest[:most - len(pick)])
    return every[sorted(pick)]


def n2_grad_pairs(name, most=120, extreme=10):
    """At most ``most`` live pairs for the N-2 gradients: every live pair when they fit, else the parallel and self-loop pairs that
    are live, the ``extreme`` pairs of smallest |det| and of most negative det, and a seeded sample."""
    tp = topo(name)
    every = n2_pairs(name, most=10 ** 9)
    live = every[~powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, every)]
    if live.shape[0] <= most:
        return live.tolist()
    det = np.stack([fc.det(live) for fc in factors(name)])
    pick = set(np.argsort(np.abs(det).min(axis=0))[:extreme].tolist()) | set(np.argsort(det.min(axis=0))[:extreme].tolist())
    rest = [i for i in np.random.default_rng(len(name)).permutation(live.shape[0]).tolist() if i not in pick]
    pick |= set(rest[:most - len(pick)])
    return live[sorted(pick)].tolist()


# ---- the probe: a topology is held to the bar only if the two float64 references agree on it

def probe_n1(name):
    """(worst scaled difference of ``dense_lodf`` and ``outage_flows`` over every outage of both grids, smallest |den| off the
    bridges, largest |flow|, islanding outages)."""
    buses, lines, gens, slack = _cpu_set(name)
    worst, min_den, top, n_isl = 0.0, np.inf, 0.0, 0
    for i in range(buses.shape[0]):
        for k in range(lines.shape[1]):
            want = cref.outage_flows(buses[i], lines[i], gens[i], slack, k)
            if want is None:
                n_isl += i == 0
                continue
            got, den = cref.dense_lodf(buses[i], lines[i], gens[i], slack, k)
            scale = max(1.0, float(want.abs().max()))
            worst, min_den, top = max(worst, float((got - want).abs().max()) / scale), min(min_den, abs(den)), max(top, scale)
    return worst, min_den, top, n_isl


def probe_n2(name, count=60):
    """Worst scaled difference of ``dense_rank2`` and ``pair_flows`` over ``count`` seeded pairs of grid 0 (every pair when fewer)."""
    buses, lines, gens, slack = _cpu_set(name)
    E = lines.shape[1]
    if E < 2:
        return 0.0
    every = powerflow._pair_list(None, E)
    at = np.random.default_rng(E).permutation(every.shape[0])[:count]
    worst = 0.0
    for j, k in every[np.sort(at)].tolist():
        want = n2ref.pair_flows(buses[0], lines[0], gens[0], slack, j, k)
        if want is None:
            continue
        got, _ = n2ref.dense_rank2(buses[0], lines[0], gens[0], slack, j, k)
        worst = max(worst, float((got - want).abs().max()) / max(1.0, float(want.abs().max())))
    return worst


# ---- constructed grids: small-integer susceptances (x a power of two, tau = 1), so sums and pivots are exact in float64

def _grid_tensors(n, f, t, x, shift, pd, g_bus, pg):
    """float32 (buses [Bt,n,6], lines [Bt,E,7], generators [Bt,Gn,7]) in the layout of ``pf_topologies.grids``."""
    x, shift, pd, pg = (np.asarray(a, dtype=np.float64) for a in (x, shift, pd, pg))
    Bt, E, Gn = x.shape[0], len(f), len(g_bus)
    buses, lines, gens = np.zeros((Bt, n, 6)), np.zeros((Bt, E, 7)), np.zeros((Bt, Gn, 7))
    buses[..., 0], buses[..., 1], buses[..., 2] = np.arange(1, n + 1), 1.0, pd
    lines[..., 0], lines[..., 1], lines[..., 3], lines[..., 5], lines[..., 6] = f, t, x, 1.0, shift
    gens[..., 0], gens[..., 1], gens[..., 4], gens[..., 3], gens[..., 6] = g_bus, 3.0, 1.0, pg, pg
    return tuple(torch.as_tensor(a, dtype=torch.float32) for a in (buses, lines, gens))


ZP_TOPO = pt.Topo('ring5_chord_leaf_two_parallel', 6, *(np.asarray(a, dtype=np.int64) for a in (
    [1, 2, 3, 4, 5, 2, 3, 6], [2, 3, 4, 5, 1, 5, 6, 3], [1, 4, 6])), 1)
ZP_LEAF, ZP_PAIR = 6, (6, 7)             # the leaf bus (1-based); its two parallel lines, the second listed the other way round


def zero_pivot_batch():
    """(buses, lines, gens, slack) of three grids on ``ZP_TOPO``: the leaf's two lines have x = 0.25 and, in grids 0, 1, 2,
    x = 0.25, -0.25, 0.5.  In grid 1 the leaf's Bbus row is 4 - 4 = 0 and -4 + 4 = 0: the pivot is exactly 0 wherever the leaf is
    eliminated (no update reaches a row whose off-diagonals are zero)."""
    rng = np.random.default_rng(61)
    x = rng.choice([0.125, 0.25, 0.5, 1.0], (3, 8))
    x[:, 6] = 0.25
    x[:, 7] = [0.25, -0.25, 0.5]
    shift = rng.integers(-4, 5, (3, 8)) / 64.0
    shift[:, 6:] = 0.0
    pd = rng.integers(0, 9, (3, 6)) / 8.0
    pg = rng.integers(1, 9, (3, 3)) / 4.0
    return _grid_tensors(6, ZP_TOPO.f, ZP_TOPO.t, x, shift, pd, ZP_TOPO.g, pg) + (ZP_TOPO.slack,)


ZD_TOPO = pt.Topo('ring5_chord_leaf_three_parallel_at_slack', 6, *(np.asarray(a, dtype=np.int64) for a in (
    [1, 2, 6, 3, 4, 1, 5, 2, 6], [2, 3, 1, 4, 5, 6, 1, 4, 1], [1, 3, 6])), 1)
ZD_LEAF = 6
ZD_B2, ZD_B4, ZD_BM4 = 2, 5, 8           # the leaf's lines with b = 2, 4 and -4 (x = 0.5, 0.25, -0.25), listed both ways round


def zero_den_batch():
    """(buses, lines, gens, slack) of two grids on ``ZD_TOPO``: the leaf hangs on the slack by three parallel lines with b = 2, 4,
    -4, so its block of B' is the 1x1 matrix [2] whatever the order of the sum.  The outage of the b = 2 line has z = 1/2 and
    den = 1 - 2 * 1/2 = 0 exactly, and no line is a bridge."""
    rng = np.random.default_rng(62)
    x = rng.choice([0.125, 0.25, 0.5, 1.0], (2, 9))
    x[:, ZD_B2], x[:, ZD_B4], x[:, ZD_BM4] = 0.5, 0.25, -0.25
    shift = rng.integers(-4, 5, (2, 9)) / 64.0
    pd = rng.integers(0, 9, (2, 6)) / 8.0
    pd[:, ZD_LEAF - 1] = [0.5, 1.25]
    pg = rng.integers(1, 9, (2, 3)) / 4.0
    return _grid_tensors(6, ZD_TOPO.f, ZD_TOPO.t, x, shift, pd, ZD_TOPO.g, pg) + (ZD_TOPO.slack,)


def zero_det_pairs():
    """Positions in the default pair list of ``ZD_TOPO`` of the pairs of the b = 2 line with a line of the ring: no pair of them
    islands, and the row kernel's determinant is exactly 0 (m11 = 0 and m12 = m21 = 0: the leaf is decoupled from the ring)."""
    every = powerflow._pair_list(None, ZD_TOPO.f.size)
    return [p for p, (j, k) in enumerate(every.tolist()) if ZD_B2 in (j, k) and not {j, k} & {ZD_B4, ZD_BM4}]
