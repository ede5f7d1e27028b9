"""The problem sets that pin the DC optimal power flow's interior point iterate by iterate (``tests/test_dc_opf_iterates_host.py``,
``tests/test_dc_opf_iterates_gpu.py``): two grids each, by the recipe of ``dc_opf_cases._build`` (feasible by construction), at the
shapes where the three kernels of ``csrc/gns_dcopf.hip`` could go wrong and on data the sets of ``dc_opf_cases`` do not reach.  They
are registered in ``dc_opf_cases.OTHER_SETS``, so ``dc_opf_cases.batch``, ``problems``, ``optimum`` and ``bars`` take their names;
they are not in ``dc_opf_cases.SETS``.

Shapes, on ``pf_topologies.wheel_many_generators`` (few buses, any Gn, the first unit on the slack: a zero column of S; no line is
a bridge, so the limits couple the units):
    gn3, gn4, gn5      the tile clamp of the normal matrix (tiles of 4 x 4: one tile short, one tile full, a second tile row of one)
    gn40, gn41         the packed triangle has 55 tiles at 40 and 66 at 41: the first Gn at which a lane takes a second tile
    gn63, gn64, gn65   every unit loop, the Cholesky's row per lane, the two solves and the wave sums at the lane edge; the factor
                       kernel runs a full chunk at 64 and a second chunk of one unit at 65
    narrow_chunk       the smallest wheel with 37 units on which ``gns_dcopf_lds_bytes`` reports a chunk width below 64
                       (``narrow_topology``, searched): 37 is no multiple of 32 or less, so the last chunk is short
Data:
    mixed_c2           c2 = 0 on every second unit, c2 > 0 on the others
    low_pmin           Pmin < 0 on every third unit, Pmin = 0 on every third
    wide               Pmax - Pmin > 2 on every second unit; every third rated line rated 1.5 above its flow at the midpoint: the
                       start takes z = -h above 1 on box rows and on line rows
    mixed_ratings      78 lines (more than a wave's 64 lanes), six units, lines with and without a rating interleaved

``check()`` asserts on the CPU, from ``dc_opf_reduced_reference``, what the sets promise."""
import functools

import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow
import dc_opf_cases as cases
import dc_opf_reduced_reference as reduced
import dc_opf_reference as full
import pf_topologies as pt

NARROW_GN = 37


def _wheel(n, gn, seed, quad, limited=0.6):
    return cases._on(pt.wheel_many_generators(n, gn), 2, seed, quad, limited)


def chunk_width(tp):
    """The chunk width W of the factor kernel on topology tp (``gns_dcopf_lds_bytes``)."""
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    return powerflow._screen_lds_bytes('gns_dcopf_lds_bytes', fd.host)[1]


@functools.lru_cache(maxsize=None)
def narrow_topology():
    """The smallest ``wheel_many_generators(n, 37)`` whose chunk width is below 64 (the factor kernel's image grows with n)."""
    make = lambda n: pt.wheel_many_generators(n, NARROW_GN)     # noqa: E731
    lo, hi = NARROW_GN + 2, 400
    assert chunk_width(make(lo)) == 64 and chunk_width(make(hi)) < 64
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if chunk_width(make(mid)) < 64 else (mid, hi)
    return make(hi)


def _mixed_c2(seed):
    b = _wheel(12, 6, seed, True)
    cost = b.cost.clone()
    cost[:, 0::2, 0] = 0.0
    return b._replace(cost=cost)


def _low_pmin(seed):
    b = _wheel(12, 6, seed, False)
    gens = b.gens.clone()
    gens[:, 0::3, 2] = -gens[:, 0::3, 2]
    gens[:, 1::3, 2] = 0.0
    return b._replace(gens=gens)


def _wide(seed):
    """Bounds widened downwards and upwards about the recipe's dispatch (which stays feasible), and every third rated line rated
    1.5 above the size of its flow at the new midpoint: those rows start with a slack above 1."""
    b = _wheel(12, 6, seed, True)
    gens, rating = b.gens.clone(), b.rating.clone()
    gens[:, 0::2, 1] += 2.0
    gens[:, 0::2, 2] -= 1.5
    for g in range(gens.shape[0]):
        mid = 0.5 * (gens[g, :, 1].double() + gens[g, :, 2].double()).numpy()
        fl = cases._flows(b.buses[g].double().numpy(), b.lines[g].double().numpy(), gens[g].double().numpy(), mid, b.slack)
        loose = np.flatnonzero(np.isfinite(rating[g].numpy()))[0::3]
        rating[g, loose] = torch.from_numpy(np.abs(fl[loose]) + 1.5)
    return b._replace(gens=gens, rating=rating)


BUILDERS = {
    'gn3': lambda seed: _wheel(8, 3, seed, True),
    'gn4': lambda seed: _wheel(8, 4, seed, False),
    'gn5': lambda seed: _wheel(8, 5, seed, True),
    'gn40': lambda seed: _wheel(44, 40, seed, True),
    'gn41': lambda seed: _wheel(44, 41, seed, False),
    'gn63': lambda seed: _wheel(68, 63, seed, False),
    'gn64': lambda seed: _wheel(68, 64, seed, True),
    'gn65': lambda seed: _wheel(68, 65, seed, True),
    'narrow_chunk': lambda seed: cases._on(narrow_topology(), 2, seed, True, 0.3),
    'mixed_c2': _mixed_c2,
    'low_pmin': _low_pmin,
    'wide': _wide,
    'mixed_ratings': lambda seed: _wheel(40, 6, seed, True, limited=0.5),
}
# The seeds are searched (``draw_seeds``), because of the count test's tie rule: a grid whose worst termination figure lies in
# [tol / 2, 2 tol] at some test may differ by one iteration, and at most a quarter of all grids may be such near ties.  The figure
# falls by about ten per iteration, so about half of all grids are: 13 of the 28 grids of ``dc_opf_cases.SETS``, whose seeds stay.
# So each set here takes the first seed of 21 + its place, + 100, + 200, ... at which neither of its grids has a figure within
# [tol / 2.2, 2.2 tol] in the reduced reference (a little wider than the rule, so that rounding elsewhere does not make a tie).
SEEDS = {'gn3': 121, 'gn4': 222, 'gn5': 423, 'gn40': 1424, 'gn41': 825, 'gn63': 26, 'gn64': 1027, 'gn65': 528, 'narrow_chunk': 2729,
         'mixed_c2': 3630, 'low_pmin': 431, 'wide': 1232, 'mixed_ratings': 533}
SETS = {name: functools.partial(BUILDERS[name], SEEDS[name]) for name in BUILDERS}


def draw_seeds(tol=reduced.DEFAULT_TOL, margin=2.2):
    """The search behind ``SEEDS`` (see there)."""
    out = {}
    for place, name in enumerate(BUILDERS):
        seed = 21 + place
        while True:
            b = BUILDERS[name](seed)
            runs_ = [reduced.solve(*p) for p in cases.problems_of(b)]
            if all(r['converged'] and not any(tol / margin <= w <= margin * tol for w in r['worst']) for r in runs_):
                break
            seed += 100
        out[name] = seed
    return out


cases.OTHER_SETS.update(SETS)
ALL_SETS = tuple(cases.SETS) + tuple(SETS)           # every set the iterates are pinned on
KS = (0, 1, 2, 3)
FIELDS = ('pg', 'mu_line', 'mu_pmax', 'mu_pmin')


@functools.lru_cache(maxsize=None)
def iterates(name, k):
    """The reduced reference's iterate after exactly k updates, of every grid of a set (computed once, not to be changed)."""
    return tuple(reduced.iterate(*p, k) for p in cases.problems(name))


@functools.lru_cache(maxsize=None)
def full_iterates(name, k):
    """The full reference's iterate after k updates (it does not converge that early on any grid: asserted)."""
    out = tuple(full.solve(*p, max_iter=k) for p in cases.problems(name))
    assert all(r['iterations'] == k and not r['converged'] for r in out), (name, k)
    return out


@functools.lru_cache(maxsize=None)
def runs(name):
    """The reduced reference run to the default tolerance, of every grid of a set."""
    return tuple(reduced.solve(*p) for p in cases.problems(name))


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / max(1.0, float(np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def yardstick(name, k):
    """How far the two references are apart after k updates: the largest over the set's grids and over pg, mu_line, mu_pmax and
    mu_pmin of max|reduced - full| / max(1, max|reduced|).  What reformulation and rounding alone move."""
    return max(_rel(f[key], r[key]) for r, f in zip(iterates(name, k), full_iterates(name, k)) for key in FIELDS)


def iterate_bar(name, k, want):
    """What the device may differ from the reduced reference's value ``want`` by after k updates: ten times the set's yardstick
    plus the DC bar, at the scale of ``want``."""
    return (10.0 * yardstick(name, k) + cases.DC_BAR) * max(1.0, float(np.abs(want).max()))


def near_ties():
    """The (set, grid) pairs whose reduced run is a near tie at the default tolerance."""
    return tuple((name, g) for name in ALL_SETS for g, r in enumerate(runs(name)) if reduced.near_tie(r['worst']))


def check(rel=1e-6):
    """What the new sets promise: the shapes, the data edges, a lower line limit, a unit at Pmin and one at Pmax active at the
    reduced reference's optimum over the sets together, a start slack above 1 on a box row and on a line row, and every grid
    converged."""
    gn = {name: cases.batch(name).gens.shape[1] for name in SETS}
    assert [gn[n] for n in ('gn3', 'gn4', 'gn5', 'gn40', 'gn41', 'gn63', 'gn64', 'gn65')] == [3, 4, 5, 40, 41, 63, 64, 65]
    assert all(cases.batch(name).buses.shape[0] == 2 for name in SETS)
    w = chunk_width(narrow_topology())
    assert w < 64 and gn['narrow_chunk'] == NARROW_GN and NARROW_GN % w != 0 and NARROW_GN > w, w
    b = cases.batch('mixed_c2')
    assert bool((b.cost[..., 0] == 0).any(dim=1).all()) and bool((b.cost[..., 0] > 0).any(dim=1).all())
    b = cases.batch('low_pmin')
    assert bool((b.gens[..., 2] < 0).any(dim=1).all()) and bool((b.gens[..., 2] == 0).any(dim=1).all())
    assert bool((b.gens[..., 2] > 0).any(dim=1).all())
    b = cases.batch('wide')
    assert bool(((b.gens[..., 1] - b.gens[..., 2]) > 2).any(dim=1).all())
    b = cases.batch('mixed_ratings')
    fin = torch.isfinite(b.rating)
    assert b.lines.shape[1] > 64 and gn['mixed_ratings'] > 2
    assert bool((fin[:, 1:] != fin[:, :-1]).sum(dim=1).ge(8).all()) and bool(fin[:, 64:].any()) and bool((~fin[:, 64:]).any())
    lower = at_pmin = at_pmax = box_above = line_above = 0
    for name in SETS:
        for p, r in zip(cases.problems(name), runs(name)):
            assert r['converged'], name
            pmax, pmin = p[2][:, 1], p[2][:, 2]
            lower += int((r['mu_line'] < -rel * max(1.0, np.abs(r['mu_line']).max())).sum())
            at_pmin += int((r['pg'] < pmin + rel * (pmax - pmin)).sum())
            at_pmax += int((r['pg'] > pmax - rel * (pmax - pmin)).sum())
            box_above += int((r['z0_box'] > 1.0).sum())
            line_above += int((r['z0_line'] > 1.0).sum())
    assert lower >= 1 and at_pmin >= 1 and at_pmax >= 1 and box_above >= 1 and line_above >= 1, \
        (lower, at_pmin, at_pmax, box_above, line_above)
    wide = runs('wide')
    assert all((r['z0_box'] > 1.0).any() and (r['z0_line'] > 1.0).any() for r in wide)
    return dict(lower=lower, at_pmin=at_pmin, at_pmax=at_pmax, box_above=box_above, line_above=line_above)
