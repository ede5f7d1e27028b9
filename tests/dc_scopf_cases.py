"""The problem sets of the security-constrained DC optimal power flow tests, feasible by construction so that no case is ever skipped.

Recipe: ``dc_opf_cases._build`` (the same random stream, so a set's grids, bounds, costs and ratings are that module's) with the
dispatch ``p0`` kept: ``rating = max(1.05 |F(p0)|, 0.02)`` on the picked lines as there, and
``contingency_rating_l = max(1.05 max_k |F'_lk(p0)|, 0.02)`` over the outages ``k`` that are not bridges, ``F'`` the float64 flows of
the network rebuilt without ``k``.  ``p0`` is then strictly feasible for the problem with every row listed.

The rows of a set are what the reference's own constraint generation lists per grid (``dc_scopf_reference.generate``, 8 rows per
round), laid out with empty slots in the middle of the list as well as at its end; a shared list is the grids' lists one after the
other without repeats.  ``check()`` asserts on the CPU that the base optimum violates a listed row and that a row is active at the
secure optimum, on every grid of every set, and that the reference's generation finishes within the rounds the driver test gives
the device."""
import functools
from collections import namedtuple

import numpy as np
import torch

from opf_graph_neural_solver_amd import synth
import dc_opf_cases as base_cases
import dc_scopf_reference as ref
import pf_topologies as pt

Case = namedtuple('Case', ['batch', 'rating_c', 'rows', 'outages'])     # batch: dc_opf_cases.Batch; rating_c f64 [E] / [Bt,E];
#                                                                         rows int32 [R,2] / [Bt,R,2]; outages: the non-bridge lines
DC_BAR = base_cases.DC_BAR
VIOLATION_TOL = 1e-5                 # the driver's default
ROWS_PER_ROUND = 8


def _build(buses, lines, gen_bus, slack, seed, quad, limited, shared_cost=False, shared_rating=False):
    """``dc_opf_cases._build`` statement for statement on the same random stream, keeping ``p0``; then the contingency rating."""
    rng = np.random.default_rng([seed, buses.shape[1], lines.shape[1], len(gen_bus)])
    Bt, E, Gn = buses.shape[0], lines.shape[1], len(gen_bus)
    gens = np.zeros((Bt, Gn, 7), dtype=np.float32)
    gens[..., 0] = gen_bus
    gens[..., 4] = 1.0
    gens[..., 6] = 7.5
    b64, l64 = buses.astype(np.float64), lines.astype(np.float64)
    rating = np.full((Bt, E), np.inf)
    rating_c = np.zeros((Bt, E))
    pick = rng.random(E) < limited
    outages = np.flatnonzero(~ref.bridges(buses.shape[1], l64[0]))
    for g in range(Bt):
        demand = (b64[g, :, 2] + b64[g, :, 4]).sum()
        share = rng.uniform(0.5, 1.5, Gn)
        p0 = demand * share / share.sum()
        gens[g, :, 1] = (p0 * rng.uniform(1.1, 1.8, Gn)).astype(np.float32)
        gens[g, :, 2] = (p0 * rng.uniform(0.3, 0.9, Gn)).astype(np.float32)
        assert np.all(gens[g, :, 2] < p0) and np.all(p0 < gens[g, :, 1])
        fl = base_cases._flows(b64[g], l64[g], gens[g].astype(np.float64), p0, slack)
        rating[g, pick] = np.maximum(1.05 * np.abs(fl[pick]), 0.02)
        post = ref.post_flows(b64[g], l64[g], gens[g].astype(np.float64), slack, p0, outages)
        rating_c[g] = np.maximum(1.05 * np.abs(post).max(axis=0), 0.02)
    if shared_rating:
        rating, rating_c = rating.max(axis=0), rating_c.max(axis=0)
    cost = np.zeros((1 if shared_cost else Bt, Gn, 2))
    cost[..., 1] = rng.uniform(10.0, 40.0, cost.shape[:2])
    if quad:
        cost[..., 0] = rng.uniform(0.5, 5.0, cost.shape[:2])
    cost = cost[0] if shared_cost else cost
    b = base_cases.Batch(torch.from_numpy(buses), torch.from_numpy(lines), torch.from_numpy(gens), torch.from_numpy(cost),
                         torch.from_numpy(rating) if limited else None, slack)
    return b, torch.from_numpy(rating_c), outages


def _on(tp, batch, seed, quad, limited=0.6, **kw):
    buses, lines = base_cases._grids(tp, batch, np.random.default_rng([seed, tp.n]))
    return _build(buses, lines, tp.g, tp.slack, seed, quad, limited, **kw)


def _case14(seed, quad, **kw):
    buses, lines, gens = synth.synth_grids(14, 3, seed=seed)
    return _build(buses.numpy(), lines.numpy(), gens[0, :, 0].numpy(), synth._solvable_slack(14), seed, quad, kw.pop('limited', 0.25), **kw)


def _three_bus():
    """``dc_opf_cases.three_bus`` without a base rating; line 1-3 (index 1) may carry 0.6 after an outage, the row is (1, 0): with
    line 1-2 out all of unit 1's output reaches bus 3 over line 1-3, so p1 <= 0.6: p = (0.6, 0.4), cost 18, the row's multiplier
    30 - 10 = 20 and lmp = (10, 30, 30)."""
    b = base_cases.three_bus()._replace(rating=None)
    return b, torch.tensor([np.inf, 0.6, np.inf], dtype=torch.float64), np.arange(3)


THREE_BUS_PG, THREE_BUS_OBJECTIVE, THREE_BUS_MU_ROW, THREE_BUS_LMP = (0.6, 0.4), 18.0, 20.0, (10.0, 30.0, 30.0)

# name: (builder, rows shared across the grids, R or None for the smallest list that holds the rows)
_WHEEL = pt.wheel_many_generators(71, 66)
SETS = {
    'three_bus': (_three_bus, True, None),
    'case14_qp': (lambda: _case14(1, True), False, None),                                           # per-grid rows, three grids
    'case14_lp': (lambda: _case14(5, False, limited=0.5, shared_cost=True, shared_rating=True), True, None),     # a shared list
    'meshed14': (lambda: _on(pt.random_meshed(14, 3), 2, 3, False, limited=0.25), False, None),    # parallel lines, a self-loop
    'stacked_units': (lambda: _on(pt.stacked_generators(24, 5), 2, 4, True), False, None),
    'ring30': (lambda: _on(pt.ring_slack_without_generator(30), 2, 37, False, limited=0.1), False, None),
    'lattice5': (lambda: _on(pt.lattice(5), 2, 4, True), False, None),
    'wheel_qp_r63': (lambda: _on(_WHEEL, 1, 22, True, limited=0.3), True, 63),                      # Gn = 66, E = 140: beyond a wave
    'wheel_qp_r64': (lambda: _on(_WHEEL, 2, 22, True, limited=0.3), False, 64),
    'wheel_lp_r65': (lambda: _on(_WHEEL, 2, 23, False, limited=0.3), False, 65),
}
# a batch whose three grids are secure at their base optimum (no row is ever listed): the driver returns dc_optimal_power_flow's bits
SECURE_FROM_THE_START = lambda: _case14(4, False, limited=0.5, shared_cost=True, shared_rating=True)      # noqa: E731
DRIVER_SETS = {'case14_qp': (4, 8), 'lattice5': (4, 8), 'wheel_qp_r63': (8, 16)}                   # name: (rounds, rows_per_round)


# sets that other modules keep (``dc_scopf_pin_cases``), registered there as name: a function that gives the ``Case``; reachable by
# name through ``case``, ``problems``, ``rows_of``, ``optimum``, ``tight_optimum`` and ``bars``, and not in ``SETS``, so that the tests
# parametrised over ``SETS`` stay as they are
OTHER_SETS = {}


def _slots(R):
    """The slots of a list of R that rows go to: every ninth slot, from the fifth, stays empty, and so do the last two."""
    return [i for i in range(R - 2) if i % 9 != 4]


def _laid_out(rows, R, cut=False):
    """``cut``: a list longer than the slots of R loses its tail (the wheel's fixed R: the set is then a problem of its own, not the
    secure dispatch, and is compared with the reference on the same rows like every other)."""
    out = np.full((R, 2), -1, dtype=np.int32)
    at = _slots(R)
    assert cut or len(rows) <= len(at), (len(rows), R)
    rows = rows[:len(at)]
    out[at[:len(rows)]] = rows
    return out


def problems(name):
    """The grids of a set one by one as the reference takes them: (buses, lines, gens, cost, rating, slack), rating_c [E]."""
    b, rating_c, _ = _built(name)
    return [(p, (rating_c if rating_c.dim() == 1 else rating_c[g]).numpy()) for g, p in enumerate(base_cases.problems_of(b))]


@functools.lru_cache(maxsize=None)
def _built(name):
    if name in OTHER_SETS:
        c = OTHER_SETS[name]()
        return c.batch, c.rating_c, c.outages
    return SETS[name][0]()


@functools.lru_cache(maxsize=None)
def generated(name, rows_per_round=ROWS_PER_ROUND, violation_tol=1e-6):
    """Per grid what the reference's own constraint generation gives: (result, rows, rounds)."""
    outages = _built(name)[2]
    if name == 'three_bus':
        p, rc = problems(name)[0]
        rows = np.array([[1, 0]])
        return ((ref.solve(*p, rows, rc), rows, 1),)
    return tuple(ref.generate(*p, rc, outages, rows_per_round, violation_tol) for p, rc in problems(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """The set as the product takes it."""
    if name in OTHER_SETS:
        return OTHER_SETS[name]()
    b, rating_c, outages = _built(name)
    _, shared, R = SETS[name]
    cut = R is not None
    lists = [g[1] for g in generated(name)]
    if shared:
        seen, rows = set(), []
        for l in lists:
            for r in map(tuple, l.tolist()):
                if r not in seen:
                    seen.add(r)
                    rows.append(r)
        n = len(rows)
        R = R or next(r for r in range(3, 10 * n + 10) if len(_slots(r)) >= n)
        out = _laid_out(np.array(rows).reshape(-1, 2), R, cut)
    else:
        n = max(len(l) for l in lists)
        R = R or next(r for r in range(3, 10 * n + 10) if len(_slots(r)) >= n)
        out = np.stack([_laid_out(l, R, cut) for l in lists])
    return Case(b, rating_c, torch.from_numpy(out), outages)


def rows_of(name, g):
    c = case(name)
    return (c.rows if c.rows.dim() == 2 else c.rows[g]).numpy()


@functools.lru_cache(maxsize=None)
def optimum(name, tol=ref.DEFAULT_TOL):
    """The reference optimum of every grid of a set with the set's rows (computed once, shared by the tests, not to be changed)."""
    return tuple(ref.solve(*p, rows_of(name, g), rc, tol=tol) for g, (p, rc) in enumerate(problems(name)))


@functools.lru_cache(maxsize=None)
def tight_optimum(name, tol=ref.DEFAULT_TOL):
    """The reference at ``tol / 1000``, as ``dc_opf_cases.tight_optimum``: the best iterate of 60, within ``tol / 100``."""
    out = tuple(ref.solve(*p, rows_of(name, g), rc, tol=tol / 1000, max_iter=60, best=True) for g, (p, rc) in enumerate(problems(name)))
    assert all(r['worst'] < tol / 100 for r in out), (name, [r['worst'] for r in out])
    return out


def _bars(a, b):
    """``dc_opf_cases.bars``' rule on the optima a (at tol) and b (at tol / 1000): ten times the reference's own movement plus the
    DC bar at the reference's scale."""
    assert all(r['converged'] for r in a)
    y = dict(objective=max(abs(x['objective'] - y['objective']) / max(1.0, abs(y['objective'])) for x, y in zip(a, b)),
             pg=max(np.abs(x['pg'] - y['pg']).max() for x, y in zip(a, b)), lmp=max(np.abs(x['lmp'] - y['lmp']).max() for x, y in zip(a, b)))
    scale = {k: max(1.0, max(np.abs(r[k]).max() for r in a)) for k in ('pg', 'lmp')}
    return dict(objective=10 * y['objective'] + DC_BAR, pg=10 * y['pg'] + DC_BAR * scale['pg'], lmp=10 * y['lmp'] + DC_BAR * scale['lmp'])


def bars(name, tol=ref.DEFAULT_TOL):
    return _bars(optimum(name, tol), tight_optimum(name, tol))


@functools.lru_cache(maxsize=None)
def secure_optimum(name, tol=ref.DEFAULT_TOL):
    """Per grid the reference optimum with every row listed (every non-bridge outage, every other line): what the driver's result
    is compared with, at the set's own ``bars``."""
    c = case(name)
    rows = ref.all_rows(c.batch.lines.shape[1], c.outages)
    out = tuple(ref.solve(*p, rows, rc, tol=tol) for p, rc in problems(name))
    assert all(r['converged'] for r in out), name
    return out


def check():
    for name in SETS:
        for g, ((p, rc), opt) in enumerate(zip(problems(name), optimum(name))):
            rows = rows_of(name, g)
            live = [i for i, (l, k) in enumerate(rows) if l >= 0]
            lim = np.array([rc[rows[i, 0]] for i in live])
            base = ref.solve(*p, np.zeros((0, 2), dtype=int), rc)
            assert base['converged'] and opt['converged'], (name, g)
            at_base, _ = ref.row_values(p[0], p[1], p[2], p[5], rows, base['pg'])
            assert (np.abs(at_base[live]) > lim * (1 + 1e-6)).any(), (name, g, 'the base optimum violates no listed row')
            assert (np.abs(opt['row_flow'][live]) > lim * (1 - 1e-6)).any(), (name, g, 'no row is active at the secure optimum')
            assert (np.abs(opt['row_flow'][live]) <= lim * (1 + 1e-7)).all(), (name, g)
    for name, (rounds, per_round) in DRIVER_SETS.items():
        outages = _built(name)[2]
        for g, (p, rc) in enumerate(problems(name)):
            _, rows, used = ref.generate(*p, rc, outages, per_round, VIOLATION_TOL)
            assert used <= rounds and len(rows) <= rounds * per_round, (name, g, used, rounds)
