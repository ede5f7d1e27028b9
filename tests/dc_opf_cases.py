"""The problem sets of the DC optimal power flow tests, feasible by construction so that no case is ever skipped.

Recipe (``_build``): a dispatch ``p0`` with ``sum p0 = demand`` (float64, from the float32 loads the product reads), bounds
``Pmin < p0 < Pmax`` strictly (rounded to float32: the product reads them from the generator rows), a chosen subset of the lines
rated ``max(1.05 |flow(p0)|, 0.02)`` and the rest ``inf``, and distinct ``c1`` so that the economic optimum differs from ``p0`` and
limits bind.  The listed ``Pg`` is 7.5 everywhere: it is ignored.  ``check_active()`` asserts on the CPU that at least one line limit
and one unit bound are active at the reference optimum of each set of ``ACTIVE_SETS``; the other sets cannot have both by their
shape and say why (``INACTIVE_SETS``).

``batch(name)`` gives what the product takes (float32 tensors, ``cost`` and ``rating`` in the set's own form: shared or per grid),
``problems(name)`` the same grids one by one as the reference takes them (float64 numpy, ``rating`` with ``inf``)."""
import functools
from collections import namedtuple

import numpy as np
import torch

from opf_graph_neural_solver_amd import synth
import dc_opf_reference as ref
import pf_topologies as pt

Batch = namedtuple('Batch', ['buses', 'lines', 'gens', 'cost', 'rating', 'slack'])

DC_BAR = 1e-9            # the project's DC bar: max|out - ref| <= 1e-9 max(1, max|ref|)


def _flows(buses, lines, gens, p, slack):
    """Line flows of one grid at dispatch p (float64 numpy), dense."""
    N = buses.shape[0]
    Bbus, Bf, pfinj, pbusinj = ref.make_bdc(lines, N)
    inj = -(buses[:, 2] + buses[:, 4] + pbusinj)
    np.add.at(inj, gens[:, 0].astype(int) - 1, p)
    r = np.array([i for i in range(N) if i != slack - 1], dtype=int)
    theta = np.zeros(N)
    if r.size:
        theta[r] = np.linalg.solve(Bbus[np.ix_(r, r)], inj[r])
    return Bf @ theta + pfinj


def _grids(tp, batch, rng):
    """float32 buses and lines of ``batch`` grids on topology tp."""
    n, e = tp.n, tp.f.size
    buses = np.zeros((batch, n, 6))
    buses[..., 0] = np.arange(1, n + 1)
    buses[..., 1] = 1.0
    buses[..., 2] = rng.uniform(0.05, 0.5, (batch, n))
    buses[..., 4] = 0.01
    lines = np.zeros((batch, e, 7))
    lines[..., 0], lines[..., 1] = tp.f, tp.t
    lines[..., 3] = rng.uniform(0.04, 0.6, (batch, e))
    lines[..., 5] = rng.uniform(0.9, 1.1, (batch, e))
    lines[..., 6] = rng.uniform(-0.2, 0.2, (batch, e)) * (np.pi / 180)
    return buses.astype(np.float32), lines.astype(np.float32)


def _build(buses, lines, gen_bus, slack, seed, quad, limited, shared_cost=False, shared_rating=False):
    """A Batch on the float32 ``buses`` and ``lines`` [Bt,...]: generator rows, cost and rating by the module's recipe.  ``limited``:
    the fraction of lines that get a rating (0: ``rating`` None)."""
    rng = np.random.default_rng([seed, buses.shape[1], lines.shape[1], len(gen_bus)])
    Bt, E, Gn = buses.shape[0], lines.shape[1], len(gen_bus)
    gens = np.zeros((Bt, Gn, 7), dtype=np.float32)
    gens[..., 0] = gen_bus
    gens[..., 4] = 1.0
    gens[..., 6] = 7.5
    b64, l64 = buses.astype(np.float64), lines.astype(np.float64)
    rating = np.full((Bt, E), np.inf)
    pick = rng.random(E) < limited
    for g in range(Bt):
        demand = (b64[g, :, 2] + b64[g, :, 4]).sum()
        share = rng.uniform(0.5, 1.5, Gn)
        p0 = demand * share / share.sum()
        gens[g, :, 1] = (p0 * rng.uniform(1.1, 1.8, Gn)).astype(np.float32)
        gens[g, :, 2] = (p0 * rng.uniform(0.3, 0.9, Gn)).astype(np.float32)
        assert np.all(gens[g, :, 2] < p0) and np.all(p0 < gens[g, :, 1])
        fl = _flows(b64[g], l64[g], gens[g].astype(np.float64), p0, slack)
        rating[g, pick] = np.maximum(1.05 * np.abs(fl[pick]), 0.02)
    if shared_rating:
        rating = rating.max(axis=0)
    cost = np.zeros((1 if shared_cost else Bt, Gn, 2))
    cost[..., 1] = rng.uniform(10.0, 40.0, cost.shape[:2])
    if quad:
        cost[..., 0] = rng.uniform(0.5, 5.0, cost.shape[:2])
    cost = cost[0] if shared_cost else cost
    return Batch(torch.from_numpy(buses), torch.from_numpy(lines), torch.from_numpy(gens), torch.from_numpy(cost),
                 torch.from_numpy(rating) if limited else None, slack)


def _on(tp, batch, seed, quad, limited=0.6, shared_cost=False, shared_rating=False):
    buses, lines = _grids(tp, batch, np.random.default_rng([seed, tp.n]))
    return _build(buses, lines, tp.g, tp.slack, seed, quad, limited, shared_cost, shared_rating)


def _case14(seed, quad, **kw):
    buses, lines, gens = synth.synth_grids(14, 3, seed=seed)
    return _build(buses.numpy(), lines.numpy(), gens[0, :, 0].numpy(), synth._solvable_slack(14), seed, quad,
                  kw.pop('limited', 0.25), **kw)


def three_bus():
    """The closed-form grid: buses 1 (slack), 2, 3 joined by three lines of x = 0.1; a unit of 10 per MW on bus 1 and one of 30 on
    bus 2, both within [0, 2]; a load of 1 on bus 3; line 1-3 rated 0.5.  Two thirds of bus 1's output and one third of bus 2's reach
    bus 3 over line 1-3, so 1/3 + p1 / 3 <= 0.5: p = (0.5, 0.5), line 1-3 binds; lmp = (10, 30, 50) (a further MW on bus 3 takes
    -1 MW of unit 1 and +2 MW of unit 2 to keep line 1-3 at its limit) and mu_line of line 1-3 is 60."""
    buses = np.zeros((1, 3, 6), dtype=np.float32)
    buses[0, :, 0], buses[0, :, 1], buses[0, 2, 2] = [1, 2, 3], 1.0, 1.0
    lines = np.zeros((1, 3, 7), dtype=np.float32)
    lines[0, :, 0], lines[0, :, 1], lines[0, :, 3], lines[0, :, 5] = [1, 1, 2], [2, 3, 3], 0.1, 1.0
    gens = np.zeros((1, 2, 7), dtype=np.float32)
    gens[0, :, 0], gens[0, :, 1], gens[0, :, 2], gens[0, :, 6] = [1, 2], 2.0, 0.0, 7.5
    cost = torch.tensor([[0.0, 10.0], [0.0, 30.0]], dtype=torch.float64)
    rating = torch.tensor([np.inf, 0.5, np.inf], dtype=torch.float64)
    return Batch(torch.from_numpy(buses), torch.from_numpy(lines), torch.from_numpy(gens), cost, rating, 1)


THREE_BUS_PG, THREE_BUS_LMP, THREE_BUS_MU = (0.5, 0.5), (10.0, 30.0, 50.0), 60.0

SETS = {
    'three_bus': three_bus,
    'case14_qp': lambda: _case14(1, True),                                         # cost [Bt,Gn,2], rating [Bt,E]
    'case14_lp': lambda: _case14(2, False, limited=0.5, shared_cost=True, shared_rating=True),    # cost [Gn,2], rating [E]
    'case14_no_rating': lambda: _case14(3, True, limited=0.0),                       # rating None
    'one_unit': lambda: _on(pt.path(9), 2, 4, True),                                 # Gn = 1
    'slack_unit': lambda: _on(pt.random_meshed(14, 3), 2, 5, False, limited=0.25),                 # a unit on the slack: a zero column of S
    'stacked_units': lambda: _on(pt.stacked_generators(24, 5), 2, 6, True),          # four units on one bus, two on the slack
    'ring30': lambda: _on(pt.ring_slack_without_generator(30), 2, 37, False, limited=0.1),
    'path64': lambda: _on(pt.path(64), 2, 8, True),                                  # E = 63
    'path65': lambda: _on(pt.path(65), 2, 9, False),                                 # E = 64
    'path66_pv': lambda: _on(pt.path(66, pv=(33,)), 2, 10, True),                    # E = 65, two units
    'hub150_qp': lambda: _on(pt.many_generators_and_lines(150), 2, 11, True),        # Gn = 70 > 64
    'hub150_lp': lambda: _on(pt.many_generators_and_lines(150), 2, 12, False),
}
# the sets that cannot have both a line limit and a unit bound active, and why
INACTIVE_SETS = {'three_bus': 'its closed form has the line active and both units inside their bounds',
                 'case14_no_rating': 'no line has a limit',
                 'one_unit': 'one unit: the balance alone fixes its output, strictly inside its bounds',
                 'path64': 'one unit', 'path65': 'one unit',
                 'slack_unit': 'two units, as path66_pv',
                 'path66_pv': 'two units: the balance leaves one degree of freedom, which one active inequality uses up'}
ACTIVE_SETS = tuple(n for n in SETS if n not in INACTIVE_SETS)
LP_SETS = tuple(n for n in SETS if n in ('three_bus', 'case14_lp', 'slack_unit', 'ring30', 'path65', 'hub150_lp'))


# sets that other modules keep (``dc_opf_pin_cases``), registered there: reachable by name through ``batch``, ``problems``,
# ``optimum``, ``yardstick`` and ``bars``, and not in ``SETS``, so that the tests parametrised over ``SETS`` stay as they are
OTHER_SETS = {}


@functools.lru_cache(maxsize=None)
def batch(name):
    return (SETS[name] if name in SETS else OTHER_SETS[name])()


def problems(name):
    """The grids of a set one by one, as the reference takes them: (buses, lines, gens, cost [Gn,2], rating [E] with inf, slack)."""
    return problems_of(batch(name))


def problems_of(b):
    """``problems`` of a Batch that need not be a registered set."""
    out = []
    for g in range(b.buses.shape[0]):
        cost = b.cost if b.cost.dim() == 2 else b.cost[g]
        E = b.lines.shape[1]
        rating = np.full(E, np.inf) if b.rating is None else (b.rating if b.rating.dim() == 1 else b.rating[g]).numpy()
        out.append((b.buses[g].double().numpy(), b.lines[g].double().numpy(), b.gens[g].double().numpy(), cost.numpy(), rating, b.slack))
    return out


@functools.lru_cache(maxsize=None)
def optimum(name, tol=ref.DEFAULT_TOL):
    """The reference optimum of every grid of a set (computed once, shared by the tests, not to be changed)."""
    return tuple(ref.solve(*p, tol=tol) for p in problems(name))


@functools.lru_cache(maxsize=None)
def tight_optimum(name, tol=ref.DEFAULT_TOL):
    """The reference at ``tol / 1000``.  Below about 2e-11 the gradient figure of the dense KKT solve stops falling on some grids
    (rounding), so a grid that does not reach ``tol / 1000`` within 60 iterations gives its iterate with the smallest worst figure;
    every grid must get within ``tol / 100``."""
    out = tuple(ref.solve(*p, tol=tol / 1000, max_iter=60, best=True) for p in problems(name))
    assert all(r['worst'] < tol / 100 for r in out), (name, [r['worst'] for r in out])
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name, tol=ref.DEFAULT_TOL):
    """How far the reference's own objective (relative), pg and lmp (absolute, the largest over the set's grids) move between
    ``tol`` and ``tol / 1000`` (``tight_optimum``): what stopping inside the tolerance ball alone allows."""
    a, b = optimum(name, tol), tight_optimum(name, tol)
    assert all(r['converged'] for r in a), name
    return dict(objective=max(abs(x['objective'] - y['objective']) / max(1.0, abs(y['objective'])) for x, y in zip(a, b)),
                pg=max(np.abs(x['pg'] - y['pg']).max() for x, y in zip(a, b)),
                lmp=max(np.abs(x['lmp'] - y['lmp']).max() for x, y in zip(a, b)))


def bars(name, tol=ref.DEFAULT_TOL):
    """What the device may differ from the reference optimum by: ten times the yardstick plus the DC bar at the reference's scale."""
    y, opt = yardstick(name, tol), optimum(name, tol)
    scale = {k: max(1.0, max(np.abs(r[k]).max() for r in opt)) for k in ('pg', 'lmp')}
    return dict(objective=10 * y['objective'] + DC_BAR, pg=10 * y['pg'] + DC_BAR * scale['pg'], lmp=10 * y['lmp'] + DC_BAR * scale['lmp'])


def active(name, rel=1e-6):
    """(line limits active, unit bounds active) at the reference optimum, the fewest over the set's grids."""
    lines_active, bounds_active = [], []
    for p, r in zip(problems(name), optimum(name)):
        rating, pmax, pmin = p[4], p[2][:, 1], p[2][:, 2]
        lim = np.isfinite(rating)
        lines_active.append(int((np.abs(r['line_flow'][lim]) > rating[lim] * (1 - rel)).sum()))
        bounds_active.append(int(((r['pg'] > pmax - rel * (pmax - pmin)) | (r['pg'] < pmin + rel * (pmax - pmin))).sum()))
    return min(lines_active), min(bounds_active)


def check_active():
    for name in ACTIVE_SETS:
        nl, nb = active(name)
        assert nl >= 1 and nb >= 1, (name, nl, nb)
