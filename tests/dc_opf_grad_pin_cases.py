"""The problem sets that pin the DC optimal power flow's adjoint (``csrc/gns_dcopf_adjoint.hip``) where a wave's 64 lanes could make
its dense KKT solve, its active-set lists and its failure paths go wrong (``tests/test_dc_opf_grad_pin_host.py``,
``tests/test_dc_opf_grad_pin_gpu.py``).  Two grids each on ``pf_topologies.wheel_many_generators(gn + 4, gn)``, by the recipe of
``dc_opf_cases._build`` with quadratic cost; registered in ``dc_opf_cases.OTHER_SETS``, not in ``dc_opf_cases.SETS``.

The KKT order of a grid is ``n = nf + 1 + k``: its free units, the balance, its active lines.  An *all-free* set moves the recipe's
optimum strictly inside every bound and every limit, so that ``nf = Gn``, ``k = 0`` and ``n = Gn + 1`` exactly (``_all_free``):
``p0`` is the midpoint of the bounds, shifted equally so that ``sum p0 = demand`` (asserted strictly inside); ``c1 = 25 - 2 c2 p0``
makes ``p0`` stationary at lambda = 25; the rated lines are rated ``max(1.3 |flow(p0)|, 0.02)``.

    free62, free63, free64   n = 63, 64, 65: the lane edge of the LU's pivot search, row swap, column update and back-substitution
    free64_linear0           free64 with c2 = 0 on unit 0 alone (its output follows from the balance): column 0 of the system holds
                             one entry that is not zero, the balance's at row 64, so the first pivot lies a full wave below the
                             diagonal: the pivot search's and the row swap's second trip, which no strictly convex all-free set
                             takes, since there every diagonal entry 2 c2 >= 1 wins its column
    free70_lines             all-free at Gn = 70, then ``LINES_M`` rated lines (a seeded draw, ``draw_lines``) re-rated to 0.98 of
                             their flow at the all-free optimum: nf >= 65 and k >= 3 on both grids, so the free units' rows and the
                             active lines' rows both sit past place 64 of the system
    cap_fits                 all-free at Gn = 129: n = 130 is exactly the order ``gns_dcopf_adjoint_lds_bytes`` reports
    cap_over                 Gn = 130, where that order is 130 too: grid 0 all-free, n = 131, one above (NaN rows); grid 1 the same
                             recipe with ``NARROWED`` units' bounds narrowed on one side of ``p0``: they bind, n <= 130

``check()`` asserts every promise on the CPU from the float64 reference, and for the two ``cap_*`` sets from the library's own host
queries too: should the image formulas move the cap, it fails; it never lets a test pass empty."""
import functools

import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow
import dc_opf_cases as cases
import dc_opf_grad_reference as gref
import dc_opf_reference as ref
import pf_topologies as pt

SEED = 77
LINES_M, LINES_DRAW = 3, 0         # free70_lines: how many lines are re-rated and the draw that chose them (``draw_lines``)
NARROWED = (3, 64, 65, 127)        # cap_over grid 1: these units bind, in turn at Pmax and at Pmin
CAP = 130                          # the order the adjoint's image holds on both cap_* topologies (asserted from the library)


def _topology(gn):
    return pt.wheel_many_generators(gn + 4, gn)


def _all_free(gn, seed=SEED, linear=()):
    """The all-free Batch at ``gn`` units and, per grid, its optimum ``p0``; the units ``linear`` get ``c2 = 0``."""
    b = cases._on(_topology(gn), 2, seed, True)
    cost, rating = b.cost.clone(), b.rating.clone()
    cost[:, list(linear), 0] = 0.0
    p0s = []
    for g in range(b.buses.shape[0]):
        bus, line, gen = b.buses[g].double().numpy(), b.lines[g].double().numpy(), b.gens[g].double().numpy()
        pmax, pmin = gen[:, 1], gen[:, 2]
        mid = 0.5 * (pmax + pmin)
        p0 = mid + ((bus[:, 2] + bus[:, 4]).sum() - mid.sum()) / gn
        assert np.all(pmin < p0) and np.all(p0 < pmax)
        cost[g, :, 1] = torch.from_numpy(25.0 - 2.0 * cost[g, :, 0].numpy() * p0)
        fl = cases._flows(bus, line, gen, p0, b.slack)
        rated = np.isfinite(rating[g].numpy())
        rating[g, torch.from_numpy(rated)] = torch.from_numpy(np.maximum(1.3 * np.abs(fl[rated]), 0.02))
        p0s.append(p0)
    return b._replace(cost=cost, rating=rating), p0s


def _with_lines(draw, m=LINES_M, gn=70):
    """All-free at ``gn`` with ``m`` of the rated lines, the same on both grids, re-rated to 0.98 of the size of their flow at the
    all-free optimum.  The lines are drawn among the rated ones whose flow there is at least 0.05 on both grids."""
    b, p0s = _all_free(gn)
    rating = b.rating.clone()
    flows = [cases._flows(b.buses[g].double().numpy(), b.lines[g].double().numpy(), b.gens[g].double().numpy(), p0s[g], b.slack)
             for g in range(2)]
    able = np.flatnonzero(np.isfinite(rating[0].numpy()) & (np.abs(flows[0]) >= 0.05) & (np.abs(flows[1]) >= 0.05))
    pick = np.sort(np.random.default_rng([SEED, gn, m, draw]).choice(able, m, replace=False))
    for g in range(2):
        rating[g, torch.from_numpy(pick)] = torch.from_numpy(0.98 * np.abs(flows[g][pick]))
    return b._replace(rating=rating)


def _cap_over():
    b, p0s = _all_free(CAP)
    gens = b.gens.clone()
    p0 = p0s[1]
    for j, q in enumerate(NARROWED):
        pmax, pmin = float(gens[1, q, 1]), float(gens[1, q, 2])
        if j % 2 == 0:
            gens[1, q, 1] = float(p0[q] - 0.25 * (p0[q] - pmin))       # binds at Pmax
        else:
            gens[1, q, 2] = float(p0[q] + 0.25 * (pmax - p0[q]))       # binds at Pmin
    return b._replace(gens=gens)


FREE = {'free62': 62, 'free63': 63, 'free64': 64, 'cap_fits': CAP - 1}      # the all-free sets and their Gn
SETS = {name: functools.partial(lambda gn: _all_free(gn)[0], gn) for name, gn in FREE.items()}
SETS['free64_linear0'] = lambda: _all_free(64, linear=(0,))[0]
SETS['free70_lines'] = functools.partial(_with_lines, LINES_DRAW)
SETS['cap_over'] = _cap_over
cases.OTHER_SETS.update(SETS)

# what the adjoint is fed by the reference on (``test_adjoint_fed_by_the_reference``) and run through the public call on
REUSED = ('gn63', 'gn64', 'gn65', 'mixed_ratings', 'mixed_c2', 'low_pmin', 'wide')      # of dc_opf_pin_cases, every grid kept
FED_SETS = tuple(SETS) + REUSED + ('hub150_lp',)


@functools.lru_cache(maxsize=None)
def tight(name):
    """The float64 reference solved to 1e-11 on every grid of a set (computed once, not to be changed)."""
    return tuple(ref.solve(*p, tol=1e-11, max_iter=60, best=True) for p in cases.problems(name))


def counts(problem, result):
    """``(nf, k, margin)`` of one grid at ``result``, by the reference's own rule (``dc_opf_grad_reference.rows``)."""
    m, _, _, _, act, marg = gref.rows(problem, result)
    nl, gn = m['lim'].size, m['Gn']
    bound = act[2 * nl:2 * nl + gn] | act[2 * nl + gn:]
    return int(gn - bound.sum()), int(act[:2 * nl].sum()), marg


@functools.lru_cache(maxsize=None)
def orders(name):
    """``(nf, k, n, margin)`` of every grid of a set at the reference solved to 1e-11."""
    out = []
    for p, r in zip(cases.problems(name), tight(name)):
        nf, k, marg = counts(p, r)
        out.append((nf, k, nf + 1 + k, marg))
    return tuple(out)


def draw_lines(m=LINES_M, draws=range(40)):
    """The search behind ``LINES_DRAW``: the first draw at which both grids of ``_with_lines`` are solved to 1e-10, keep
    nf >= 65 and k >= m active lines, and have a margin of at least five times ``MARGIN_MIN``."""
    for draw in draws:
        b = _with_lines(draw, m)
        ok = True
        for p in cases.problems_of(b):
            r = ref.solve(*p, tol=1e-11, max_iter=60, best=True)
            nf, k, marg = counts(p, r)
            ok &= r['worst'] < 1e-10 and nf >= 65 and k >= m and marg >= 5 * gref.MARGIN_MIN
        if ok:
            return draw
    return None


def lds_queries(gn):
    """``(forward image bytes, adjoint image bytes, adjoint order cap)`` of ``_topology(gn)``, from the library's host queries."""
    tp = _topology(gn)
    fd = powerflow.analyse_fd_topology(tp.n, tp.f, tp.t, tp.g, tp.slack)
    forward = powerflow._screen_lds_bytes('gns_dcopf_lds_bytes', fd.host)[0]
    adjoint, cap = powerflow._screen_lds_bytes('gns_dcopf_adjoint_lds_bytes', fd.host)
    return forward, adjoint, cap


def check():
    """What the sets promise (module docstring).  Returns ``{set: orders(set)}``."""
    out = {}
    for name in SETS:
        b = cases.batch(name)
        assert b.buses.shape[0] == 2 and b.cost.dim() == 3 and b.rating.dim() == 2, name
        assert bool((b.cost[..., 0] >= 0.5).all()) or name == 'free64_linear0', name       # 2 c2 >= 1: the diagonal wins its column
        assert b.buses.shape[1] == b.gens.shape[1] + 4 <= 134, name
        for r, (nf, k, n, marg) in zip(tight(name), orders(name)):
            assert r['worst'] < 1e-10 and marg >= gref.MARGIN_MIN, (name, r['worst'], marg)       # every grid is kept
        out[name] = orders(name)
    for name, gn in FREE.items():
        assert cases.batch(name).gens.shape[1] == gn
        assert [(nf, k, n) for nf, k, n, _ in orders(name)] == [(gn, 0, gn + 1)] * 2, (name, orders(name))
    assert [o[2] for o in orders('free62') + orders('free63') + orders('free64')] == [63, 63, 64, 64, 65, 65]
    b = cases.batch('free64_linear0')
    assert bool((b.cost[:, 0, 0] == 0).all()) and bool((b.cost[:, 1:, 0] >= 0.5).all())
    assert [o[:3] for o in orders('free64_linear0')] == [(64, 0, 65)] * 2, orders('free64_linear0')
    assert cases.batch('free70_lines').gens.shape[1] == 70
    assert all(nf >= 65 and k >= 3 for nf, k, _, _ in orders('free70_lines')), orders('free70_lines')
    # the cap, from the library: the forward's image fits; order = cap on cap_fits; cap + 1 on grid 0 of cap_over, <= cap on grid 1
    for name, gn in (('cap_fits', CAP - 1), ('cap_over', CAP)):
        forward, adjoint, cap = lds_queries(gn)
        assert cases.batch(name).gens.shape[1] == gn
        assert forward <= pt.LDS_LIMIT and adjoint <= pt.LDS_LIMIT and cap == CAP, (name, forward, adjoint, cap)
    assert [o[2] for o in orders('cap_fits')] == [CAP, CAP]
    over = orders('cap_over')
    assert over[0][:3] == (CAP, 0, CAP + 1) and over[1][2] <= CAP and over[1][0] == CAP - len(NARROWED), over
    return out
