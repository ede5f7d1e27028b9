"""Test-side float64 gradient of the DC optimal power flow (dense numpy), the reference of the DC OPF gradient tests.

It differentiates the optimum ``dc_opf_reference.solve`` returns for one grid by the implicit-function theorem on the KKT conditions
of the full ``(theta_r, p)`` formulation (``dc_opf_reference._model``): the N bus balances are equalities with one multiplier each,
the rows of ``A`` that are active are held as equalities, the multipliers of the others are constants.  One dense
``numpy.linalg.solve`` of the whole symmetric system

    [ H    G^T   Aa^T ] [a_x  ]   [dl/dx  ]
    [ G    0     0    ] [a_lam] = [dl/dlam]
    [ Aa   0     0    ] [a_mu ]   [dl/dmu ]

gives the adjoint; there are no shift factors and no reduced matrix, so it shares no algebra with the product's backward.  A row is
active when its multiplier exceeds its slack, ``mu_i > max(z_i, 0)`` with ``z = ub - A x``; the grid's margin is
``min_i max(z_i, mu_i)`` over every inequality row: at a margin near zero a row is neither clearly active nor clearly inactive and
the optimum has no derivative.

The loss is a weighted sum of the eight outputs, ``sum_k <weights[k], out[k]>`` (a missing weight is zero).  With ``F(u, d) = 0`` the
KKT conditions in the unknowns ``u = (x, lam, mu_a)`` and the data ``d``, the gradient is ``dl/dd - a^T dF/dd``:

    Pd_i, Gs_i    the load of balance i                         +a_lam_i
    c1_g          the stationarity row of p_g                   -a_p_g       + w_objective p_g
    c2_g                                                        -2 p_g a_p_g + w_objective p_g^2
    rating_l      ub of the line's active row (upper or lower)  +a_mu
    Pmax_g        ub of the unit's upper row                    +a_mu
    Pmin_g        ub = -Pmin of the unit's lower row            -a_mu
"""
import functools

import numpy as np

import dc_opf_reference as ref

OUTPUTS = ('pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective')
INPUTS = ('Pd', 'c2', 'c1', 'Pmax', 'Pmin', 'rating')


def loss(result, weights):
    """``sum_k <weights[k], result[k]>`` in float64."""
    return float(sum(np.sum(np.asarray(w, dtype=np.float64) * np.asarray(result[k], dtype=np.float64)) for k, w in weights.items()))


def rows(problem, result):
    """The model, the point ``x``, every row's slack and multiplier, the active mask and the margin of one grid at ``result``."""
    buses, lines, gens = (np.asarray(v, dtype=np.float64) for v in problem[:3])
    m = ref._model(buses, lines, gens, problem[3], problem[4], problem[5])
    lim = m['lim']
    pg, theta, mu_line = (np.asarray(result[k], dtype=np.float64) for k in ('pg', 'theta', 'mu_line'))
    x = np.concatenate([theta[m['r']], pg])
    z = m['ub'] - m['A'] @ x
    mu = np.concatenate([np.maximum(mu_line[lim], 0.0), np.maximum(-mu_line[lim], 0.0), np.asarray(result['mu_pmax'], dtype=np.float64),
                         np.asarray(result['mu_pmin'], dtype=np.float64)])
    act = mu > np.maximum(z, 0.0)
    return m, x, z, mu, act, float(np.min(np.maximum(z, mu)))


def margin(problem, result):
    return rows(problem, result)[5]


def gradients(problem, result, weights):
    """The gradients of ``loss(result, weights)`` with respect to ``Pd`` [N] (``Gs`` gets the same), ``c2``, ``c1``, ``Pmax``,
    ``Pmin`` [Gn] and ``rating`` [E] (0 at a line without a limit), and ``margin``, for one grid: ``problem`` as
    ``dc_opf_cases.problems`` lists it, ``result`` what ``dc_opf_reference.solve`` returned for it."""
    m, x, z, mu, act, marg = rows(problem, result)
    N, E, Gn, nth, r, lim = m['N'], m['E'], m['Gn'], m['nth'], m['r'], m['lim']
    nl, n = lim.size, nth + Gn
    w = {k: np.zeros_like(np.asarray(result[k], dtype=np.float64)) for k in OUTPUTS}
    for k, v in weights.items():
        w[k] = np.asarray(v, dtype=np.float64)
    p = x[nth:]
    w_obj = float(w['objective'])
    # the cotangents of (x, lam, mu): theta and line_flow = Bf theta + Pfinj, pg and the objective, lmp = -lam, mu_line = mu_u - mu_d
    gx = np.concatenate([w['theta'][r] + m['Bf'][:, r].T @ w['line_flow'], w['pg'] + w_obj * (2.0 * m['c2'] * p + m['c1'])])
    glam = -w['lmp']
    gmu = np.concatenate([w['mu_line'][lim], -w['mu_line'][lim], w['mu_pmax'], w['mu_pmin']])
    ia = np.flatnonzero(act)
    Aa = m['A'][ia]
    na = ia.size
    K = np.zeros((n + N + na, n + N + na))
    K[np.arange(nth, n), np.arange(nth, n)] = 2.0 * m['c2']
    K[:n, n:n + N] = m['G'].T
    K[n:n + N, :n] = m['G']
    K[:n, n + N:] = Aa.T
    K[n + N:, :n] = Aa
    a = np.linalg.solve(K, np.concatenate([gx, glam, gmu[ia]]))
    a_p, a_lam = a[nth:n], a[n:n + N]
    a_mu = np.zeros(mu.size)
    a_mu[ia] = a[n + N:]
    rating = np.zeros(E)
    rating[lim] = a_mu[:nl] + a_mu[nl:2 * nl]
    return dict(Pd=a_lam.copy(), c2=-2.0 * p * a_p + w_obj * p * p, c1=-a_p + w_obj * p, Pmax=a_mu[2 * nl:2 * nl + Gn].copy(),
                Pmin=-a_mu[2 * nl + Gn:], rating=rating, margin=marg)


def perturbed(problem, name, index, step):
    """``problem`` with entry ``index`` of input ``name`` moved by ``step`` (a copy)."""
    buses, lines, gens, cost, rating, slack = problem
    buses, gens, cost, rating = buses.copy(), gens.copy(), np.array(cost, dtype=np.float64), np.array(rating, dtype=np.float64)
    if name == 'Pd':
        buses[index, 2] += step
    elif name in ('c2', 'c1'):
        cost[index, 0 if name == 'c2' else 1] += step
    elif name in ('Pmax', 'Pmin'):
        gens[index, 1 if name == 'Pmax' else 2] += step
    else:
        rating[index] += step
    return buses, lines, gens, cost, rating, slack


def central_difference(problem, weights, name, index, step=1e-5, tol=1e-11):
    """``(l(+step) - l(-step)) / (2 step)`` of the loss at the reference's own optimum, solved to ``tol``."""
    vals = [loss(ref.solve(*perturbed(problem, name, index, s), tol=tol, max_iter=60, best=True), weights) for s in (+step, -step)]
    return (vals[0] - vals[1]) / (2.0 * step)


def random_weights(problem, rng, only=None):
    """One random weighting of the eight outputs (``only``: of that output alone), entries uniform in [-1, 1]."""
    N, E, Gn = problem[0].shape[0], problem[1].shape[0], problem[2].shape[0]
    shapes = dict(pg=Gn, theta=N, line_flow=E, lmp=N, mu_line=E, mu_pmax=Gn, mu_pmin=Gn, objective=())
    w = {k: rng.uniform(-1.0, 1.0, shapes[k]) for k in OUTPUTS}       # every output draws, so a weighting does not depend on `only`
    return {k: v for k, v in w.items() if only is None or k == only}


MARGIN_MIN = 1e-4        # a grid whose margin is below this has no derivative worth comparing: the tests leave it out


@functools.lru_cache(maxsize=None)
def kept_grids(name):
    """The grids of a set of ``dc_opf_cases`` the gradient tests keep: those whose margin, at the reference's optimum solved to
    1e-11, is at least ``MARGIN_MIN``.  Returns ``(kept indices, margins of every grid)``."""
    import dc_opf_cases as cases
    margins = [margin(p, ref.solve(*p, tol=1e-11, max_iter=60, best=True)) for p in cases.problems(name)]
    return tuple(g for g, x in enumerate(margins) if x >= MARGIN_MIN), tuple(margins)


def set_weights(name, only=None, seed=20):
    """The seeded random weighting of every grid of a set (``only``: of that output alone), a list of dicts.  A set of
    ``dc_opf_cases.SETS`` draws from its place among them; any other name from a place of its own past ``len(SETS)``, the CRC-32 of
    the name, so that no set registered later moves it."""
    import zlib
    import dc_opf_cases as cases
    names = sorted(cases.SETS)
    place = names.index(name) if name in cases.SETS else len(names) + zlib.crc32(name.encode())
    return [random_weights(p, np.random.default_rng([seed, place, g]), only) for g, p in enumerate(cases.problems(name))]
