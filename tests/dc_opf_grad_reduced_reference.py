"""Test-side float64 transcription (dense numpy) of the reduced algebra of the DC optimal power flow's adjoint
(``include/gns_powerflow.h``, "DC optimal power flow: adjoint"), the second reference of the gradient pins: the yardstick of their
bars is how far it lies from ``dc_opf_grad_reference`` (the full ``(theta_r, p)`` formulation), so that the kernel is never its own
yardstick (the pattern of ``dc_opf_pin_cases.iterate_bar``).

The problem is reduced to the dispatch ``p`` by dense shift factors ``S = B_f,r A^-1 C_g,r`` with ``A = Bbus[r, r]``.  A unit is at
``Pmax`` when ``mu_pmax > max(Pmax - p, 0)``, else at ``Pmin`` when ``mu_pmin > max(p - Pmin, 0)``, else free; a line's upper limit is
active when ``mu_line > max(rating - flow, 0)``, its lower one when ``-mu_line > max(rating + flow, 0)``; the rule is strict.  With
``F`` the free units, ``b`` those on a bound and ``a`` the active lines, the adjoint of a unit on a bound is the cotangent of its own
multiplier, ``a_p,b = g_nu,b``, and the rest solves the symmetric system

    [ diag(2 c2_F)  1    S_aF^T ] [a_p,F   ]   [g_p,F                 ]
    [ 1^T           0    0      ] [a_lambda] = [g_lambda - 1^T a_p,b   ]
    [ S_aF          0    0      ] [a_mu    ]   [g_mu - S_ab a_p,b      ]

by ``numpy.linalg.solve``; ``a_nu,b = g_p,b - 2 c2_b a_p,b - a_lambda - S_ab^T a_mu`` from the stationarity rows.  The cotangents:
theta and line_flow pull back through ``t = A^-1 (w_theta,r + B_f,r^T w_flow)`` to ``C_g^T t`` on ``p`` and ``-t`` on the loads;
``lmp = -lambda - A^-1 B_f,r^T mu_line`` gives ``-sum w_lmp`` to lambda and ``-B_f,r A^-1 w_lmp,r`` to the active lines.  A third
network solve, ``v = A^-1 B_f,r^T a_mu``, carries ``a_mu`` through ``f0`` to the loads.

Inputs and the returned dict are ``dc_opf_grad_reference.gradients``'s."""
import numpy as np

import dc_opf_reference as full

OUTPUTS = ('pg', 'theta', 'line_flow', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin', 'objective')


def active_set(problem, result):
    """``(state [Gn]: 0 free, 1 at Pmax, 2 at Pmin; row [E]: +1 upper limit active, -1 lower, 0 neither; margin)`` of one grid."""
    gens, rating = np.asarray(problem[2], dtype=np.float64), np.asarray(problem[4], dtype=np.float64)
    get = lambda k: np.asarray(result[k], dtype=np.float64)     # noqa: E731
    p, flow, mu, mu_u, mu_d = get('pg'), get('line_flow'), get('mu_line'), get('mu_pmax'), get('mu_pmin')
    pmax, pmin = gens[:, 1], gens[:, 2]
    at_max = mu_u > np.maximum(pmax - p, 0.0)
    at_min = ~at_max & (mu_d > np.maximum(p - pmin, 0.0))
    state = np.where(at_max, 1, np.where(at_min, 2, 0))
    lim = np.isfinite(rating)
    row = np.zeros(rating.size, dtype=int)
    up = lim & (mu > np.maximum(rating - flow, 0.0))
    down = lim & ~up & (-mu > np.maximum(rating + flow, 0.0))
    row[up], row[down] = 1, -1
    z = np.concatenate([(rating - flow)[lim], (rating + flow)[lim], pmax - p, p - pmin])
    m = np.concatenate([np.maximum(mu[lim], 0.0), np.maximum(-mu[lim], 0.0), mu_u, mu_d])
    return state, row, float(np.min(np.maximum(z, m)))


def gradients(problem, result, weights):
    """The gradients of ``sum_k <weights[k], result[k]>`` with respect to ``Pd`` [N] (``Gs`` gets the same), ``c2``, ``c1``,
    ``Pmax``, ``Pmin`` [Gn] and ``rating`` [E], and ``margin``, of one grid."""
    buses, lines, gens = (np.asarray(v, dtype=np.float64) for v in problem[:3])
    cost = np.asarray(problem[3], dtype=np.float64)
    N, E, Gn = buses.shape[0], lines.shape[0], gens.shape[0]
    r = np.array([i for i in range(N) if i != int(problem[5]) - 1], dtype=int)
    Bbus, Bf, _, _ = full.make_bdc(lines, N)
    A, Bfr = Bbus[np.ix_(r, r)], Bf[:, r]
    bus_of = gens[:, 0].astype(int) - 1

    def network(rhs_r):                       # A^-1 on the buses but the slack, 0 there
        out = np.zeros(N)
        if r.size:
            out[r] = np.linalg.solve(A, rhs_r)
        return out

    S = np.zeros((E, Gn))
    for q in range(Gn):
        e = np.zeros(N)
        e[bus_of[q]] = 1.0
        S[:, q] = Bf @ network(e[r])
    w = {k: np.zeros_like(np.asarray(result[k], dtype=np.float64)) for k in OUTPUTS}
    for k, v in weights.items():
        w[k] = np.asarray(v, dtype=np.float64)
    state, row, marg = active_set(problem, result)
    p = np.asarray(result['pg'], dtype=np.float64)
    c2, c1 = cost[:, 0], cost[:, 1]
    w_obj = float(w['objective'])
    F, b, a = np.flatnonzero(state == 0), np.flatnonzero(state != 0), np.flatnonzero(row != 0)
    nf, k = F.size, a.size
    # the cotangents of (p, lambda, mu_line at the active lines, nu at the units on a bound)
    t = network(w['theta'][r] + Bfr.T @ w['line_flow'])
    gp = w['pg'] + w_obj * (2.0 * c2 * p + c1) + t[bus_of]
    glam = -w['lmp'].sum()
    gmu = w['mu_line'] - Bf @ network(w['lmp'][r])
    gnu = np.where(state == 1, w['mu_pmax'], np.where(state == 2, -w['mu_pmin'], 0.0))
    # the system over the free units, the balance and the active lines
    n = nf + 1 + k
    K = np.zeros((n, n))
    K[np.arange(nf), np.arange(nf)] = 2.0 * c2[F]
    K[:nf, nf] = K[nf, :nf] = 1.0
    K[nf + 1:, :nf] = S[np.ix_(a, F)]
    K[:nf, nf + 1:] = S[np.ix_(a, F)].T
    rhs = np.concatenate([gp[F], [glam - gnu[b].sum()], gmu[a] - S[np.ix_(a, b)] @ gnu[b]])
    x = np.linalg.solve(K, rhs)
    a_p = gnu.copy()
    a_p[F] = x[:nf]
    a_lam = x[nf]
    a_mu = np.zeros(E)
    a_mu[a] = x[nf + 1:]
    a_nu = np.zeros(Gn)
    a_nu[b] = gp[b] - 2.0 * c2[b] * a_p[b] - a_lam - S[np.ix_(a, b)].T @ a_mu[a]
    v = network(Bfr.T @ a_mu)
    return dict(Pd=a_lam + v - t, c2=w_obj * p * p - 2.0 * p * a_p, c1=w_obj * p - a_p, Pmax=np.where(state == 1, a_nu, 0.0),
                Pmin=np.where(state == 2, a_nu, 0.0), rating=row * a_mu, margin=marg)
