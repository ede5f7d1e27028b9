"""Test-side float64 transcription (dense numpy) of the method of ``include/gns_powerflow.h``, "DC optimal power flow", written from
the contract's text and not from the kernels: the problem reduced to the dispatch ``p`` by generator shift factors, one scalar
``lambda`` for the balance ``sum p = demand``, the ``Gn x Gn`` matrix ``M`` with ``delta trace(M) / Gn`` on its diagonal, and the
contract's three termination figures with ``|p|_inf`` (``dc_opf_reference`` puts ``|x|_inf`` with theta there, so its iteration
count is not the contract's; its iterates are, see ``tests/test_dc_opf_iterates_host.py``).

What it is for: the iterate after exactly ``k`` updates (``iterate``), ``k = 0`` included, and on a run to ``tol`` (``solve``) the
iteration count and the worst termination figure at every test.  ``S`` and ``f0`` come from ``np.linalg.solve`` on ``Bbus[r, r]``,
the two systems in ``M`` from ``np.linalg.solve`` too (no Cholesky factorisation, no packed triangle, no tiles).

Rows of ``A_in``, in this order: the limited lines' upper limits, their lower limits, ``p <= Pmax``, ``-p <= -Pmin``."""
import numpy as np

import dc_opf_reference as full

XI, SIGMA, DELTA = 0.99995, 0.1, 1e-14
DEFAULT_TOL, DEFAULT_MAX_ITER = full.DEFAULT_TOL, full.DEFAULT_MAX_ITER


def model(buses, lines, gens, cost, rating, slack_bus):
    """The reduced problem of one grid (float64 numpy inputs, 1-based slack): S [E,Gn], f0 [E], PTDF [E,N] (a zero column at the
    slack), the stacked A_in and its right-hand side ub (h = A_in p - ub), the costs, the bounds and the demand."""
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
    N, E, Gn = buses.shape[0], lines.shape[0], gens.shape[0]
    s = int(slack_bus) - 1
    r = np.array([i for i in range(N) if i != s], dtype=int)
    Bbus, Bf, pfinj, pbusinj = full.make_bdc(lines, N)
    Cg = np.zeros((N, Gn))
    Cg[gens[:, 0].astype(int) - 1, np.arange(Gn)] = 1.0
    ptdf = np.zeros((E, N))
    f0 = pfinj.copy()
    if r.size:
        ptdf[:, r] = np.linalg.solve(Bbus[np.ix_(r, r)], Bf[:, r].T).T          # Bbus[r, r] is symmetric
        f0 = f0 + Bf[:, r] @ np.linalg.solve(Bbus[np.ix_(r, r)], -(buses[:, 2] + buses[:, 4] + pbusinj)[r])
    S = ptdf @ Cg
    rating = np.full(E, np.inf) if rating is None else np.asarray(rating, dtype=np.float64)
    lim = np.flatnonzero(np.isfinite(rating))
    A = np.vstack([S[lim], -S[lim], np.eye(Gn), -np.eye(Gn)])
    ub = np.concatenate([rating[lim] - f0[lim], rating[lim] + f0[lim], gens[:, 1], -gens[:, 2]])
    cost = np.asarray(cost, dtype=np.float64)
    return dict(N=N, E=E, Gn=Gn, lim=lim, S=S, f0=f0, ptdf=ptdf, A=A, ub=ub, c2=cost[:, 0], c1=cost[:, 1], pmin=gens[:, 2],
                pmax=gens[:, 1], demand=float((buses[:, 2] + buses[:, 4]).sum()))


def _figures(m, p, z, mu, lam):
    g = p.sum() - m['demand']
    h = m['A'] @ p - m['ub']
    Lx = 2.0 * m['c2'] * p + m['c1'] + lam + m['A'].T @ mu
    pinf = np.abs(p).max()
    feas = max(abs(g), h.max()) / (1.0 + max(pinf, np.abs(z).max()))
    grad = np.abs(Lx).max() / (1.0 + max(abs(lam), np.abs(mu).max()))
    comp = (z @ mu) / (1.0 + pinf)
    return g, h, Lx, (feas, grad, comp)


def _result(m, p, z, mu, lam, z0, it, converged, worst):
    nl, Gn = m['lim'].size, m['Gn']
    mu_line = np.zeros(m['E'])
    mu_line[m['lim']] = mu[:nl] - mu[nl:2 * nl]
    lmp = -lam - m['ptdf'].T @ mu_line
    return dict(pg=p.copy(), mu_line=mu_line, mu_pmax=mu[2 * nl:2 * nl + Gn].copy(), mu_pmin=mu[2 * nl + Gn:].copy(), lam=float(lam),
                lmp=lmp, objective=float(m['c2'] @ p ** 2 + m['c1'] @ p), line_flow=m['f0'] + m['S'] @ p, iterations=it,
                converged=converged, worst=worst,
                z0_line=z0[:2 * nl].copy(), z0_box=z0[2 * nl:].copy())


def solve(buses, lines, gens, cost, rating, slack_bus, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
    """The contract's iteration on one grid.  A dict of the last iterate (pg, mu_line, mu_pmax, mu_pmin, lam, lmp, objective,
    line_flow), ``iterations`` (the updates made), ``converged``, ``worst`` (the largest of the three figures at every test, in
    order: ``len(worst) == iterations + 1``), and the start's slacks ``z0_line`` (upper rows, then lower) and ``z0_box``."""
    with np.errstate(all='ignore'):
        m = model(buses, lines, gens, cost, rating, slack_bus)
        A, ub, Gn = m['A'], m['ub'], m['Gn']
        p = 0.5 * (m['pmin'] + m['pmax'])
        h = A @ p - ub
        z = np.where(-h > 1.0, -h, 1.0)
        z0 = z.copy()
        gamma, lam = 1.0, 0.0
        mu = gamma / z
        it, converged, worst = 0, False, []
        while True:
            g, h, Lx, fig = _figures(m, p, z, mu, lam)
            worst.append(max(fig))
            if all(f < tol for f in fig):
                converged = True
                break
            if it >= max_iter:
                break
            M = np.diag(2.0 * m['c2']) + A.T @ ((mu / z)[:, None] * A)
            M[np.arange(Gn), np.arange(Gn)] += DELTA * np.trace(M) / Gn
            try:
                w = np.linalg.solve(M, -(Lx + A.T @ ((gamma + mu * h) / z)))
                u = np.linalg.solve(M, np.ones(Gn))
            except np.linalg.LinAlgError:
                break
            dlam = (w.sum() + g) / u.sum()
            dp = w - dlam * u
            dz = -h - z - A @ dp
            dmu = -mu + (gamma - mu * dz) / z
            if not (np.isfinite(dlam) and np.all(np.isfinite(dp)) and np.all(np.isfinite(dz)) and np.all(np.isfinite(dmu))):
                break
            k = dz < 0
            ap = min(XI * np.min(z[k] / -dz[k]), 1.0) if k.any() else 1.0
            k = dmu < 0
            ad = min(XI * np.min(mu[k] / -dmu[k]), 1.0) if k.any() else 1.0
            p, z, lam, mu = p + ap * dp, z + ap * dz, lam + ad * dlam, mu + ad * dmu
            gamma = SIGMA * (z @ mu) / z.size
            it += 1
        return _result(m, p, z, mu, lam, z0, it, converged, worst)


def iterate(buses, lines, gens, cost, rating, slack_bus, k):
    """The iterate after exactly ``k`` updates, from ``k`` alone: no tolerance ends the run (the figures are never below 0)."""
    out = solve(buses, lines, gens, cost, rating, slack_bus, tol=0.0, max_iter=k)
    assert out['iterations'] == k and not out['converged'], (k, out['iterations'])
    return out


def near_tie(worst, tol=DEFAULT_TOL):
    """Whether a run is a near tie: at some test its worst figure lies in [tol / 2, 2 tol], so that rounding may move the count by
    one."""
    return any(0.5 * tol <= w <= 2.0 * tol for w in worst)
