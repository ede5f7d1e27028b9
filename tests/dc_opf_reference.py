"""Test-side float64 DC optimal power flow (dense numpy), written independently of the product code from PYPOWER's dcopf /
dcopf_solver and PIPS, as the reference of the DC OPF tests.

It works in the full ``(theta_r, p)`` formulation: the N bus balances are equalities with one multiplier each, every iteration forms
and solves the whole dense KKT system with ``Bbus``; there are no shift factors and no reduced matrix.  What it shares with the
product is the contract of ``include/gns_powerflow.h`` ("DC optimal power flow"): the start (p at the midpoint of the bounds, theta
the DC solution there, z = max(1, -h), gamma = 1, mu = gamma / z, lambda = 0), PIPS's step rule (xi = 0.99995, separate primal and
dual lengths, sigma = 0.1), ``delta trace / Gn`` on the diagonal of the Hessian's p block with delta = 1e-14, and the three termination
quantities tested before every update.  The locational marginal prices are minus the bus balances' multipliers.
Its iteration count is not the contract's: its termination figures take ``|x|_inf`` with theta in x where the contract has ``|p|_inf``,
so it can stop an iteration or two earlier; ``dc_opf_reduced_reference`` follows the contract's figures and is what pins the count.

Default tolerance.  The probe ``probe_default_tol()`` runs this reference at 1e-8, 1e-7 and 1e-6 on every grid of every set of
``dc_opf_cases`` and reports the tightest at which all converge within 150 iterations.  Outcome (CPU, all 13 sets, 28 grids):
every grid converges at 1e-6 in 7 to 19 iterations, at 1e-7 in 8 to 20 and at 1e-8 in 9 to 21; so the default ``tol`` of
``powerflow.dc_optimal_power_flow`` is 1e-8.  At 1e-11 the gradient figure stops falling near 2e-11 on some grids (the rounding of
the dense KKT solve), which is why ``solve`` can return its best iterate (``best``)."""
import numpy as np

XI, SIGMA, DELTA = 0.99995, 0.1, 1e-14
DEFAULT_TOL, DEFAULT_MAX_ITER = 1e-8, 150


def make_bdc(lines, n_bus):
    """(Bbus [N,N], Bf [E,N], Pfinj [E], Pbusinj [N]) of makeBdc: b = 1 / (x tau), Pfinj = -b shift."""
    f, t = lines[:, 0].astype(int) - 1, lines[:, 1].astype(int) - 1
    b = 1.0 / (lines[:, 3] * lines[:, 5])
    E = lines.shape[0]
    Bf = np.zeros((E, n_bus))
    np.add.at(Bf, (np.arange(E), f), b)
    np.add.at(Bf, (np.arange(E), t), -b)
    Cft = np.zeros((E, n_bus))
    np.add.at(Cft, (np.arange(E), f), 1.0)
    np.add.at(Cft, (np.arange(E), t), -1.0)
    pfinj = -b * lines[:, 6]
    return Cft.T @ Bf, Bf, pfinj, Cft.T @ pfinj


def _model(buses, lines, gens, cost, rating, slack_bus):
    """The matrices of the (theta_r, p) problem of one grid (float64 numpy inputs, 1-based slack)."""
    N, E, Gn = buses.shape[0], lines.shape[0], gens.shape[0]
    s = int(slack_bus) - 1
    r = np.array([i for i in range(N) if i != s], dtype=int)
    Bbus, Bf, pfinj, pbusinj = make_bdc(lines, N)
    Cg = np.zeros((N, Gn))
    Cg[gens[:, 0].astype(int) - 1, np.arange(Gn)] = 1.0
    load = buses[:, 2] + buses[:, 4] + pbusinj
    rating = np.full(E, np.inf) if rating is None else np.asarray(rating, dtype=np.float64)
    lim = np.flatnonzero(np.isfinite(rating))
    nth = N - 1
    # equalities G v = load: -Bbus[:, r] theta_r + Cg p = load
    G = np.hstack([-Bbus[:, r], Cg])
    # inequalities A v <= ub
    A = np.zeros((2 * lim.size + 2 * Gn, nth + Gn))
    A[:lim.size, :nth] = Bf[lim][:, r]
    A[lim.size:2 * lim.size, :nth] = -Bf[lim][:, r]
    A[2 * lim.size:2 * lim.size + Gn, nth:] = np.eye(Gn)
    A[2 * lim.size + Gn:, nth:] = -np.eye(Gn)
    ub = np.concatenate([rating[lim] - pfinj[lim], rating[lim] + pfinj[lim], gens[:, 1], -gens[:, 2]])
    c2, c1 = np.asarray(cost, dtype=np.float64)[:, 0], np.asarray(cost, dtype=np.float64)[:, 1]
    return dict(N=N, E=E, Gn=Gn, s=s, r=r, Bbus=Bbus, Bf=Bf, pfinj=pfinj, Cg=Cg, load=load, rating=rating, lim=lim, nth=nth, G=G, A=A,
                ub=ub, c2=c2, c1=c1, pmin=gens[:, 2], pmax=gens[:, 1])


def solve(buses, lines, gens, cost, rating, slack_bus, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, delta=DELTA, best=False):
    """The optimum of one grid: a dict of pg, theta, line_flow, lmp, mu_line, mu_pmax, mu_pmin, objective, converged, iterations and
    worst (the largest of the three termination figures at the returned iterate).  ``best``: a run that does not reach ``tol``
    returns its iterate with the smallest ``worst`` rather than its last one (what a tolerance below the rounding floor of the
    dense KKT solve gives: the figures bottom out and then grow)."""
    with np.errstate(all='ignore'):
        return _solve(buses, lines, gens, cost, rating, slack_bus, tol, max_iter, delta, best)


def _solve(buses, lines, gens, cost, rating, slack_bus, tol, max_iter, delta, best):
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
    m = _model(buses, lines, gens, cost, rating, slack_bus)
    N, Gn, nth, r, G, A, ub = m['N'], m['Gn'], m['nth'], m['r'], m['G'], m['A'], m['ub']
    n, nl = nth + Gn, m['lim'].size
    H = np.zeros(n)
    H[nth:] = 2.0 * m['c2']
    c = np.zeros(n)
    c[nth:] = m['c1']
    p0 = 0.5 * (m['pmin'] + m['pmax'])
    x = np.zeros(n)
    x[nth:] = p0
    if nth:
        x[:nth] = np.linalg.solve(m['Bbus'][np.ix_(r, r)], (m['Cg'] @ p0 - m['load'])[r])
    lam = np.zeros(N)
    h = A @ x - ub
    z = np.where(-h > 1.0, -h, 1.0)
    gamma = 1.0
    mu = gamma / z
    converged, it, kept = False, 0, None
    while True:
        g = G @ x - m['load']
        h = A @ x - ub
        Lx = H * x + c + G.T @ lam + A.T @ mu
        feas = max(np.abs(g).max(), h.max()) / (1.0 + max(np.abs(x).max(), np.abs(z).max()))
        grad = np.abs(Lx).max() / (1.0 + max(np.abs(lam).max(), np.abs(mu).max()))
        comp = (z @ mu) / (1.0 + np.abs(x).max())
        worst = max(feas, grad, comp)
        if worst == worst and (kept is None or worst < kept[0]):
            kept = (worst, x, lam, mu, it)
        if feas < tol and grad < tol and comp < tol:
            converged = True
            break
        if it >= max_iter:
            break
        M = np.diag(H) + A.T @ ((mu / z)[:, None] * A)
        # the contract's shift is scaled to the Gn x Gn matrix in p.  Here that is the p block, delta trace(M_pp) / Gn on its
        # diagonal alone: the theta block carries b^2 mu / z, orders of magnitude above the costs, and a shift scaled by its trace
        # moved the accepted dispatch by 1e-5 at delta = 1e-12 (measured on hub150_qp), which no yardstick should do
        pp = np.arange(nth, n)
        M[pp, pp] += delta * M[pp, pp].sum() / Gn
        Nv = Lx + A.T @ ((gamma + mu * h) / z)
        K = np.block([[M, G.T], [G, np.zeros((N, N))]])
        try:
            sol = np.linalg.solve(K, np.concatenate([-Nv, -g]))
        except np.linalg.LinAlgError:
            break
        if not np.all(np.isfinite(sol)):
            break
        dx, dlam = sol[:n], sol[n:]
        dz = -h - z - A @ dx
        dmu = -mu + (gamma - mu * dz) / z
        k = dz < 0
        ap = min(XI * np.min(z[k] / -dz[k]), 1.0) if k.any() else 1.0
        k = dmu < 0
        ad = min(XI * np.min(mu[k] / -dmu[k]), 1.0) if k.any() else 1.0
        x, z, lam, mu = x + ap * dx, z + ap * dz, lam + ad * dlam, mu + ad * dmu
        gamma = SIGMA * (z @ mu) / z.size
        it += 1
    if best and not converged and kept is not None:
        worst, x, lam, mu, it = kept
    theta = np.zeros(N)
    theta[r] = x[:nth]
    pg = x[nth:]
    mu_line = np.zeros(m['E'])
    mu_line[m['lim']] = mu[:nl] - mu[nl:2 * nl]
    return dict(pg=pg, theta=theta, line_flow=m['Bf'] @ theta + m['pfinj'], lmp=-lam, mu_line=mu_line,
                mu_pmax=mu[2 * nl:2 * nl + Gn].copy(), mu_pmin=mu[2 * nl + Gn:].copy(), objective=float(m['c2'] @ pg ** 2 + m['c1'] @ pg),
                converged=converged, iterations=it, worst=worst)


def kkt_residuals(result, inputs):
    """The termination quantities, the dual signs and the primal feasibility of one grid, recomputed in float64 from the returned
    values alone (pg, theta, lmp, mu_line, mu_pmax, mu_pmin) and ``inputs = (buses, lines, gens, cost, rating, slack_bus)``.  The
    slacks are taken as z = max(-h, 0), the line multipliers as the positive and the negative part of mu_line, the bus balances'
    multipliers as -lmp.  Returns a dict: feas, grad, comp (PIPS's three figures), max_h (the worst inequality, <= 0 when
    feasible), max_g (the worst bus balance), feas_scale (1 + max(|x|_inf, |z|_inf), what feas divides them by), min_mu (the smallest
    of mu_pmax and mu_pmin), mu_off (mu_line on the lines whose slack is not small, see below) and scale, the largest of 1, |x|_inf,
    |lmp|_inf and |mu|_inf."""
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in inputs[:3])
    m = _model(buses, lines, gens, inputs[3], inputs[4], inputs[5])
    get = lambda k: np.asarray(result[k], dtype=np.float64)     # noqa: E731
    pg, theta, lmp, mu_line, mu_pmax, mu_pmin = (get(k) for k in ('pg', 'theta', 'lmp', 'mu_line', 'mu_pmax', 'mu_pmin'))
    lim, r = m['lim'], m['r']
    flow = m['Bf'] @ theta + m['pfinj']
    g = -m['Bbus'] @ theta + m['Cg'] @ pg - m['load']
    h = np.concatenate([flow[lim] - m['rating'][lim], -flow[lim] - m['rating'][lim], pg - m['pmax'], m['pmin'] - pg])
    mu = np.concatenate([np.maximum(mu_line[lim], 0.0), np.maximum(-mu_line[lim], 0.0), mu_pmax, mu_pmin])
    z = np.maximum(-h, 0.0)
    x = np.concatenate([theta, pg])
    lx_p = 2.0 * m['c2'] * pg + m['c1'] - m['Cg'].T @ lmp + mu_pmax - mu_pmin
    lx_th = m['Bbus'][r] @ lmp + m['Bf'][:, r].T @ mu_line
    lx = np.concatenate([lx_th, lx_p])
    xmax, mumax = np.abs(x).max(), max(np.abs(mu).max(), 0.0)
    # a line's own product mu_l z_l is at most z.mu <= comp (1 + |x|_inf), so |mu_line_l| min(1, slack_l / (1 + |x|_inf)) <= comp:
    # the multiplier itself where the slack is not small (a line without a limit has an infinite slack), a share of it elsewhere
    slack = np.maximum(np.minimum(m['rating'] - flow, m['rating'] + flow), 0.0)
    mu_off = (np.abs(mu_line) * np.minimum(1.0, slack / (1.0 + xmax))).max()
    return dict(feas=max(np.abs(g).max(), h.max()) / (1.0 + max(xmax, z.max())),
                grad=np.abs(lx).max() / (1.0 + max(np.abs(lmp).max(), mumax)),
                comp=(z @ mu) / (1.0 + xmax), max_h=h.max(), max_g=np.abs(g).max(), feas_scale=1.0 + max(xmax, z.max()),
                min_mu=min(mu_pmax.min(), mu_pmin.min()), mu_off=mu_off, scale=max(1.0, xmax, np.abs(lmp).max(), mumax))


def optimal_cost(buses, lines, gens, cost, rating, slack_bus, tol=1e-11):
    """The optimal cost alone, at a tight tolerance: what the central differences of the lmp test evaluate."""
    return solve(buses, lines, gens, cost, rating, slack_bus, tol=tol, max_iter=60, best=True)['objective']


def probe_default_tol():
    """The tightest of 1e-8, 1e-7, 1e-6 at which this reference converges on every grid of every set of ``dc_opf_cases``; prints
    the iteration range per tolerance."""
    import dc_opf_cases as cases
    best = None
    for tol in (1e-6, 1e-7, 1e-8):
        its, ok = [], True
        for name in cases.SETS:
            for inputs in cases.problems(name):
                res = solve(*inputs, tol=tol)
                ok &= res['converged']
                its.append(res['iterations'])
        print(f'tol {tol:g}: every grid converged: {ok}; iterations {min(its)} .. {max(its)} over {len(its)} grids')
        if ok:
            best = tol
    return best


if __name__ == '__main__':
    print('default tol:', probe_default_tol())
