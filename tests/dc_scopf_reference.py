"""Test-side float64 reference (dense numpy) of the security-constrained DC optimal power flow, independent of the line-outage
formula the product uses: for every distinct outage ``k`` it rebuilds the network without line ``k`` (``make_bdc`` on the remaining
lines) and takes that network's own shift factors and ``f0``; a row ``(l, k)`` is then line ``l``'s row of the network without
``k``.  No ``z_k``, no ``1 - b_k d_k``.

``solve`` runs the contract's iteration (PIPS as in ``dc_opf_reduced_reference``) with the rows behind the lines' rows:
``A_in = [S_lim; -S_lim; S_rows; -S_rows; I; -I]``.  ``solve_full`` solves the same problem in the full formulation, one angle
vector per network (the base and each outage) with the bus balances of each as equalities (the slack's only once: every network's
balances sum to the same ``sum p = demand``); the two must agree.  The locational
marginal price is the derivative of the optimal cost with respect to ``Pd``: in the full formulation minus the sum of the balance
multipliers over all networks, in the reduced one ``-lambda - PTDF^T mu_line - sum_r PTDF_k(r)[l_r]^T mu_r``.

``post_flows`` gives the float64 post-outage flows of a dispatch, ``generate`` the reference's own constraint generation."""
import numpy as np

import dc_opf_reference as full
import dc_opf_reduced_reference as red

XI, SIGMA, DELTA = red.XI, red.SIGMA, red.DELTA
DEFAULT_TOL, DEFAULT_MAX_ITER = red.DEFAULT_TOL, red.DEFAULT_MAX_ITER


def bridges(n_bus, lines):
    """bool [E]: lines whose removal disconnects the grid, by connectivity of the graph without each (quadratic, test-sized)."""
    f, t = lines[:, 0].astype(int) - 1, lines[:, 1].astype(int) - 1
    out = np.zeros(f.size, dtype=bool)
    for k in range(f.size):
        seen, stack = {0}, [0]
        adj = [[] for _ in range(n_bus)]
        for e in range(f.size):
            if e != k:
                adj[f[e]].append(t[e])
                adj[t[e]].append(f[e])
        while stack:
            for j in adj[stack.pop()]:
                if j not in seen:
                    seen.add(j)
                    stack.append(j)
        out[k] = len(seen) < n_bus
    return out


def outage_models(buses, lines, gens, slack_bus, outages):
    """{k: (S [E,Gn], f0 [E], ptdf [E,N])} of the grid without line k, from the network rebuilt without it; zeros at line k."""
    E, Gn, N = lines.shape[0], gens.shape[0], buses.shape[0]
    out = {}
    for k in outages:
        keep = np.array([l for l in range(E) if l != k], dtype=int)
        m = red.model(buses, lines[keep], gens, np.zeros((Gn, 2)), None, slack_bus)
        S, f0, ptdf = np.zeros((E, Gn)), np.zeros(E), np.zeros((E, N))
        S[keep], f0[keep], ptdf[keep] = m['S'], m['f0'], m['ptdf']
        out[int(k)] = (S, f0, ptdf)
    return out


def post_flows(buses, lines, gens, slack_bus, pg, outages):
    """[K,E] float64: the flows at dispatch pg with each line of ``outages`` out (0 at the line itself)."""
    o = outage_models(buses, lines, gens, slack_bus, outages)
    return np.array([o[int(k)][1] + o[int(k)][0] @ pg for k in outages])


def _live(rows, rating_c):
    rows = np.asarray(rows, dtype=int).reshape(-1, 2)
    return [i for i, (l, k) in enumerate(rows) if not (l == -1 and k == -1) and np.isfinite(rating_c[l])]


def solve(buses, lines, gens, cost, rating, slack_bus, rows, rating_c, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, best=False):
    """The contract's iteration on one grid with the rows ``[R,2]`` (empty slots (-1, -1) and rows on a line without a contingency
    rating skipped).  A dict: pg, mu_line, mu_row [R] (0 in a skipped slot), row_flow [R] (NaN there), mu_pmax, mu_pmin, lam, lmp,
    objective, line_flow, iterations, converged, worst (the largest figure at the returned iterate), figures (the largest figure at
    every termination test of the run, in order: ``iterations + 1`` of them, so that a near tie can be judged over the whole run).
    ``best``: as ``dc_opf_reference.solve``."""
    with np.errstate(all='ignore'):
        buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
        rows = np.asarray(rows, dtype=int).reshape(-1, 2)
        m = red.model(buses, lines, gens, cost, rating, slack_bus)
        rating_c = m_rating(rating, lines.shape[0]) if rating_c is None else np.asarray(rating_c, dtype=np.float64)
        live = _live(rows, rating_c)
        nl, Gn, nr = m['lim'].size, m['Gn'], len(live)
        o = outage_models(buses, lines, gens, slack_bus, sorted({int(rows[i, 1]) for i in live}))
        Sr = np.array([o[rows[i, 1]][0][rows[i, 0]] for i in live]).reshape(nr, Gn)
        fr = np.array([o[rows[i, 1]][1][rows[i, 0]] for i in live])
        pr = np.array([o[rows[i, 1]][2][rows[i, 0]] for i in live]).reshape(nr, m['N'])
        rc = np.array([rating_c[rows[i, 0]] for i in live])
        A = np.vstack([m['A'][:2 * nl], Sr, -Sr, m['A'][2 * nl:]])
        ub = np.concatenate([m['ub'][:2 * nl], rc - fr, rc + fr, m['ub'][2 * nl:]])
        p = 0.5 * (m['pmin'] + m['pmax'])
        h = A @ p - ub
        z = np.where(-h > 1.0, -h, 1.0)
        gamma, lam = 1.0, 0.0
        mu = gamma / z
        it, converged, kept, figures = 0, False, None, []
        while True:
            g = p.sum() - m['demand']
            h = A @ p - ub
            Lx = 2.0 * m['c2'] * p + m['c1'] + lam + A.T @ mu
            pinf = np.abs(p).max()
            fig = (max(abs(g), h.max()) / (1.0 + max(pinf, np.abs(z).max())), np.abs(Lx).max() / (1.0 + max(abs(lam), np.abs(mu).max())),
                   (z @ mu) / (1.0 + pinf))
            worst = max(fig)
            figures.append(float(worst))
            if worst == worst and (kept is None or worst < kept[0]):
                kept = (worst, p, z, lam, mu, it)
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
        if best and not converged and kept is not None:
            worst, p, z, lam, mu, it = kept
        mu_line = np.zeros(m['E'])
        mu_line[m['lim']] = mu[:nl] - mu[nl:2 * nl]
        mr = mu[2 * nl:2 * nl + nr] - mu[2 * nl + nr:2 * nl + 2 * nr]
        mu_row, row_flow = np.zeros(rows.shape[0]), np.full(rows.shape[0], np.nan)
        mu_row[live], row_flow[live] = mr, fr + Sr @ p
        b = 2 * nl + 2 * nr
        return dict(pg=p.copy(), mu_line=mu_line, mu_row=mu_row, row_flow=row_flow, mu_pmax=mu[b:b + Gn].copy(), mu_pmin=mu[b + Gn:].copy(),
                    lam=float(lam), lmp=-lam - m['ptdf'].T @ mu_line - pr.T @ mr, objective=float(m['c2'] @ p ** 2 + m['c1'] @ p),
                    line_flow=m['f0'] + m['S'] @ p, iterations=it, converged=converged, worst=worst, figures=figures)


def m_rating(rating, E):
    return np.full(E, np.inf) if rating is None else np.asarray(rating, dtype=np.float64)


def row_values(buses, lines, gens, slack_bus, rows, pg):
    """[R] float64: the post-outage flow of every row at dispatch pg (NaN in an empty slot), and the rows' gradients [R,Gn]."""
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
    rows = np.asarray(rows, dtype=int).reshape(-1, 2)
    live = [i for i, (l, k) in enumerate(rows) if not (l == -1 and k == -1)]
    o = outage_models(buses, lines, gens, slack_bus, sorted({int(rows[i, 1]) for i in live}))
    val, S = np.full(rows.shape[0], np.nan), np.zeros((rows.shape[0], gens.shape[0]))
    for i in live:
        l, k = rows[i]
        S[i] = o[k][0][l]
        val[i] = o[k][1][l] + S[i] @ pg
    return val, S


def solve_full(buses, lines, gens, cost, rating, slack_bus, rows, rating_c, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, path=None):
    """The same problem with one angle vector per network: x = (theta_r of the base, theta_r of each distinct outage, p), the bus
    balances of every network as equalities.  A dict of pg, objective, lmp (minus the balance multipliers summed over the
    networks), mu_row [R], mu_line [E], mu_pmax, mu_pmin (the slices of mu that ``solve`` takes them from), converged, iterations.
    ``path``: a list that takes the same dict at every termination test, so that one run gives the iterate after 0, 1, 2, ... updates
    (what ``max_iter = k`` returns)."""
    with np.errstate(all='ignore'):
        buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
        rows = np.asarray(rows, dtype=int).reshape(-1, 2)
        E = lines.shape[0]
        rating_c = m_rating(rating, E) if rating_c is None else np.asarray(rating_c, dtype=np.float64)
        live = _live(rows, rating_c)
        outs = sorted({int(rows[i, 1]) for i in live})
        base = full._model(buses, lines, gens, cost, rating, slack_bus)
        N, Gn, nth, r = base['N'], base['Gn'], base['nth'], base['r']
        nets = [base] + [full._model(buses, lines[[l for l in range(E) if l != k]], gens, cost, None, slack_bus) for k in outs]
        nn = len(nets)
        n = nn * nth + Gn
        # the base network's N balances, and the N - 1 of every other network at the buses but the slack: a network's balances sum to
        # sum p = demand, which the base network states already
        neq = N + (nn - 1) * nth
        G = np.zeros((neq, n))
        load = np.concatenate([base['load']] + [m['load'][r] for m in nets[1:]])
        G[:N, :nth], G[:N, nn * nth:] = -base['Bbus'][:, r], base['Cg']
        for j, m in enumerate(nets[1:], 1):
            at = slice(N + (j - 1) * nth, N + j * nth)
            G[at, j * nth:(j + 1) * nth] = -m['Bbus'][np.ix_(r, r)]
            G[at, nn * nth:] = m['Cg'][r]
        nl, nr = base['lim'].size, len(live)
        A = np.zeros((2 * nl + 2 * nr + 2 * Gn, n))
        A[:nl, :nth] = base['Bf'][base['lim']][:, r]
        A[nl:2 * nl, :nth] = -base['Bf'][base['lim']][:, r]
        ubr = np.zeros((2, nr))
        for q, i in enumerate(live):
            l, k = rows[i]
            j = 1 + outs.index(k)
            lk = l if l < k else l - 1                             # line l's index in the network without k
            A[2 * nl + q, j * nth:(j + 1) * nth] = nets[j]['Bf'][lk, r]
            A[2 * nl + nr + q, j * nth:(j + 1) * nth] = -nets[j]['Bf'][lk, r]
            ubr[0, q], ubr[1, q] = rating_c[l] - nets[j]['pfinj'][lk], rating_c[l] + nets[j]['pfinj'][lk]
        A[2 * nl + 2 * nr:2 * nl + 2 * nr + Gn, nn * nth:] = np.eye(Gn)
        A[2 * nl + 2 * nr + Gn:, nn * nth:] = -np.eye(Gn)
        ub = np.concatenate([base['ub'][:2 * nl], ubr[0], ubr[1], base['ub'][2 * nl:]])
        H, c = np.zeros(n), np.zeros(n)
        H[nn * nth:], c[nn * nth:] = 2.0 * base['c2'], base['c1']
        p0 = 0.5 * (base['pmin'] + base['pmax'])
        x = np.zeros(n)
        x[nn * nth:] = p0
        for j, m in enumerate(nets):
            x[j * nth:(j + 1) * nth] = np.linalg.solve(m['Bbus'][np.ix_(r, r)], (m['Cg'] @ p0 - m['load'])[r])
        lam = np.zeros(neq)
        h = A @ x - ub
        z = np.where(-h > 1.0, -h, 1.0)
        gamma = 1.0
        mu = gamma / z
        converged, it = False, 0
        pp = np.arange(nn * nth, n)

        def result():
            pg = x[nn * nth:].copy()
            mu_row, mu_line = np.zeros(rows.shape[0]), np.zeros(E)
            mu_row[live] = mu[2 * nl:2 * nl + nr] - mu[2 * nl + nr:2 * nl + 2 * nr]
            mu_line[base['lim']] = mu[:nl] - mu[nl:2 * nl]
            lmp = -lam[:N].copy()
            lmp[r] -= lam[N:].reshape(nn - 1, nth).sum(axis=0)
            b = 2 * nl + 2 * nr
            return dict(pg=pg, objective=float(base['c2'] @ pg ** 2 + base['c1'] @ pg), lmp=lmp, mu_row=mu_row, mu_line=mu_line,
                        mu_pmax=mu[b:b + Gn].copy(), mu_pmin=mu[b + Gn:].copy(), converged=converged, iterations=it)

        while True:
            if path is not None:
                path.append(result())
            g = G @ x - load
            h = A @ x - ub
            Lx = H * x + c + G.T @ lam + A.T @ mu
            feas = max(np.abs(g).max(), h.max()) / (1.0 + max(np.abs(x).max(), np.abs(z).max()))
            grad = np.abs(Lx).max() / (1.0 + max(np.abs(lam).max(), np.abs(mu).max()))
            comp = (z @ mu) / (1.0 + np.abs(x).max())
            if feas < tol and grad < tol and comp < tol:
                converged = True
                break
            if it >= max_iter:
                break
            M = np.diag(H) + A.T @ ((mu / z)[:, None] * A)
            M[pp, pp] += DELTA * M[pp, pp].sum() / Gn
            K = np.block([[M, G.T], [G, np.zeros((neq, neq))]])
            try:
                sol = np.linalg.solve(K, np.concatenate([-(Lx + A.T @ ((gamma + mu * h) / z)), -g]))
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
        return result()


def all_rows(E, outages):
    """Every (l, k), k in outages, l != k, in the outages' order."""
    return np.array([(l, k) for k in outages for l in range(E) if l != k], dtype=int).reshape(-1, 2)


def generate(buses, lines, gens, cost, rating, slack_bus, rating_c, outages, rows_per_round, violation_tol, max_rounds=32):
    """The reference's own constraint generation: solve, take the ``rows_per_round`` worst pairs above ``1 + violation_tol`` that are not
    listed yet, until none is.  Returns (result, rows [R,2], rounds that added rows)."""
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
    rows, rounds = [], 0
    res = solve(buses, lines, gens, cost, rating, slack_bus, np.zeros((0, 2), dtype=int), rating_c)
    while rounds < max_rounds:
        load = np.abs(post_flows(buses, lines, gens, slack_bus, res['pg'], outages)) / np.asarray(rating_c)[None, :]
        cand = [(load[i, l], l, int(k)) for i, k in enumerate(outages) for l in range(lines.shape[0])
                if l != k and np.isfinite(rating_c[l]) and load[i, l] > 1.0 + violation_tol and (l, int(k)) not in rows]
        if not cand:
            break
        cand.sort(key=lambda c: -c[0])
        rows += [(l, k) for _, l, k in cand[:rows_per_round]]
        rounds += 1
        res = solve(buses, lines, gens, cost, rating, slack_bus, np.array(rows), rating_c)
    return res, np.array(rows, dtype=int).reshape(-1, 2), rounds


def kkt_residuals(result, inputs, rows, rating_c):
    """``dc_opf_reference.kkt_residuals`` extended by the rows, in the reduced variables: from the returned pg, lmp, mu_line, mu_row,
    mu_pmax, mu_pmin alone.  The stationarity in p is ``2 c2 p + c1 - Cg^T lmp + mu_pmax - mu_pmin`` (the lmp carries lambda and every
    congestion term, the rows' included, by its definition); the rows' feasibility and complementarity use the reference's own
    post-outage flows at the returned pg.  Returns grad, comp, max_h (over lines, rows and boxes), min_mu, scale."""
    buses, lines, gens, cost, rating, slack_bus = inputs
    buses, lines, gens = (np.asarray(x, dtype=np.float64) for x in (buses, lines, gens))
    m = red.model(buses, lines, gens, cost, rating, slack_bus)
    get = lambda k: np.asarray(result[k], dtype=np.float64)     # noqa: E731
    pg, lmp, mu_line, mu_row, mu_pmax, mu_pmin = (get(k) for k in ('pg', 'lmp', 'mu_line', 'mu_row', 'mu_pmax', 'mu_pmin'))
    rows = np.asarray(rows, dtype=int).reshape(-1, 2)
    rating_c = m_rating(rating, m['E']) if rating_c is None else np.asarray(rating_c, dtype=np.float64)
    live = _live(rows, rating_c)
    val, _ = row_values(buses, lines, gens, slack_bus, rows, pg)
    flow = m['f0'] + m['S'] @ pg
    lim = m['lim']
    rt = np.asarray(m_rating(rating, m['E']))
    rc = np.array([rating_c[rows[i, 0]] for i in live])
    h = np.concatenate([flow[lim] - rt[lim], -flow[lim] - rt[lim], val[live] - rc, -val[live] - rc, pg - m['pmax'], m['pmin'] - pg])
    mu = np.concatenate([np.maximum(mu_line[lim], 0.0), np.maximum(-mu_line[lim], 0.0), np.maximum(mu_row[live], 0.0),
                         np.maximum(-mu_row[live], 0.0), mu_pmax, mu_pmin])
    z = np.maximum(-h, 0.0)
    Cg = np.zeros((m['N'], m['Gn']))
    Cg[gens[:, 0].astype(int) - 1, np.arange(m['Gn'])] = 1.0
    lx = 2.0 * m['c2'] * pg + m['c1'] - Cg.T @ lmp + mu_pmax - mu_pmin
    # the lmp against its own definition from the multipliers: -lambda 1 - PTDF^T mu_line - sum_r PTDF_k[l]^T mu_r, lambda read at the slack
    o = outage_models(buses, lines, gens, slack_bus, sorted({int(rows[i, 1]) for i in live}))
    cong = m['ptdf'].T @ mu_line + sum((o[rows[i, 1]][2][rows[i, 0]] * mu_row[i] for i in live), np.zeros(m['N']))
    lmp_def = np.abs(lmp - (lmp[int(slack_bus) - 1] + cong[int(slack_bus) - 1] - cong)).max()
    xmax, mumax = np.abs(pg).max(), np.abs(mu).max()
    return dict(grad=np.abs(lx).max() / (1.0 + max(np.abs(lmp).max(), mumax)), comp=(z @ mu) / (1.0 + xmax), max_h=h.max(),
                feas_scale=1.0 + max(xmax, z.max()), lmp_def=lmp_def / (1.0 + max(np.abs(lmp).max(), mumax)),
                min_mu=min(mu_pmax.min(), mu_pmin.min()), scale=max(1.0, xmax, np.abs(lmp).max(), mumax))
