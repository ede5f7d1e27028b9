"""Test-side float64 gradient of the AC N-2 contingency screen (the reference for gns_acn2_adjoint), written independently of the
product code on ``ac_contingency_grad_reference``, ``ac_n2_reference`` and ``nr_grad_reference``.  Per (grid, (j, k)): both line rows
are deleted, the smaller grid is solved by the reference's own Newton-Raphson from the base solution (``ac_n2_reference.pair``), the
weighted loss of all nine outputs is built in torch complex128 (the flows from the full line list with both lines' zeroed), the
dense Jacobian of the mismatch is taken by autograd and the implicit function theorem applied:

    dl/dp = dl/dp|_x - lambda^T dF_jk/dp|_x,   J_jk^T lambda = dl/dx,

and two zero rows are inserted back into the line gradient.  The summaries follow ``ac_contingency_grad_reference``'s rules."""
import numpy as np
import torch

import ac_contingency_grad_reference as gref
import ac_contingency_reference as aref
import ac_n2_reference as n2ref
import nr_grad_reference as ngr

OUTPUTS = gref.OUTPUTS
DIFF_COLS = gref.DIFF_COLS


def row_loss(grid, x, rest, gen, out_lines, j, k, w, rating, at):
    """The weighted loss of row (j, k)'s nine outputs (j < k) at the unknowns x; ``rest`` is the line list without the two lines
    (``out_lines`` [2,7], constants)."""
    vm, th = ngr._state(grid, x, gen)
    full = torch.cat([rest[:j], out_lines[:1], rest[j:k - 1], out_lines[1:], rest[k - 1:]])
    sf, st = gref._flows(full, vm, th, [j, k])
    loss = torch.zeros((), dtype=torch.float64)
    for name, val in (('v', vm), ('theta', th), ('p_from', sf.real), ('q_from', sf.imag), ('p_to', st.real), ('q_to', st.imag)):
        if w.get(name) is not None:
            loss = loss + (torch.as_tensor(w[name], dtype=torch.float64) * val).sum()
    if w.get('worst_loading') is not None:
        af, at_ = sf.detach().abs().numpy(), st.detach().abs().numpy()
        load = np.maximum(af, at_) / (1.0 if rating is None else np.asarray(rating, dtype=np.float64))
        wi = at.get('worst_line', int(np.flatnonzero(load == load.max())[0]))
        if max(af[wi], at_[wi]) > 0.0:
            s = sf[wi].abs() if af[wi] >= at_[wi] else st[wi].abs()
            loss = loss + float(w['worst_loading']) * s / (1.0 if rating is None else float(np.asarray(rating)[wi]))
    vd = vm.detach().numpy()
    if w.get('v_min') is not None:
        loss = loss + float(w['v_min']) * vm[at.get('v_min_bus', int(np.flatnonzero(vd == vd.min())[0]))]
    if w.get('v_max') is not None:
        loss = loss + float(w['v_max']) * vm[at.get('v_max_bus', int(np.flatnonzero(vd == vd.max())[0]))]
    return loss


def row_gradient(buses, lines, generators, slack_bus, pair, row, w, rating=None, at=None):
    """d(weighted loss of the row of ``pair``)/d(buses, lines, generators) in float64 numpy at the reference's solved ``row`` (an
    ``ac_contingency_reference.Row`` of ``ac_n2_reference.pair``), and the condition number of the row's Jacobian.  ``w``: a dict of
    the weights of ``OUTPUTS`` ([N], [E] or scalars; a missing one is zero).  Either order of the pair is the same row."""
    at = at or {}
    j, k = min(pair), max(pair)
    assert j != k
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    rest = np.delete(ln, [j, k], axis=0)
    grid = ngr._Grid(bus, rest, gen, slack_bus)
    p = [torch.as_tensor(a).clone() for a in (bus, rest, gen)]
    out_lines = torch.as_tensor(ln[[j, k]]).clone()
    x0 = torch.as_tensor(np.r_[row.theta[grid.pvpq] - row.theta[grid.slack], row.v[grid.pq]])
    Y = gref._ybus(grid, p[0], p[1])
    assert torch.equal(gref._mismatch(grid, x0, p[0], p[2], Y), ngr.mismatch(grid, x0, *p))
    J = torch.autograd.functional.jacobian(lambda x: gref._mismatch(grid, x, p[0], p[2], Y), x0).numpy()
    x = x0.clone().requires_grad_(True)
    loss = row_loss(grid, x, p[1], p[2], out_lines, j, k, w, rating, at)
    dl_dx = torch.autograd.grad(loss, x, allow_unused=True)[0] if loss.requires_grad else None
    dl_dx = np.zeros(x0.numel()) if dl_dx is None else dl_dx.numpy()
    lam = torch.as_tensor(np.linalg.solve(J.T, dl_dx))
    pp = [t.clone().requires_grad_(True) for t in p]
    total = (row_loss(grid, x0, pp[1], pp[2], out_lines, j, k, w, rating, at)
             - (lam * gref._mismatch(grid, x0, pp[0], pp[2], gref._ybus(grid, pp[0], pp[1]))).sum())
    gb, gl, gg = (g.numpy() for g in torch.autograd.grad(total, pp))
    return [gb, np.insert(np.insert(gl, j, 0.0, axis=0), k, 0.0, axis=0), gg], float(np.linalg.cond(J))


def solve_rows(buses, lines, generators, slack_bus, pairs, tol=1e-8, max_iter=10):
    """The reference's rows of one grid for the pairs of the list (``Row``, or None for an islanding pair), from its own base."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    base = aref.base_case(bus, ln, gen, slack_bus, tol, max_iter)
    return [n2ref.pair(bus, ln, gen, slack_bus, int(min(p)), int(max(p)), base[0], base[1], tol, max_iter) for p in pairs]


def gradients(buses, lines, generators, slack_bus, pairs, rows, use, weights, rating=None):
    """The gradient of the loss summed over the rows r of the list with ``use[r]`` (each must be solved and converged):
    ``weights[name][r]`` weighs output ``name`` of row r.  Returns ([d buses, d lines, d generators], largest condition number)."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    total = [np.zeros_like(bus), np.zeros_like(ln), np.zeros_like(gen)]
    cond = 0.0
    for r, pair in enumerate(pairs):
        if not use[r]:
            continue
        assert rows[r] is not None and rows[r].converged, (r, pair)
        w = {name: None if weights.get(name) is None else ngr._np(weights[name][r]) for name in OUTPUTS}
        g, c = row_gradient(bus, ln, gen, slack_bus, (int(pair[0]), int(pair[1])), rows[r], w, rating)
        cond = max(cond, c)
        for a, b in zip(total, g):
            a += b
    return total, cond
