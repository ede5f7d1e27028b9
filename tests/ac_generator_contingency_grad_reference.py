"""Test-side float64 gradient of the AC generator contingency screen (the reference for gns_acg1_adjoint), written independently
of the product code on ``ac_generator_contingency_reference``, ``ac_contingency_grad_reference`` and ``nr_grad_reference``.  Per
(grid, (g, k)): generator row g is deleted, the pickup is applied to the others' ``Pg`` INSIDE the torch graph (so the chain rule
reaches ``Pg_g`` and the weights), line k's row is deleted (k >= 0), the smaller grid is solved by the reference's own
Newton-Raphson from the base solution, the weighted loss of all nine outputs is built in torch complex128 (the flows from the full
line list with line k's zeroed), the dense Jacobian of the mismatch is taken by autograd and the implicit function theorem applied:

    dl/dp = dl/dp|_x - lambda^T dF_gk/dp|_x,   J_gk^T lambda = dl/dx,

as ``ac_n2_grad_reference.row_gradient`` does.  The generator gradient is taken with respect to the full table, so row g comes back
with what the pickup sends to ``Pg_g`` and zeros elsewhere; line k's zero row is inserted back.  The bus roles and the set points
are whatever ``nr_grad_reference._Grid`` makes of the grid without the row: a freed bus is PQ, a shared bus takes the next unit's
``vg``, a slack without a unit the constant 1.  The summaries follow ``ac_contingency_grad_reference``'s rules.  Nothing here reads
the product's analysis or kernels."""
import numpy as np
import torch

import ac_contingency_grad_reference as gref
import ac_contingency_reference as aref
import ac_generator_contingency_reference as agref
import nr_grad_reference as ngr

OUTPUTS = gref.OUTPUTS
DIFF_COLS = gref.DIFF_COLS


def redispatch(gen, g, w):
    """The generator table ``[Gn-1,7]`` without row ``g`` as a torch expression of the full table ``gen`` ``[Gn,7]`` and the weights
    ``w`` (``[Gn]`` or None): ``ac_generator_contingency_reference.without``, the same branch (nothing is shared when the others'
    weights sum to exactly zero, and that branch is not differentiated)."""
    others = [h for h in range(gen.shape[0]) if h != g]
    rest = gen[others]
    if w is None:
        return rest
    total = torch.zeros((), dtype=torch.float64)
    for h in others:
        total = total + w[h]
    if not float(total.detach()) > 0.0:
        return rest
    pg = rest[:, 6] + gen[g, 6] * (w[others] / total)
    return torch.cat([rest[:, :6], pg[:, None]], dim=1)


def row_loss(grid, x, full, gen, out, w, rating, at):
    """The weighted loss of a row's nine outputs at the unknowns x: ``full`` is the whole line list, ``out`` the lines whose flows are
    the constant 0 (``[k]`` or ``[]``), ``gen`` the table without the lost unit."""
    vm, th = ngr._state(grid, x, gen)
    sf, st = gref._flows(full, vm, th, out)
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


def row_gradient(buses, lines, generators, slack_bus, g, k, row, w, pickup=None, rating=None, at=None):
    """d(weighted loss of row (g, k))/d(buses, lines, generators, pickup weights) in float64 numpy at the reference's solved ``row``
    (``ac_generator_contingency_reference.outage``'s), and the condition number of the row's Jacobian.  ``w``: a dict of the
    weights of ``OUTPUTS`` ([N], [E] or scalars; a missing one is zero); ``pickup``: the grid's float64 weights ``[Gn]`` or None
    (the weights' gradient is then zeros)."""
    at = at or {}
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    pw = None if pickup is None else np.asarray(pickup, dtype=np.float64)
    out = [k] if k >= 0 else []
    keep = [e for e in range(ln.shape[0]) if e != k]
    grid = ngr._Grid(bus, ln[keep], agref.without(gen, g, pw), slack_bus)
    p = [torch.as_tensor(a).clone() for a in (bus, ln, gen)] + [None if pw is None else torch.as_tensor(pw).clone()]

    def parts(q):
        """(buses, the lines that are in service, the whole line list, the redispatched table without g) of the parameters q"""
        return q[0], q[1][keep], q[1], redispatch(q[2], g, q[3])

    b0, rest0, full0, gen0 = parts(p)
    assert np.array_equal(gen0.numpy(), agref.without(gen, g, pw))
    x0 = torch.as_tensor(np.r_[row.theta[grid.pvpq] - row.theta[grid.slack], row.v[grid.pq]])
    Y = gref._ybus(grid, b0, rest0)
    assert torch.equal(gref._mismatch(grid, x0, b0, gen0, Y), ngr.mismatch(grid, x0, b0, rest0, gen0))
    J = torch.autograd.functional.jacobian(lambda x: gref._mismatch(grid, x, b0, gen0, Y), x0).numpy()
    x = x0.clone().requires_grad_(True)
    loss = row_loss(grid, x, full0, gen0, out, w, rating, at)
    dl_dx = torch.autograd.grad(loss, x, allow_unused=True)[0] if loss.requires_grad else None
    dl_dx = np.zeros(x0.numel()) if dl_dx is None else dl_dx.numpy()
    lam = torch.as_tensor(np.linalg.solve(J.T, dl_dx))
    pp = [None if t is None else t.clone().requires_grad_(True) for t in p]
    b1, rest1, full1, gen1 = parts(pp)
    total = row_loss(grid, x0, full1, gen1, out, w, rating, at) - (lam * gref._mismatch(grid, x0, b1, gen1, gref._ybus(grid, b1, rest1))).sum()
    grads = torch.autograd.grad(total, [t for t in pp if t is not None], allow_unused=True)
    grads = [np.zeros(t.shape) if a is None else a.numpy() for a, t in zip(grads, [t for t in pp if t is not None])]
    gb, gl, gg = grads[:3]
    gw = grads[3] if pw is not None else np.zeros(gen.shape[0])
    return [gb, gl, gg, gw], float(np.linalg.cond(J))


def solve_rows(buses, lines, generators, slack_bus, rows, pickup=None, tol=1e-8, max_iter=10):
    """The reference's rows of one grid for the (g, k) of the list (``Row``, or None for an islanding row), from its own base;
    ``pickup``: the grid's float64 weights ``[Gn]`` or None."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    base = aref.base_case(bus, ln, gen, slack_bus, tol, max_iter)
    return [agref.outage(bus, ln, gen, slack_bus, int(g), int(k), base[0], base[1], pickup, tol, max_iter) for g, k in rows]


def gradients(buses, lines, generators, slack_bus, rows, solved, use, weights, pickup=None, rating=None):
    """The gradient of the loss summed over the rows r of the list with ``use[r]`` (each must be solved and converged):
    ``weights[name][r]`` weighs output ``name`` of row r.  Returns ([d buses, d lines, d generators, d pickup weights], largest
    condition number)."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    total = [np.zeros_like(bus), np.zeros_like(ln), np.zeros_like(gen), np.zeros(gen.shape[0])]
    cond = 0.0
    for r, (g, k) in enumerate(rows):
        if not use[r]:
            continue
        assert solved[r] is not None and solved[r].converged, (r, g, k)
        w = {name: None if weights.get(name) is None else ngr._np(weights[name][r]) for name in OUTPUTS}
        grads, c = row_gradient(bus, ln, gen, slack_bus, int(g), int(k), solved[r], w, pickup, rating)
        cond = max(cond, c)
        for a, b in zip(total, grads):
            a += b
    return total, cond
