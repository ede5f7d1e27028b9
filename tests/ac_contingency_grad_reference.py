"""Test-side float64 gradient of the AC contingency screen (the reference for gns_acn1_adjoint), written independently of the product
code on ``nr_reference`` / ``nr_grad_reference`` / ``ac_contingency_reference``.  Per (grid, k): line k's row is deleted, the smaller
grid is solved by the reference's own Newton-Raphson from the base solution, the weighted loss of all nine outputs is built in torch
complex128 (the flows from the full line list with line k's zeroed), the dense Jacobian of the mismatch is taken by autograd and the
implicit function theorem applied:

    dl/dp = dl/dp|_x - lambda^T dF_k/dp|_x,   J_k^T lambda = dl/dx,

and k's zero row is added back into the line gradient.  ``rating`` is a constant; ``worst_loading`` differentiates the end of its
line that attains the maximum (the from end on equality; nothing at |S| = 0), ``v_min`` / ``v_max`` the bus that attains them: the
lowest of equals, or the index given in ``at``."""
import numpy as np
import torch

import ac_contingency_reference as aref
import nr_grad_reference as ngr

OUTPUTS = ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'v_min', 'v_max')
# the differentiable columns (gns_pf_adjoint's); every other column's gradient is exactly 0
DIFF_COLS = ngr.DIFF_COLS


def _flows(line, vm, th, k):
    """S_f, S_t [E] (complex) of the full line list at (vm, th), zeros at line k."""
    ys = 1.0 / torch.complex(line[:, 2], line[:, 3])
    tap = torch.polar(line[:, 5], line[:, 6])
    ytt = ys + 1j * line[:, 4] / 2
    yff, yft, ytf = ytt / (tap * tap.conj()), -ys / tap.conj(), -ys / tap
    f = torch.as_tensor(line[:, 0].detach().numpy().astype(int) - 1)
    t = torch.as_tensor(line[:, 1].detach().numpy().astype(int) - 1)
    V = torch.polar(vm, th)
    sf = V[f] * (yff * V[f] + yft * V[t]).conj()
    st = V[t] * (ytf * V[f] + ytt * V[t]).conj()
    keep = torch.ones(line.shape[0], dtype=torch.bool)
    keep[k] = False
    zero = torch.zeros_like(sf)
    return torch.where(keep, sf, zero), torch.where(keep, st, zero)


def _ybus(grid, bus, line):
    """The dense Y-bus of ``nr_grad_reference.mismatch`` (makeYbus), apart from the state: the Jacobian with respect to x does not
    differentiate it."""
    ys = 1.0 / torch.complex(line[:, 2], line[:, 3])
    tap = torch.polar(line[:, 5], line[:, 6])
    ytt = ys + 1j * line[:, 4] / 2
    yff, yft, ytf = ytt / (tap * tap.conj()), -ys / tap.conj(), -ys / tap
    Cf, Ct = grid.Cf, grid.Ct
    return (Cf.T @ (yff[:, None] * Cf) + Cf.T @ (yft[:, None] * Ct) + Ct.T @ (ytf[:, None] * Cf) + Ct.T @ (ytt[:, None] * Ct)
            + torch.diag(torch.complex(bus[:, 4], bus[:, 5])))


def _mismatch(grid, x, bus, gen, Y):
    """``nr_grad_reference.mismatch`` on a given Y-bus."""
    vm, th = ngr._state(grid, x, gen)
    V = torch.polar(vm, th)
    S = V * (Y @ V).conj()
    P = S.real - (grid.Cg.T @ gen[:, 6] - bus[:, 2])
    Q = S.imag + bus[:, 3]
    return torch.cat([P[torch.as_tensor(grid.pvpq, dtype=torch.long)], Q[torch.as_tensor(grid.pq, dtype=torch.long)]])


def row_loss(grid, x, rest, gen, line_k, k, w, rating, at):
    """The weighted loss of row k's nine outputs at the unknowns x; ``rest`` is the line list without line k (``line_k``, a constant)."""
    vm, th = ngr._state(grid, x, gen)
    full = torch.cat([rest[:k], line_k[None], rest[k:]])
    sf, st = _flows(full, vm, th, k)
    zero = torch.zeros((), dtype=torch.float64)
    loss = zero
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


def row_gradient(buses, lines, generators, slack_bus, k, row, w, rating=None, at=None):
    """d(weighted loss of row k)/d(buses, lines, generators) in float64 numpy at the reference's solved ``row`` (an
    ``ac_contingency_reference.Row``), and the condition number of the row's Jacobian.  ``w``: a dict of the weights of ``OUTPUTS``
    ([N], [E] or scalars; a missing one is zero)."""
    at = at or {}
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    rest = np.delete(ln, k, axis=0)
    grid = ngr._Grid(bus, rest, gen, slack_bus)
    p = [torch.as_tensor(a).clone() for a in (bus, rest, gen)]
    line_k = torch.as_tensor(ln[k]).clone()
    x0 = torch.as_tensor(np.r_[row.theta[grid.pvpq] - row.theta[grid.slack], row.v[grid.pq]])
    Y = _ybus(grid, p[0], p[1])
    assert torch.equal(_mismatch(grid, x0, p[0], p[2], Y), ngr.mismatch(grid, x0, *p))
    J = torch.autograd.functional.jacobian(lambda x: _mismatch(grid, x, p[0], p[2], Y), x0).numpy()
    x = x0.clone().requires_grad_(True)
    loss = row_loss(grid, x, p[1], p[2], line_k, k, w, rating, at)
    dl_dx = torch.autograd.grad(loss, x, allow_unused=True)[0]
    dl_dx = np.zeros(x0.numel()) if dl_dx is None else dl_dx.numpy()
    lam = torch.as_tensor(np.linalg.solve(J.T, dl_dx))
    pp = [t.clone().requires_grad_(True) for t in p]
    total = row_loss(grid, x0, pp[1], pp[2], line_k, k, w, rating, at) - (lam * _mismatch(grid, x0, pp[0], pp[2], _ybus(grid, pp[0], pp[1]))).sum()
    gb, gl, gg = (g.numpy() for g in torch.autograd.grad(total, pp))
    return [gb, np.insert(gl, k, 0.0, axis=0), gg], float(np.linalg.cond(J))


def solve_rows(buses, lines, generators, slack_bus, outages, tol=1e-8, max_iter=10):
    """The reference's rows of one grid for the outages of the list (``Row``, or None for an islanding outage), from its own base."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    base = aref.base_case(bus, ln, gen, slack_bus, tol, max_iter)
    return [aref.outage(bus, ln, gen, slack_bus, int(k), base[0], base[1], tol, max_iter) for k in outages]


def gradients(buses, lines, generators, slack_bus, outages, rows, use, weights, rating=None):
    """The gradient of the loss summed over the rows j of the list with ``use[j]`` (each must be solved and converged):
    ``weights[name][j]`` weighs output ``name`` of row j.  Returns ([d buses, d lines, d generators], largest condition number)."""
    bus, ln, gen = (ngr._np(t) for t in (buses, lines, generators))
    total = [np.zeros_like(bus), np.zeros_like(ln), np.zeros_like(gen)]
    cond = 0.0
    for j, k in enumerate(outages):
        if not use[j]:
            continue
        assert rows[j] is not None and rows[j].converged, (j, k)
        w = {name: None if weights.get(name) is None else ngr._np(weights[name][j]) for name in OUTPUTS}
        g, c = row_gradient(bus, ln, gen, slack_bus, int(k), rows[j], w, rating)
        cond = max(cond, c)
        for a, b in zip(total, g):
            a += b
    return total, cond
