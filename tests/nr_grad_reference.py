"""Test-side float64 gradient of the Newton-Raphson power flow (the reference for gns_pf_adjoint), written independently of the
product code: the mismatch F(x, p) of include/gns_powerflow.h from MATPOWER's makeYbus / Sbus formulas in torch float64, its
dense Jacobians by torch autograd, and the implicit function theorem at a solution x*:

    dl/dp = dl/dp|_x - lambda^T dF/dp|_x,   J^T lambda = dl/dx,   J = dF/dx.

x = [theta at PV+PQ ; |V| at PQ], p = (buses [N,6], lines [E,7], generators [Gn,7]); |V| at PV / slack buses is the vg of the
first generator listed there, so the loss's direct dependence on it appears in dl/dp|_x."""
import numpy as np
import torch

import nr_reference as ref


def _np(x):
    """float64 numpy of an array or (possibly tracked) tensor."""
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


class _Grid:
    """The index structure of one grid (host arrays from its id columns)."""

    def __init__(self, buses, lines, generators, slack_bus):
        bus, ln, gen = _np(buses), _np(lines), _np(generators)
        self.n = bus.shape[0]
        self.slack, self.pv, self.pq = ref.roles(bus, gen, slack_bus)
        self.pvpq = np.r_[self.pv, self.pq]
        eye = np.eye(self.n)
        self.Cf = torch.as_tensor(eye[ln[:, 0].astype(int) - 1], dtype=torch.complex128)
        self.Ct = torch.as_tensor(eye[ln[:, 1].astype(int) - 1], dtype=torch.complex128)
        gb = gen[:, 0].astype(int) - 1
        self.Cg = torch.as_tensor(eye[gb], dtype=torch.float64)                      # [Gn, N]
        first = np.full(self.n, -1)
        for j in range(gen.shape[0] - 1, -1, -1):                                     # the first generator listed on a bus
            first[gb[j]] = j
        first[self.pq] = -1
        self.first = first


def _state(grid, x, gen):
    """|V| and theta [N] from the unknowns x and the generators' vg."""
    n, npvpq = grid.n, grid.pvpq.size
    th = torch.zeros(n, dtype=torch.float64).index_put((torch.as_tensor(grid.pvpq, dtype=torch.long),), x[:npvpq])
    has = torch.as_tensor(grid.first >= 0)
    vg = gen[torch.as_tensor(np.maximum(grid.first, 0)), 4]
    vm = torch.where(has, vg, torch.ones(n, dtype=torch.float64))
    vm = vm.index_put((torch.as_tensor(grid.pq, dtype=torch.long),), x[npvpq:])
    return vm, th


def mismatch(grid, x, bus, line, gen):
    """F(x, p) = [Re(S - S_spec) at PV+PQ ; Im(S - S_spec) at PQ], S = V conj(Y V), S_spec = Cg^T Pg - Pd - j Qd."""
    ys = 1.0 / torch.complex(line[:, 2], line[:, 3])
    tap = torch.polar(line[:, 5], line[:, 6])
    ytt = ys + 1j * line[:, 4] / 2
    yff = ytt / (tap * tap.conj())
    yft = -ys / tap.conj()
    ytf = -ys / tap
    Cf, Ct = grid.Cf, grid.Ct
    Y = (Cf.T @ (yff[:, None] * Cf) + Cf.T @ (yft[:, None] * Ct) + Ct.T @ (ytf[:, None] * Cf) + Ct.T @ (ytt[:, None] * Ct)
         + torch.diag(torch.complex(bus[:, 4], bus[:, 5])))
    vm, th = _state(grid, x, gen)
    V = torch.polar(vm, th)
    S = V * (Y @ V).conj()
    P = S.real - (grid.Cg.T @ gen[:, 6] - bus[:, 2])
    Q = S.imag + bus[:, 3]
    return torch.cat([P[torch.as_tensor(grid.pvpq, dtype=torch.long)], Q[torch.as_tensor(grid.pq, dtype=torch.long)]])


def implicit_gradient(buses, lines, generators, slack_bus, v, theta, a, b):
    """d(a . v + b . theta)/d(buses, lines, generators) at the solution (v, theta) of one grid, in float64 numpy
    ([N,6], [E,7], [Gn,7]).  The slack's theta is constant (b there does not matter); columns that do not enter F are 0."""
    grid = _Grid(buses, lines, generators, slack_bus)
    p = [torch.as_tensor(_np(t)).clone() for t in (buses, lines, generators)]
    v, theta = _np(v), _np(theta)
    x0 = torch.as_tensor(np.r_[theta[grid.pvpq] - theta[grid.slack], v[grid.pq]])
    a_t, b_t = torch.as_tensor(_np(a)), torch.as_tensor(_np(b))
    mask_b = torch.ones_like(b_t)
    mask_b[grid.slack] = 0.0

    def loss(x, gen):
        vm, th = _state(grid, x, gen)
        return (a_t * vm).sum() + (b_t * mask_b * th).sum()

    J = torch.autograd.functional.jacobian(lambda x: mismatch(grid, x, *p), x0).numpy()
    x = x0.clone().requires_grad_(True)
    dl_dx = torch.autograd.grad(loss(x, p[2]), x)[0].numpy()
    lam = torch.as_tensor(np.linalg.solve(J.T, dl_dx))
    pp = [t.clone().requires_grad_(True) for t in p]
    total = loss(x0, pp[2]) - (lam * mismatch(grid, x0, *pp)).sum()
    return [g.numpy() for g in torch.autograd.grad(total, pp)]


# the differentiable columns (include/gns_powerflow.h, "Gradients"); every other column's gradient is exactly 0
DIFF_COLS = {'buses': [2, 3, 4, 5], 'lines': [2, 3, 4, 5, 6], 'generators': [4, 6]}
