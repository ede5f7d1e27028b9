"""Test-side float64 Newton-Raphson power flow (numpy / scipy), written independently of the product code from MATPOWER's
makeYbus / newtonpf, as the reference for the power-flow tests."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def ybus(buses, lines):
    """Complex Y-bus (scipy CSR) of one grid from its raw [N,6] / [E,7] arrays."""
    bus = np.asarray(buses, dtype=np.float64)
    ln = np.asarray(lines, dtype=np.float64)
    n = bus.shape[0]
    f, t = ln[:, 0].astype(int) - 1, ln[:, 1].astype(int) - 1
    ys = 1.0 / (ln[:, 2] + 1j * ln[:, 3])
    tap = ln[:, 5] * np.exp(1j * ln[:, 6])
    ytt = ys + 1j * ln[:, 4] / 2
    yff = ytt / (tap * np.conj(tap))
    yft = -ys / np.conj(tap)
    ytf = -ys / tap
    rows = np.concatenate([f, t, f, t, np.arange(n)])
    cols = np.concatenate([f, t, t, f, np.arange(n)])
    vals = np.concatenate([yff, ytt, yft, ytf, bus[:, 4] + 1j * bus[:, 5]])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def roles(buses, generators, slack_bus):
    n = np.asarray(buses).shape[0]
    gb = np.asarray(generators, dtype=np.float64)[:, 0].astype(int) - 1
    slack = int(slack_bus) - 1
    pv = np.array(sorted(set(gb.tolist()) - {slack}), dtype=int)
    pq = np.array(sorted(set(range(n)) - set(gb.tolist()) - {slack}), dtype=int)
    return slack, pv, pq


def specified(buses, generators):
    bus = np.asarray(buses, dtype=np.float64)
    gen = np.asarray(generators, dtype=np.float64)
    s = np.zeros(bus.shape[0], dtype=np.complex128)
    np.add.at(s, gen[:, 0].astype(int) - 1, gen[:, 6])
    return s - bus[:, 2] - 1j * bus[:, 3]


def _state(vm, va):
    return np.asarray(vm, dtype=np.float64) * np.exp(1j * np.asarray(va, dtype=np.float64))


def mismatch_vector(buses, lines, generators, slack_bus, v, theta, Y=None):
    """F = [Re(V conj(YV) - S) at PV+PQ ; Im(...) at PQ] of include/gns_powerflow.h at (v, theta), rows in the order of
    ``jacobian``'s unknowns (``roles``: PV ascending, then PQ ascending)."""
    slack, pv, pq = roles(buses, generators, slack_bus)
    V = _state(v, theta)
    Y = ybus(buses, lines) if Y is None else Y
    mis = V * np.conj(Y @ V) - specified(buses, generators)
    return np.r_[mis[np.r_[pv, pq]].real, mis[pq].imag]


def jacobian(buses, lines, generators, slack_bus, v, theta, Y=None):
    """dF/dx at (v, theta) (MATPOWER dSbus_dV, polar), scipy CSC, for x = [theta at PV+PQ ; |V| at PQ] in ``roles``' order."""
    slack, pv, pq = roles(buses, generators, slack_bus)
    pvpq = np.r_[pv, pq]
    V = _state(v, theta)
    Y = ybus(buses, lines) if Y is None else Y
    Ibus = Y @ V
    dV = sp.diags(V)
    dS_dVa = 1j * dV @ np.conj(sp.diags(Ibus) - Y @ dV)
    dS_dVm = dV @ np.conj(Y @ sp.diags(V / np.abs(V))) + np.conj(sp.diags(Ibus)) @ sp.diags(V / np.abs(V))
    return sp.vstack([sp.hstack([dS_dVa[pvpq][:, pvpq].real, dS_dVm[pvpq][:, pq].real]),
                      sp.hstack([dS_dVa[pq][:, pvpq].imag, dS_dVm[pq][:, pq].imag])]).tocsc()


def mismatch(buses, lines, generators, slack_bus, v, theta):
    """||F||_inf of (v, theta) with the power-flow mismatch F of include/gns_powerflow.h."""
    return float(np.max(np.abs(mismatch_vector(buses, lines, generators, slack_bus, v, theta)), initial=0.0))


def start(buses, generators, slack_bus, v0=None, theta0=None):
    """The starting point (|V|, theta) [N] of include/gns_powerflow.h: vg of the first generator listed on each PV / slack bus, 1
    elsewhere, theta 0; a warm start sets |V| at PQ buses from v0 and theta = theta0 - theta0[slack]."""
    bus = np.asarray(buses, dtype=np.float64)
    gen = np.asarray(generators, dtype=np.float64)
    n = bus.shape[0]
    slack, pv, pq = roles(bus, gen, slack_bus)
    vm = np.ones(n)
    for j in range(gen.shape[0] - 1, -1, -1):          # the first generator listed on a bus wins
        b = int(gen[j, 0]) - 1
        if b == slack or b in pv:
            vm[b] = gen[j, 4]
    va = np.zeros(n)
    if v0 is not None:
        vm[pq] = np.asarray(v0, dtype=np.float64)[pq]
    if theta0 is not None:
        th = np.asarray(theta0, dtype=np.float64)
        va = th - th[slack]
        va[slack] = 0.0
    return vm, va


def newton_raphson(buses, lines, generators, slack_bus, tol=1e-8, max_iter=10, v0=None, theta0=None):
    """Returns (v, theta, converged, iterations, mismatch) of one grid."""
    bus = np.asarray(buses, dtype=np.float64)
    gen = np.asarray(generators, dtype=np.float64)
    slack, pv, pq = roles(bus, gen, slack_bus)
    Y = ybus(bus, lines)
    vm, va = start(bus, gen, slack_bus, v0, theta0)
    pvpq = np.r_[pv, pq]
    npvpq = pvpq.size
    it = 0
    while True:
        F = mismatch_vector(bus, lines, gen, slack_bus, vm, va, Y)
        nrm = float(np.max(np.abs(F), initial=0.0))
        if not np.isfinite(nrm):
            return vm, va, False, it, nrm
        if nrm < tol:
            return vm, va, True, it, nrm
        if it >= max_iter:
            return vm, va, False, it, nrm
        J = jacobian(bus, lines, gen, slack_bus, vm, va, Y)
        dx = spla.spsolve(J, F)
        if not np.all(np.isfinite(dx)):
            return vm, va, False, it, nrm
        va[pvpq] -= dx[:npvpq]
        vm[pq] -= dx[npvpq:]
        it += 1
