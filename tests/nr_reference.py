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


def mismatch(buses, lines, generators, slack_bus, v, theta):
    """||F||_inf of (v, theta) with the power-flow mismatch F of include/gns_powerflow.h."""
    slack, pv, pq = roles(buses, generators, slack_bus)
    V = np.asarray(v, dtype=np.float64) * np.exp(1j * np.asarray(theta, dtype=np.float64))
    mis = V * np.conj(ybus(buses, lines) @ V) - specified(buses, generators)
    pvpq = np.r_[pv, pq]
    return float(np.max(np.abs(np.r_[mis[pvpq].real, mis[pq].imag]), initial=0.0))


def newton_raphson(buses, lines, generators, slack_bus, tol=1e-8, max_iter=10, v0=None, theta0=None):
    """Returns (v, theta, converged, iterations, mismatch) of one grid."""
    bus = np.asarray(buses, dtype=np.float64)
    gen = np.asarray(generators, dtype=np.float64)
    n = bus.shape[0]
    slack, pv, pq = roles(bus, gen, slack_bus)
    Y = ybus(bus, lines)
    S = specified(bus, gen)
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
    pvpq = np.r_[pv, pq]
    npvpq = pvpq.size
    it = 0
    while True:
        V = vm * np.exp(1j * va)
        mis = V * np.conj(Y @ V) - S
        F = np.r_[mis[pvpq].real, mis[pq].imag]
        nrm = float(np.max(np.abs(F), initial=0.0))
        if not np.isfinite(nrm):
            return vm, va, False, it, nrm
        if nrm < tol:
            return vm, va, True, it, nrm
        if it >= max_iter:
            return vm, va, False, it, nrm
        Ibus = Y @ V
        dV = sp.diags(V)
        dS_dVa = 1j * dV @ np.conj(sp.diags(Ibus) - Y @ dV)
        dS_dVm = dV @ np.conj(Y @ sp.diags(V / np.abs(V))) + np.conj(sp.diags(Ibus)) @ sp.diags(V / np.abs(V))
        J = sp.vstack([sp.hstack([dS_dVa[pvpq][:, pvpq].real, dS_dVm[pvpq][:, pq].real]),
                       sp.hstack([dS_dVa[pq][:, pvpq].imag, dS_dVm[pq][:, pq].imag])]).tocsc()
        dx = spla.spsolve(J, F)
        if not np.all(np.isfinite(dx)):
            return vm, va, False, it, nrm
        va[pvpq] -= dx[:npvpq]
        vm[pq] -= dx[npvpq:]
        it += 1
