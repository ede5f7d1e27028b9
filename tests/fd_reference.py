"""Test-side float64 fast-decoupled power flow (numpy / scipy), written independently of the product code from PYPOWER's makeB /
fdpf, as the reference for the fast-decoupled tests.  It reuses ``nr_reference``'s Y-bus, roles, injections and start."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nr_reference as ref

ALG = {'XB': 2, 'BX': 3}


def make_b(buses, lines, variant):
    """(B', B'') as dense float64 [N,N] arrays: -Im(Y) of the modified grids of makeB (per-unit shunts, as nr_reference.ybus)."""
    bus = np.asarray(buses, dtype=np.float64)
    ln = np.asarray(lines, dtype=np.float64)
    bus_p, ln_p = bus.copy(), ln.copy()
    bus_p[:, 5] = 0.0                    # Bs
    ln_p[:, 4] = 0.0                     # b
    ln_p[:, 5] = 1.0                     # tau
    if variant == 'XB':
        ln_p[:, 2] = 0.0                 # r
    ln_pp = ln.copy()
    ln_pp[:, 6] = 0.0                    # shift
    if variant == 'BX':
        ln_pp[:, 2] = 0.0
    return -ref.ybus(bus_p, ln_p).toarray().imag, -ref.ybus(bus, ln_pp).toarray().imag


def _scaled_mismatch(Y, V, S, pvpq, pq):
    mis = (V * np.conj(Y @ V) - S) / np.abs(V)
    return mis[pvpq].real, mis[pq].imag


def setting(buses, lines, generators, slack_bus):
    """(pvpq, pq, Y, S) of one grid: the unknowns' buses in ``roles``' order, the Y-bus and the specified injections."""
    slack, pv, pq = ref.roles(buses, generators, slack_bus)
    return np.r_[pv, pq], pq, ref.ybus(buses, lines), ref.specified(buses, generators)


def scaled_norm(Y, S, pvpq, pq, vm, va):
    """(P, Q, max(||P||_inf, ||Q||_inf)) of the scaled mismatch at (vm, va): the norm every test of the iteration reads."""
    P, Q = _scaled_mismatch(Y, vm * np.exp(1j * va), S, pvpq, pq)
    return P, Q, float(max(np.max(np.abs(P), initial=0.0), np.max(np.abs(Q), initial=0.0)))


def norm_rounding_bound(Y, S, vm):
    """What float64 rounding may move the scaled norm by: the bound of the Newton-Raphson zero-steps test on ||F||_inf, 4 deg eps
    max_i(|V_i| (|Y| |V|)_i + |S_i|) with deg the longest Y-bus row + 2, divided by the smallest |V| the mismatch is scaled by."""
    scale = np.max(np.abs(vm) * (abs(Y) @ np.abs(vm)) + np.abs(S))
    deg = int(np.max(np.diff(Y.indptr))) + 2
    return 4 * deg * np.finfo(np.float64).eps * scale / np.min(np.abs(vm))


def fast_decoupled(buses, lines, generators, slack_bus, variant, tol=1e-8, max_iter=30, v0=None, theta0=None):
    """Returns (v, theta, converged, iterations, mismatch) of one grid, with the per-grid failure rules of
    include/gns_powerflow.h ("Fast-decoupled"): mismatch is max(||P||_inf, ||Q||_inf) of the scaled mismatch at the last test."""
    bus = np.asarray(buses, dtype=np.float64)
    gen = np.asarray(generators, dtype=np.float64)
    slack, pv, pq = ref.roles(bus, gen, slack_bus)
    pvpq = np.r_[pv, pq]
    Y = ref.ybus(bus, lines)
    S = ref.specified(bus, gen)
    vm, va = ref.start(bus, gen, slack_bus, v0, theta0)
    Bp, Bpp = make_b(bus, lines, variant)

    def test():
        P, Q = _scaled_mismatch(Y, vm * np.exp(1j * va), S, pvpq, pq)
        nrm = max(np.max(np.abs(P), initial=0.0), np.max(np.abs(Q), initial=0.0))
        if not (np.all(np.isfinite(P)) and np.all(np.isfinite(Q))):
            nrm = float('nan')
        return P, Q, float(nrm)

    P, Q, nrm = test()
    if nrm < tol:
        return vm, va, True, 0, nrm
    if not np.isfinite(nrm):
        return vm, va, False, 0, nrm
    solvers = []
    for M, idx in ((Bp, pvpq), (Bpp, pq)):
        if idx.size == 0:
            solvers.append(lambda r: np.zeros(0))
            continue
        sub = sp.csc_matrix(M[np.ix_(idx, idx)])
        try:
            lu = spla.splu(sub, permc_spec='NATURAL', diag_pivot_thresh=0.0)
        except RuntimeError:                                   # exactly singular
            return vm, va, False, 0, nrm
        d = lu.U.diagonal()
        if np.any(d == 0) or not np.all(np.isfinite(d)):
            return vm, va, False, 0, nrm
        solvers.append(lu.solve)
    it = 0
    while it < max_iter:
        dva = -solvers[0](P)
        if not np.all(np.isfinite(va[pvpq] + dva)):
            break
        va[pvpq] = va[pvpq] + dva
        it += 1
        P, Q, nrm = test()
        if not np.isfinite(nrm):
            break
        if nrm < tol:
            return vm, va, True, it, nrm
        dvm = -solvers[1](Q)
        if not np.all(np.isfinite(vm[pq] + dvm)):
            break
        vm[pq] = vm[pq] + dvm
        P, Q, nrm = test()
        if not np.isfinite(nrm):
            break
        if nrm < tol:
            return vm, va, True, it, nrm
    return vm, va, False, it, nrm
