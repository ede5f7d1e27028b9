"""Test-side float64 reference of the AC contingency screen, on top of ``nr_reference``: the line's row is deleted from the grid,
``nr_reference.newton_raphson`` is run on the smaller grid warm-started from the base solution, and the branch flows at both ends
of every line are computed from the dense makeYbus quantities of each line (0 at the outaged line).  Islanding is decided by a
search of the smaller grid's own graph.  Nothing here reads the product's analysis or kernels."""
from collections import namedtuple

import numpy as np

import nr_reference as nr
from dc_contingency_reference import islands

Row = namedtuple('Row', ['v', 'theta', 'converged', 'iterations', 'mismatch', 'p_from', 'q_from', 'p_to', 'q_to'])


def line_admittances(lines):
    """(f, t, Y_ff, Y_tt, Y_ft, Y_tf) of every line (0-based ends, complex [E]): the stamps of MATPOWER's makeYbus."""
    ln = np.asarray(lines, dtype=np.float64)
    f, t = ln[:, 0].astype(int) - 1, ln[:, 1].astype(int) - 1
    ys = 1.0 / (ln[:, 2] + 1j * ln[:, 3])
    tap = ln[:, 5] * np.exp(1j * ln[:, 6])
    ytt = ys + 1j * ln[:, 4] / 2
    return f, t, ytt / (tap * np.conj(tap)), ytt, -ys / np.conj(tap), -ys / tap


def ybus_skipping(buses, lines, k):
    """Dense complex Y-bus of a grid on its base pattern with the four stamps of line ``k`` skipped (``k`` None: none skipped): what
    the screen's rows use.  Entries that lose their only line stay in the pattern as zeros."""
    bus = np.asarray(buses, dtype=np.float64)
    n = bus.shape[0]
    f, t, yff, ytt, yft, ytf = line_admittances(lines)
    Y = np.zeros((n, n), dtype=np.complex128)
    Y[np.arange(n), np.arange(n)] = bus[:, 4] + 1j * bus[:, 5]
    for e in range(f.size):
        if e == k:
            continue
        Y[f[e], f[e]] += yff[e]
        Y[t[e], t[e]] += ytt[e]
        Y[f[e], t[e]] += yft[e]
        Y[t[e], f[e]] += ytf[e]
    return Y


def branch_flows(lines, v, theta, k=None):
    """(p_from, q_from, p_to, q_to) [E] at the state (v, theta): S_f = V_f conj(Y_ff V_f + Y_ft V_t), S_t = V_t conj(Y_tf V_f + Y_tt
    V_t); zeros at line ``k``."""
    f, t, yff, ytt, yft, ytf = line_admittances(lines)
    V = np.asarray(v, dtype=np.float64) * np.exp(1j * np.asarray(theta, dtype=np.float64))
    sf = V[f] * np.conj(yff * V[f] + yft * V[t])
    st = V[t] * np.conj(ytf * V[f] + ytt * V[t])
    if k is not None:
        sf[k] = st[k] = 0.0
    return sf.real.copy(), sf.imag.copy(), st.real.copy(), st.imag.copy()


def bus_balance(buses, lines, generators, v, theta, k=None):
    """sum S_from + sum S_to + shunt - S_injected per bus (complex [N]) at (v, theta), the flows of line ``k`` left out; the injection
    of every bus is what the network absorbs there, so only the buses whose equations the power flow solves are near zero: the real
    part at PV and PQ buses, the imaginary part at PQ buses."""
    bus = np.asarray(buses, dtype=np.float64)
    f, t, _, _, _, _ = line_admittances(lines)
    pf, qf, pt, qt = branch_flows(lines, v, theta, k)
    V = np.asarray(v, dtype=np.float64) * np.exp(1j * np.asarray(theta, dtype=np.float64))
    s = np.zeros(bus.shape[0], dtype=np.complex128)
    np.add.at(s, f, pf + 1j * qf)
    np.add.at(s, t, pt + 1j * qt)
    s += np.abs(V) ** 2 * np.conj(bus[:, 4] + 1j * bus[:, 5])
    return s - nr.specified(buses, generators)


def base_case(buses, lines, generators, slack_bus, tol=1e-8, max_iter=10):
    """``nr_reference.newton_raphson`` on the whole grid from the flat start."""
    return nr.newton_raphson(buses, lines, generators, slack_bus, tol=tol, max_iter=max_iter)


def outage(buses, lines, generators, slack_bus, k, v0, theta0, tol=1e-8, max_iter=10):
    """Row ``k`` of one grid: a ``Row`` (numpy float64), or None when deleting line ``k`` (0-based) islands a bus."""
    ln = np.asarray(lines, dtype=np.float64)
    rest = np.delete(ln, k, axis=0)
    if islands(np.asarray(buses).shape[0], rest[:, 0], rest[:, 1], slack_bus):
        return None
    vm, va, conv, it, mis = nr.newton_raphson(buses, rest, generators, slack_bus, tol=tol, max_iter=max_iter, v0=v0, theta0=theta0)
    return Row(vm, va, bool(conv), int(it), float(mis), *branch_flows(ln, vm, va, k))


def loading(row, rating=None):
    """max(|S_f|, |S_t|) / rating per line [E]."""
    s = np.maximum(np.hypot(row.p_from, row.q_from), np.hypot(row.p_to, row.q_to))
    return s if rating is None else s / np.asarray(rating, dtype=np.float64)


def extreme(x, largest=True):
    """(value, lowest index that attains it, distance to the runner-up at another index) of the largest (or smallest) of x."""
    x = np.asarray(x, dtype=np.float64)
    y = x if largest else -x
    i = int(np.flatnonzero(y == y.max())[0])
    rest = np.delete(y, i)
    gap = float(y[i] - rest.max()) if rest.size else float('inf')
    return float(x[i]), i, gap
