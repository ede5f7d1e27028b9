"""Test-side float64 reference of the AC N-2 contingency screen, on top of ``nr_reference`` and ``ac_contingency_reference``: both
line rows are deleted from the grid, ``nr_reference.newton_raphson`` is run on the smaller grid warm-started from the reference's own
base solution, and the branch flows at both ends of every line are computed from the dense makeYbus quantities of each line (0 at
both outaged lines).  Islanding is decided by a search of the smaller grid's own graph.  Nothing here reads the product's analysis
or kernels."""
import numpy as np

import ac_contingency_reference as aref
import nr_reference as nr
from ac_contingency_reference import Row
from dc_contingency_reference import islands


def ybus_skipping(buses, lines, skip=()):
    """``ac_contingency_reference.ybus_skipping`` for any set of lines: the dense complex Y-bus of a grid on its base pattern with
    the four stamps of every line of ``skip`` left out.  Entries that lose their only lines stay in the pattern as zeros."""
    bus = np.asarray(buses, dtype=np.float64)
    n = bus.shape[0]
    f, t, yff, ytt, yft, ytf = aref.line_admittances(lines)
    Y = np.zeros((n, n), dtype=np.complex128)
    Y[np.arange(n), np.arange(n)] = bus[:, 4] + 1j * bus[:, 5]
    for e in range(f.size):
        if e in skip:
            continue
        Y[f[e], f[e]] += yff[e]
        Y[t[e], t[e]] += ytt[e]
        Y[f[e], t[e]] += yft[e]
        Y[t[e], f[e]] += ytf[e]
    return Y


def pair_islands(n_bus, lines, slack_bus, j, k):
    """Whether the grid without lines ``j`` and ``k`` (0-based) leaves a bus without a path of lines to the 1-based slack."""
    rest = np.delete(np.asarray(lines, dtype=np.float64), [j, k], axis=0)
    return islands(n_bus, rest[:, 0], rest[:, 1], slack_bus)


def pair(buses, lines, generators, slack_bus, j, k, v0, theta0, tol=1e-8, max_iter=10):
    """Row ``(j, k)`` of one grid: a ``Row`` (numpy float64), or None when deleting lines ``j`` and ``k`` (0-based) islands a bus."""
    assert j != k
    ln = np.asarray(lines, dtype=np.float64)
    if pair_islands(np.asarray(buses).shape[0], ln, slack_bus, j, k):
        return None
    rest = np.delete(ln, [j, k], axis=0)
    vm, va, conv, it, mis = nr.newton_raphson(buses, rest, generators, slack_bus, tol=tol, max_iter=max_iter, v0=v0, theta0=theta0)
    flows = aref.branch_flows(ln, vm, va)
    for x in flows:
        x[[j, k]] = 0.0
    return Row(vm, va, bool(conv), int(it), float(mis), *flows)


def spare(row, max_iter=10):
    """Whether the reference converged with at least two iterations to spare: the rows a device row is compared on."""
    return row is not None and row.converged and row.iterations <= max_iter - 2
