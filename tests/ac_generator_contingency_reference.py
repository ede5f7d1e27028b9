"""Test-side float64 reference of the AC generator contingency screen, on top of ``nr_reference`` and ``ac_contingency_reference``:
the generator's row is deleted from the grid, the pickup is applied to the remaining rows' ``Pg`` in float64, and the smaller
generator table is solved by ``ac_contingency_reference.outage`` (a line out as well: the line's row deleted too) or by
``nr_reference.newton_raphson`` (no line), warm-started from the base solution.  The bus roles, the set points and the start of the
row are then whatever ``nr_reference`` makes of the grid without the row: a sole unit's bus becomes PQ, a shared bus takes the next
unit's ``vg``, a slack without a unit takes 1.  The branch flows come from ``ac_contingency_reference.branch_flows``.  Nothing here
reads the product's analysis or kernels."""
import numpy as np

import ac_contingency_reference as aref
import nr_reference as nr


def weights(pickup, generators, i=None):
    """The float64 pickup weights ``[Gn]`` of one grid: None, ``'pmax'`` (the generators' column 1), ``[Gn]``, or row ``i`` of
    ``[Bt,Gn]``."""
    if pickup is None:
        return None
    if isinstance(pickup, str):
        assert pickup == 'pmax'
        return np.asarray(generators, dtype=np.float64)[:, 1].copy()
    w = np.asarray(pickup, dtype=np.float64)
    return w if w.ndim == 1 else w[i]


def without(generators, g, w=None):
    """The generator table ``[Gn-1,7]`` (float64) with row ``g`` deleted and its ``Pg`` shared among the others by the weights ``w``
    (None, or a zero sum of the others' weights: nothing is shared and the slack picks the loss up)."""
    gen = np.asarray(generators, dtype=np.float64).copy()
    pg = gen[g, 6]
    others = [h for h in range(gen.shape[0]) if h != g]
    if w is not None:
        total = 0.0
        for h in others:
            total += float(w[h])
        if total > 0.0:
            for h in others:
                gen[h, 6] += pg * (float(w[h]) / total)
    return gen[others]


def outage(buses, lines, generators, slack_bus, g, k, v0, theta0, w=None, tol=1e-8, max_iter=10):
    """Row ``(g, k)`` of one grid (``k`` -1: no line out): an ``ac_contingency_reference.Row``, or None when deleting line ``k``
    islands a bus."""
    rest = without(generators, g, w)
    if k >= 0:
        return aref.outage(buses, lines, rest, slack_bus, k, v0, theta0, tol, max_iter)
    vm, va, conv, it, mis = nr.newton_raphson(buses, lines, rest, slack_bus, tol=tol, max_iter=max_iter, v0=v0, theta0=theta0)
    return aref.Row(vm, va, bool(conv), int(it), float(mis), *aref.branch_flows(lines, vm, va))
