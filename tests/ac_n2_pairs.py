"""The pair lists of the AC N-2 tests, host and device: every pair of a topology, the pairs whose eight Y-bus entries overlap by
kind, the list the row-level tests screen (``rows_pairs``) and its islanding mask.  Pure Python on the topology's id arrays; nothing
here needs a device."""
import numpy as np

from opf_graph_neural_solver_amd import powerflow
import ac_n2_reference as n2ref


def every_pair(E):
    return [tuple(p) for p in powerflow._pair_list(None, E, 'ac_contingency_screen').tolist()]


def pair_kinds(tp):
    """{(j, k): kind} of every pair of a topology whose eight entries overlap: 'parallel' (the same two different buses),
    'shared_bus', 'loop_at_bus' (a line from a bus to itself with a line at that bus), 'loop_elsewhere'."""
    ends = [tuple(sorted(p)) for p in zip(tp.f.tolist(), tp.t.tolist())]
    kinds = {}
    for j, k in every_pair(tp.f.size):
        a, b = ends[j], ends[k]
        loops = (a[0] == a[1]) + (b[0] == b[1])
        if loops == 1:
            kinds[j, k] = 'loop_at_bus' if set(a) & set(b) else 'loop_elsewhere'
        elif loops == 0 and a == b:
            kinds[j, k] = 'parallel'
        elif loops == 0 and set(a) & set(b):
            kinds[j, k] = 'shared_bus'
    return kinds


KINDS = ('parallel', 'shared_bus', 'loop_at_bus', 'loop_elsewhere')
EDGE_LINES = (0, 62, 63, 64, 65)               # and E - 1: the lines at the ends of a wave's 64 lanes


def rows_pairs(tp):
    """The pairs (j < k) of a topology that the row-level tests screen: every pair when there are at most 128, else 128 of them, in
    this order and without repeats: the first pair of each kind ``pair_kinds`` knows for the topology; every pair among the lines 0,
    62, 63, 64, 65 and E - 1 that exist; a fill in the order of ``np.random.default_rng(E).permutation`` of every pair."""
    E = tp.f.size
    every = every_pair(E)
    if len(every) <= 128:
        return every
    kinds = pair_kinds(tp)
    pairs = [next(p for p, kd in kinds.items() if kd == kind) for kind in KINDS if kind in kinds.values()]
    edge = sorted({e for e in EDGE_LINES + (E - 1,) if e < E})
    pairs += [(j, k) for a, j in enumerate(edge) for k in edge[a + 1:]]
    pairs += [every[p] for p in np.random.default_rng(E).permutation(len(every))]
    return list(dict.fromkeys(pairs))[:128]


def rows_islanding(tp, pairs):
    """[P] bool, from the reference's own graph search on each pair, and equal to the product's mask (``_pair_islanding``)."""
    lines = np.stack([tp.f, tp.t], axis=1).astype(np.float64)
    isl = np.array([n2ref.pair_islands(tp.n, lines, tp.slack, j, k) for j, k in pairs])
    assert np.array_equal(powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, np.asarray(pairs, dtype=np.int64)), isl), tp.name
    return isl
