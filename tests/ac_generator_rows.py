"""The row lists of the AC generator screen's row-level tests, host and device: the topologies by name, the list the tests screen
(``rows_list``), its islanding mask, the pickups and what the float64 reference makes of one row.  Numpy on the topology's id arrays
and on host copies of the grids; nothing here needs a device."""
from types import SimpleNamespace

import numpy as np

from opf_graph_neural_solver_amd import powerflow
import ac_generator_contingency_reference as gref
from ac_n2_pairs import EDGE_LINES
import nr_reference as nr
import pf_topologies as pt

FAMILIES = ('toy', 'random40_parallel_selfloop', 'random24_stacked_gens', 'ring63', 'ring64', 'ring65', 'wheel71',
            'hub150_70lines_70gens', 'wheel71_66gens')
MAX_ROWS = 256
FILL = 32                                      # rows kept for the seeded fill when the edge rows are trimmed


def topology(name):
    if name == 'toy':
        from test_ac_contingency_host import toy
        return toy()
    if name.startswith('ring'):
        return pt.ring_slack_without_generator(int(name[4:]))
    if name == 'wheel71':
        return pt.wheel(71)
    if name == 'wheel71_66gens':
        return pt.wheel_many_generators()
    return pt.families()[name]


def rows_list(tp):
    """The rows (g, k) of a topology that the row-level tests screen, k = -1 for no line out: every row, generator-major, when there
    are at most 256 (Gn (E + 1)), else 256 of them, in this order and without repeats: every generator alone; every generator with
    each of the lines 0, 62, 63, 64, 65 and E - 1 that exist, generator-major with the generators 0, 62, 63, 64, 65 and Gn - 1 that
    exist first, trimmed to 224 rows in all when there are more; a fill in the order of ``np.random.default_rng(E).permutation`` of
    every row."""
    E, Gn = tp.f.size, tp.g.size
    every = [(g, k) for g in range(Gn) for k in range(-1, E)]
    if len(every) <= MAX_ROWS:
        return every
    rows = [(g, -1) for g in range(Gn)]
    lines = sorted({e for e in EDGE_LINES + (E - 1,) if e < E})
    first = sorted({g for g in EDGE_LINES + (Gn - 1,) if g < Gn})
    rows += [(g, k) for g in first + [g for g in range(Gn) if g not in first] for k in lines]
    rows = rows[:MAX_ROWS - FILL]
    rows += [every[p] for p in np.random.default_rng(E).permutation(len(every))]
    return list(dict.fromkeys(rows))[:MAX_ROWS]


PICKUPS = ('none', 'random', 'one')


def pickup_weights(kind, Bt, Gn):
    """The pickup of a row-level test, float64 numpy: 'none' None; 'random' weights [Bt,Gn] in [0.1, 1.1) with column Gn // 2 exactly
    zero; 'one' weights [Gn] (shared by the grids) that are zero but for the last unit's: W_g is exactly 0 in that unit's rows
    alone, and every other row sends the whole lost output to it."""
    if kind == 'none':
        return None
    if kind == 'one':
        w = np.zeros(Gn)
        w[Gn - 1] = 1.0
        return w
    assert kind == 'random'
    w = 0.1 + np.random.default_rng(Gn).random((Bt, Gn))
    w[:, Gn // 2] = 0.0
    return w


def row_reference(s, i, g, k, w):
    """What the reference makes of row (g, k) of grid ``i`` of a set-up ``s`` (``b``, ``l``, ``g`` float64 [Bt,...], ``base_v``,
    ``base_theta``, ``tp``) with the grid's pickup weights ``w`` ([Gn] or None): (a view of ``s`` whose generator table of grid
    ``i`` is the one without row g, the pickup applied, and whose start of grid ``i`` is ``nr.start`` on it; the lines that are
    out as an index array, empty for k = -1).  The view has the fields the N-1 file's row checks read."""
    rest = gref.without(s.g[i], g, w)
    start = nr.start(s.b[i], rest, s.tp.slack, s.base_v[i], s.base_theta[i])
    return (SimpleNamespace(tp=s.tp, b=s.b, l=s.l, g={i: rest}, starts={i: start}),
            np.array([k] if k >= 0 else [], dtype=np.int64))


def rows_islanding(tp, rows):
    """[P] bool: the row's line is a bridge of the topology (``powerflow._bridges``); a generator alone never islands."""
    bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
    return np.array([k >= 0 and bool(bridges[k]) for _, k in rows], dtype=bool)
