"""Pair lists that the host and GPU tests of the DC N-2 screen's gradients share (no device needed)."""
import numpy as np

from opf_graph_neural_solver_amd import powerflow

FAMILIES = ('random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen', 'lattice8x8')


def live_pairs(n, f, t):
    """Every pair ``j < k`` of the topology (1-based ends) that does not island, ``[P,2]`` int64."""
    every = powerflow._pair_list(None, f.size)
    return every[~powerflow._pair_islanding(n, f - 1, t - 1, every)]


def special_pairs(tp):
    """The pairs a sample must hold where the family has them: the first two parallel lines that do not island together, and the
    self-loop with the first line that is not a bridge."""
    out = []
    ends = {}
    for e, (a, b) in enumerate(zip(tp.f.tolist(), tp.t.tolist())):
        if a != b:
            ends.setdefault((min(a, b), max(a, b)), []).append(e)
    for v in ends.values():
        if len(v) > 1 and not powerflow._pair_islanding(tp.n, tp.f - 1, tp.t - 1, np.array([v[:2]]))[0]:
            out.append(v[:2])
            break
    loops = np.flatnonzero(tp.f == tp.t)
    if loops.size:
        bridges = powerflow._bridges(tp.n, tp.f - 1, tp.t - 1)
        first = next(e for e in range(tp.f.size) if e != loops[0] and not bridges[e])
        out.append([int(loops[0]), first])
    return out


def family_pairs(name, tp, most=120):
    """A seeded sample of at most ``most`` non-islanding pairs of a generated family, the special pairs first."""
    live = live_pairs(tp.n, tp.f, tp.t)
    special = special_pairs(tp)
    room = most - len(special)
    rng = np.random.default_rng(len(name))
    pick = live if live.shape[0] <= room else live[np.sort(rng.choice(live.shape[0], room, replace=False))]
    return special + pick.tolist()


def case300_pairs(n, f, t, lines=41, most=60):
    """About ``most`` pairs of case300 over exactly ``lines`` distinct lines: two pairs that island although neither line is a
    bridge (the two lines of a bus with no other), a pair with the last line, and a seeded choice that names every line."""
    E = f.size
    bridges = powerflow._bridges(n, f - 1, t - 1)
    at_bus = {}
    for e, (a, b) in enumerate(zip(f.tolist(), t.tolist())):
        at_bus.setdefault(a, []).append(e)
        at_bus.setdefault(b, []).append(e)
    series = [v for v in at_bus.values() if len(v) == 2 and v[0] != v[1] and not bridges[v[0]] and not bridges[v[1]]][:2]
    assert len(series) == 2 and len({e for v in series for e in v}) == 4
    chosen = [e for v in series for e in v] + [E - 1]
    rng = np.random.default_rng(300)
    rest = [e for e in np.flatnonzero(~bridges).tolist() if e not in chosen]
    chosen += rng.choice(rest, lines - len(chosen), replace=False).tolist()
    others = chosen[5:]
    pairs = [list(v) for v in series] + [[E - 1, others[0]]] + [[others[i], others[i + 1]] for i in range(len(others) - 1)]
    while len(pairs) < most:
        j, k = rng.choice(chosen, 2, replace=False).tolist()
        pairs.append([j, k])
    assert np.unique(pairs).size == lines
    return pairs
