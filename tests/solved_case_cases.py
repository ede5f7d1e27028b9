"""The grids the ``powerflow.solved_case`` tests share, made once on the CPU and never changed: the generated families of
``pf_topologies`` at the shapes where the kernel could go wrong, in both value regimes, and the synthetic cases; each with two states
(its manufactured solution and ``pf_topologies.perturbed_start`` of it), a per-grid rating, and the float64 reference of every grid
(``solved_case_reference.forward``), computed once."""
import functools
from collections import namedtuple

import torch

import pf_topologies as pt
import solved_case_reference as sref
from opf_graph_neural_solver_amd import synth

Grids = namedtuple('Grids', ['name', 'slack', 'buses', 'lines', 'gens', 'v', 'theta'])

# pair: N = 2; path63 / 64 / 65: the lane boundary; parallel lines and a line from a bus to itself; four units on one bus and two on
# the slack; a slack without a unit; more than 64 lines at one bus and more than 64 units
FAMILIES = ('pair', 'path63', 'path64', 'path65', 'random40_parallel_selfloop', 'random24_stacked_gens', 'ring30_slack_no_gen',
            'hub150_70lines_70gens')
SYNTH = ((14, 3), (118, 2), (300, 1))
STATES = ('solution', 'perturbed')
FAMILY_BATCH = 3


def names():
    return [f'{f}-{r}' for f in FAMILIES for r in pt.REGIMES] + [f'case{c}' for c, _ in SYNTH]


@functools.lru_cache(maxsize=None)
def grids(name):
    if name.startswith('case'):
        case = int(name[4:])
        buses, lines, gens, slack, v, theta = synth.solvable_grids(case, dict(SYNTH)[case])
        return Grids(name, slack, buses, lines, gens, v.double(), theta.double())
    family, regime = name.rsplit('-', 1)
    tp = pt.families()[family]
    buses, lines, gens, v, theta = pt.grids(tp, regime, FAMILY_BATCH, seed=11)
    return Grids(name, tp.slack, buses, lines, gens, v, theta)


@functools.lru_cache(maxsize=None)
def state(name, which):
    """(v, theta) float64 [Bt,N] on the CPU."""
    g = grids(name)
    if which == 'solution':
        return g.v, g.theta
    return pt.perturbed_start(g.v, g.theta, g.slack, seed=5)


@functools.lru_cache(maxsize=None)
def rating(name):
    """[Bt,E] float64 in [0.5, 2.5), seeded."""
    g = grids(name)
    gen = torch.Generator().manual_seed(len(name) + g.lines.shape[1])
    return 0.5 + 2.0 * torch.rand(g.lines.shape[:2], generator=gen, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def reference(name, which, rated=True):
    """The ``solved_case_reference.Case`` of every grid, a list."""
    g = grids(name)
    v, th = state(name, which)
    rt = rating(name) if rated else None
    return [sref.forward(g.buses[b].double().numpy(), g.lines[b].double().numpy(), g.gens[b].double().numpy(), g.slack, v[b].numpy(),
                         th[b].numpy(), None if rt is None else rt[b].numpy()) for b in range(g.buses.shape[0])]
