"""Test-side topologies and grid values for the power-flow programs (``powerflow.analyse_topology``, ``gns_pf_solve`` and
``gns_pf_adjoint``; through the ``fd_`` functions ``powerflow.analyse_fd_topology`` and ``gns_fd_solve``): generated families at the
shapes where the analysis and the kernels could go wrong, finders of the largest topologies whose LDS image fits the 160 KiB limit,
grids on a topology in two value regimes, and the one-step residual bound.

A topology is ``Topo(name, n, f, t, g, slack)``: 1-based int64 numpy ids of the lines' ends and the generators' buses."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PF_LDS_MAX_BYTES

Topo = namedtuple('Topo', ['name', 'n', 'f', 't', 'g', 'slack'])
LDS_LIMIT = PF_LDS_MAX_BYTES            # 163 840 B: 160 KiB, the LDS of one workgroup on gfx950
# the bound of the one-step test: ||J dx - F||_inf <= STEP_TOL (||J||_inf ||dx||_inf + ||F||_inf)
STEP_TOL = 1e-10
# refusal messages (powerflow._check, powerflow.analyse_topology)
LDS_MESSAGE = r"LDS image of (\d+) B exceeds the 163840 B"
SLOTS_MESSAGE = r"needs (\d+) slots, nnz\(L\+U\) \+ dim, more than the 65535-slot limit"


def _ids(*a):
    return tuple(np.asarray(x, dtype=np.int64) for x in a)


def path(n, pv=()):
    """A chain 1 - 2 - ... - n, slack and its generator at bus 1, one more generator on every bus of ``pv``."""
    f, t, g = _ids(np.arange(1, n), np.arange(2, n + 1), [1, *pv])
    return Topo(f'path{n}' + (f'_pv{len(pv)}' if pv else ''), n, f, t, g, 1)


def star(n, form):
    """Hub bus 1 with n - 1 leaves.  ``pq``: the slack and the only generator at the hub; ``pv``: the slack at the hub and a generator
    on every leaf (every leaf's theta couples only to the slack: J is diagonal); ``leaf_slack``: the slack and its generator on leaf
    2, so every other bus's unknowns couple through the hub."""
    f, t = _ids(np.ones(n - 1), np.arange(2, n + 1))
    if form == 'pq':
        return Topo(f'star{n}_pq', n, f, t, _ids([1])[0], 1)
    if form == 'pv':
        return Topo(f'star{n}_pv', n, f, t, _ids(np.arange(1, n + 1))[0], 1)
    return Topo(f'star{n}_leaf_slack', n, f, t, _ids([2])[0], 2)


def lattice(k, slack=1):
    """A k x k grid graph, bus (r, c) = r k + c + 1; the slack's generator and one on every fifth bus."""
    f, t = [], []
    for r in range(k):
        for c in range(k):
            i = r * k + c + 1
            if c + 1 < k:
                f.append(i), t.append(i + 1)
            if r + 1 < k:
                f.append(i), t.append(i + k)
    g = sorted({slack, *range(5, k * k + 1, 5)})
    return Topo(f'lattice{k}x{k}', k * k, *_ids(f, t, g), slack)


def complete(n):
    """K_n: a line between every pair of buses; slack and its generator at bus 1 only (every other bus PQ)."""
    f, t = np.triu_indices(n, 1)
    return Topo(f'complete{n}', n, *_ids(f + 1, t + 1, [1]), 1)


def random_meshed(n, seed):
    """A random spanning tree plus extra lines, three of them parallel to tree lines, and one line whose two ends are one bus."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n) + 1
    f, t = [], []
    for i in range(1, n):
        f.append(int(order[rng.integers(0, i)])), t.append(int(order[i]))
    for _ in range(n // 2):
        a, b = rng.choice(n, 2, replace=False) + 1
        f.append(int(a)), t.append(int(b))
    for j in rng.choice(n - 1, 3, replace=False):
        f.append(t[j]), t.append(f[j])                      # parallel, the other way round
    loop = int(rng.integers(1, n + 1))
    f.append(loop), t.append(loop)
    g = np.sort(rng.choice(n, max(2, n // 6), replace=False) + 1)
    return Topo(f'random{n}_parallel_selfloop', n, *_ids(f, t, g), int(g[0]))


def ring_slack_without_generator(n):
    """A ring with a chord; the slack (bus 1) carries no generator, PV buses do."""
    f, t = list(range(1, n + 1)) + [1], list(range(2, n + 1)) + [1, n // 2]
    return Topo(f'ring{n}_slack_no_gen', n, *_ids(f, t, [3, n // 3, 2 * n // 3]), 1)


def stacked_generators(n, seed):
    """A random meshed graph where bus 4 carries four generators (listed apart from each other) and the slack carries two."""
    base = random_meshed(n, seed)
    f, t = base.f[:-1], base.t[:-1]                          # without its self-loop
    g = _ids([4, 1, 7, 4, 1, 4, 9, 4])[0]
    return Topo(f'random{n}_stacked_gens', n, f, t, g, 1)


def many_generators_and_lines(n=150):
    """Bus 1 with 70 lines (more than a wave's 64 lanes) to buses 2..71, a chain through 71..n, and 70 generators on distinct buses."""
    f = [1] * 70 + list(range(71, n))
    t = list(range(2, 72)) + list(range(72, n + 1))
    g = [1] + list(range(3, 2 * 69 + 3, 2))
    return Topo(f'hub{n}_70lines_70gens', n, *_ids(f, t, g), 1)


def wheel(n=71):
    """Hub bus 1 joined to each of the rim buses 2..n (n - 1 lines at one bus: 70, more than a wave's 64 lanes) and the rim ring
    2 - 3 - ... - n - 2: no line is a bridge.  The slack is rim bus 2, so the hub is a PQ bus whose diagonal the solve reads.  Not in
    ``families()``."""
    rim = np.arange(2, n + 1)
    f, t = np.r_[np.ones(n - 1, dtype=np.int64), rim], np.r_[rim, rim[1:], 2]
    return Topo(f'wheel{n}', n, *_ids(f, t, [2, n // 3, 2 * n // 3]), 2)


def wheel_many_generators(n=71, gn=66):
    """``wheel(n)`` with a generator on each of the rim buses 2..gn + 1 (66 units: more generator rows than a wave's 64 lanes, every
    one the sole unit of its bus, the first on the slack).  Not in ``families()``."""
    return wheel(n)._replace(name=f'wheel{n}_{gn}gens', g=np.arange(2, gn + 2, dtype=np.int64))


def _info(tp, analyse=powerflow.analyse_topology):
    """The info dict of ``analyse`` (``powerflow.analyse_topology`` or ``powerflow.analyse_fd_topology``) on tp."""
    return analyse(tp.n, tp.f, tp.t, tp.g, tp.slack).info


def _largest(make, lo, hi, analyse=powerflow.analyse_topology):
    """The largest size s in [lo, hi) with make(s)'s LDS image (of ``analyse``) within the limit (monotone in s); an analysis refusal
    counts as over."""
    def fits(s):
        try:
            return _info(make(s), analyse)['lds_bytes'] <= LDS_LIMIT
        except gns_mod.GNSError:
            return False
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def _boundary(analyse):
    n_path = _largest(path, 2, 4096, analyse)
    n_k = _largest(complete, 2, 256, analyse)
    return {'path_fit': path(n_path), 'path_over': path(n_path + 1), 'complete_fit': complete(n_k)}


@functools.lru_cache(maxsize=None)
def boundary():
    """The largest path and complete graph whose LDS image fits, and the smallest path over the limit (searched, not assumed)."""
    return _boundary(powerflow.analyse_topology)


@functools.lru_cache(maxsize=None)
def fd_boundary():
    """``boundary()`` for the fast-decoupled LDS image, 8 * (nnz_lu_p + dim_p + nnz_lu_pp + dim_pp + 6 N) bytes
    (``powerflow.analyse_fd_topology``)."""
    return _boundary(powerflow.analyse_fd_topology)


def _near_multiples(makes, lo, hi, key, analyse=powerflow.analyse_topology):
    """The first topologies make(s), s in [lo, hi), of any of ``makes`` whose info[key] (of ``analyse``) is one below and one above a
    multiple of 64."""
    out = {}
    for make in makes:
        for s in range(lo, hi):
            r = _info(make(s), analyse)[key] % 64
            if r in (63, 1) and r not in out:
                out[r] = make(s)
    assert sorted(out) == [1, 63], (key, out)
    return list(out.values())


@functools.lru_cache(maxsize=None)
def families():
    """name -> Topo: every generated family (the LDS boundary ones are in ``boundary()``)."""
    fam = [path(2), path(63), path(64), path(65), path(129), path(33, pv=(2,)), path(65, pv=(20, 40)), path(66, pv=(33,)),
           star(200, 'pq'), star(200, 'pv'), star(200, 'leaf_slack'), star(65, 'pv'),
           lattice(8), lattice(16), complete(20), complete(33),
           random_meshed(40, 1), random_meshed(97, 2), ring_slack_without_generator(30), stacked_generators(24, 3),
           many_generators_and_lines()]
    # a path's nnz(L+U) grows by 12 per bus: one PV bus shifts it to 1 mod 4, three to 3 mod 4
    fam += _near_multiples([lambda s: path(s, pv=(2,)), lambda s: path(s, pv=(2, 3, 4))], 20, 60, 'nnz_lu')
    fam = {tp.name: tp for tp in fam}
    fam['pair'] = fam.pop('path2')._replace(name='pair')
    return fam


def coverage(topos, keys=('n_bus', 'dim', 'nnz_lu'), analyse=powerflow.analyse_topology):
    """For N, dim and nnz_lu (or ``keys`` of ``analyse``'s info): which residues mod 64 among {63, 0, 1} the topologies reach."""
    out = {}
    for key in keys:
        out[key] = sorted({_info(tp, analyse)[key] % 64 for tp in topos} & {63, 0, 1})
    return out


FD_KEYS = ('n_bus', 'dim_p', 'dim_pp', 'nnz_lu_p', 'nnz_lu_pp')


@functools.lru_cache(maxsize=None)
def fd_families():
    """name -> Topo: ``families()`` and paths with PV buses that bring nnz(L+U) of B' and of B'' (``analyse_fd_topology``) to one
    below and one above a multiple of 64, which no family reaches on a factor of more than one slot."""
    # a path's B' has 3 N - 5 nonzeros in L + U whatever its PV buses; B'' loses the PV buses' rows and the chain breaks there
    makes = [lambda s: path(s, pv=(2,)), lambda s: path(s, pv=(2, 3, 4))]
    fam = dict(families())
    for key in ('nnz_lu_p', 'nnz_lu_pp'):
        fam.update({tp.name: tp for tp in _near_multiples(makes, 20, 80, key, powerflow.analyse_fd_topology)})
    return fam


def fd_coverage(topos):
    """``coverage`` of the fast-decoupled analysis: N, both dimensions and both nnz(L+U)."""
    return coverage(topos, FD_KEYS, powerflow.analyse_fd_topology)


# ------------------------------------------------------------------------------------------------------------------------ values

REGIMES = ('reference', 'wide')


def grids(tp, regime, batch, seed, spread=0.1, v_spread=0.05, device='cpu'):
    """``batch`` grids on topology ``tp`` made solvable by ``synth.manufacture_solution`` (the recipe of
    ``test_powerflow_gpu._manufacture``): float32 ``(buses, lines, generators)`` on ``device``, and the chosen solution ``(v, theta)``
    float64 ``[batch, N]`` (theta ~ U[-spread, spread], 0 at the slack; |V| ~ 1 + U[-v_spread, v_spread], the first generator's vg on
    its bus).

    ``reference``: the ranges of ``synth.synth_grids`` (r in [0, 0.25] on 85 % of lines, x in [0.04, 0.6], b in [0, 0.06] on 70 %,
    tau in [0.8, 1.2], shift within +-0.2 degrees).  ``wide``: tau in [0.5, 1.5], shift within +-30 degrees, line charging b in
    [0, 1.5], and about one line in eight series-compensated (x in [-0.3, -0.05])."""
    rng = np.random.default_rng([seed, tp.n, tp.f.size, tp.g.size, REGIMES.index(regime)])
    n, e, gn = tp.n, tp.f.size, tp.g.size
    B = batch
    if regime == 'reference':
        r = rng.uniform(0.0, 0.25, (B, e)) * (rng.random((B, e)) < 0.85)
        x = rng.uniform(0.04, 0.6, (B, e))
        b = rng.uniform(0.0, 0.06, (B, e)) * (rng.random((B, e)) < 0.7)
        tau = rng.uniform(0.8, 1.2, (B, e))
        shift = rng.uniform(-0.2, 0.2, (B, e)) * (math.pi / 180)
    else:
        r = rng.uniform(0.0, 0.1, (B, e))
        x = np.where(rng.random((B, e)) < 0.125, -rng.uniform(0.05, 0.3, (B, e)), rng.uniform(0.04, 0.6, (B, e)))
        b = rng.uniform(0.0, 1.5, (B, e))
        tau = rng.uniform(0.5, 1.5, (B, e))
        shift = rng.uniform(-30.0, 30.0, (B, e)) * (math.pi / 180)
    buses = np.zeros((B, n, 6))
    buses[..., 0] = np.arange(1, n + 1)
    buses[..., 1] = 1.0
    buses[..., 2] = rng.uniform(0.0, 1.0, (B, n))
    buses[..., 3] = rng.uniform(-0.05, 0.25, (B, n))
    buses[..., 4] = 0.01
    buses[..., 5] = -0.01
    lines = np.zeros((B, e, 7))
    lines[..., 0], lines[..., 1] = tp.f, tp.t
    lines[..., 2], lines[..., 3], lines[..., 4], lines[..., 5], lines[..., 6] = r, x, b, tau, shift
    gens = np.zeros((B, gn, 7))
    gens[..., 0] = tp.g
    gens[..., 1], gens[..., 2] = 3.0, 0.0
    gens[..., 3] = gens[..., 6] = rng.uniform(0.2, 1.5, (B, gn))
    gens[..., 4] = rng.uniform(0.95, 1.09, (B, gn))
    gens[..., 5] = rng.uniform(-0.2, 0.5, (B, gn))
    buses, lines, gens = (torch.as_tensor(a, dtype=torch.float32, device=device) for a in (buses, lines, gens))
    theta = torch.as_tensor(rng.uniform(-spread, spread, (B, n)), device=device)
    theta[:, tp.slack - 1] = 0.0
    v = torch.as_tensor(rng.uniform(1 - v_spread, 1 + v_spread, (B, n)), device=device)
    gb = gens[..., 0].long() - 1
    for j in range(gn - 1, -1, -1):                           # the first generator listed on a bus sets its |V|
        v.scatter_(1, gb[:, j:j + 1], gens[:, j:j + 1, 4].double())
    if tp.slack not in tp.g:
        v[:, tp.slack - 1] = 1.0                              # a slack without a generator is held at |V| = 1
    buses, gens = synth.manufacture_solution(buses, lines, gens, tp.slack, v, theta)
    return buses, lines, gens, v, theta


def perturbed_start(v, theta, slack, seed, d_theta=0.05, d_v=0.02):
    """(v0, theta0): the manufactured solution moved by about d_theta rad and d_v pu (uniform, both signs), theta0[slack] = 0."""
    g = torch.Generator().manual_seed(seed)
    th = theta + (torch.rand(theta.shape, generator=g, dtype=torch.float64) * 2 - 1).to(theta.device) * d_theta
    th[:, slack - 1] = 0.0
    return v + (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1).to(v.device) * d_v, th


def one_step_ratio(J, F, dx):
    """||J dx - F||_inf / (||J||_inf ||dx||_inf + ||F||_inf): the relative residual of a Newton step dx of J dx = F."""
    J = J.tocsr() if hasattr(J, 'tocsr') else np.asarray(J)
    res = np.max(np.abs(J @ dx - F))
    jn = float(abs(J).sum(axis=1).max())
    return float(res / (jn * np.max(np.abs(dx)) + np.max(np.abs(F))))
