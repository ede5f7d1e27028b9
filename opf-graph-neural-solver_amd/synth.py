"""Synthetic power grids in the layout the GNS hot path consumes.

No case30/118/300 data exists offline and the reference's shipped case14 pickles cannot be opened
with a non-executing loader, so every test and benchmark input is generated here.  The generator
mirrors, vectorised over the batch and on any torch device,
  * the perturbation ranges of the reference's ``GNS/augment_grids.py:12-53`` (r, x, b x U[0.9,1.1];
    tau ~ U[0.8,1.2]; shift ~ U[-0.2,0.2] degrees; vg x U[0.95,1.05]; Pg ~ U[.25,.75] of the unit's
    range; Pd x U[.5,1.5] then rescaled so that sum(Pd) == sum(Pg); Qd x U[.5,1.5]), and
  * the column selection / per-unit normalisation of ``GNS/utils.py:17-41`` (``prepare_grid``):
    buses [N,6] = (bus_i, type, Pd, Qd, Gs=1/baseMVA, Bs=-1/baseMVA), lines [E,7] =
    (f_bus, t_bus, r, x, b, tau, shift[rad]), generators [Gn,7] = (bus_i, Pmax, Pmin, Pg_set, vg, qg, Pg).
Topology is one fixed graph per case and is shared by the whole batch, exactly like the reference's
data (``augment_grids.py`` perturbs continuous columns only).  Sizes come from ``GNS/utils.py:45-56``.
case14 uses the public IEEE 14-bus test system as its base; the larger cases are case-SHAPED random
connected graphs with contiguous bus ids (the real case300 has non-contiguous ids, which the reference's
``bus_id - 1`` indexing cannot address).
"""
from __future__ import annotations

import math

import numpy as np
import torch

# 200 is not a reference case: a case-shaped synthetic grid between case118 and case300 (exercises the 64-160 KB LDS plane of the
# lane-per-grid forward, which case118 (59 KB) and case300 (HBM path) both miss)
CASE_SHAPES = {14: (14, 20, 5), 30: (30, 41, 6), 118: (118, 186, 54), 200: (200, 290, 45), 300: (300, 411, 69)}
BASE_MVA = 100.0

# IEEE 14-bus test system (public data): from, to, r, x, b
_IEEE14_BRANCH = [
    (1, 2, 0.01938, 0.05917, 0.0528), (1, 5, 0.05403, 0.22304, 0.0492), (2, 3, 0.04699, 0.19797, 0.0438),
    (2, 4, 0.05811, 0.17632, 0.0340), (2, 5, 0.05695, 0.17388, 0.0346), (3, 4, 0.06701, 0.17103, 0.0128),
    (4, 5, 0.01335, 0.04211, 0.0), (4, 7, 0.0, 0.20912, 0.0), (4, 9, 0.0, 0.55618, 0.0),
    (5, 6, 0.0, 0.25202, 0.0), (6, 11, 0.09498, 0.19890, 0.0), (6, 12, 0.12291, 0.25581, 0.0),
    (6, 13, 0.06615, 0.13027, 0.0), (7, 8, 0.0, 0.17615, 0.0), (7, 9, 0.0, 0.11001, 0.0),
    (9, 10, 0.03181, 0.08450, 0.0), (9, 14, 0.12711, 0.27038, 0.0), (10, 11, 0.08205, 0.19207, 0.0),
    (12, 13, 0.22092, 0.19988, 0.0), (13, 14, 0.17093, 0.34802, 0.0)]
_IEEE14_PD = [0.0, 21.7, 94.2, 47.8, 7.6, 11.2, 0.0, 0.0, 29.5, 9.0, 3.5, 6.1, 13.5, 14.9]
_IEEE14_QD = [0.0, 12.7, 19.0, -3.9, 1.6, 7.5, 0.0, 0.0, 16.6, 5.8, 1.8, 1.6, 5.8, 5.0]
# bus, Pg, Qg, Vg, Pmax, Pmin
_IEEE14_GEN = [(1, 232.4, -16.9, 1.06, 332.4, 0.0), (2, 40.0, 42.4, 1.045, 140.0, 0.0), (3, 0.0, 23.4, 1.01, 100.0, 0.0),
               (6, 0.0, 12.2, 1.07, 100.0, 0.0), (8, 0.0, 17.4, 1.09, 100.0, 0.0)]


def base_case(case_nr: int) -> dict:
    """Un-augmented base quantities (float64 numpy, MW / MVAr / p.u. like a PYPOWER case)."""
    if case_nr not in CASE_SHAPES:
        raise ValueError(f'unknown case {case_nr}; known: {sorted(CASE_SHAPES)}')
    n, e, gn = CASE_SHAPES[case_nr]
    if case_nr == 14:
        br = np.array(_IEEE14_BRANCH, dtype=np.float64)
        gen = np.array(_IEEE14_GEN, dtype=np.float64)
        return dict(f_bus=br[:, 0].astype(np.int64), t_bus=br[:, 1].astype(np.int64), r=br[:, 2], x=br[:, 3], b=br[:, 4],
                    Pd=np.array(_IEEE14_PD), Qd=np.array(_IEEE14_QD), gen_bus=gen[:, 0].astype(np.int64),
                    Pg=gen[:, 1], Qg=gen[:, 2], Vg=gen[:, 3], Pmax=gen[:, 4], Pmin=gen[:, 5])
    rng = np.random.default_rng(1000 + case_nr)
    # random spanning tree over a random bus order, then extra lines (parallel lines allowed)
    order = rng.permutation(n) + 1
    f, t = [], []
    for i in range(1, n):
        a, b_ = int(order[rng.integers(0, i)]), int(order[i])
        if rng.random() < 0.5:
            a, b_ = b_, a
        f.append(a); t.append(b_)
    while len(f) < e:
        a, b_ = (int(z) for z in rng.integers(1, n + 1, size=2))
        if a != b_:
            f.append(a); t.append(b_)
    perm = rng.permutation(e)
    f_bus, t_bus = np.array(f, dtype=np.int64)[perm], np.array(t, dtype=np.int64)[perm]
    gen_bus = np.sort(rng.choice(n, size=gn, replace=False) + 1).astype(np.int64)
    pmax = rng.uniform(100.0, 350.0, size=gn)
    load = rng.uniform(0.0, 1.0, size=n) * (rng.random(n) < 0.8)
    return dict(f_bus=f_bus, t_bus=t_bus, r=rng.uniform(0.0, 0.25, size=e) * (rng.random(e) < 0.85),
                x=rng.uniform(0.04, 0.6, size=e), b=rng.uniform(0.0, 0.06, size=e) * (rng.random(e) < 0.7),
                Pd=load * pmax.sum() * 0.5 / max(load.sum(), 1e-9), Qd=rng.uniform(-5.0, 25.0, size=n),
                gen_bus=gen_bus, Pg=pmax * 0.5, Qg=rng.uniform(-20.0, 50.0, size=gn), Vg=rng.uniform(1.0, 1.09, size=gn),
                Pmax=pmax, Pmin=np.zeros(gn))


def case_topology(case_nr: int):
    """(f_bus[E], t_bus[E], gen_bus[Gn]) as 1-based int64 numpy arrays."""
    c = base_case(case_nr)
    return c['f_bus'], c['t_bus'], c['gen_bus']


def _hash32(x):
    """lowbias32 integer hash on int64 tensors holding 32-bit values (same bits on CPU and GPU)."""
    m = 0xFFFFFFFF
    x = (x ^ (x >> 16)) & m
    x = (x * 0x7FEB352D) & m
    x = (x ^ (x >> 15)) & m
    x = (x * 0x846CA68B) & m
    return (x ^ (x >> 16)) & m


def counter_uniform(seed: int, stream: int, first_index: int, batch: int, width: int, device) -> torch.Tensor:
    """Counter-based U[0,1) of shape [batch, width]: the value for (grid g, element j) is a hash of
    (seed, stream, first_index + g, j) and of nothing else - no generator state - so any shard of a batch, on any
    device, reproduces the rows of the unsharded batch bit for bit (every GPU count sees the same grids)."""
    g = torch.arange(first_index, first_index + batch, dtype=torch.int64, device=device).unsqueeze(1)
    j = torch.arange(width, dtype=torch.int64, device=device).unsqueeze(0)
    key = _hash32(torch.full((1, 1), (int(seed) * 0x9E3779B1 + int(stream) * 0x85EBCA6B + 0x1234567) & 0xFFFFFFFF,
                             dtype=torch.int64, device=device))
    h = _hash32((key + (g & 0xFFFFFFFF)) & 0xFFFFFFFF)
    h = _hash32((h ^ ((g >> 32) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    h = _hash32((h + j * 0x27D4EB2F) & 0xFFFFFFFF)
    return (h >> 8).to(torch.float32) * (1.0 / 16777216.0)          # 24 random bits: exact in fp32


def synth_grids(case_nr: int, batch: int, seed: int = 0, device='cpu', load_scale: float = 1.0, augment: bool = True,
                first_index: int = 0):
    """Return (buses[B,N,6], lines[B,E,7], generators[B,Gn,7]) float32 on ``device`` for the grids
    ``first_index .. first_index + batch - 1`` of the (seed, case) data set.

    Every random draw is a counter-based hash of (seed, grid index, column, element): ``synth_grids(c, 8, s)[..][2:5]``
    equals ``synth_grids(c, 3, s, first_index=2)`` bit for bit, on the CPU and on the device.
    ``load_scale`` multiplies Pd after balancing; < ~0.6 drives the lambda < 0.5 branch of
    ``global_active_compensation`` (GNS/main.py:48,54), which balanced random-weight grids never reach.
    """
    c = base_case(case_nr)
    n, e, gn = CASE_SHAPES[case_nr]
    dev = torch.device(device)
    f32 = dict(dtype=torch.float32, device=dev)
    stream = [0]

    def tens(a):
        return torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)

    def uni(lo, hi, *shape):
        stream[0] += 1
        assert shape[0] == batch and len(shape) == 2
        return counter_uniform(seed, stream[0], first_index, batch, shape[1], dev) * (hi - lo) + lo

    def rowsum(t):
        # fixed left-to-right order in float64: the same bits whatever the batch size or the device's reduction strategy
        acc = torch.zeros(t.shape[0], dtype=torch.float64, device=dev)
        for j in range(t.shape[1]):
            acc = acc + t[:, j].double()
        return acc.unsqueeze(1)

    one = lambda *shape: torch.ones(shape, **f32)
    amp = (lambda lo, hi, *s: uni(lo, hi, *s)) if augment else (lambda lo, hi, *s: one(*s))
    r = tens(c['r']) * amp(0.9, 1.1, batch, e)
    x = tens(c['x']) * amp(0.9, 1.1, batch, e)
    b = tens(c['b']) * amp(0.9, 1.1, batch, e)
    tau = uni(0.8, 1.2, batch, e) if augment else one(batch, e)
    shift_deg = uni(-0.2, 0.2, batch, e) if augment else torch.zeros(batch, e, **f32)
    vg = tens(c['Vg']) * amp(0.95, 1.05, batch, gn)
    pmax, pmin = tens(c['Pmax']).expand(batch, gn), tens(c['Pmin']).expand(batch, gn)
    span = pmax - pmin
    pg = (pmin + span * 0.25) + uni(0.0, 1.0, batch, gn) * (span * 0.75 - (pmin + span * 0.25)) if augment \
        else tens(c['Pg']).expand(batch, gn)
    pd = tens(c['Pd']) * amp(0.5, 1.5, batch, n)
    ratio = (rowsum(pg) / rowsum(pd).clamp_min(1e-9)).to(torch.float32)        # sum(Pd) == sum(Pg) (augment_grids.py:51)
    pd = pd * ratio * load_scale
    qd = tens(c['Qd']) * amp(0.5, 1.5, batch, n)
    qg = tens(c['Qg']).expand(batch, gn)

    buses = torch.zeros(batch, n, 6, **f32)
    buses[:, :, 0] = torch.arange(1, n + 1, **f32)
    buses[:, :, 1] = 1.0
    buses[:, :, 2] = pd / BASE_MVA
    buses[:, :, 3] = qd / BASE_MVA
    buses[:, :, 4] = 1.0 / BASE_MVA
    buses[:, :, 5] = -1.0 / BASE_MVA
    lines = torch.zeros(batch, e, 7, **f32)
    lines[:, :, 0] = tens(c['f_bus'])
    lines[:, :, 1] = tens(c['t_bus'])
    lines[:, :, 2], lines[:, :, 3], lines[:, :, 4] = r, x, b
    lines[:, :, 5] = torch.where(tau == 0, torch.ones_like(tau), tau)
    lines[:, :, 6] = shift_deg * (math.pi / 180.0)
    gens = torch.zeros(batch, gn, 7, **f32)
    gens[:, :, 0] = tens(c['gen_bus'])
    gens[:, :, 1] = pmax / BASE_MVA
    gens[:, :, 2] = pmin / BASE_MVA
    gens[:, :, 3] = pg / BASE_MVA
    gens[:, :, 4] = vg
    gens[:, :, 5] = qg / BASE_MVA
    gens[:, :, 6] = pg / BASE_MVA
    return buses, lines, gens


def raw_case_arrays(case_nr: int, batch: int, seed: int = 0, zero_tau_fraction: float = 0.3):
    """Synthetic PYPOWER case-format arrays ``bus[B,N,13]``, ``branch[B,E,13]``, ``gen[B,Gn,21]`` (float64, MW / degrees)
    for the input producer ``prepare.prepare_grids``.  A fraction of the lines carries ratio 0 (= "no transformer" in
    MATPOWER), which ``GNS/utils.py:33`` maps to 1."""
    c = base_case(case_nr)
    n, e, gn = CASE_SHAPES[case_nr]
    g = torch.Generator().manual_seed(int(seed))
    f64 = torch.float64
    u = lambda lo, hi, *s: torch.rand(s, generator=g, dtype=f64) * (hi - lo) + lo
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    bus = torch.zeros(batch, n, 13, dtype=f64)
    bus[:, :, 0] = torch.arange(1, n + 1, dtype=f64)
    bus[:, :, 1] = 1
    bus[:, :, 2] = T(c['Pd']) * u(0.5, 1.5, batch, n)
    bus[:, :, 3] = T(c['Qd']) * u(0.5, 1.5, batch, n)
    bus[:, :, 4] = u(0.0, 5.0, batch, n)             # Gs, Bs of the raw case are overwritten by prepare_grid
    bus[:, :, 5] = u(0.0, 20.0, batch, n)
    bus[:, :, 7], bus[:, :, 9], bus[:, :, 11], bus[:, :, 12] = 1.0, 135.0, 1.06, 0.94
    br = torch.zeros(batch, e, 13, dtype=f64)
    br[:, :, 0], br[:, :, 1] = T(c['f_bus']), T(c['t_bus'])
    br[:, :, 2] = T(c['r']) * u(0.9, 1.1, batch, e)
    br[:, :, 3] = T(c['x']) * u(0.9, 1.1, batch, e)
    br[:, :, 4] = T(c['b']) * u(0.9, 1.1, batch, e)
    tau = u(0.8, 1.2, batch, e)
    br[:, :, 8] = torch.where(torch.rand(batch, e, generator=g) < zero_tau_fraction, torch.zeros_like(tau), tau)
    br[:, :, 9] = u(-0.2, 0.2, batch, e)
    br[:, :, 10], br[:, :, 11], br[:, :, 12] = 1, -360, 360
    ge = torch.zeros(batch, gn, 21, dtype=f64)
    ge[:, :, 0] = T(c['gen_bus'])
    ge[:, :, 8], ge[:, :, 9] = T(c['Pmax']), T(c['Pmin'])
    ge[:, :, 1] = T(c['Pmin']) + (T(c['Pmax']) - T(c['Pmin'])) * u(0.25, 0.75, batch, gn)
    ge[:, :, 2] = T(c['Qg'])
    ge[:, :, 3], ge[:, :, 4] = 100.0, -50.0
    ge[:, :, 5] = T(c['Vg']) * u(0.95, 1.05, batch, gn)
    ge[:, :, 6], ge[:, :, 7] = BASE_MVA, 1
    return bus, br, ge


def contingency_grids(case_nr: int, batch: int, outages, seed: int = 0, device='cpu', shuffle: bool = False):
    """N-1 contingency variants of a case: grid ``i`` is ``synth_grids(case_nr, batch, seed)[i]`` with line ``outages[j]`` (0-based)
    removed, ``j = i % len(outages)`` (round-robin) or, with ``shuffle``, drawn per grid from a generator seeded with ``seed``.
    Every variant keeps the other lines in their order, so all stack into one ``lines[batch, E-1, 7]`` tensor whose id columns differ
    between variants: a batch that mixes topologies (``GNS.topology_check = 'group'``).

    Returns ``(buses[batch,N,6], lines[batch,E-1,7], generators[batch,Gn,7], outage[batch])`` with ``outage[i]`` the line removed
    from grid ``i``.  The reference reads per-line arrays at bus ids (GNS/main.py:41), so a variant is only valid when every bus id
    of its remaining lines is at most ``E-1``: an outage list that breaks this is refused (ValueError)."""
    if case_nr not in CASE_SHAPES:
        raise ValueError(f'unknown case {case_nr}; known: {sorted(CASE_SHAPES)}')
    e = CASE_SHAPES[case_nr][1]
    outages = [int(j) for j in outages]
    if not outages:
        raise ValueError('contingency_grids needs at least one outage')
    f_bus, t_bus, _ = case_topology(case_nr)
    for j in outages:
        if not 0 <= j < e:
            raise ValueError(f'outage {j} is not a line index of case{case_nr} (0..{e - 1})')
        keep = np.arange(e) != j
        top = int(max(f_bus[keep].max(), t_bus[keep].max()))
        if top > e - 1:
            raise ValueError(f'outage of line {j} leaves bus id {top} on a line of case{case_nr}, above E-1 = {e - 1}: the reference '
                             'reads per-line arrays at bus ids (GNS/main.py:41), so this variant has no valid interpretation')
    if shuffle:
        pick = torch.as_tensor(np.random.default_rng(seed).integers(0, len(outages), size=batch))
    else:
        pick = torch.arange(batch) % len(outages)
    outage = torch.as_tensor(outages, dtype=torch.int64)[pick]
    buses, lines, gens = synth_grids(case_nr, batch, seed=seed, device=device)
    cols = torch.arange(e - 1).unsqueeze(0)
    kept = cols + (cols >= outage.unsqueeze(1)).to(torch.int64)          # line indices of each variant, in order
    lines = torch.gather(lines, 1, kept.to(lines.device).unsqueeze(2).expand(batch, e - 1, 7)).contiguous()
    return buses, lines, gens, outage.to(buses.device)


def _first_generator_mask(gen_bus):
    """[B,Gn] bool: generator j is the first one listed on its bus (per grid)."""
    gn = gen_bus.shape[1]
    earlier = torch.ones(gn, gn, dtype=torch.bool, device=gen_bus.device).tril(-1)          # [j, j'] : j' < j
    return ~((gen_bus.unsqueeze(2) == gen_bus.unsqueeze(1)) & earlier).any(dim=2)


def manufacture_solution(buses, lines, generators, slack_bus, v, theta):
    """Make ``(v, theta) [B,N]`` an exact power-flow solution of the grids ("manufactured solution"; the grids of ``synth_grids``
    mostly have none).  With ``V = v e^{j theta}`` and the Y-bus of the lines and shunts (``include/gns_powerflow.h``), the
    injections ``S = V conj(Y V)`` are computed in float64, then
      * PQ buses (no generator, not the slack): Pd := -Re S, Qd := -Im S;
      * PV buses (a generator, not the slack): Pg (columns 3 and 6) of the first generator listed on the bus := Re S + Pd - the
        Pg of the bus's other generators; Qd is left as is (Q is free at a PV bus);
      * every generator bus: vg of its first generator := v (the solver holds |V| at vg there).
    The slack bus (1-based ``slack_bus``) is left as is.  Returns the adjusted ``(buses, generators)`` in the inputs' dtype
    (float32 inputs: the rounded powers make the chosen point a solution to ~1e-8).  Lines, theta and the PQ magnitudes are
    not checked against anything: ``v`` at generator buses should already be the vg the caller wants."""
    dev = buses.device
    f64 = torch.float64
    Bt, N = buses.shape[0], buses.shape[1]
    slack = int(slack_bus) - 1
    V = torch.polar(v.to(dev, f64), theta.to(dev, f64))
    f = lines[..., 0].long() - 1
    t = lines[..., 1].long() - 1
    r, x, b = lines[..., 2].to(f64), lines[..., 3].to(f64), lines[..., 4].to(f64)
    tau, sh = lines[..., 5].to(f64), lines[..., 6].to(f64)
    ys = 1.0 / torch.complex(r, x)
    ytt = ys + 0.5j * b
    yff = ytt / (tau * tau)
    yft = -ys * torch.polar(torch.ones_like(sh), sh) / tau
    ytf = -ys * torch.polar(torch.ones_like(sh), -sh) / tau
    Vf, Vt = torch.gather(V, 1, f), torch.gather(V, 1, t)
    inj = torch.cat([yff * Vf + yft * Vt, ytf * Vf + ytt * Vt], dim=1)
    idx = torch.cat([f, t], dim=1)
    I = torch.zeros(Bt, N, dtype=torch.complex128, device=dev)
    I = torch.complex(I.real.scatter_add(1, idx, inj.real), I.imag.scatter_add(1, idx, inj.imag))
    I = I + torch.complex(buses[..., 4].to(f64), buses[..., 5].to(f64)) * V
    S = V * I.conj()
    gb = generators[..., 0].long() - 1
    has_gen = torch.zeros(Bt, N, dtype=torch.bool, device=dev).scatter(1, gb, True)
    is_slack = torch.zeros(N, dtype=torch.bool, device=dev)
    is_slack[slack] = True
    pq = ~has_gen & ~is_slack
    out_b = buses.clone()
    out_b[..., 2] = torch.where(pq, -S.real, buses[..., 2].to(f64)).to(buses.dtype)
    out_b[..., 3] = torch.where(pq, -S.imag, buses[..., 3].to(f64)).to(buses.dtype)
    first = _first_generator_mask(gb)
    pg = generators[..., 6].to(f64)
    bus_pg = torch.zeros(Bt, N, dtype=f64, device=dev).scatter_add(1, gb, pg)
    others = torch.gather(bus_pg, 1, gb) - pg
    want = torch.gather(S.real + out_b[..., 2].to(f64), 1, gb) - others
    pv_first = first & (gb != slack)
    out_g = generators.clone()
    new_pg = torch.where(pv_first, want, pg).to(generators.dtype)
    out_g[..., 3] = torch.where(pv_first, new_pg, generators[..., 3])
    out_g[..., 6] = new_pg
    out_g[..., 4] = torch.where(first, torch.gather(v.to(dev, f64), 1, gb), generators[..., 4].to(f64)).to(generators.dtype)
    return out_b, out_g


def solvable_grids(case_nr: int, batch: int, seed: int = 0, angle_spread: float = 0.1, device='cpu'):
    """Grids of ``synth_grids(case_nr, batch, seed)`` made solvable by construction (``manufacture_solution``): theta ~
    U[-angle_spread, angle_spread] at every bus but the slack (theta_slack = 0), |V| ~ U[0.95, 1.05] at PQ buses and the (fp32)
    vg of the first generator at generator buses.  The slack is the bus of the case's generator with the largest Pmax.

    Returns ``(buses, lines, generators, slack_bus, v, theta)``: float32 tensors on ``device``, the 1-based slack bus, and the
    chosen solution as float64 ``[batch,N]``.  All draws are counter-based, as in ``synth_grids``, so any device gives the same
    grids.  At angle_spread 0.1 a flat-start Newton-Raphson recovers the chosen point; larger spreads can give grids with other
    valid solutions (the solver may converge to one of those)."""
    buses, lines, gens = synth_grids(case_nr, batch, seed=seed, device=device)
    slack_bus = _solvable_slack(case_nr)
    v, theta = _draw_solution(gens, buses.shape[1], slack_bus, seed, angle_spread)
    buses, gens = manufacture_solution(buses, lines, gens, slack_bus, v, theta)
    return buses, lines, gens, slack_bus, v, theta


def solvable_contingency_grids(case_nr: int, batch: int, outages, seed: int = 0, angle_spread: float = 0.1, device='cpu',
                               shuffle: bool = False):
    """N-1 contingency variants (``contingency_grids``) made solvable as ``solvable_grids`` makes its grids: the same slack, the
    same draws of ``(v, theta)``, then ``manufacture_solution`` on each variant's own lines.  A batch that mixes topologies, for
    ``powerflow.newton_raphson(..., mixed_topologies=True)``.  An outage that islands buses from the slack is allowed: its ``(v,
    theta)`` is not a reachable solution (the solver reports such grids as not solved).

    Returns ``(buses, lines, generators, slack_bus, v, theta, outage)``."""
    buses, lines, gens, outage = contingency_grids(case_nr, batch, outages, seed=seed, device=device, shuffle=shuffle)
    slack_bus = _solvable_slack(case_nr)
    v, theta = _draw_solution(gens, buses.shape[1], slack_bus, seed, angle_spread)
    buses, gens = manufacture_solution(buses, lines, gens, slack_bus, v, theta)
    return buses, lines, gens, slack_bus, v, theta, outage


def _solvable_slack(case_nr):
    """The slack of ``solvable_grids``: the bus of the case's generator with the largest Pmax (1-based)."""
    c = base_case(case_nr)
    return int(c['gen_bus'][int(np.argmax(c['Pmax']))])


def _draw_solution(gens, n, slack_bus, seed, angle_spread):
    """The chosen point of ``solvable_grids``: theta ~ U[-angle_spread, angle_spread] (0 at the slack), |V| ~ U[0.95, 1.05], then
    the vg of the first generator listed on each generator bus.  float64 ``(v, theta) [batch, n]`` on ``gens``' device."""
    batch, dev = gens.shape[0], gens.device
    f64 = torch.float64
    theta = (counter_uniform(seed, 201, 0, batch, n, dev).to(f64) * 2.0 - 1.0) * float(angle_spread)
    theta[:, slack_bus - 1] = 0.0
    v = counter_uniform(seed, 202, 0, batch, n, dev).to(f64) * 0.1 + 0.95
    gb = gens[..., 0].long() - 1
    first = _first_generator_mask(gb)
    at = torch.where(first, gb, torch.full_like(gb, n))                         # non-first generators write a dummy column
    vg = torch.cat([v, torch.zeros(batch, 1, dtype=f64, device=dev)], dim=1).scatter(1, at, gens[..., 4].to(f64))[:, :n]
    v = torch.where(torch.zeros(batch, n + 1, dtype=torch.bool, device=dev).scatter(1, at, True)[:, :n], vg, v)
    return v, theta
