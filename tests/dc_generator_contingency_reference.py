"""Test-side float64 reference of the DC generator contingency screen, written independently of distribution factors: the outaged
generator's ``Pg`` is set to 0, its shares are added to the other generators' ``Pg``, the row's line (if any) is removed from the
grid, the modified grid is solved from scratch with ``dc_reference.dc_power_flow`` (a dense solve), and 0 is put back at the outaged
line.  Islanding is decided by ``dc_contingency_reference.islands`` on the smaller grid's own graph.

``by_factors`` is a second float64 method (the screen's formulas on dense solves with the base matrix), used only to probe on the CPU
whether the two methods agree on a family of grids before that family is held to the bar."""
import numpy as np
import torch

import dc_contingency_reference as cref
import dc_reference as dref


def weights(pickup, generators, i=None):
    """The float64 pickup weights ``[Gn]`` of one grid: None, ``'pmax'`` (the generators' column 1), ``[Gn]``, or row ``i`` of
    ``[Bt,Gn]``."""
    if pickup is None:
        return None
    if isinstance(pickup, str):
        assert pickup == 'pmax'
        return torch.as_tensor(generators, dtype=torch.float64)[:, 1].clone()
    w = torch.as_tensor(pickup, dtype=torch.float64)
    return w if w.dim() == 1 else w[i]


def redispatched(generators, g, w):
    """The generators ``[Gn,7]`` (float64) with generator ``g`` out: its ``Pg`` set to 0 and shared among the others by ``w`` (None or
    a zero sum of the others' weights: nothing is shared, the slack picks the loss up)."""
    gens = torch.as_tensor(generators, dtype=torch.float64).clone()
    pg = float(gens[g, 6])
    gens[g, 6] = 0.0
    if w is not None:
        others = [h for h in range(gens.shape[0]) if h != g]
        total = sum(float(w[h]) for h in others)
        if total > 0.0:
            for h in others:
                gens[h, 6] += pg * (float(w[h]) / total)
    return gens


def direct(buses, lines, generators, slack_bus, g, k, w=None):
    """Post-outage flows ``[E]`` (float64 torch, 0 at line ``k``) of one grid with generator ``g`` out, its ``Pg`` shared by the
    weights ``w``, and line ``k`` (0-based, -1: none) removed; None when the removal islands a bus."""
    buses, lines = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines))
    gens = redispatched(generators, g, w)
    E = lines.shape[0]
    keep = torch.tensor([e for e in range(E) if e != k], dtype=torch.long)
    rest = lines[keep]
    if cref.islands(buses.shape[0], rest[:, 0].numpy(), rest[:, 1].numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, gens, slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def by_factors(buses, lines, generators, slack_bus, g, k, w=None):
    """The same flows by the screen's formulas on dense solves with the base matrix (float64), and ``1 - b_k H_k[k]`` (1 without a
    line)."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    n = buses.shape[0]
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, _, _ = dref.make_bdc(lines, n)
    A = Bbus[keep][:, keep]
    _, flow, _ = dref.dc_power_flow(buses, lines, generators, slack_bus)
    f, t = lines[:, 0].long() - 1, lines[:, 1].long() - 1
    dP = dref.injections(buses, lines, redispatched(generators, g, w)) - dref.injections(buses, lines, generators)
    u = torch.zeros(n, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(A, dP[keep]))
    fg = flow + b * (u[f] - u[t])
    if k < 0:
        return fg, 1.0
    a = torch.zeros(n, dtype=torch.float64)
    a[f[k]] += 1.0
    a[t[k]] -= 1.0
    z = torch.zeros(n, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(A, a[keep]))
    H = z[f] - z[t]
    den = 1.0 - b[k] * H[k]
    out = fg + (b * H) * (fg[k] / den)
    out[k] = 0.0
    return out, float(den)
