"""Test-side float64 reference of the DC N-2 contingency screen, written independently of distribution factors: both lines are
removed from the grid, the smaller grid is solved from scratch with ``dc_reference.dc_power_flow`` (a dense solve), and 0 is put back
at both outaged positions.  Islanding is decided by ``dc_contingency_reference.islands`` on the smaller grid's own graph.

``dense_rank2`` is a second float64 method (the rank-2 formulas on dense solves), used only to probe on the CPU whether the two
methods agree on a family of grids before that family is held to the bar."""
import numpy as np
import torch

import dc_contingency_reference as cref
import dc_reference as dref


def pair_islands(n_bus, f_bus, t_bus, slack_bus, j, k):
    """Whether the graph (1-based ends) without lines ``j`` and ``k`` (0-based) leaves a bus without a path to the 1-based slack."""
    return cref.islands(n_bus, np.delete(np.asarray(f_bus), [j, k]), np.delete(np.asarray(t_bus), [j, k]), slack_bus)


def pair_flows(buses, lines, generators, slack_bus, j, k):
    """Post-outage flows ``[E]`` (float64 torch, 0 at lines ``j`` and ``k``) of one grid with both lines (0-based) removed, or None
    when the removal islands a bus."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    E = lines.shape[0]
    assert j != k
    keep = torch.tensor([e for e in range(E) if e != j and e != k], dtype=torch.long)
    rest = lines[keep]
    if cref.islands(buses.shape[0], rest[:, 0].numpy(), rest[:, 1].numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, generators, slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def dense_rank2(buses, lines, generators, slack_bus, j, k):
    """The same flows by the rank-2 update on dense solves with the base matrix (float64), and the determinant of the 2x2 system."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    n = buses.shape[0]
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, _, _ = dref.make_bdc(lines, n)
    _, flow, _ = dref.dc_power_flow(buses, lines, generators, slack_bus)
    f, t = lines[:, 0].long() - 1, lines[:, 1].long() - 1
    M = torch.zeros(n, 2, dtype=torch.float64)
    for c, e in enumerate((j, k)):
        M[f[e], c] += 1.0
        M[t[e], c] -= 1.0
    Z = torch.zeros(n, 2, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(Bbus[keep][:, keep], M[keep]))
    H = Z[f] - Z[t]                                          # [E, 2]
    S = torch.tensor([j, k])
    A = torch.eye(2, dtype=torch.float64) - b[S].unsqueeze(1) * H[S]
    a = torch.linalg.solve(A, flow[S])
    out = flow + b * (H @ a)
    out[S] = 0.0
    return out, float(torch.linalg.det(A))
