"""Test-side float64 reference of the DC contingency screen, written independently of line-outage distribution factors: the line
is removed from the grid, the smaller grid is solved from scratch with ``dc_reference.dc_power_flow`` (a dense solve), and 0 is put
back at the outaged position.  Islanding is decided by a search of the smaller grid's own graph.

``dense_lodf`` is a second float64 method (the rank-1 formulas on a dense inverse), used only to probe on the CPU whether the two
methods agree on a family of grids before that family is held to the bar."""
import numpy as np
import torch

import dc_reference as dref


def islands(n_bus, f_bus, t_bus, slack_bus):
    """Whether a bus has no path of lines (1-based ends) to the 1-based slack."""
    reach = {int(slack_bus)}
    nb = {}
    for a, b in zip(np.asarray(f_bus).tolist(), np.asarray(t_bus).tolist()):
        nb.setdefault(int(a), []).append(int(b))
        nb.setdefault(int(b), []).append(int(a))
    todo = [int(slack_bus)]
    while todo:
        for k in nb.get(todo.pop(), ()):
            if k not in reach:
                reach.add(k)
                todo.append(k)
    return len(reach) < n_bus


def outage_flows(buses, lines, generators, slack_bus, k):
    """Post-outage flows ``[E]`` (float64 torch, 0 at line ``k``) of one grid with line ``k`` (0-based) removed, or None when the
    removal islands a bus."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    E = lines.shape[0]
    keep = torch.tensor([e for e in range(E) if e != k], dtype=torch.long)
    rest = lines[keep]
    if islands(buses.shape[0], rest[:, 0].numpy(), rest[:, 1].numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, generators, slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def worst(flow, rating=None):
    """(worst loading, its line: the lowest of equals) of a flow row."""
    load = flow.abs() if rating is None else flow.abs() / torch.as_tensor(rating, dtype=torch.float64)
    top = load.max()
    return float(top), int(torch.nonzero(load == top).flatten()[0])


def dense_lodf(buses, lines, generators, slack_bus, k):
    """The same flows by the rank-1 update on a dense inverse (float64), and ``1 - b_k d_k``."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    n = buses.shape[0]
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, _, _ = dref.make_bdc(lines, n)
    _, flow, _ = dref.dc_power_flow(buses, lines, generators, slack_bus)
    f, t = lines[:, 0].long() - 1, lines[:, 1].long() - 1
    a = torch.zeros(n, dtype=torch.float64)
    a[f[k]] += 1.0
    a[t[k]] -= 1.0
    z = torch.zeros(n, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(Bbus[keep][:, keep], a[keep]))
    den = 1.0 - b[k] * (z[f[k]] - z[t[k]])
    out = flow + b * (z[f] - z[t]) * (flow[k] / den)
    out[k] = 0.0
    return out, float(den)
