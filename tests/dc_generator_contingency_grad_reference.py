"""Test-side float64 gradient reference of the DC generator contingency screen, by autograd through "redispatch, remove the line,
solve the smaller grid": for each row ``(g, k)`` the outaged unit's ``Pg`` is zeroed and shared out among the others by
differentiable tensor arithmetic (so ``Pg``, the weights and Pmax all carry gradient), line ``k`` is deleted,
``dc_reference.dc_power_flow`` (a dense solve, differentiable) runs on the rest, and 0 is put back at the outaged position.  No
distribution factors, no adjoint formulas.

The loss is that of ``dc_n2_grad_reference.gradients``: ``sum_p sum_l W_pl F'_pl + g_p max_l |F'_pl| / rating_l``, the maximum taken
at the lowest line that attains it.  An islanding row has no flows: it is skipped and its weights are never read.

``method='factors'`` is a second float64 method, autograd through the formulas of
``dc_generator_contingency_reference.by_factors``; it is used only to probe on the CPU whether the two methods agree on a family
of grids before that family is held to the bar."""
import torch

import dc_contingency_reference as cref
import dc_reference as dref


def redispatched(generators, g, w):
    """The generators ``[Gn,7]`` on the autograd graph with generator ``g`` out: its ``Pg`` zeroed and shared among the others by the
    weights ``w`` (``[Gn]`` on the graph, or None; a zero sum of the others' weights: nothing is shared, and that branch is not
    differentiated)."""
    Gn = generators.shape[0]
    out = torch.ones(Gn, dtype=torch.float64)
    out[g] = 0.0
    pg = generators[:, 6] * out
    if w is not None:
        others = w * out
        total = others.sum()
        if float(total.detach()) > 0.0:
            pg = pg + generators[g, 6] * (others / total)
    return torch.cat([generators[:, :6], pg.unsqueeze(1)], dim=1)


def row_flows(buses, lines, generators, slack_bus, g, k, w):
    """Post-outage flows ``[E]`` of one grid (float64 tensors on the autograd graph of the inputs and of ``w``) with generator ``g``
    out and line ``k`` (0-based, -1: none) removed, 0 at ``k``; None when the removal islands a bus."""
    E = lines.shape[0]
    keep = torch.tensor([e for e in range(E) if e != k], dtype=torch.long)
    rest = lines[keep]
    if cref.islands(buses.shape[0], rest[:, 0].detach().numpy(), rest[:, 1].detach().numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, redispatched(generators, g, w), slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def factor_flows(buses, lines, generators, slack_bus, g, k, w):
    """The same flows on the autograd graph by the screen's formulas on dense solves with the base matrix (``by_factors``')."""
    n, E = buses.shape[0], lines.shape[0]
    f, t = lines[:, 0].detach().long() - 1, lines[:, 1].detach().long() - 1
    if k >= 0:
        keep_l = [e for e in range(E) if e != k]
        if cref.islands(n, lines[keep_l, 0].detach().numpy(), lines[keep_l, 1].detach().numpy(), slack_bus):
            return None
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, _, _ = dref.make_bdc(lines, n)
    A = Bbus[keep][:, keep]
    _, flow, _ = dref.dc_power_flow(buses, lines, generators, slack_bus)
    dP = dref.injections(buses, lines, redispatched(generators, g, w)) - dref.injections(buses, lines, generators)
    u = torch.zeros(n, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(A, dP[keep]))
    fg = flow + b * (u[f] - u[t])
    if k < 0:
        return fg
    a = torch.zeros(n, dtype=torch.float64)
    a[f[k]] += 1.0
    a[t[k]] -= 1.0
    z = torch.zeros(n, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(A, a[keep]))
    H = z[f] - z[t]
    out = fg + (b * H) * (fg[k] / (1.0 - b[k] * H[k]))
    mask = torch.ones(E, dtype=torch.float64)
    mask[k] = 0.0
    return out * mask


def gradients(buses, lines, generators, slack_bus, rows, w_flow=None, w_worst=None, rating=None, pickup=None, method='remove'):
    """``((d loss / d buses, d lines, d generators), d loss / d pickup, flows)`` float64 of one grid: the post-outage flows
    ``[P, E]`` have NaN rows where the row islands.  ``w_flow`` ``[P, E]`` and ``w_worst`` ``[P]`` weigh ``line_flow`` and
    ``worst_loading`` (None: left out of the loss); ``rating`` ``[E]`` or None.  ``pickup``: None, ``'pmax'`` (the weights are the
    generators' column 1: their gradient lands there and the second result is None) or weights ``[Gn]`` (the second result is their
    gradient)."""
    one = row_flows if method == 'remove' else factor_flows
    ins = [torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True) for x in (buses, lines, generators)]
    if pickup is None:
        w = None
    elif isinstance(pickup, str):
        assert pickup == 'pmax'
        w = ins[2][:, 1]
    else:
        w = torch.as_tensor(pickup, dtype=torch.float64).clone().requires_grad_(True)
    leaves = ins + ([w] if w is not None and w.is_leaf else [])
    E = ins[1].shape[0]
    rating = None if rating is None else torch.as_tensor(rating, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    flows = torch.full((len(rows), E), float('nan'), dtype=torch.float64)
    for p, (g, k) in enumerate(rows):
        flow = one(*ins, slack_bus, int(g), int(k), w)
        if flow is None:
            continue
        flows[p] = flow.detach()
        if w_flow is not None:
            loss = loss + (torch.as_tensor(w_flow[p], dtype=torch.float64) * flow).sum()
        if w_worst is not None:
            _, at = cref.worst(flow.detach(), rating)
            load = flow[at].abs() if rating is None else flow[at].abs() / rating[at]
            loss = loss + float(w_worst[p]) * load
    grads = torch.autograd.grad(loss, leaves, allow_unused=True) if loss.requires_grad else [None] * len(leaves)
    grads = [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, grads)]
    return tuple(grads[:3]), (grads[3] if len(grads) == 4 else None), flows
