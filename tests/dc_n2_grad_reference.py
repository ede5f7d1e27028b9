"""Test-side float64 gradient reference of the DC N-2 contingency screen, by autograd through "remove both lines, solve the smaller
grid": for each pair both lines are deleted and ``dc_reference.dc_power_flow`` (a dense solve, differentiable) runs on the rest, with
0 put back at the two outaged positions.  No distribution factors, no adjoint formulas.

The loss is ``sum_p sum_l W_pl F'_pl + g_p max_l |F'_pl| / rating_l``, the maximum taken at the lowest line that attains it.  An
islanding pair has no flows: it is skipped and its weights are never read.

``method='rank2'`` is a second float64 method, autograd through the formulas of ``dc_n2_reference.dense_rank2``; it is used only to
probe on the CPU whether the two methods agree on a family of grids before that family is held to the bar."""
import torch

import dc_contingency_reference as cref
import dc_n2_reference as n2ref
import dc_reference as dref


def pair_flows(buses, lines, generators, slack_bus, j, k):
    """Post-outage flows ``[E]`` of one grid (float64 tensors on the autograd graph of the inputs) with lines ``j`` and ``k``
    (0-based) removed, 0 at both; None when the removal islands a bus."""
    E = lines.shape[0]
    keep = torch.tensor([e for e in range(E) if e != j and e != k], dtype=torch.long)
    rest = lines[keep]
    if cref.islands(buses.shape[0], rest[:, 0].detach().numpy(), rest[:, 1].detach().numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, generators, slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def rank2_flows(buses, lines, generators, slack_bus, j, k):
    """The same flows on the autograd graph by the rank-2 update on dense solves with the base matrix (``dense_rank2``'s formulas)."""
    n, E = buses.shape[0], lines.shape[0]
    if n2ref.pair_islands(n, lines[:, 0].detach().numpy(), lines[:, 1].detach().numpy(), slack_bus, j, k):
        return None
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, _, _ = dref.make_bdc(lines, n)
    _, flow, _ = dref.dc_power_flow(buses, lines, generators, slack_bus)
    f, t = lines[:, 0].detach().long() - 1, lines[:, 1].detach().long() - 1
    M = torch.zeros(n, 2, dtype=torch.float64)
    for c, e in enumerate((j, k)):
        M[f[e], c] += 1.0
        M[t[e], c] -= 1.0
    Z = torch.zeros(n, 2, dtype=torch.float64).index_add(0, keep, torch.linalg.solve(Bbus[keep][:, keep], M[keep]))
    H = Z[f] - Z[t]
    S = torch.tensor([j, k])
    A = torch.eye(2, dtype=torch.float64) - b[S].unsqueeze(1) * H[S]
    a = torch.linalg.solve(A, flow[S])
    out = flow + b * (H @ a)
    mask = torch.ones(E, dtype=torch.float64)
    mask[S] = 0.0
    return out * mask


def gradients(buses, lines, generators, slack_bus, pairs, w_flow=None, w_worst=None, rating=None, method='remove'):
    """``(d loss / d buses, d lines, d generators)`` float64 of one grid, and the post-outage flows ``[P, E]`` (NaN rows where the
    pair islands).  ``w_flow`` ``[P, E]`` and ``w_worst`` ``[P]`` weigh ``line_flow`` and ``worst_loading`` (None: left out of the
    loss); ``rating`` ``[E]`` or None."""
    one = pair_flows if method == 'remove' else rank2_flows
    ins = [torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True) for x in (buses, lines, generators)]
    E = ins[1].shape[0]
    rating = None if rating is None else torch.as_tensor(rating, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    flows = torch.full((len(pairs), E), float('nan'), dtype=torch.float64)
    for p, (j, k) in enumerate(pairs):
        flow = one(*ins, slack_bus, int(j), int(k))
        if flow is None:
            continue
        flows[p] = flow.detach()
        if w_flow is not None:
            loss = loss + (torch.as_tensor(w_flow[p], dtype=torch.float64) * flow).sum()
        if w_worst is not None:
            _, at = cref.worst(flow.detach(), rating)
            load = flow[at].abs() if rating is None else flow[at].abs() / rating[at]
            loss = loss + float(w_worst[p]) * load
    grads = torch.autograd.grad(loss, ins, allow_unused=True) if loss.requires_grad else (None, None, None)
    return tuple(torch.zeros_like(x) if g is None else g for x, g in zip(ins, grads)), flows
