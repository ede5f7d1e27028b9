"""Test-side float64 gradient reference of the DC contingency screen, by autograd through "remove the line, solve the smaller grid":
for each outage the line is deleted and ``dc_reference.dc_power_flow`` (a dense solve, differentiable) runs on the rest, with 0 put
back at the outaged position.  No distribution factors, no adjoint formulas.  (``dc_contingency_reference.outage_flows`` is not used
for the flows: it converts its inputs to numpy, which cuts the graph; its islanding search is.)

The loss is ``sum_k sum(G_k * flow_k) + g_k * max(|flow_k| / rating)``, the maximum taken at the lowest line that attains it."""
import torch

import dc_contingency_reference as cref
import dc_reference as dref


def outage_flows(buses, lines, generators, slack_bus, k):
    """Post-outage flows ``[E]`` of one grid (float64 tensors, on the autograd graph of the inputs) with line ``k`` (0-based)
    removed, 0 at line ``k``; None when the removal islands a bus."""
    E = lines.shape[0]
    keep = torch.tensor([e for e in range(E) if e != k], dtype=torch.long)
    rest = lines[keep]
    if cref.islands(buses.shape[0], rest[:, 0].detach().numpy(), rest[:, 1].detach().numpy(), slack_bus):
        return None
    _, flow, _ = dref.dc_power_flow(buses, rest, generators, slack_bus)
    return torch.zeros(E, dtype=torch.float64).index_add(0, keep, flow)


def gradients(buses, lines, generators, slack_bus, outages, w_flow=None, w_worst=None, rating=None):
    """``(d loss / d buses, d lines, d generators)`` float64 of one grid, and the post-outage flows ``[K, E]`` (NaN rows where the
    outage islands).  ``w_flow`` ``[K, E]`` and ``w_worst`` ``[K]`` weigh ``line_flow`` and ``worst_loading`` (None: left out of the
    loss); ``rating`` ``[E]`` or None.  An islanding outage has no flows: its weights are not read."""
    ins = [torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True) for x in (buses, lines, generators)]
    E = ins[1].shape[0]
    rating = None if rating is None else torch.as_tensor(rating, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    flows = torch.full((len(outages), E), float('nan'), dtype=torch.float64)
    for j, k in enumerate(outages):
        flow = outage_flows(*ins, slack_bus, int(k))
        if flow is None:
            continue
        flows[j] = flow.detach()
        if w_flow is not None:
            loss = loss + (torch.as_tensor(w_flow[j], dtype=torch.float64) * flow).sum()
        if w_worst is not None:
            _, at = cref.worst(flow.detach(), rating)
            load = flow[at].abs() if rating is None else flow[at].abs() / rating[at]
            loss = loss + float(w_worst[j]) * load
    grads = torch.autograd.grad(loss, ins, allow_unused=True) if loss.requires_grad else (None, None, None)
    return tuple(torch.zeros_like(x) if g is None else g for x, g in zip(ins, grads)), flows
