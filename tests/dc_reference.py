"""Test-side float64 DC power flow (dense torch), written independently of the product code from PYPOWER's makeBdc / dcpf and
the DC branch of runpf, as the reference for the DC power-flow tests.  It is differentiable by autograd, so it is the gradient
reference too."""
import torch


def make_bdc(lines, n_bus):
    """(Bbus [N,N], b [E], Pfinj [E], Pbusinj [N]) of makeBdc: b = 1 / (x tau) with tau as given, Pfinj = -b shift."""
    f, t = lines[:, 0].long() - 1, lines[:, 1].long() - 1
    b = 1.0 / (lines[:, 3] * lines[:, 5])
    pfinj = -b * lines[:, 6]
    flat = torch.zeros(n_bus * n_bus, dtype=lines.dtype)
    flat = flat.index_add(0, f * n_bus + f, b).index_add(0, t * n_bus + t, b)
    flat = flat.index_add(0, f * n_bus + t, -b).index_add(0, t * n_bus + f, -b)
    pbusinj = torch.zeros(n_bus, dtype=lines.dtype).index_add(0, f, pfinj).index_add(0, t, -pfinj)
    return flat.view(n_bus, n_bus), b, pfinj, pbusinj


def injections(buses, lines, generators):
    """P = sum Pg on each bus - Pd - Gs - Pbusinj."""
    n = buses.shape[0]
    pg = torch.zeros(n, dtype=buses.dtype).index_add(0, generators[:, 0].long() - 1, generators[:, 6])
    return pg - buses[:, 2] - buses[:, 4] - make_bdc(lines, n)[3]


def dc_power_flow(buses, lines, generators, slack_bus):
    """(theta [N], line_flow [E], slack_p) of one grid from float64 torch tensors (1-based ``slack_bus``)."""
    buses, lines, generators = (torch.as_tensor(x, dtype=torch.float64) for x in (buses, lines, generators))
    n = buses.shape[0]
    slack = int(slack_bus) - 1
    keep = torch.tensor([i for i in range(n) if i != slack], dtype=torch.long)
    Bbus, b, pfinj, _ = make_bdc(lines, n)
    P = injections(buses, lines, generators)
    theta = torch.zeros(n, dtype=torch.float64)
    if keep.numel():
        theta = theta.index_add(0, keep, torch.linalg.solve(Bbus[keep][:, keep], P[keep]))
    f, t = lines[:, 0].long() - 1, lines[:, 1].long() - 1
    flow = b * (theta[f] - theta[t]) + pfinj
    slack_p = Bbus[slack] @ theta - P[slack]
    return theta, flow, slack_p


def gradients(buses, lines, generators, slack_bus, w_theta, w_flow, w_slack):
    """d(sum(w_theta theta) + sum(w_flow line_flow) + w_slack slack_p) / d(buses, lines, generators) by autograd, float64; a weight
    that is None leaves its output out of the loss."""
    ins = [torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True) for x in (buses, lines, generators)]
    theta, flow, slack_p = dc_power_flow(*ins, slack_bus)
    loss = torch.zeros((), dtype=torch.float64)
    for w, out in ((w_theta, theta), (w_flow, flow), (w_slack, slack_p)):
        if w is not None:
            loss = loss + (torch.as_tensor(w, dtype=torch.float64) * out).sum()
    return torch.autograd.grad(loss, ins, allow_unused=True)
