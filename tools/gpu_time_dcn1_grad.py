"""Forward + backward of the DC contingency screen (``dc_contingency_screen(differentiable=True)``) against the route it replaces, on
the (grid, outage) pairs of tools/gpu_time_dcn1.py: forward + backward of ``dc_power_flow(mixed_topologies=True)`` on the expanded
batch (each grid once per outage, with that line removed; autograd sums over the copies), timed after its caches are warm.  The loss
weighs every post-outage flow and the worst loading of every pair with a rating, on both routes.  Each figure is one forward +
backward between HIP events: 5 repeats after 2 warm-ups, each repeat timed on its own, so the spread is shown next to the mean.  The
screen's forward alone (no gradient) and its backward alone are timed too, and the two routes' gradients are compared.  The exit status is non-zero when the ranges of the two routes overlap at case118 or
larger, or when their gradients differ by more than the float32 bar of the tests.
usage: python tools/gpu_time_dcn1_grad.py [case:batch ...] > profiles/dcn1_grad/gpu_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth


def event_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        out = fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms), out


def show(ms):
    return f'{ms.mean():.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


specs = sys.argv[1:] or ['14:2048', '118:256', '300:64']
failed = []
for spec in specs:
    case, bt = (int(x) for x in spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    fd = powerflow.analyse_fd_topology(case, f, t, g, slack)
    lds, lanes = powerflow._dcn1_lds_bytes(fd.host)
    alds, alanes = powerflow._dcn1_adjoint_lds_bytes(fd.host)
    outages = np.flatnonzero(~powerflow._bridges(case, f - 1, t - 1))
    K = outages.size
    print(f"case{case} x {bt} grids x {K} non-islanding outages of {E} lines = {bt * K} pairs: screen LDS {lds} B with W = {lanes} "
          f"({-(-K // lanes)} workgroups per grid); adjoint LDS {alds} B with Wa = {alanes} ({-(-K // alanes)} workgroups per grid, "
          f"{powerflow.PF_LDS_MAX_BYTES // alds} per CU by LDS), workspace {8 * bt * -(-K // alanes) * (case + 2 * E + 1) / 1e6:.2f} MB",
          flush=True)
    gen = torch.Generator().manual_seed(case)
    wf = torch.randn(bt, K, E, generator=gen, dtype=torch.float64).cuda()
    ww = torch.randn(bt, K, generator=gen, dtype=torch.float64).cuda()
    rating = (0.5 + 2.0 * torch.rand(E, generator=gen, dtype=torch.float64)).cuda()
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device='cuda')           # [K, E-1]
    wfx = torch.gather(wf, 2, keep.unsqueeze(0).expand(bt, K, E - 1))
    ins = [x.clone().requires_grad_(True) for x in (bu, li, ge)]

    def screen_fwd_bwd(flows=True):
        res = powerflow.dc_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating, flows=flows, differentiable=True)
        loss = (ww * res.worst_loading).sum()
        if flows:
            loss = loss + (wf * res.line_flow).sum()
        return torch.autograd.grad(loss, ins)

    def expanded_fwd_bwd():
        xl = ins[1][:, keep].reshape(bt * K, E - 1, 7)
        xb, xg = ins[0].repeat_interleave(K, dim=0), ins[2].repeat_interleave(K, dim=0)
        res = powerflow.dc_power_flow(xb, xl, xg, slack_bus=slack, mixed_topologies=True)
        flow = res.line_flow.reshape(bt, K, E - 1)
        loss = (wfx * flow).sum() + (ww * (flow.abs() / rating[keep]).amax(dim=2)).sum()
        return torch.autograd.grad(loss, ins)

    ms_x, gx = event_ms(expanded_fwd_bwd)
    ms_s, gs = event_ms(screen_fwd_bwd)
    ms_slim, _ = event_ms(lambda: screen_fwd_bwd(flows=False))
    ms_fwd, _ = event_ms(lambda: powerflow.dc_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages, rating=rating))
    res = powerflow.dc_contingency_screen(*ins, slack_bus=slack, outages=outages, rating=rating, differentiable=True)
    loss = (wf * res.line_flow).sum() + (ww * res.worst_loading).sum()
    ms_bwd, _ = event_ms(lambda: torch.autograd.grad(loss, ins, retain_graph=True))
    # the float32 bar of the gradient tests, per grid and column: max|a - b| <= 1e-5 max|b| + 1e-7; err is the worst ratio to it
    err = max(float(((a - b).abs().amax(dim=1) / (1e-5 * b.abs().amax(dim=1) + 1e-7)).max()) for a, b in zip(gs, gx))
    print(f"  expanded dc_power_flow(mixed_topologies=True) forward + backward, {bt * K} grids on {K} topologies, caches warm: "
          f"{show(ms_x)}", flush=True)
    print(f"  dc_contingency_screen(differentiable=True) forward + backward, flows=True : {show(ms_s)}", flush=True)
    print(f"  dc_contingency_screen(differentiable=True) forward + backward, flows=False: {show(ms_slim)}", flush=True)
    print(f"  the screen's forward alone (no gradient, flows=True): {show(ms_fwd)}", flush=True)
    print(f"  the screen's backward alone (the adjoint's two kernels and autograd's own work): {show(ms_bwd)}", flush=True)
    print(f"  expanded / screen: {ms_x.mean() / ms_s.mean():.1f}x; slowest screen repeat against fastest expanded repeat: "
          f"{ms_x.min() / ms_s.max():.1f}x (ranges {'do not overlap' if ms_s.max() < ms_x.min() else 'OVERLAP'}); worst difference "
          f"of the two routes' float32 gradients per grid and column, as a fraction of the bar 1e-5 scale + 1e-7: {err:.3f}", flush=True)
    if case >= 118 and not ms_s.max() < ms_x.min():
        failed.append(f'case{case}: the ranges overlap')
    if not err <= 1.0:
        failed.append(f'case{case}: the two routes\' gradients differ by {err:.3f} of the bar')
if failed:
    sys.exit('FAILED: ' + '; '.join(failed))
