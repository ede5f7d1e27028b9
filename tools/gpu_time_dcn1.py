"""The DC contingency screen against the route it replaces, on the same (grid, outage) pairs: ``dc_contingency_screen`` with
``flows=True`` and ``flows=False`` on Bt grids and every non-islanding outage, and ``dc_power_flow(mixed_topologies=True)`` on the
expanded batch (each grid once per outage, with that line removed), timed after its caches are warm.  Each figure is one call between
HIP events: 5 repeats after 2 warm-ups, each repeat timed on its own, so the spread is shown next to the mean.  The two routes'
flows are compared too.  Bt is chosen per case so that the expanded batch stays small next to the device memory.
usage: python tools/gpu_time_dcn1.py [case:batch ...] > profiles/dcn1/gpu_time_dcn1.txt"""
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
for spec in specs:
    case, bt = (int(x) for x in spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    fd = powerflow.analyse_fd_topology(case, f, t, g, slack)
    lds, lanes = powerflow._dcn1_lds_bytes(fd.host)
    outages = np.flatnonzero(~powerflow._bridges(case, f - 1, t - 1))
    K = outages.size
    print(f"case{case} x {bt} grids x {K} non-islanding outages of {E} lines = {bt * K} pairs: B' dim {fd.info['dim_p']} nnz(L+U) "
          f"{fd.info['nnz_lu_p']}, solve {fd.info['solve_p_ops']} ops in {fd.info['solve_p_steps']} steps; screen LDS {lds} B with "
          f"W = {lanes} outages per workgroup ({-(-K // lanes)} workgroups per grid), DC LDS {powerflow._dc_lds_bytes(fd.host)} B",
          flush=True)
    # the expanded batch of the parent's route: pair (i, j) is grid i without line outages[j]
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device='cuda')           # [K, E-1]
    xl = li[:, keep].reshape(bt * K, E - 1, 7).contiguous()
    xb = bu.repeat_interleave(K, dim=0).contiguous()
    xg = ge.repeat_interleave(K, dim=0).contiguous()

    def mixed():
        return powerflow.dc_power_flow(xb, xl, xg, slack_bus=slack, mixed_topologies=True)

    ms_mixed, ref = event_ms(mixed)
    ms_full, full = event_ms(lambda: powerflow.dc_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages, flows=True))
    ms_slim, slim = event_ms(lambda: powerflow.dc_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages, flows=False))
    ms_base, _ = event_ms(lambda: powerflow.dc_power_flow(bu, li, ge, slack_bus=slack))
    assert bool(ref.converged.all()) and bool(full.converged.all()) and not bool(full.islanding.any())
    want = ref.line_flow.reshape(bt, K, E - 1)
    got = torch.gather(full.line_flow, 2, keep.unsqueeze(0).expand(bt, K, E - 1))
    err = float(((got - want).abs().amax(dim=2) / want.abs().amax(dim=2).clamp(min=1.0)).max())
    assert torch.equal(torch.nan_to_num(slim.worst_loading), torch.nan_to_num(full.worst_loading))
    print(f"  expanded dc_power_flow(mixed_topologies=True), {bt * K} grids on {K} topologies, caches warm: {show(ms_mixed)}", flush=True)
    print(f"  dc_contingency_screen flows=True  ({8 * bt * K * E / 1e6:.1f} MB of flows written): {show(ms_full)}", flush=True)
    print(f"  dc_contingency_screen flows=False ({12 * bt * K / 1e6:.2f} MB of summaries written): {show(ms_slim)}", flush=True)
    print(f"  dc_power_flow on the {bt} base grids (part of each screen call): {show(ms_base)}", flush=True)
    print(f"  expanded / screen: {ms_mixed.mean() / ms_full.mean():.1f}x with flows, {ms_mixed.mean() / ms_slim.mean():.1f}x without; "
          f"slowest screen repeat against fastest expanded repeat: {ms_mixed.min() / ms_full.max():.1f}x, "
          f"{ms_mixed.min() / ms_slim.max():.1f}x; worst scaled difference of the two routes' flows {err:.2e}", flush=True)
