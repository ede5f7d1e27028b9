"""The AC contingency screen against the route it replaces, on the same (grid, outage) pairs: ``ac_contingency_screen`` on Bt grids
and every non-islanding outage, and ``newton_raphson(mixed_topologies=True)`` on the expanded batch (each grid once per outage, with
that line's row deleted), warm-started from the base solution, timed after its caches are warm.  Each figure is one call between
HIP events: 5 repeats after 2 warm-ups, each repeat timed on its own, so the spread is shown next to the mean.  Also: the first
(cold cache) call of both routes, their workspace and input bytes, the mean iterations of warm and flat starts and the largest
difference between the two routes' ``v`` and ``theta``.  Exits non-zero if the screen's mean is above the expanded route's at
case118, or if the routes differ by more than 1e-9 on the pairs both converge on.
usage: python tools/gpu_time_acn1.py [case:batch ...] > profiles/acn1/gpu_time.txt"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig, load_library


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


def first_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def show(ms):
    return f'{ms.mean():.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


def nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts)


failed = []
specs = sys.argv[1:] or ['14:2048', '118:256', '300:32']
for spec in specs:
    case, bt = (int(x) for x in spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    topo = powerflow.analyse_topology(case, f, t, g, slack)
    outages = np.flatnonzero(~powerflow._bridges(case, f - 1, t - 1))
    K = outages.size
    print(f"case{case} x {bt} grids x {K} non-islanding outages of {E} lines = {bt * K} pairs: Jacobian dim {topo.info['dim']} nnz(L+U) "
          f"{topo.info['nnz_lu']}, {topo.info['n_ops']} ops in {topo.info['n_steps']} steps, nnz(Y) {topo.info['nnz_ybus']}, LDS image "
          f"{topo.info['lds_bytes']} B per pair", flush=True)
    base = powerflow.newton_raphson(bu, li, ge, slack_bus=slack)
    assert bool(base.converged.all())
    # the expanded batch of the parent's route: pair (i, j) is grid i without line outages[j], warm-started from grid i's base
    keep = torch.tensor(np.array([np.delete(np.arange(E), k) for k in outages]), device='cuda')           # [K, E-1]
    xl = li[:, keep].reshape(bt * K, E - 1, 7).contiguous()
    xb = bu.repeat_interleave(K, dim=0).contiguous()
    xg = ge.repeat_interleave(K, dim=0).contiguous()
    xv, xth = base.v.repeat_interleave(K, dim=0).contiguous(), base.theta.repeat_interleave(K, dim=0).contiguous()

    def expanded(warm=True):
        kw = dict(v0=xv, theta0=xth) if warm else {}
        return powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, **kw)

    def screen(**kw):
        return powerflow.ac_contingency_screen(bu, li, ge, slack_bus=slack, outages=outages, **kw)

    cold_x, _ = first_ms(expanded)                  # K analyses, K blobs into the device set
    cold_s, _ = first_ms(screen)                    # the base analysis is cached by the base solve above: nothing is analysed
    ms_x, ref = event_ms(expanded)
    ms_s, got = event_ms(screen)
    ms_slim, slim = event_ms(lambda: screen(flows=False, states=False))
    ms_base, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack))
    flat = expanded(warm=False)
    both = ref.converged.reshape(bt, K) & got.converged
    dv = float((ref.v.reshape(bt, K, -1) - got.v).abs().amax(dim=-1)[both].max())
    dth = float((ref.theta.reshape(bt, K, -1) - got.theta).abs().amax(dim=-1)[both].max())
    same_conv = bool(torch.equal(ref.converged.reshape(bt, K), got.converged))
    assert torch.equal(torch.nan_to_num(slim.worst_loading), torch.nan_to_num(got.worst_loading))
    lib, need = load_library(), ctypes.c_size_t()
    cfg = PfConfig(case, E, g.size, 10, 1e-8)
    lib.gns_acn1_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, bt, K, ctypes.byref(need))
    ws_s = need.value
    plan = powerflow._plan_mixed(xb, xl, xg, slack)
    xcfg = PfConfig(case, E - 1, g.size, 10, 1e-8)
    lib.gns_pf_workspace_bytes_set(ctypes.byref(xcfg), plan.topo_set.host.ctypes.data, plan.topo_set.host.size,
                                   plan.member_off.ctypes.data, plan.member_off.size, bt * K, ctypes.byref(need))
    ws_x = need.value
    it_w = got.iterations[got.converged].double().mean()
    it_xw = ref.iterations[ref.converged].double().mean()
    it_xf = flat.iterations[flat.converged].double().mean()
    print(f"  expanded newton_raphson(mixed_topologies=True, warm start), {bt * K} grids on {K} topologies, caches warm: {show(ms_x)}", flush=True)
    print(f"  ac_contingency_screen, states and flows ({8 * bt * K * (2 * case + 4 * E) / 1e6:.1f} MB written): {show(ms_s)}", flush=True)
    print(f"  ac_contingency_screen states=False flows=False (summaries alone): {show(ms_slim)}", flush=True)
    print(f"  newton_raphson on the {bt} base grids (part of each screen call): {show(ms_base)}", flush=True)
    print(f"  first call (cold caches, wall clock): expanded {cold_x:.1f} ms ({K} analyses), screen {cold_s:.1f} ms (the base analysis "
          f"already made by the base solve)", flush=True)
    print(f"  workspace: expanded {ws_x / 1e6:.2f} MB, screen {ws_s / 1e6:.2f} MB; inputs: expanded {nbytes(xb, xl, xg, xv, xth) / 1e6:.2f} MB "
          f"(+ {plan.topo_set.host.nbytes / 1e6:.2f} MB of blobs), screen {nbytes(bu, li, ge) / 1e6:.2f} MB (+ {topo.host.nbytes / 1e6:.3f} MB blob)",
          flush=True)
    print(f"  converged pairs: expanded {int(ref.converged.sum())}, screen {int(got.converged.sum())} of {bt * K} (same set: {same_conv}); "
          f"mean iterations of converged pairs: screen {float(it_w):.2f}, expanded warm {float(it_xw):.2f}, expanded flat start "
          f"{float(it_xf):.2f} ({int(flat.converged.sum())} converged)", flush=True)
    print(f"  expanded / screen: {ms_x.mean() / ms_s.mean():.2f}x with states and flows, {ms_x.mean() / ms_slim.mean():.2f}x summaries alone; "
          f"max |dv| {dv:.2e}, max |dtheta| {dth:.2e} on the pairs both routes converge on", flush=True)
    if case == 118 and ms_s.mean() > ms_x.mean():
        failed.append(f'case118: the screen ({ms_s.mean():.3f} ms) is slower than the expanded route ({ms_x.mean():.3f} ms)')
    if max(dv, dth) > 1e-9:
        failed.append(f'case{case}: the routes differ by {max(dv, dth):.2e} > 1e-9')
for msg in failed:
    print('FAILED: ' + msg, flush=True)
sys.exit(1 if failed else 0)
