"""The AC N-2 contingency screen against the route it replaces.  ``ac_n2_contingency_screen`` with ``flows=False, states=False`` on Bt
grids and a pair list is timed as the whole Python call (host islanding, copies, the base solve, the Y-bus kernel and the pair
kernel); the two kernels together as one ``gns_acn2_screen`` call on prebuilt device lists and a base solution solved beforehand,
between HIP events with no host work in them.  The other route is ``newton_raphson(mixed_topologies=True)`` on the expanded batch
(each grid once per non-islanding pair of the list, with both line rows removed), warm-started from the base solution, timed after
its caches are warm (every topology analysed, the set on the device).  5 repeats after 2 warm-ups, each repeat timed on its own; the
median is quoted with the spread.  The two routes' convergence flags and lowest voltages are compared on every row.
usage: python tools/gpu_time_acn2.py [case:batch:pairs ...] > profiles/acn2/gpu_time_acn2.txt     (pairs 0: every pair)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import gns as gns_mod
from opf_graph_neural_solver_amd import powerflow, synth
from opf_graph_neural_solver_amd._lib import PfConfig, load_library

TOL, MAX_IT = 1e-8, 10


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
    return f'{np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


def direct_call(bu, li, ge, topo, pairs, isl_np, base):
    """One ``gns_acn2_screen`` call (both kernels, summaries alone) on the pair list, every list built and copied beforehand."""
    lib = load_library()
    bt, N, E = bu.shape[0], bu.shape[1], li.shape[1]
    cfg = PfConfig(N, E, ge.shape[1], MAX_IT, TOL)
    pairs32 = np.ascontiguousarray(pairs.astype(np.int32))
    P = pairs32.shape[0]
    pairs_dev = torch.from_numpy(pairs32).cuda()
    isl = torch.from_numpy(isl_np.astype(np.uint8)).cuda()
    base_conv = base.converged.to(torch.uint8)
    f64 = [torch.empty(bt, P, dtype=torch.float64, device='cuda') for _ in range(4)]
    i32 = [torch.empty(bt, P, dtype=torch.int32, device='cuda') for _ in range(4)]
    conv = torch.empty(bt, P, dtype=torch.uint8, device='cuda')
    nbytes = ctypes.c_size_t()
    powerflow._check(lib.gns_acn2_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, bt, P, ctypes.byref(nbytes)),
                     'gns_acn2_workspace_bytes')
    ws = gns_mod._workspace(nbytes.value, bu.device)

    def call():
        stream = torch.cuda.current_stream().cuda_stream
        powerflow._check(lib.gns_acn2_screen(ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                             ge.data_ptr(), bt, pairs32.ctypes.data, pairs_dev.data_ptr(), P, isl.data_ptr(), None, 0,
                                             base.v.data_ptr(), base.theta.data_ptr(), base_conv.data_ptr(), None, None, None, None,
                                             None, None, f64[0].data_ptr(), i32[0].data_ptr(), f64[1].data_ptr(), i32[1].data_ptr(),
                                             f64[2].data_ptr(), i32[2].data_ptr(), conv.data_ptr(), i32[3].data_ptr(),
                                             f64[3].data_ptr(), ws.data_ptr(), ws.numel(), stream), 'gns_acn2_screen')
        return f64[0]
    return call


specs = sys.argv[1:] or ['14:512:0', '118:64:512', '300:8:256']
for spec in specs:
    case, bt, n_pairs = map(int, spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    topo = powerflow.analyse_topology(case, f, t, g, slack, device=bu.device)
    every = powerflow._pair_list(None, E)
    rng = np.random.default_rng(case)
    pairs = every if n_pairs <= 0 or n_pairs >= every.shape[0] else every[np.sort(rng.choice(every.shape[0], n_pairs, replace=False))]
    P = pairs.shape[0]
    isl = powerflow._pair_islanding(case, f - 1, t - 1, pairs)
    print(f"case{case} x {bt} grids x {P} pairs ({int(isl.sum())} islanding) of {E} lines = {bt * P} rows: dim {topo.info['dim']} "
          f"nnz(L+U) {topo.info['nnz_lu']}, LDS {topo.info['lds_bytes']} B per wave", flush=True)

    def screen(**kw):
        return powerflow.ac_n2_contingency_screen(bu, li, ge, slack_bus=slack, pairs=pairs, tol=TOL, max_iter=MAX_IT, **kw)

    ms_screen, res = event_ms(screen)
    base = res.base
    ms_both, both = event_ms(direct_call(bu, li, ge, topo, pairs, isl, base))
    ms_base, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, tol=TOL, max_iter=MAX_IT))
    assert int(res.islanding.sum()) == int(isl.sum())
    assert torch.equal(torch.nan_to_num(both), torch.nan_to_num(res.worst_loading))
    live = np.flatnonzero(~isl)
    solved = res.converged[:, torch.from_numpy(live).cuda()]
    print(f"  ac_n2_contingency_screen flows=False states=False, the whole Python call ({int(res.base.converged.sum())} of {bt} base "
          f"grids converged; {int(solved.sum())} of {solved.numel()} non-islanding rows converged, mean iterations "
          f"{float(res.iterations[res.converged].float().mean()):.2f}): {show(ms_screen)}", flush=True)
    print(f"  both kernels, one gns_acn2_screen call on prebuilt lists: {show(ms_both)}", flush=True)
    print(f"  newton_raphson on the {bt} base grids (part of each Python call): {show(ms_base)}", flush=True)
    # the expanded batch of the other route: row (i, p) is grid i without the two lines of the non-islanding pair p
    S = live.size
    keep = torch.tensor(np.array([np.delete(np.arange(E), pairs[p]) for p in live]), device='cuda')          # [S, E-2]
    xl = li[:, keep].reshape(bt * S, E - 2, 7).contiguous()
    xb = bu.repeat_interleave(S, dim=0).contiguous()
    xg = ge.repeat_interleave(S, dim=0).contiguous()
    v0, th0 = base.v.repeat_interleave(S, dim=0).contiguous(), base.theta.repeat_interleave(S, dim=0).contiguous()
    ms_mixed, ref = event_ms(lambda: powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=v0, theta0=th0,
                                                              tol=TOL, max_iter=MAX_IT))
    conv = ref.converged.reshape(bt, S)
    same = bool(torch.equal(conv, solved))
    err = float((ref.v.reshape(bt, S, -1).amin(dim=-1) - res.v_min[:, torch.from_numpy(live).cuda()]).abs()[conv & solved].max())
    print(f"  expanded newton_raphson(mixed_topologies=True), warm-started, {bt * S} grids on {S} topologies (every non-islanding pair of "
          f"the list), caches warm: {show(ms_mixed)}", flush=True)
    print(f"  expanded / screen: {np.median(ms_mixed) / np.median(ms_screen):.2f}x; the two routes' converged flags equal: {same}; worst "
          f"difference of their lowest voltages on the rows both converge {err:.2e}", flush=True)
