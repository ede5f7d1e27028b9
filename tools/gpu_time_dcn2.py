"""The DC N-2 contingency screen against the route it replaces.  ``dc_n2_contingency_screen`` with ``flows=False`` on Bt grids and a
pair list is timed as the whole Python call (host islanding, ``np.unique``, copies, both kernels and the base solve); the two kernels
together as one ``gns_dcn2_screen`` call on prebuilt device lists; the factor kernel alone as the same call on the same candidate
lines with a single pair (one row per grid for the pair kernel); the pair kernel as the difference of those two direct calls, both
between HIP events with no host work in them.  The other route is ``dc_power_flow(mixed_topologies=True)`` on the expanded batch
(each grid once per pair, with both line rows removed), timed after its caches are warm, on a seeded sample of at most ``sample``
non-islanding pairs of the list: the full expansion would not fit, and each of its topologies is analysed on the host once.  Its time
per (grid, pair) is scaled to the whole list for the ratio, and said so.  5 repeats after 2 warm-ups, each repeat timed on its own;
the median is quoted with the spread.  The two routes' worst loadings are compared on the sample.
usage: python tools/gpu_time_dcn2.py [case:batch:pairs[:sample] ...] > profiles/dcn2/gpu_time.txt     (pairs 0: every pair)"""
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


def direct_call(bu, li, ge, fd, cand, cols, isl_np):
    """One ``gns_dcn2_screen`` call (both kernels, summaries alone) on the candidate lines ``cand`` and the pairs ``cols`` (positions
    into ``cand``), every list built and copied beforehand."""
    lib = load_library()
    bt, N, E = bu.shape[0], bu.shape[1], li.shape[1]
    cfg = PfConfig(N, E, ge.shape[1], 0, 0.0)
    cand32 = cand.astype(np.int32)
    cols32 = np.ascontiguousarray(cols.astype(np.int32).reshape(-1, 2))
    P = cols32.shape[0]
    cand_dev, cols_dev = torch.from_numpy(cand32).cuda(), torch.from_numpy(cols32).cuda()
    isl = torch.from_numpy(isl_np.astype(np.uint8)).cuda()
    worst = torch.empty(bt, P, dtype=torch.float64, device='cuda')
    worst_line = torch.empty(bt, P, dtype=torch.int32, device='cuda')
    conv = torch.empty(bt, dtype=torch.uint8, device='cuda')
    nbytes = ctypes.c_size_t()
    powerflow._check(lib.gns_dcn2_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, bt, cand32.size, ctypes.byref(nbytes)),
                     'gns_dcn2_workspace_bytes')
    ws = gns_mod._workspace(nbytes.value, bu.device)

    def call():
        stream = torch.cuda.current_stream().cuda_stream
        powerflow._check(lib.gns_dcn2_screen(ctypes.byref(cfg), fd.host.ctypes.data, fd.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                             ge.data_ptr(), bt, cand32.ctypes.data, cand_dev.data_ptr(), cand32.size,
                                             cols32.ctypes.data, cols_dev.data_ptr(), P, isl.data_ptr(), None, 0, None,
                                             worst.data_ptr(), worst_line.data_ptr(), conv.data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream), 'gns_dcn2_screen')
        return worst
    return call


specs = sys.argv[1:] or ['14:512:0', '118:64:0', '300:8:20000']
for spec in specs:
    case, bt, n_pairs, sample = (list(map(int, spec.split(':'))) + [2000])[:4]
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E = f.size
    fd = powerflow.analyse_fd_topology(case, f, t, g, slack, device=bu.device)
    lds, lanes = powerflow._dcn1_lds_bytes(fd.host)
    every = powerflow._pair_list(None, E)
    rng = np.random.default_rng(case)
    pairs = every if n_pairs <= 0 or n_pairs >= every.shape[0] else every[np.sort(rng.choice(every.shape[0], n_pairs, replace=False))]
    P = pairs.shape[0]
    isl = powerflow._pair_islanding(case, f - 1, t - 1, pairs)
    cand, cols = np.unique(pairs, return_inverse=True)
    cols = cols.reshape(P, 2)
    print(f"case{case} x {bt} grids x {P} pairs ({int(isl.sum())} islanding) of {E} lines = {bt * P} rows: B' dim {fd.info['dim_p']} "
          f"nnz(L+U) {fd.info['nnz_lu_p']}; factor kernel LDS {lds} B with W = {lanes} lines per workgroup "
          f"({-(-cand.size // lanes)} workgroups per grid), pair kernel LDS {24 * E} B; H is {8 * cand.size * E / 1e3:.0f} KB per grid, "
          f"{8 * bt * cand.size * E / 1e6:.1f} MB in all", flush=True)
    ms_screen, res = event_ms(lambda: powerflow.dc_n2_contingency_screen(bu, li, ge, slack_bus=slack, pairs=pairs))
    ms_both, both = event_ms(direct_call(bu, li, ge, fd, cand, cols, isl))
    ms_factor, _ = event_ms(direct_call(bu, li, ge, fd, cand, np.array([[0, 1]]), np.zeros(1, dtype=bool)))
    ms_base, _ = event_ms(lambda: powerflow.dc_power_flow(bu, li, ge, slack_bus=slack))
    assert bool(res.converged.all()) and int(res.islanding.sum()) == int(isl.sum())
    assert torch.equal(torch.nan_to_num(both), torch.nan_to_num(res.worst_loading))
    print(f"  dc_n2_contingency_screen flows=False, the whole Python call ({12 * bt * P / 1e6:.2f} MB of summaries written): "
          f"{show(ms_screen)}", flush=True)
    print(f"  both kernels, one gns_dcn2_screen call on prebuilt lists: {show(ms_both)}", flush=True)
    print(f"  the factor kernel alone ({cand.size} solves per grid and H stored; with a one-pair pair kernel): {show(ms_factor)}", flush=True)
    print(f"  the pair kernel, both kernels less the factor kernel: {np.median(ms_both) - np.median(ms_factor):.3f} ms", flush=True)
    print(f"  dc_power_flow on the {bt} base grids (part of each Python call): {show(ms_base)}", flush=True)
    # the expanded batch of the other route on a sample: pair (i, p) is grid i without the two lines of pair p
    live = np.flatnonzero(~isl)
    pick = live if live.size <= sample else np.sort(rng.choice(live, sample, replace=False))
    S = pick.size
    keep = torch.tensor(np.array([np.delete(np.arange(E), pairs[p]) for p in pick]), device='cuda')          # [S, E-2]
    xl = li[:, keep].reshape(bt * S, E - 2, 7).contiguous()
    xb = bu.repeat_interleave(S, dim=0).contiguous()
    xg = ge.repeat_interleave(S, dim=0).contiguous()
    ms_mixed, ref = event_ms(lambda: powerflow.dc_power_flow(xb, xl, xg, slack_bus=slack, mixed_topologies=True))
    assert bool(ref.converged.all())
    want = ref.line_flow.reshape(bt, S, E - 2).abs().amax(dim=2)
    got = res.worst_loading[:, torch.from_numpy(pick).cuda()]
    err = float(((got - want).abs() / want.clamp(min=1.0)).max())
    scaled = np.median(ms_mixed) * live.size / S
    print(f"  expanded dc_power_flow(mixed_topologies=True), {bt * S} grids on {S} topologies (a sample of the {live.size} non-islanding "
          f"pairs), caches warm: {show(ms_mixed)}; scaled to {live.size} pairs: {scaled:.1f} ms", flush=True)
    print(f"  expanded (scaled) / screen: {scaled / np.median(ms_screen):.1f}x; worst scaled difference of the two routes' worst "
          f"loadings on the sample {err:.2e}", flush=True)
