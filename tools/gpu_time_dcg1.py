"""The DC generator contingency screen against the route it replaces.  ``dc_generator_contingency_screen`` with ``flows=False`` on Bt
grids and the default list (every generator alone and with every line) is timed as the whole Python call (host islanding,
``np.unique``, copies, both kernels and the base solve) between HIP events, with ``pickup='pmax'`` and, for comparison, with the
slack picking up; the two kernels together as one ``gns_dcg1_screen`` call on prebuilt device lists.  The other route is
``dc_power_flow`` on the expanded batch: each grid once per row with the outaged generator's Pg set to 0 and its shares added to the
others (in float32, as a caller of that route would), the rows with a line with that line row removed and
``mixed_topologies=True``, the rows without a line in a second, plain call.  It is timed after its caches are warm on a seeded sample
of at most ``sample`` non-islanding rows with a line and ``sample / 8`` rows without: the full expansion would not fit, and each of its
topologies is analysed on the host once.  Its time per (grid, row) is scaled to the whole list for the ratio, and said so.  5 repeats
after 2 warm-ups, each repeat timed on its own; the mean is quoted with min and max.  The two routes' worst loadings are compared
on the sample (the expanded route's redispatch is rounded to float32, so they agree to about 1e-6, not to the DC bar).
Exits non-zero if the screen's mean is above the expanded route's (scaled) at case118.
usage: python tools/gpu_time_dcg1.py [case:batch[:sample] ...] > profiles/dcg1/gpu_time.txt"""
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
    return f'{ms.mean():.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})'


def direct_call(bu, li, ge, fd, rows, isl_np, pickup):
    """One ``gns_dcg1_screen`` call (both kernels, summaries alone) on the rows ``rows``, every list built and copied beforehand."""
    lib = load_library()
    bt, N, E = bu.shape[0], bu.shape[1], li.shape[1]
    cfg = PfConfig(N, E, ge.shape[1], 0, 0.0)
    gen_np, gen_col = np.unique(rows[:, 0], return_inverse=True)
    k = rows[:, 1]
    line_np = np.unique(k[k >= 0])
    cols32 = np.ascontiguousarray(np.stack([gen_col, np.where(k >= 0, np.searchsorted(line_np, k), -1)], axis=1).astype(np.int32))
    line32, gen32 = line_np.astype(np.int32), gen_np.astype(np.int32)
    P = cols32.shape[0]
    line_dev, gen_dev, cols_dev = (torch.from_numpy(a).cuda() for a in (line32, gen32, cols32))
    isl = torch.from_numpy(isl_np.astype(np.uint8)).cuda()
    worst = torch.empty(bt, P, dtype=torch.float64, device='cuda')
    worst_line = torch.empty(bt, P, dtype=torch.int32, device='cuda')
    conv = torch.empty(bt, dtype=torch.uint8, device='cuda')
    nbytes = ctypes.c_size_t()
    powerflow._check(lib.gns_dcg1_workspace_bytes(ctypes.byref(cfg), fd.host.ctypes.data, bt, line32.size, gen32.size,
                                                  ctypes.byref(nbytes)), 'gns_dcg1_workspace_bytes')
    ws = gns_mod._workspace(nbytes.value, bu.device)

    def call():
        stream = torch.cuda.current_stream().cuda_stream
        powerflow._check(lib.gns_dcg1_screen(ctypes.byref(cfg), fd.host.ctypes.data, fd.blob.data_ptr(), bu.data_ptr(), li.data_ptr(),
                                             ge.data_ptr(), bt, line32.ctypes.data, line_dev.data_ptr(), line32.size,
                                             gen32.ctypes.data, gen_dev.data_ptr(), gen32.size, cols32.ctypes.data,
                                             cols_dev.data_ptr(), P, isl.data_ptr(), None, 0, pickup.data_ptr(), 1, None,
                                             worst.data_ptr(), worst_line.data_ptr(), conv.data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream), 'gns_dcg1_screen')
        return worst
    return call


def redispatched(ge, rows, pickup):
    """[Bt * S, Gn, 7] float32: grid i once per row of ``rows``, with the row's generator out and its Pg shared by ``pickup``
    [Bt, Gn]."""
    bt, Gn = ge.shape[0], ge.shape[1]
    S = rows.shape[0]
    g = torch.from_numpy(rows[:, 0]).cuda()
    x = ge.unsqueeze(1).repeat(1, S, 1, 1)                                       # [Bt, S, Gn, 7]
    out = torch.zeros(S, Gn, dtype=torch.bool, device='cuda')
    out[torch.arange(S, device='cuda'), g] = True
    pg = x[:, :, :, 6].double()
    lost = (pg * out).sum(dim=2, keepdim=True)                                   # [Bt, S, 1]
    w = pickup.unsqueeze(1) * ~out                                               # [Bt, S, Gn]
    total = w.sum(dim=2, keepdim=True)
    share = torch.where(total > 0, lost * w / total.clamp(min=1e-300), torch.zeros_like(w))
    x[:, :, :, 6] = (torch.where(out, torch.zeros_like(pg), pg) + share).float()
    return x.reshape(bt * S, Gn, 7).contiguous()


failed = False
specs = sys.argv[1:] or ['14:512', '118:64', '300:8']
for spec in specs:
    case, bt, sample = (list(map(int, spec.split(':'))) + [1000])[:3]
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E, Gn = f.size, g.size
    fd = powerflow.analyse_fd_topology(case, f, t, g, slack, device=bu.device)
    lds, lanes = powerflow._dcn1_lds_bytes(fd.host)
    rows = powerflow._generator_contingency_list(None, Gn, E)
    P = rows.shape[0]
    isl = powerflow._generator_islanding(powerflow._bridges(case, f - 1, t - 1), rows)
    pmax = ge[:, :, 1].double().contiguous()
    n_cand = E + Gn
    print(f"case{case} x {bt} grids x {P} rows ({Gn} generators x (1 + {E} lines), {int(isl.sum())} islanding) = {bt * P} rows: B' dim "
          f"{fd.info['dim_p']} nnz(L+U) {fd.info['nnz_lu_p']}; factor kernel LDS {lds} B with W = {lanes} candidates per workgroup "
          f"({-(-n_cand // lanes)} workgroups per grid), row kernel LDS {24 * E} B; the workspace rows are {8 * n_cand * E / 1e3:.0f} KB "
          f"per grid, {8 * bt * n_cand * E / 1e6:.1f} MB in all", flush=True)
    ms_screen, res = event_ms(lambda: powerflow.dc_generator_contingency_screen(bu, li, ge, slack_bus=slack, pickup='pmax'))
    ms_slack, _ = event_ms(lambda: powerflow.dc_generator_contingency_screen(bu, li, ge, slack_bus=slack))
    ms_both, both = event_ms(direct_call(bu, li, ge, fd, rows, isl, pmax))
    ms_base, _ = event_ms(lambda: powerflow.dc_power_flow(bu, li, ge, slack_bus=slack))
    assert bool(res.converged.all()) and int(res.islanding.sum()) == int(isl.sum())
    assert torch.equal(torch.nan_to_num(both), torch.nan_to_num(res.worst_loading))
    print(f"  dc_generator_contingency_screen flows=False pickup='pmax', the whole Python call ({12 * bt * P / 1e6:.2f} MB of summaries "
          f"written): {show(ms_screen)}", flush=True)
    print(f"  the same with the slack picking up (pickup=None): {show(ms_slack)}", flush=True)
    print(f"  both kernels, one gns_dcg1_screen call on prebuilt lists: {show(ms_both)}", flush=True)
    print(f"  dc_power_flow on the {bt} base grids (part of each Python call): {show(ms_base)}", flush=True)
    # the expanded batch of the other route on a sample: row (i, p) is grid i redispatched, without the row's line
    rng = np.random.default_rng(case)
    live = np.flatnonzero(~isl & (rows[:, 1] >= 0))
    alone = np.flatnonzero(rows[:, 1] < 0)
    pick = live if live.size <= sample else np.sort(rng.choice(live, sample, replace=False))
    pick_a = alone if alone.size <= max(1, sample // 8) else np.sort(rng.choice(alone, max(1, sample // 8), replace=False))
    S, Sa = pick.size, pick_a.size
    keep = torch.tensor(np.array([np.delete(np.arange(E), rows[p, 1]) for p in pick]), device='cuda')            # [S, E-1]
    xl = li[:, keep].reshape(bt * S, E - 1, 7).contiguous()
    xb = bu.repeat_interleave(S, dim=0).contiguous()
    xg = redispatched(ge, rows[pick], pmax)
    ms_mixed, ref = event_ms(lambda: powerflow.dc_power_flow(xb, xl, xg, slack_bus=slack, mixed_topologies=True))
    ab, al, ag = bu.repeat_interleave(Sa, dim=0).contiguous(), li.repeat_interleave(Sa, dim=0).contiguous(), redispatched(ge, rows[pick_a], pmax)
    ms_plain, ref_a = event_ms(lambda: powerflow.dc_power_flow(ab, al, ag, slack_bus=slack))
    assert bool(ref.converged.all()) and bool(ref_a.converged.all())
    err = 0.0
    for want, at in ((ref.line_flow.reshape(bt, S, E - 1).abs().amax(dim=2), pick), (ref_a.line_flow.reshape(bt, Sa, E).abs().amax(dim=2), pick_a)):
        got = res.worst_loading[:, torch.from_numpy(at).cuda()]
        err = max(err, float(((got - want).abs() / want.clamp(min=1.0)).max()))
    scaled = ms_mixed.mean() * live.size / S + ms_plain.mean() * alone.size / Sa
    print(f"  expanded dc_power_flow(mixed_topologies=True), {bt * S} grids on {np.unique(rows[pick, 1]).size} topologies (a sample of the "
          f"{live.size} non-islanding rows with a line), caches warm: {show(ms_mixed)}; dc_power_flow on {bt * Sa} grids (a sample of the "
          f"{alone.size} rows without a line): {show(ms_plain)}; scaled to the list: {scaled:.1f} ms", flush=True)
    ratio = scaled / ms_screen.mean()
    print(f"  expanded (scaled) / screen: {ratio:.1f}x; worst scaled difference of the two routes' worst loadings on the sample "
          f"{err:.2e} (the expanded route's redispatch is rounded to float32)", flush=True)
    if case == 118 and ms_screen.mean() > scaled:
        failed = True
        print('  FAILED: the screen is slower than the expanded route at case118', flush=True)
sys.exit(1 if failed else 0)
