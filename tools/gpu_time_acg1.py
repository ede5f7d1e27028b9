"""The AC generator contingency screen against the route it replaces.  ``ac_generator_contingency_screen`` with ``flows=False,
states=False, pickup='pmax'`` on Bt grids and a row list (every generator alone, plus a sample of generator-plus-line rows) is timed
as the whole Python call (the list, copies, the base solve, the Y-bus kernel and the row kernel), after its caches are warm (one
analysis per generator, the set on the device).  The other route is ``newton_raphson(mixed_topologies=True)`` on the expanded,
redispatched batch (each grid once per non-islanding row of the list, with the generator's row removed, the pickup added to the
others' Pg in float64 and rounded to the inputs' float32, and the line's row removed), warm-started from the base solution: two
calls, one for the rows without a line (E lines) and one for the rows with one (E - 1 lines), timed together after their caches are
warm (every topology analysed, the set on the device).  5 repeats after 2 warm-ups, each repeat timed on its own; the median is
quoted with the spread.  The two routes' convergence flags and lowest voltages are compared on every row; the expanded route's Pg
is rounded to float32 after the redispatch, the screen's is not, so the flags of a few marginal rows may differ.
The host time of the screen's analyses (one per generator, ``analyse_topology(..., out_gen=g)``, uncached) is measured on its own.
usage: python tools/gpu_time_acg1.py [case:batch:rows_with_a_line ...] > profiles/acg1/gpu_time.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth

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


def redispatched(ge, g):
    """``ge`` [Bt,Gn,7] without row g, its Pg shared among the others in proportion to their column 1 (float64, rounded to float32)."""
    Gn = ge.shape[1]
    keep = [h for h in range(Gn) if h != g]
    w = ge[:, keep, 1].double()
    W = w.sum(dim=1, keepdim=True)
    out = ge[:, keep].clone()
    share = ge[:, g:g + 1, 6].double() * (w / W)
    out[:, :, 6] = torch.where(W > 0, out[:, :, 6].double() + share, out[:, :, 6].double()).float()
    return out


specs = sys.argv[1:] or ['14:512:64', '118:64:256', '300:8:128']
for spec in specs:
    case, bt, n_line_rows = map(int, spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E, Gn = f.size, g.size
    topo = powerflow.analyse_topology(case, f, t, g, slack, device=bu.device)
    every = powerflow._generator_contingency_list(None, Gn, E)
    with_line = every[every[:, 1] >= 0]
    rng = np.random.default_rng(case)
    pick = np.sort(rng.choice(with_line.shape[0], min(n_line_rows, with_line.shape[0]), replace=False))
    rows = np.concatenate([every[every[:, 1] < 0], with_line[pick]])
    P = rows.shape[0]
    isl = powerflow._generator_islanding(powerflow._bridges(case, f - 1, t - 1), rows)
    if case in (118, 300):
        t0 = time.perf_counter()
        members = [powerflow.analyse_topology(case, f, t, g, slack, out_gen=h) for h in range(Gn)]
        host_s = time.perf_counter() - t0
        dims = [m.info['dim'] for m in members]
        print(f"case{case}: the {Gn} host analyses without one generator each (uncached): {host_s:.2f} s, {1e3 * host_s / Gn:.1f} ms each; "
              f"dim {min(dims)} .. {max(dims)} (base {topo.info['dim']}), largest LDS image {max(m.info['lds_bytes'] for m in members)} B, "
              f"{sum(m.host.nbytes for m in members) / 2 ** 20:.1f} MiB of blobs", flush=True)
    print(f"case{case} x {bt} grids x {P} rows ({Gn} generators alone, {P - Gn} with a line, {int(isl.sum())} islanding) = {bt * P} rows: "
          f"base dim {topo.info['dim']} nnz(L+U) {topo.info['nnz_lu']}, LDS {topo.info['lds_bytes']} B per wave", flush=True)

    def screen():
        return powerflow.ac_generator_contingency_screen(bu, li, ge, slack_bus=slack, contingencies=rows, pickup='pmax', tol=TOL,
                                                         max_iter=MAX_IT, flows=False, states=False)

    ms_screen, res = event_ms(screen)
    base = res.base
    ms_base, _ = event_ms(lambda: powerflow.newton_raphson(bu, li, ge, slack_bus=slack, tol=TOL, max_iter=MAX_IT))
    live = np.flatnonzero(~isl)
    live_t = torch.from_numpy(live).cuda()
    solved = res.converged[:, live_t]
    print(f"  ac_generator_contingency_screen flows=False states=False pickup='pmax', the whole Python call ({int(base.converged.sum())} of "
          f"{bt} base grids converged; {int(solved.sum())} of {solved.numel()} non-islanding rows converged, mean iterations "
          f"{float(res.iterations[res.converged].float().mean()):.2f}): {show(ms_screen)}", flush=True)
    print(f"  newton_raphson on the {bt} base grids (part of each Python call): {show(ms_base)}", flush=True)
    # the expanded, redispatched batch of the other route, in the order of the live rows: [Bt, S] grids
    gens_without = {h: redispatched(ge, h) for h in range(Gn)}
    groups = []
    for has_line in (False, True):
        sel = [p for p in live if (rows[p, 1] >= 0) == has_line]
        if not sel:
            continue
        S = len(sel)
        xg = torch.stack([gens_without[int(rows[p, 0])] for p in sel], dim=1).reshape(bt * S, Gn - 1, 7).contiguous()
        if has_line:
            keep = torch.tensor(np.array([np.delete(np.arange(E), rows[p, 1]) for p in sel]), device='cuda')      # [S, E-1]
            xl = li[:, keep].reshape(bt * S, E - 1, 7).contiguous()
        else:
            xl = li.repeat_interleave(S, dim=0).contiguous()
        xb = bu.repeat_interleave(S, dim=0).contiguous()
        v0, th0 = base.v.repeat_interleave(S, dim=0).contiguous(), base.theta.repeat_interleave(S, dim=0).contiguous()
        groups.append((sel, xb, xl, xg, v0, th0))

    def expanded():
        return [powerflow.newton_raphson(xb, xl, xg, slack_bus=slack, mixed_topologies=True, v0=v0, theta0=th0, tol=TOL, max_iter=MAX_IT)
                for _, xb, xl, xg, v0, th0 in groups]

    ms_mixed, refs = event_ms(expanded)
    n_flag = n_rows = 0
    err = 0.0
    for (sel, *_), ref in zip(groups, refs):
        S = len(sel)
        cols = torch.tensor(sel, device='cuda')
        conv, mine = ref.converged.reshape(bt, S), res.converged[:, cols]
        n_flag += int((conv != mine).sum())
        n_rows += conv.numel()
        both = conv & mine
        if bool(both.any()):
            err = max(err, float((ref.v.reshape(bt, S, -1).amin(dim=-1) - res.v_min[:, cols]).abs()[both].max()))
    print(f"  expanded newton_raphson(mixed_topologies=True), warm-started, {n_rows} grids on {len(live)} topologies in "
          f"{len(groups)} calls (every non-islanding row of the list), caches warm: {show(ms_mixed)}", flush=True)
    print(f"  expanded / screen: {np.median(ms_mixed) / np.median(ms_screen):.2f}x; rows whose converged flags differ between the routes: "
          f"{n_flag} of {n_rows}; worst difference of their lowest voltages on the rows both converge {err:.2e} (the expanded route's "
          f"Pg is float32 after the redispatch)", flush=True)
