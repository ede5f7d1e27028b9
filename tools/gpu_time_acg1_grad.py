"""Forward + backward of the differentiable AC generator screen against the route it replaces, on the same (grid, row) rows:
``ac_generator_contingency_screen_differentiable`` with ``flows=False, states=False, pickup='pmax'`` and the loss
``worst_loading[converged].sum()`` on Bt grids and a row list (every generator alone, plus a sample of generator-plus-line rows: the
lists and shapes of tools/gpu_time_acg1.py), and ``newton_raphson(mixed_topologies=True)`` with requires_grad on the expanded,
redispatched batch (each grid once per non-islanding row of the list, with the generator's row removed, the pickup added to the
others' Pg in float64 inside the graph and rounded to the inputs' float32, and the line's row removed, warm-started from the base
solution, every analysis cached: two calls, E and E - 1 lines), autograd summing over the copies.  That route returns ``v`` and
``theta`` alone, so its loss weighs those on the rows both routes converge on: the cheapest loss it can have.  The screen is timed
with that loss too (``states=True``).  The two routes' gradients of that loss are compared against the project's gradient bar (1e-5
max|ref| + 1e-7 per column per grid, column 1 of the generators included: 'pmax'), untimed: on every row both routes converge on and
on those both converge on with two iterations to spare (the rows the tests compare).  Those two figures are reported, not judged:
the expanded route rounds the redispatched Pg to its float32 inputs, which alone moves the float64 reference gradient by up to 1.1
of the bar on a case14 grid (more on a row that needs nine or ten iterations, close to the end of its solutions).  What decides the
exit status is the same comparison with ``pickup=None``, where nothing is redispatched and both routes solve the same inputs.
Each figure is one forward + backward between HIP events, after the caches are warm: the median of 5 repeats after 2 warm-ups, each
repeat timed on its own, with the spread.  Also: the screen's forward alone with and without gradients (the backward's share is
what is left), the adjoint's workspace and the rows per wave.
usage: python tools/gpu_time_acg1_grad.py [--no-expanded] [case:batch:rows_with_a_line ...] > profiles/acg1_grad/gpu_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth

CONTRACT = ((2, 3, 4, 5), (2, 3, 4, 5, 6), (1, 4, 6))
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
    """``ge`` [Bt,Gn,7] (on the graph) without row g, its Pg shared among the others in proportion to their column 1 (float64,
    rounded to float32)."""
    keep = [h for h in range(ge.shape[1]) if h != g]
    rest = ge[:, keep]
    w = rest[:, :, 1].double()
    W = w.sum(dim=1, keepdim=True)
    share = ge[:, g:g + 1, 6].double() * (w / W)
    pg = torch.where(W > 0, rest[:, :, 6].double() + share, rest[:, :, 6].double()).float()
    return torch.cat([rest[:, :, :6], pg.unsqueeze(2)], dim=2)


failed = []
args = sys.argv[1:]
with_expanded = '--no-expanded' not in args
specs = [a for a in args if not a.startswith('--')] or ['14:512:64', '118:64:256', '300:8:128']
for spec in specs:
    case, bt, n_line_rows = map(int, spec.split(':'))
    bu, li, ge, slack, _, _ = synth.solvable_grids(case, bt, seed=1, device='cuda')
    f, t, g = synth.case_topology(case)
    E, Gn = f.size, g.size
    every = powerflow._generator_contingency_list(None, Gn, E)
    with_line = every[every[:, 1] >= 0]
    rng = np.random.default_rng(case)
    pick = np.sort(rng.choice(with_line.shape[0], min(n_line_rows, with_line.shape[0]), replace=False))
    rows = np.concatenate([every[every[:, 1] < 0], with_line[pick]])
    P = rows.shape[0]
    isl = powerflow._generator_islanding(powerflow._bridges(case, f - 1, t - 1), rows)
    C = max(1, -(-P // 64))
    chunks = -(-P // C)
    partial = 4 * case + 5 * E + 4 * Gn + 1
    print(f"case{case} x {bt} grids x {P} rows ({Gn} generators alone, {P - Gn} with a line, {int(isl.sum())} islanding) = {bt * P} rows; "
          f"adjoint: {chunks} chunks per grid of up to {C} rows, partials {bt * chunks * 8 * partial / 1e6:.2f} MB", flush=True)
    kw = dict(slack_bus=slack, contingencies=rows, pickup='pmax', tol=TOL, max_iter=MAX_IT)

    def inputs():
        return [x.detach().clone().requires_grad_(True) for x in (bu, li, ge)]

    def summaries():
        ins = inputs()
        r = powerflow.ac_generator_contingency_screen_differentiable(*ins, flows=False, states=False, **kw)
        return torch.autograd.grad(r.worst_loading[r.converged].sum(), ins)

    plain = powerflow.ac_generator_contingency_screen(bu, li, ge, flows=False, states=False, **kw)
    ms_sum, _ = event_ms(summaries)
    ms_plain, _ = event_ms(lambda: powerflow.ac_generator_contingency_screen(bu, li, ge, flows=False, states=False, **kw))
    ms_fwd, _ = event_ms(lambda: powerflow.ac_generator_contingency_screen_differentiable(*inputs(), flows=False, states=False, **kw))
    live = np.flatnonzero(~isl)
    live_t = torch.from_numpy(live).cuda()
    S = live.size
    n_conv = int(plain.converged.sum())
    back = np.median(ms_sum) - np.median(ms_fwd)
    print(f"  ac_generator_contingency_screen_differentiable flows=False states=False pickup='pmax', forward + backward of "
          f"worst_loading[converged].sum() ({n_conv} of {bt * S} non-islanding rows): {show(ms_sum)}", flush=True)
    print(f"  the screen's forward alone (flows=False, states=False): {show(ms_plain)} without gradients, {show(ms_fwd)} with (the base "
          f"solve on the graph; v and theta kept for the backward, {16 * bt * P * case / 1e6:.1f} MB); the backward is the rest: "
          f"{back:.3f} ms, {100 * back / np.median(ms_sum):.0f}% of forward + backward", flush=True)
    if not with_expanded:
        continue
    gen = torch.Generator().manual_seed(case)
    wv, wth = (torch.randn(bt, S, case, generator=gen, dtype=torch.float64).cuda() for _ in range(2))
    groups = []
    for has_line in (False, True):
        sel = [q for q, p in enumerate(live) if (rows[p, 1] >= 0) == has_line]
        if not sel:
            continue
        keep = torch.tensor(np.array([np.delete(np.arange(E), rows[live[q], 1]) for q in sel]), device='cuda') if has_line else None
        n = len(sel)
        v0 = plain.base.v.repeat_interleave(n, dim=0).contiguous()
        th0 = plain.base.theta.repeat_interleave(n, dim=0).contiguous()
        groups.append((sel, keep, v0, th0))

    def expanded_forward(ins, share=True):
        """v, theta, converged, iterations as [Bt,S,...] in the order of the live rows; ``share`` False: the slack picks up."""
        without = {}
        v, th, conv, its = [None] * S, [None] * S, [None] * S, [None] * S
        for sel, keep, v0, th0 in groups:
            n = len(sel)
            for q in sel:
                h = int(rows[live[q], 0])
                if h not in without:
                    without[h] = redispatched(ins[2], h) if share else ins[2][:, [x for x in range(Gn) if x != h]]
            xg = torch.stack([without[int(rows[live[q], 0])] for q in sel], dim=1).reshape(bt * n, Gn - 1, 7)
            xl = ins[1].repeat_interleave(n, dim=0) if keep is None else ins[1][:, keep].reshape(bt * n, E - 1, 7)
            r = powerflow.newton_raphson(ins[0].repeat_interleave(n, dim=0), xl, xg, slack_bus=slack, mixed_topologies=True, v0=v0,
                                         theta0=th0, tol=TOL, max_iter=MAX_IT)
            rv, rth = r.v.reshape(bt, n, -1), r.theta.reshape(bt, n, -1)
            rc, ri = r.converged.reshape(bt, n), r.iterations.reshape(bt, n)
            for j, q in enumerate(sel):
                v[q], th[q], conv[q], its[q] = rv[:, j], rth[:, j], rc[:, j], ri[:, j]
        return torch.stack(v, dim=1), torch.stack(th, dim=1), torch.stack(conv, dim=1), torch.stack(its, dim=1)

    def masks(screened, share):
        """(the rows both routes converge on, those of them both converge on with two iterations to spare) [Bt,S]"""
        first = expanded_forward(inputs(), share)
        both = screened.converged[:, live_t] & first[2]
        return both, both & (screened.iterations[:, live_t] <= MAX_IT - 2) & (first[3] <= MAX_IT - 2)

    used, spare = masks(plain, True)

    def expanded(mask=None, share=True):
        mask = used if mask is None else mask
        ins = inputs()
        v, th, _, _ = expanded_forward(ins, share)
        return torch.autograd.grad((wv[mask] * v[mask]).sum() + (wth[mask] * th[mask]).sum(), ins)

    def states(mask=None, share=True):
        mask = used if mask is None else mask
        ins = inputs()
        r = powerflow.ac_generator_contingency_screen_differentiable(*ins, flows=False, states=True, **dict(kw, pickup='pmax' if share else None))
        return torch.autograd.grad((wv[mask] * r.v[:, live_t][mask]).sum() + (wth[mask] * r.theta[:, live_t][mask]).sum(), ins)

    def difference(got, want):
        """(the largest difference over the bar, where: input, column, grid)"""
        worst = (0.0, None)
        for name, a, b, cols in zip(('buses', 'lines', 'generators'), got, want, CONTRACT):
            for c in cols:
                err = (a[..., c].double() - b[..., c].double()).abs().amax(dim=1)
                ratio = err / (1e-5 * b[..., c].double().abs().amax(dim=1) + 1e-7)
                worst = max(worst, (float(ratio.max()), (name, c, int(ratio.argmax()))))
        return worst

    ms_exp, want = event_ms(expanded)
    ms_states, got = event_ms(states)
    every, every_at = difference(got, want)
    shared, shared_at = difference(states(spare), expanded(spare))
    _, spare_none = masks(powerflow.ac_generator_contingency_screen(bu, li, ge, flows=False, states=False, **dict(kw, pickup=None)), False)
    worst, worst_at = difference(states(spare_none, False), expanded(spare_none, False))
    print(f"  expanded, redispatched newton_raphson(mixed_topologies=True) forward + backward, {bt * S} grids on {S} topologies in "
          f"{len(groups)} calls, loss on v and theta of {int(used.sum())} rows: {show(ms_exp)}", flush=True)
    print(f"  the screen with states=True, forward + backward of the same loss: {show(ms_states)}", flush=True)
    print(f"  expanded / screen: {np.median(ms_exp) / np.median(ms_sum):.2f}x against the summaries' loss, "
          f"{np.median(ms_exp) / np.median(ms_states):.2f}x on the same loss", flush=True)
    print(f"  largest gradient difference between the routes, pickup='pmax' (the expanded route's Pg is float32 after the redispatch): "
          f"{every:.3f} of the bar on the {int(used.sum())} rows both converge on, at {every_at}; {shared:.3f} of the bar on the "
          f"{int(spare.sum())} of them both converge on with two iterations to spare, at {shared_at}", flush=True)
    print(f"  the same with pickup=None (nothing is redispatched: both routes solve the same float32 inputs), {int(spare_none.sum())} rows "
          f"with two iterations to spare: {worst:.3f} of the bar, at {worst_at}", flush=True)
    if worst > 1.0:
        failed.append(f'case{case}: with pickup=None the routes\' gradients differ by {worst:.3f} of the bar on the rows with iterations to spare')
for msg in failed:
    print('FAILED: ' + msg, flush=True)
sys.exit(1 if failed else 0)
