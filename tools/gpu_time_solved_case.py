"""``powerflow.solved_case`` against a float64 torch-op formulation of the same outputs on the same device (gather / ``index_add_``,
written here): the whole Python call between device events, warmed up, for the forward alone and for the forward + backward of
``worst_loading.sum() + gen_q.sum()`` with ``requires_grad`` on the three inputs and the state.  The two routes alternate in one
process, repeat by repeat; each figure is the median of the repeats with their spread.  Next to each time: the bytes the call must
move (the inputs and the state read once, every output written once; the Y-bus workspace the kernel also writes is listed apart)
over the HBM peak of MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured with a float4 copy), which gives the share of the byte
bound.  The two routes' outputs and gradients are compared, untimed.
usage: python tools/gpu_time_solved_case.py [case:batch ...] > profiles/solved_case/gpu_time.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from opf_graph_neural_solver_amd import powerflow, synth

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
REPS, WARM = 9, 3


def torch_solved_case(bu, li, ge, v, th, rating, ix):
    """The outputs of ``solved_case`` in float64 torch ops; ``ix``: the index tensors of the one topology (made once, untimed)."""
    bu, li, ge = bu.double(), li.double(), ge.double()
    ys = 1.0 / torch.complex(li[..., 2], li[..., 3])
    tap = torch.polar(li[..., 5], li[..., 6])
    ytt = ys + 0.5j * li[..., 4]
    yff = ytt / (tap * tap.conj())
    yft, ytf = -ys / tap.conj(), -ys / tap
    V = torch.polar(v, th)
    Vf, Vt = V[:, ix['f']], V[:, ix['t']]
    sf = Vf * (yff * Vf + yft * Vt).conj()
    st = Vt * (ytf * Vf + ytt * Vt).conj()
    S = torch.zeros_like(V).index_add_(1, ix['f'], sf).index_add_(1, ix['t'], st) + v * v * torch.complex(bu[..., 4], bu[..., 5]).conj()
    pg = torch.zeros_like(v).index_add_(1, ix['gb'], ge[..., 6])
    fp = (S.real - (pg - bu[..., 2]))[:, ix['pvpq']].abs()
    fq = (S.imag + bu[..., 3])[:, ix['pq']].abs()
    mismatch = torch.cat([fp, fq], dim=1).amax(dim=1)
    gen_q = (S.imag[:, ix['gb']] + bu[:, ix['gb'], 3]) / ix['count']
    ps = S.real[:, ix['slack']] + bu[:, ix['slack'], 2]
    on = ge[:, ix['on_slack'], 6]
    slack_p = ps - on.sum(dim=1)
    gen_p = ge[..., 6]
    if ix['on_slack'].numel():
        gen_p = gen_p.clone()
        gen_p[:, ix['on_slack'][0]] = ps - on[:, 1:].sum(dim=1)
    load = torch.maximum(sf.abs(), st.abs()) / rating
    worst, worst_line = load.max(dim=1)
    v_min, v_min_bus = v.min(dim=1)
    v_max, v_max_bus = v.max(dim=1)
    return powerflow.SolvedCase(sf.real, sf.imag, st.real, st.imag, S.real, S.imag, mismatch, gen_p, gen_q, slack_p, worst,
                                worst_line.int(), v_min, v_min_bus.int(), v_max, v_max_bus.int())


def alternate(fns, reps=REPS, warm=WARM):
    """The event times (ms) of each of ``fns``, one after the other, repeat by repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [np.array(m) for m in ms]


def show(ms):
    return f'{np.median(ms):.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}, spread {100 * (ms.max() - ms.min()) / np.median(ms):.0f}%)'


def bound(nbytes, ms):
    t = np.median(ms) * 1e-3
    return (f'{nbytes / 1e6:.1f} MB: {1e3 * nbytes / HBM_SPEC:.3f} ms at 8.0 TB/s, the byte bound is {100 * nbytes / HBM_SPEC / t:.1f}% of the '
            f'measured time ({100 * nbytes / HBM_COPY / t:.1f}% at the 6.29 TB/s a copy reaches)')


def main():
    short = []
    specs = [a for a in sys.argv[1:] if not a.startswith('--')] or ['14:16384', '118:16384', '300:2048']
    for spec in specs:
        case, bt = map(int, spec.split(':'))
        bu, li, ge, slack, v, th = synth.solvable_grids(case, bt, seed=1, device='cuda')
        v, th = v.double().contiguous(), th.double().contiguous()
        N, E, Gn = bu.shape[1], li.shape[1], ge.shape[1]
        gen = torch.Generator().manual_seed(case)
        rating = (0.5 + 2.0 * torch.rand(bt, E, generator=gen, dtype=torch.float64)).cuda()
        f, t, g = synth.case_topology(case)
        gb = torch.as_tensor(np.asarray(g, dtype=np.int64) - 1)
        has = torch.zeros(N, dtype=torch.bool)
        has[gb] = True
        role_pq = ~has
        role_pq[slack - 1] = False
        not_slack = torch.ones(N, dtype=torch.bool)
        not_slack[slack - 1] = False
        ix = dict(f=torch.as_tensor(np.asarray(f, dtype=np.int64) - 1).cuda(), t=torch.as_tensor(np.asarray(t, dtype=np.int64) - 1).cuda(),
                  gb=gb.cuda(), count=torch.bincount(gb, minlength=N)[gb].double().cuda(), slack=slack - 1,
                  on_slack=torch.nonzero(gb == slack - 1).flatten().cuda(), pvpq=torch.nonzero(not_slack).flatten().cuda(),
                  pq=torch.nonzero(role_pq).flatten().cuda())
        topo = powerflow.analyse_topology(N, f, t, g, slack)
        nnzy = topo.info['nnz_ybus']
        in_bytes = bt * (24 * N + 28 * E + 28 * Gn + 16 * N + 8 * E)
        out_bytes = bt * (32 * E + 16 * N + 16 * Gn + 5 * 8 + 3 * 4)
        # the backward reads the inputs, the state, the rating and the three indices again and the two incoming gradients the loss has
        # (worst_loading [Bt], gen_q [Bt,Gn]); it writes the five gradients
        bwd_bytes = in_bytes + bt * (12 + 8 + 8 * Gn) + bt * (16 * N + 24 * N + 28 * E + 28 * Gn)
        print(f'case{case} x {bt} grids (N {N}, E {E}, Gn {Gn}, nnz(Y) {nnzy}); Y-bus workspace written and read back by the forward: '
              f'{16 * nnzy * bt / 1e6:.1f} MB', flush=True)

        def ours_fwd():
            return powerflow.solved_case(bu, li, ge, v, th, slack_bus=slack, rating=rating)

        def torch_fwd():
            return torch_solved_case(bu, li, ge, v, th, rating, ix)

        ins = [x.detach().clone().requires_grad_(True) for x in (bu, li, ge, v, th)]     # leaves made once: autograd.grad accumulates nothing

        def grads(route):
            r = powerflow.solved_case(*ins, slack_bus=slack, rating=rating) if route == 'ours' else torch_solved_case(*ins, rating, ix)
            # (this loss does not reach the generators: the torch route then has no gradient for them, solved_case writes zeros)
            return torch.autograd.grad(r.worst_loading.sum() + r.gen_q.sum(), ins, allow_unused=True)

        # the two routes compute the same thing (untimed)
        a, b = ours_fwd(), torch_fwd()
        worst = max(float(((x - y).abs().max() / y.abs().max().clamp(min=1.0))) for x, y in zip(a, b) if x.dtype == torch.float64)
        same_idx = all(bool((x == y).all()) for x, y in zip(a, b) if x.dtype == torch.int32)
        ga, gb_ = grads('ours'), grads('torch')
        gworst = max(float(((x.double() - y.double()).abs().max() / y.double().abs().max().clamp(min=1e-30))) for x, y in zip(ga, gb_) if y is not None)
        print(f'  the routes agree: largest output difference {worst:.2e} of max(1, max|.|), indices equal: {same_idx}; largest gradient '
              f'difference {gworst:.2e} of max|.| (the inputs\' gradients are float32)', flush=True)
        del a, b, ga, gb_

        ms_o, ms_t = alternate([ours_fwd, torch_fwd])
        print(f'  forward, solved_case: {show(ms_o)}; must move {bound(in_bytes + out_bytes, ms_o)}', flush=True)
        print(f'  forward, torch ops:   {show(ms_t)}; torch / solved_case: {np.median(ms_t) / np.median(ms_o):.2f}x', flush=True)
        spread = max(ms_o.max() - ms_o.min(), ms_t.max() - ms_t.min())
        if np.median(ms_o) > np.median(ms_t) + spread:
            short.append(f'case{case} x {bt} forward: solved_case {np.median(ms_o):.3f} ms, torch ops {np.median(ms_t):.3f} ms')
        ms_o, ms_t = alternate([lambda: grads('ours'), lambda: grads('torch')])
        print(f'  forward + backward of worst_loading.sum() + gen_q.sum(), solved_case: {show(ms_o)}; must move '
              f'{bound(in_bytes + out_bytes + bwd_bytes, ms_o)}', flush=True)
        print(f'  forward + backward, torch ops: {show(ms_t)}; torch / solved_case: {np.median(ms_t) / np.median(ms_o):.2f}x', flush=True)
        spread = max(ms_o.max() - ms_o.min(), ms_t.max() - ms_t.min())
        if np.median(ms_o) > np.median(ms_t) + spread:
            short.append(f'case{case} x {bt} forward + backward: solved_case {np.median(ms_o):.3f} ms, torch ops {np.median(ms_t):.3f} ms')
    for msg in short:
        print('SHORT: slower than the torch-op formulation by more than the spread of the repeats: ' + msg, flush=True)
    print('every shape is no slower than the torch-op formulation, within the spread of the repeats' if not short else
          f'{len(short)} figure(s) fall short', flush=True)
    return 1 if short else 0


if __name__ == '__main__':
    sys.exit(main())
