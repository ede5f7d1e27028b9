#!/usr/bin/env python3
"""Benchmark of the GNS hot path on MI355X: grids/s for forward+backward on batched case118, K=4.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

N > 1 without a launcher: this process spawns the N ranks itself (``python -m torch.distributed.run``, one rank per GPU,
rendezvous on 127.0.0.1) BEFORE anything touches a GPU, waits for them and exits with their code; under
``torch.distributed.run`` (RANK / WORLD_SIZE in the environment) it is one of those ranks.

One "step" = one training step over a resident synthetic batch: fused forward, fused backward, ONE all-reduce of the
flat gradient (N>1), Adam step.  Inputs are generated on the device before the timed region by a counter-based
generator keyed by (seed, GLOBAL grid index): every GPU count sees the same grids.  Rank 0 prints one JSON line (see
DESIGN.md "Measurement" for every field).  At N=1 the line also carries the CPU baseline: the oracle (a torch-CPU
restatement of the reference's per-grid forward/backward), one single-threaded process per core, on a bounded sample
of the same workload - run BEFORE the GPU is initialised.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# BASELINE.json configs that fit one GPU (per-GPU batch).  --config 3 (default) is the one the metric is quoted on.
CONFIGS = {
    2: dict(case=30, batch=4096, K=4, name='configs[1]: case30, batch 4096, K=4 (correctness gate)'),
    3: dict(case=118, batch=16384, K=4, name='configs[2]: case118, batch 16384, K=4 (the metric; configs[3] = 8 x this)'),
    5: dict(case=300, batch=8192, K=10, name='configs[4]: case300, batch 65536 on 8 GPUs = 8192 per GPU, K=10, multiple_phi'),
}
SHAPES = {14: (14, 20, 5), 30: (30, 41, 6), 118: (118, 186, 54), 300: (300, 411, 69)}      # GNS/utils.py:45-56
D, H, GAMMA, MULTI = 20, 10, 0.9, True
CASE, BATCH_PER_GPU, K = 118, 16384, 4          # set from --config in main()
DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs: per-grid outputs beyond this are cut to a fixed, seeded sample of grids
DUMP_SAMPLE_SEED = 0
HBM_PEAK_GBS = 8000.0           # MI355X spec (MI355X_MICROARCH.md)
FP32_PEAK_TFLOPS = 157.3
DATA_SEED = 1234


def bytes_per_grid(case):
    """Compulsory bytes: every input element read once + every output written once: 10 504 for case118."""
    N, E, Gn = SHAPES[case]
    return 4 * (6 * N + 7 * E + 7 * Gn) + 4 * (2 * N + 2)


def mflop_fwd_per_grid(case, k):
    """Nominal MLP flops of one forward (MACs x 2), the reference's formulation, three phis: 4.19 for case118, K=4."""
    N, E, Gn = SHAPES[case]
    macs = k * (E * 3 * ((D + 5) * H + H * H + H * D) + N * (2 * ((4 + 2 * D) * H + H * H + H) + (4 + 2 * D) * H + H * H + H * D))
    return macs * 2 / 1e6


def _cpu_worker(args):
    """One single-threaded process: time the oracle's per-grid forward+backward (and forward only) for ~seconds."""
    seconds, seed, CASE, K = args
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, ROOT)
    from oracle import gns_oracle as orc
    import importlib.util
    spec = importlib.util.spec_from_file_location('synth_cpu', os.path.join(ROOT, 'opf-graph-neural-solver_amd', 'synth.py'))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    buses, lines, gens = synth.synth_grids(CASE, 8, seed=DATA_SEED, first_index=8 * seed)   # a slice of the benchmark's own data set
    flat = orc.flatten_params(orc.init_params(D, H, K, MULTI, seed=0))
    params = orc.unflatten_params(flat.clone().requires_grad_(True), D, H, K, MULTI)
    kw = dict(latent_dim=D, K=K, gamma=GAMMA, multiple_phi=MULTI)
    out = {}
    for mode in ('fwd', 'fwd_bwd'):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds * (0.3 if mode == 'fwd' else 0.7):
            i = n % 8
            if mode == 'fwd':
                with torch.no_grad():
                    orc.gns_forward(params, buses[i], lines[i], gens[i], **kw)
            else:
                _, _, tot, _ = orc.gns_forward(params, buses[i], lines[i], gens[i], **kw)
                tot.backward()
            n += 1
        out[mode] = (n, time.perf_counter() - t0)
    return out


def cpu_baseline(seconds=14.0, case=118, k=4):
    import multiprocessing as mp
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    # The GPU box's process guard allows 6 processes with the device open and `import torch` opens it: 5 workers + this one.
    cores = max(1, min(cores, 5))
    ctx = mp.get_context('spawn')     # fresh interpreters; the parent has not touched the GPU yet
    with ctx.Pool(cores) as pool:
        res = pool.map(_cpu_worker, [(seconds, i, case, k) for i in range(cores)])
    rate = {m: sum(r[m][0] / r[m][1] for r in res) for m in ('fwd', 'fwd_bwd')}
    grids = sum(r['fwd_bwd'][0] for r in res)
    return {'value': round(rate['fwd_bwd'], 1), 'unit': 'grids/s', 'cores': cores, 'kind': 'port',
            'forward_only_grids_per_s': round(rate['fwd'], 1),
            'sample': f'{grids} case{case} grids (K={k}, d=20, h=10, multiple_phi), one grid per call like GNS/main.py:279-288, '
                      f'{cores} single-threaded processes x ~{seconds:.0f} s, torch {__import__("torch").__version__} CPU'}


def dump_outputs(out_dir, outs):
    """Write what the last timed step computed as float32 .npy files: the per-grid outputs of the forward (v, theta,
    total_loss, last_loss: rank 0's grids) and the flat gradient and the parameters after the Adam step (state_dict order).
    Past DUMP_LIMIT_BYTES the per-grid outputs keep a fixed, seeded sample of grids, whose indices go to grid_index.npy."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in outs.items()}
    per_grid = ('v', 'theta', 'total_loss', 'last_loss')
    n = arrays['v'].shape[0]
    fixed = sum(a.nbytes for k, a in arrays.items() if k not in per_grid)
    row = sum(arrays[k].nbytes for k in per_grid) // max(n, 1) + 8
    keep = max(0, (DUMP_LIMIT_BYTES - 4096 - fixed) // row)         # 4096: room for the .npy headers
    if keep < n:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, size=keep, replace=False))
        for k in per_grid:
            arrays[k] = np.ascontiguousarray(arrays[k][idx])
        arrays['grid_index'] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + '.npy'), a)


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def self_launch(argv, gpus):
    """--gpus N without a launcher: run the N ranks as CHILD processes of a fresh torch.distributed.run (this process has
    not initialised any GPU and never will), stream their output through, return their exit code."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: RCCL needs it on this host driver
    env.setdefault('OMP_NUM_THREADS', '4')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--config', type=int, default=3, choices=sorted(CONFIGS),
                    help='BASELINE.json config number (1-based): 3 = case118 x 16384, K=4 (default, the metric); 2 = case30 x 4096; 5 = case300 x 8192 per GPU, K=10')
    ap.add_argument('--batch-per-gpu', type=int, default=None)
    ap.add_argument('--sustained-steps', type=int, default=2000,
                    help='extra untimed-by-the-contract run reported as "sustained" (0 = skip): the K-step burst ends before the chip settles at its power limit')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy, float32, at most 64 MB')
    ap.add_argument('--rehearse-cpu', action='store_true',
                    help='launcher / rendezvous / collective / JSON plumbing only, over gloo, without touching a GPU (CPU test)')
    a = ap.parse_args()
    global CASE, BATCH_PER_GPU, K
    CASE, BATCH_PER_GPU, K = CONFIGS[a.config]['case'], CONFIGS[a.config]['batch'], CONFIGS[a.config]['K']
    if a.batch_per_gpu is None:
        a.batch_per_gpu = BATCH_PER_GPU
    BYTES_PER_GRID, MFLOP_FWD_PER_GRID = bytes_per_grid(CASE), mflop_fwd_per_grid(CASE, K)
    NB, NE, NG = SHAPES[CASE]
    if a.gpus < 1:
        raise SystemExit('--gpus must be >= 1')
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit('--steps must be >= 1 and --warmup >= 0')
    launched = 'WORLD_SIZE' in os.environ and 'RANK' in os.environ
    if not launched and a.gpus > 1:
        sys.exit(self_launch(sys.argv[1:], a.gpus))
    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != a.gpus:
        raise SystemExit(f'WORLD_SIZE={world} does not match --gpus {a.gpus}')
    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline and not a.rehearse_cpu:
        cpu = cpu_baseline(case=CASE, k=K)

    import torch
    import torch.distributed as dist

    if a.rehearse_cpu:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(_free_port()))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        dist.all_reduce(t)
        dist.barrier()
        if rank == 0:
            print(json.dumps({'metric': 'rehearsal', 'n_gpus': world, 'sum_of_ranks': float(t.item()), 'config': a.config,
                              'workload': CONFIGS[a.config]['name'], 'global_batch': a.batch_per_gpu * world}), flush=True)
        dist.destroy_process_group()
        return

    import ctypes
    import opf_graph_neural_solver_amd as amd

    # Rehearsal switches for a ONE-GPU box (never set by the driver): every rank uses cuda:0 and the collective runs
    # over gloo, which exercises launch / rendezvous / barrier / all-reduce / max-over-ranks / JSON exactly like the RCCL run.
    share = os.environ.get('GNS_BENCH_SHARE_GPU') == '1'
    backend = os.environ.get('GNS_BENCH_BACKEND', 'nccl')
    if share:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)     # RCCL over xGMI
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    lib = amd.load_library()

    torch.manual_seed(0)                       # identical replicas on every rank
    model = amd.GNS(latent_dim=D, hidden_dim=H, K=K, gamma=GAMMA, multiple_phi=MULTI).to(dev)
    opt = amd.training.make_optimizer(model)               # the reference's optimiser: Adam, lr 1e-3 (GNS/main.py:241-243)
    bt = a.batch_per_gpu
    # rank r holds grids [r*bt, (r+1)*bt) of ONE data set: the same grids whatever the GPU count
    buses, lines, gens = amd.synth.synth_grids(CASE, bt, seed=DATA_SEED, device=dev, first_index=rank * bt)
    Bc, Lc, Gc = amd.get_BLG()
    # What training.fit() does with a resident data set (GNS/main.py:255 loads it whole): the id columns of every grid are compared
    # once and the set is brought into the kernels' input layout once (GNS.bind_dataset -> gns_prepack); the steps then read
    # that copy.  "ms_per_step_packing_per_call" below is the same step on inputs the model has never seen (packed on every call).
    model.bind_dataset(buses, lines, gens)
    model.topology_check = 'first'

    def step():
        opt.zero_grad(set_to_none=True)
        v, th, tot, last = model(buses, lines, gens, Bc, Lc, Gc)
        tot.mean().backward()
        grad = amd.dist.allreduce_gradients(model, global_batch=bt * world, local_batch=bt)
        opt.step()
        return v, th, tot, last, grad

    def fence():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def timed(nsteps):
        fence()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            outs_ = step()
        fence()
        dt_ = time.perf_counter() - t0
        tmax = torch.tensor([dt_], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        # the last step's (v, theta, total, last, flat gradient), detached: no autograd graph may outlive the timed steps (an
        # AccumulateGrad node kept alive ties the eager stream into the capture of training.GraphedStep below)
        return float(tmax.item()), tuple(x.detach() for x in outs_)

    for _ in range(a.warmup):
        step()
    lib.gns_profile_enable(max(a.steps, 1))
    dt, outs = timed(a.steps)
    tot = outs[2].mean()
    dumped = None
    if a.dump_outputs and rank == 0:
        # copied now: every later step replaces the parameters and the gradient
        dumped = {k: x.cpu().numpy() for k, x in zip(('v', 'theta', 'total_loss', 'last_loss', 'grad'), outs)}
        dumped['params'] = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()
    del outs
    ms_f, n_f, ms_b, n_b = ctypes.c_float(), ctypes.c_int(), ctypes.c_float(), ctypes.c_int()
    lib.gns_profile_read(0, ctypes.byref(ms_f), ctypes.byref(n_f))
    lib.gns_profile_read(1, ctypes.byref(ms_b), ctypes.byref(n_b))
    lib.gns_profile_enable(0)
    final_loss = float(tot.item())
    packed_hits = model._resident['hits'] if model._resident is not None else 0
    # the same step without the resident copy: inputs are packed by gns_pack_inputs_kernel inside every forward call
    model.unbind_dataset()
    for _ in range(2):
        step()
    dt_pack = timed(a.steps)[0]
    model.bind_dataset(buses, lines, gens)
    sustained = None
    if a.sustained_steps > 0:
        sdt = timed(a.sustained_steps)[0]
        sustained = {'steps': a.sustained_steps, 'value': round(bt * world * a.sustained_steps / sdt, 1), 'unit': 'grids/s',
                     'ms_per_step': round(sdt / a.sustained_steps * 1e3, 4)}
    # The same step as ONE captured HIP graph (training.GraphedStep on the resident, bound batch; one process only): what a loop gains
    # when launch gaps matter (config 2: -10 %, config 3: nothing).  Reported beside the eager headline, never instead of it.
    captured = None
    if world == 1 and a.sustained_steps > 0:
        try:
            gstep = amd.training.GraphedStep(model, opt, buses, lines, gens, copy_inputs=False)
            for _ in range(3):
                gstep.run(buses, lines, gens)
            fence()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                gstep.run(buses, lines, gens)
            fence()
            gdt = time.perf_counter() - t1
            captured = {'ms_per_step': round(gdt / a.steps * 1e3, 4), 'value': round(bt * a.steps / gdt, 1), 'unit': 'grids/s'}
            del gstep
        except Exception as e:                       # never let the extra measurement break the contract line
            captured = {'error': str(e)[:200]}
    # forward-only throughput (evaluation mode), not part of the headline value
    with torch.no_grad():
        for _ in range(2):
            model(buses, lines, gens, Bc, Lc, Gc)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(max(a.steps // 2, 1)):
            model(buses, lines, gens, Bc, Lc, Gc)
        torch.cuda.synchronize(dev)
        fwd_only = bt * max(a.steps // 2, 1) / (time.perf_counter() - t1)

    if rank == 0:
        grids = bt * world * a.steps
        value = grids / dt
        fwd_ms = ms_f.value / max(n_f.value, 1)
        bwd_ms = ms_b.value / max(n_b.value, 1)
        train_map = {0: 'auto', 1: 'lane-per-grid', 2: 'grid-per-workgroup'}[amd.get_option('train_mapping')]
        kfwd = 'gns_gw_forward_kernel' if train_map == 'grid-per-workgroup' else 'gns_forward_kernel'
        kbwd = 'gns_gw_backward_kernel' if train_map == 'grid-per-workgroup' else 'gns_backward_kernel'
        if train_map != 'grid-per-workgroup' and amd.get_option('bwd_variant') == 4:
            # the split backward: K x (gns_bwds_phys_kernel + the sweep kernels of the mode); timed as ONE unit by the library's
            # event pair around the whole sequence, which is what the persistent gns_backward_kernel was
            kbwd = 'gns_backward[split: %d x (gns_bwds_phys_kernel + gns_bwds_sweep_kernel x %d)]' % (K, {0: 3, 1: 2, 2: 1}[amd.get_option('bwds_mode')])
        dom_ms, dom, dom_is_bwd = (bwd_ms, kbwd, True) if bwd_ms >= fwd_ms else (fwd_ms, kfwd, False)
        ach_gbs = BYTES_PER_GRID * bt / (dom_ms * 1e-3) / 1e9
        dom_flop = (2.0 if dom_is_bwd else 1.0) * MFLOP_FWD_PER_GRID * 1e6 * bt
        traffic, traffic_src = None, None
        pmc = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')
        if os.path.exists(pmc):
            try:
                traffic = json.load(open(pmc)).get(f'config{a.config}', {}).get('backward' if dom_is_bwd else 'forward')
                traffic_src = 'profiles/pmc_traffic.json (static: rocprofv3 PMC run of the same workload, not measured in this run)'
            except Exception:
                traffic = None
        line = {
            'metric': 'grids/sec (fwd+bwd) on batched case118, K=4' if a.config == 3 else f'grids/sec (fwd+bwd) on batched case{CASE}, K={K}',
            'value': round(value, 1), 'unit': 'grids/s',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': round(dt / a.steps * 1e3, 4),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': f'BASELINE {CONFIGS[a.config]["name"]}: case{CASE}-shaped grids ({NB} buses, {NE} lines, {NG} generators), '
                                   f'batch {bt} per GPU, K={K}, latent_dim=20, hidden_dim=10, multiple_phi=True, gamma=0.9; step = fused forward + '
                                   'backward + flat-gradient all-reduce + Adam; grids = counter-based synthetic data set '
                                   f'(seed {DATA_SEED}), rank r holds global grids [r*{bt}, (r+1)*{bt})',
                       'inputs': f'resident data set, id columns compared and pre-packed ONCE before the timed region (GNS.bind_dataset -> gns_prepack: '
                                 f'{4 * 4 * (3 * NB + 4 * NE + 1) / 1024:.1f} KB/grid instead of the reference layout\'s {(BYTES_PER_GRID - 4 * (2 * NB + 2)) / 1024:.1f} KB/grid), '
                                 f'as training.fit() does; {packed_hits} of the timed + warm-up forwards read that copy',
                       'global_batch': bt * world, 'parallelism': f'dp{world} (grid-sharded)', 'training_kernels': train_map},
            'ms_per_step_packing_per_call': round(dt_pack / a.steps * 1e3, 4),
            'roofline': {'bound': 'hbm', 'kernel': dom, 'achieved': round(ach_gbs, 2), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                         'frac': round(ach_gbs / HBM_PEAK_GBS, 5), 'traffic': traffic, 'traffic_source': traffic_src,
                         'algorithmic_bytes_per_launch': BYTES_PER_GRID * bt, 'kernel_ms': round(dom_ms, 4)},
            'roofline_fp32': {'bound': 'fp32 vector FMA (the binding one: ~400 flop/B); NOMINAL flops of the reference formulation (incl. the dead '
                                       'last-step m family and the unfolded networks the kernels skip)', 'kernel': dom,
                              'achieved': round(dom_flop / (dom_ms * 1e-3) / 1e12, 3), 'peak': FP32_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                              'frac': round(dom_flop / (dom_ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, 4),
                              'nominal_flop_per_launch': dom_flop},
            'kernels_ms': {kfwd: round(fwd_ms, 4), kbwd: round(bwd_ms, 4)},
            'glue_ms_per_step': round(dt / a.steps * 1e3 - fwd_ms - bwd_ms, 4),
            'sustained': sustained,
            'captured_graph_step': captured,
            'forward_only_grids_per_s': round(fwd_only * world, 1),
            'final_mean_total_loss': final_loss,
        }
        if cpu is not None:
            line['cpu_baseline'] = cpu
        if dumped is not None:
            dump_outputs(a.dump_outputs, dumped)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
