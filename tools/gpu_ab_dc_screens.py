"""Bit-for-bit A/B of the three DC contingency screens between two builds of the project on one GPU.

dump     imports the package (and with it the library) from ROOT, runs a fixed set of seeded calls of ``dc_contingency_screen``,
         ``dc_n2_contingency_screen`` and ``dc_generator_contingency_screen_differentiable``, each differentiable, with ``flows`` on
         and off, and saves every returned tensor and every gradient to OUT.
compare  runs dump once per root, each in a fresh child process, and compares the two files tensor by tensor: the same shape and
         dtype, NaN at the same positions and the same bits everywhere else (so -0 and +0 differ).  One line per tensor; the exit
         status is 1 when a tensor differs.

The calls: ``synth.solvable_grids(14, 3, seed=0)`` with no rating, ``[E]`` and ``[Bt,E]``; pickup None, ``'pmax'``, a ``[Gn]`` and a
``[Bt,Gn]`` tensor that requires grad; the default lists (they hold islanding rows; the generator screen's holds rows without a
line), lists of 1, 8, 9 and 65 rows (a chunk of Q = 8, its tail, the gather's scan of 64 rows plus one), a generator list without a
line; one grid with a line that cannot be solved; a loss over ``worst_loading`` alone, over ``line_flow`` alone and over both; and
case300 x 2 grids with the candidates over three chunks of the 16 lanes.

usage: python tools/gpu_ab_dc_screens.py dump ROOT OUT
       python tools/gpu_ab_dc_screens.py compare ROOT_A ROOT_B > profiles/.../ab_bitwise.txt"""
import os
import subprocess
import sys
import tempfile


def dump(root, out_path):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch

    from opf_graph_neural_solver_amd import powerflow, synth

    dev = 'cuda'
    out = {}

    def weights(shape, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dev)

    def run(name, call, grids, slack, flows_modes=(True, False), pickup_grad=None, **kw):
        """One configuration: per ``flows`` and per loss a fresh forward and backward."""
        for flows in flows_modes:
            for loss_kind in (('worst', 'flow', 'both') if flows else ('worst',)):
                bu, li, ge = (t.clone().requires_grad_(True) for t in grids)
                pk = pickup_grad.clone().requires_grad_(True) if pickup_grad is not None else None
                res = call(bu, li, ge, slack_bus=slack, flows=flows, **({'pickup': pk} if pk is not None else {}), **kw)
                keep = ~res.islanding
                loss = 0.0
                if loss_kind != 'flow':
                    wl = res.worst_loading[:, keep]
                    loss = loss + (wl * weights(wl.shape, 11)).sum()
                if loss_kind != 'worst':
                    fl = res.line_flow[:, keep]
                    loss = loss + (fl * weights(fl.shape, 12)).sum()
                loss.backward()
                tag = f'{name} flows={int(flows)} loss={loss_kind}'
                if loss_kind == 'worst':
                    out[f'{tag} worst_loading'] = res.worst_loading.detach().cpu()
                    out[f'{tag} worst_line'] = res.worst_line.detach().cpu()
                    out[f'{tag} converged'] = res.converged.detach().cpu()
                    out[f'{tag} islanding'] = res.islanding.detach().cpu()
                    if flows:
                        out[f'{tag} line_flow'] = res.line_flow.detach().cpu()
                for label, t in (('grad_buses', bu), ('grad_lines', li), ('grad_generators', ge), ('grad_pickup', pk)):
                    if t is not None:
                        out[f'{tag} {label}'] = t.grad.detach().cpu()

    def n1(bu, li, ge, **kw):
        return powerflow.dc_contingency_screen(bu, li, ge, differentiable=True, **kw)

    def n2(bu, li, ge, **kw):
        return powerflow.dc_n2_contingency_screen(bu, li, ge, differentiable=True, **kw)

    g1 = powerflow.dc_generator_contingency_screen_differentiable

    buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 3, seed=0, device=dev)
    grids = (buses, lines, gens)
    Bt, E, Gn = lines.shape[0], lines.shape[1], gens.shape[1]
    rng = np.random.default_rng(5)
    ratings = {'none': None, 'E': 0.5 + weights((E,), 21).abs(), 'BtE': 0.5 + weights((Bt, E), 22).abs()}
    all_pairs = powerflow._pair_list(None, E).tolist()
    all_rows = powerflow._generator_contingency_list(None, Gn, E).tolist()
    for rname, rating in ratings.items():
        run(f'case14 n1 default rating={rname}', n1, grids, slack, rating=rating)
        run(f'case14 n2 default rating={rname}', n2, grids, slack, rating=rating)
        run(f'case14 g1 default pmax rating={rname}', g1, grids, slack, rating=rating, pickup='pmax')
    run('case14 g1 default pickup=None', g1, grids, slack)
    run('case14 g1 default pickup=[Gn]', g1, grids, slack, pickup_grad=0.5 + weights((Gn,), 23).abs())
    run('case14 g1 default pickup=[Bt,Gn]', g1, grids, slack, pickup_grad=0.5 + weights((Bt, Gn), 24).abs(), rating=ratings['BtE'])
    run('case14 g1 no line', g1, grids, slack, contingencies=[[g, -1] for g in range(Gn)], pickup='pmax')
    for n in (1, 8, 9, 65):
        run(f'case14 n1 rows={n}', n1, grids, slack, outages=rng.integers(0, E, n).tolist())
        run(f'case14 n2 rows={n}', n2, grids, slack, pairs=[all_pairs[i] for i in rng.integers(0, len(all_pairs), n)])
        run(f'case14 g1 rows={n}', g1, grids, slack, contingencies=[all_rows[i] for i in rng.integers(0, len(all_rows), n)],
            pickup_grad=0.5 + weights((Bt, Gn), 25).abs())
    bad = lines.clone()
    bad[2, 7, 3] = float('nan')                                  # grid 2 has a line that cannot be solved
    run('case14 n1 failed grid', n1, (buses, bad, gens), slack)
    run('case14 n2 failed grid', n2, (buses, bad, gens), slack)
    run('case14 g1 failed grid', g1, (buses, bad, gens), slack, pickup='pmax')

    # case300: 16 lanes per chunk, the candidates over three chunks
    buses, lines, gens, slack, _, _ = synth.solvable_grids(300, 2, seed=0, device=dev)
    grids = (buses, lines, gens)
    E, Gn = lines.shape[1], gens.shape[1]
    cand = rng.choice(E, 41, replace=False)
    pairs = [[int(cand[i]), int(cand[(i + 5) % 41])] for i in range(41)] + [[int(cand[i]), int(cand[(i + 1) % 41])] for i in range(19)]
    run('case300 n2 41 candidates', n2, grids, slack, pairs=pairs, rating=0.5 + weights((E,), 26).abs())
    rows = [[int(g), int(k)] for g, k in zip(rng.integers(0, Gn, 60), rng.choice(E, 60, replace=False))] + [[int(g), -1] for g in range(9)]
    run('case300 g1 60 lines', g1, grids, slack, contingencies=rows, pickup='pmax')
    run('case300 n1 40 outages', n1, grids, slack, outages=rng.choice(E, 40, replace=False).tolist())
    torch.cuda.synchronize()
    torch.save(out, out_path)
    print(f'{root}: {len(out)} tensors from {powerflow.__file__}', flush=True)


def compare(root_a, root_b):
    import torch

    tmp = tempfile.mkdtemp()
    files = []
    for tag, root in (('a', root_a), ('b', root_b)):
        files.append(os.path.join(tmp, f'{tag}.pt'))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), 'dump', root, files[-1]], timeout=600)
        if done.returncode != 0:
            print(f'dump of {root} ended with status {done.returncode}: nothing compared')
            return 2
    a, b = (torch.load(f) for f in files)
    differ = sorted(set(a) ^ set(b))
    for name in differ:
        print(f'{name}: in one build only')

    def bits(t):
        return t.view({8: torch.int64, 4: torch.int32}[t.element_size()]) if t.is_floating_point() else t

    for name in a:
        if name not in b:
            continue
        x, y = a[name], b[name]
        same = x.shape == y.shape and x.dtype == y.dtype
        if same and x.is_floating_point():
            nx, ny = x.isnan(), y.isnan()
            same = torch.equal(nx, ny) and torch.equal(bits(torch.where(nx, 0, x)), bits(torch.where(ny, 0, y)))
        elif same:
            same = torch.equal(x, y)
        nans = int(x.isnan().sum()) if x.is_floating_point() else 0
        print(f'{name}: shape {tuple(x.shape)} {x.dtype}, {nans} NaN: {"bit-identical" if same else "DIFFERENT"}')
        if not same:
            differ.append(name)
    print(f'{root_a} vs {root_b}: {len(a)} tensors, ' + ('the same bits' if not differ else f'{len(differ)} DIFFER'))
    return 1 if differ else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'dump':
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
