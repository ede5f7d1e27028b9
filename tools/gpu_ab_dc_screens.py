"""Bit-for-bit A/B between two builds of the project on one GPU: the three DC screens (``dc``), the two AC screens (``ac``) or the
GNS training step (``gns``: forward, parameter gradient, input gradients), or the other consumers of the AC line and bus arithmetic
(``pf``: Newton-Raphson, the solved case, the AC generator screen).

dump     imports the package (and with it the library) from ROOT, runs the fixed set of seeded calls of SET, each differentiable,
         and saves every returned tensor and every gradient to OUT.
compare  runs dump once per root, each in a fresh child process, and compares the two files tensor by tensor: the same shape and
         dtype, NaN at the same positions and the same bits everywhere else (so -0 and +0 differ).  One line per tensor; the exit
         status is 1 when a tensor differs.

The ``dc`` calls (``dc_contingency_screen``, ``dc_n2_contingency_screen``, ``dc_generator_contingency_screen_differentiable``, with
``flows`` on and off): ``synth.solvable_grids(14, 3, seed=0)`` with no rating, ``[E]`` and ``[Bt,E]``; pickup None, ``'pmax'``, a
``[Gn]`` and a ``[Bt,Gn]`` tensor that requires grad; the default lists (they hold islanding rows; the generator screen's holds rows
without a line), lists of 1, 8, 9 and 65 rows (a chunk of Q = 8, its tail, the gather's scan of 64 rows plus one), a generator list
without a line; one grid with a line that cannot be solved; a loss over ``worst_loading`` alone, over ``line_flow`` alone and over
both; and case300 x 2 grids with the candidates over three chunks of the 16 lanes.

The ``ac`` calls (``ac_contingency_screen(differentiable=True)``, ``ac_n2_contingency_screen_differentiable``): the same base batch
with no rating, ``[E]`` and ``[Bt,E]``; ``flows`` / ``states`` both on, both off and one of each; a loss over the states alone, the
flows alone, the summaries alone (``worst_loading``, ``v_min``, ``v_max``) and all, on the converged rows.  N-1 lists by the adjoint's
rows per wave C = min(8, max(1, ceil(K / 32))): the default list (20 rows, C = 1, islanding rows included), 33 outages (C = 2, a tail
chunk of 1), 257 outages with repeats (C = 8, the cap: 33 chunks, the last of 1).  N-2 lists by C = max(1, ceil(P / 64)): every pair
(190 rows: C = 3, 64 chunks, the last of 1), 64 pairs (C = 1), 65 pairs (C = 2 with a tail), and a list that names pairs in both
orders, pairs that share a bus and, where the topology has them, parallel lines.  One grid whose base solve fails (a NaN in a line),
with zero and with non-zero incoming gradients into it.  case118 x 2 grids with 40 outages and 40 pairs (parallel lines among
them), where the lane loops make a second trip (N = 118 > 64).

The ``pf`` calls: ``newton_raphson`` forward and backward (a loss over v and theta) on the same case14 batch, cold and warm-started,
on case118 x 2 and on one mixed-topology batch (case14 x 6 over two outages); ``solved_case`` forward and backward at that solution
with no rating, ``[E]`` and ``[Bt,E]``, away from the solution, with two units on the slack and on case118, each under a loss over the
flows alone, the injections and generators alone, the summaries alone and all, the state among the inputs that require grad; through
the C entry points one batch with a line whose id columns are not buses (NaN flows, a NaN gradient row), which the Python call
refuses; and ``ac_generator_contingency_screen_differentiable`` on its default list with the ``ac`` set's modes and losses.

The ``gns`` calls (``GNS.forward`` in training mode and ``.backward()`` under a loss with every upstream gradient non-zero; each
saves v, theta, total, last and the flat parameter gradient, and the three input gradients where they are asked for) are the smallest
that reach each branch of the backward kernels' line-physics adjoint (gns_phys_device.h) and per-bus gather, always from the
inputs and goldens of the tree the TOOL lies in, so both builds see the same numbers:
  goldens   the lane-per-grid kernels with the split and the persistent backward on ``odd_hub_indegree_40`` (the gather's tail rounds),
            ``odd_hub_all_gens`` and ``odd_random_40_one_gen`` (generator ends), ``odd_chain_one_way`` (empty lists), ``c14_b3 lowload``
            (dead lanes)
  persist   ``bwd_variant`` 1, 2, 3 on case118 x 130, K = 4; ``team`` 1, 2, 4 on case14 x 3
  split     ``bwds_mode`` 0, 1, 2 on case118 x 130 (plane level 2), case300 x 70 (level 1) and the 320-bus ring with chords of
            tests/helpers.py x 3 (level 0); ``dw_mfma`` = 0 once
  igrad     ``gns_backward_inputs`` on case30 x 70 and on ``odd_random_33_many_gens`` (generator ends)
  gridwg    ``train_mapping`` 2 at ``gw_pack`` 1 and 4 on case30 x 77, and the same batch with a 1 rad phase shift on every line of its
            first 20 grids: those grids' waves fail the pi / 4 vote and take the library's sincosf.  The tool prints, from the
            returned theta (the state the FIRST reverse step, k = K-1, reads; the other steps are not checked), how many live grids pass or
            fail that vote (case30 is one wave per grid; the dead lanes of a wave vote too and are not counted).
  grouped   one mixed-topology call (``topology_check = 'group'``): case14 x 150 over two outages

usage: python tools/gpu_ab_dc_screens.py dump dc|ac|pf|gns ROOT OUT
       python tools/gpu_ab_dc_screens.py compare dc|ac|pf|gns ROOT_A ROOT_B > profiles/.../ab_bitwise.txt"""
import os
import subprocess
import sys
import tempfile


def dump(which, root, out_path):
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch

    from opf_graph_neural_solver_amd import powerflow, synth

    dev = 'cuda'
    out = {}

    def weights(shape, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dev)

    def dc_calls():
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

    GROUPS = {'state': ('v', 'theta'), 'flow': ('p_from', 'q_from', 'p_to', 'q_to'), 'summary': ('worst_loading', 'v_min', 'v_max')}
    FORWARD = ('v', 'theta', 'p_from', 'q_from', 'p_to', 'q_to', 'worst_loading', 'worst_line', 'v_min', 'v_min_bus', 'v_max',
               'v_max_bus', 'converged', 'iterations', 'mismatch', 'islanding')
    ALL_MODES = ((True, True), (False, False), (True, False), (False, True))

    def ac_run(name, call, grids, slack, modes=ALL_MODES, also_grid=None, **kw):
        """One configuration: per (``flows``, ``states``) and per loss a fresh forward and backward.  The loss weighs the
        converged rows; with ``also_grid`` every row of that grid too (non-zero gradients into rows without a solution)."""
        for flows, states in modes:
            kinds = ['summary'] + (['state'] if states else []) + (['flow'] if flows else []) + (['all'] if flows and states else [])
            for n_kind, kind in enumerate(kinds):
                bu, li, ge = (t.clone().requires_grad_(True) for t in grids)
                res = call(bu, li, ge, slack_bus=slack, flows=flows, states=states, **kw)
                rows = res.converged.clone()
                if also_grid is not None:
                    rows[also_grid] = True
                loss = 0.0
                for group, fields in GROUPS.items():
                    if kind in (group, 'all'):
                        for seed, field in enumerate(fields):
                            x = getattr(res, field)[rows]
                            loss = loss + (x * weights(x.shape, 31 + seed)).sum()
                loss.backward()
                tag = f'{name} flows={int(flows)} states={int(states)} loss={kind}'
                if n_kind == 0:
                    for field in FORWARD:
                        if getattr(res, field) is not None:
                            out[f'{tag} {field}'] = getattr(res, field).detach().cpu()
                    for field in ('v', 'theta', 'converged', 'iterations'):
                        out[f'{tag} base.{field}'] = getattr(res.base, field).detach().cpu()
                for label, t in (('grad_buses', bu), ('grad_lines', li), ('grad_generators', ge)):
                    out[f'{tag} {label}'] = t.grad.detach().cpu()

    def pf_calls():
        import ctypes

        import opf_graph_neural_solver_amd as amd
        from opf_graph_neural_solver_amd._lib import PfConfig

        def nr(name, grids, slack, **kw):
            """``newton_raphson`` forward and backward under a loss over v and theta of the converged grids"""
            bu, li, ge = (t.clone().requires_grad_(True) for t in grids)
            res = powerflow.newton_raphson(bu, li, ge, slack_bus=slack, **kw)
            ok = res.converged
            ((res.v[ok] * weights(res.v[ok].shape, 51)).sum() + (res.theta[ok] * weights(res.theta[ok].shape, 52)).sum()).backward()
            for field in powerflow.PowerFlowResult._fields:
                out[f'{name} {field}'] = getattr(res, field).detach().cpu()
            for label, t in (('grad_buses', bu), ('grad_lines', li), ('grad_generators', ge)):
                out[f'{name} {label}'] = t.grad.detach().cpu()
            return res

        SC_GROUPS = {'flow': ('p_from', 'q_from', 'p_to', 'q_to'), 'injection': ('p_inj', 'q_inj', 'gen_p', 'gen_q', 'slack_p'),
                     'summary': ('worst_loading', 'v_min', 'v_max')}

        def sc(name, grids, slack, v, theta, rating=None):
            """``solved_case`` at (v, theta): per loss a fresh forward and backward, the state among the inputs that require grad"""
            for n_kind, kind in enumerate(('flow', 'injection', 'summary', 'all')):
                bu, li, ge, vv, th = (t.clone().requires_grad_(True) for t in (*grids, v, theta))
                res = powerflow.solved_case(bu, li, ge, vv, th, slack_bus=slack, rating=rating)
                loss = 0.0
                for group, fields in SC_GROUPS.items():
                    if kind in (group, 'all'):
                        for seed, field in enumerate(fields):
                            x = getattr(res, field)
                            loss = loss + (x * weights(x.shape, 61 + seed)).sum()
                loss.backward()
                tag = f'{name} loss={kind}'
                if n_kind == 0:
                    for field in powerflow.SolvedCase._fields:
                        out[f'{tag} {field}'] = getattr(res, field).detach().cpu()
                for label, t in (('grad_buses', bu), ('grad_lines', li), ('grad_generators', ge), ('grad_v', vv), ('grad_theta', th)):
                    out[f'{tag} {label}'] = t.grad.detach().cpu()

        def sc_raw(name, grids, slack, v, theta, clean_lines):
            """``gns_pfs_evaluate`` and ``gns_pfs_adjoint`` through the C entry points on the blob of ``clean_lines``' topology, for
            lines the Python call refuses in its analysis (id columns that are not buses); every incoming gradient non-zero"""
            lib = amd.load_library()
            bu, li, ge = (t.contiguous() for t in grids)
            Bt, N, E, Gn = bu.shape[0], bu.shape[1], li.shape[1], ge.shape[1]
            ids = clean_lines[0].cpu().numpy()
            topo = powerflow.analyse_topology(N, ids[:, 0], ids[:, 1], ge[0, :, 0].cpu().numpy(), slack, device=dev)
            cfg = PfConfig(N, E, Gn, 0, 0.0)
            need = ctypes.c_size_t(0)
            assert lib.gns_pfs_workspace_bytes(ctypes.byref(cfg), topo.host.ctypes.data, Bt, ctypes.byref(need)) == 0
            ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
            res = {k: torch.empty(Bt, dict(E=E, N=N, Gn=Gn)[d], dtype=torch.float64, device=dev) for k, d in powerflow._PFS_ROWS}
            res.update({k: torch.empty(Bt, dtype=dt, device=dev) for k, dt in powerflow._PFS_SCALARS})
            head = (ctypes.byref(cfg), topo.host.ctypes.data, topo.blob.data_ptr(), bu.data_ptr(), li.data_ptr(), ge.data_ptr(), Bt,
                    v.data_ptr(), theta.data_ptr(), None, 0)
            stream = torch.cuda.current_stream().cuda_stream
            assert lib.gns_pfs_evaluate(*head, *(res[k].data_ptr() for k in powerflow._PFS_C_ORDER), ws.data_ptr(), need.value, stream) == 0
            incoming = [weights(res[k].shape, 71 + n).contiguous() for n, k in enumerate(powerflow._PFS_DIFF)]
            grads = {'grad_v': torch.empty_like(v), 'grad_theta': torch.empty_like(theta), 'grad_buses': torch.empty_like(bu),
                     'grad_lines': torch.empty_like(li), 'grad_generators': torch.empty_like(ge)}
            assert lib.gns_pfs_adjoint(*head, res['worst_line'].data_ptr(), res['v_min_bus'].data_ptr(), res['v_max_bus'].data_ptr(),
                                       *(t.data_ptr() for t in incoming), *(t.data_ptr() for t in grads.values()), None, 0, stream) == 0
            torch.cuda.synchronize()
            for k, t in {**res, **grads}.items():
                out[f'{name} {k}'] = t.cpu()

        buses, lines, gens, slack, v, theta = synth.solvable_grids(14, 3, seed=0, device=dev)
        grids = (buses, lines, gens)
        Bt, E = lines.shape[0], lines.shape[1]
        base = nr('case14 newton_raphson', grids, slack)
        nr('case14 newton_raphson warm start', grids, slack, v0=v, theta0=theta, max_iter=3)
        for rname, rating in (('none', None), ('E', 0.5 + weights((E,), 21).abs()), ('BtE', 0.5 + weights((Bt, E), 22).abs())):
            sc(f'case14 solved_case rating={rname}', grids, slack, base.v.detach(), base.theta.detach(), rating)
        sc('case14 solved_case away from the solution', grids, slack, v.to(dev), (1.5 * theta).to(dev))
        bad = lines.clone()
        bad[:, 5, 0] = float(buses.shape[1] + 1)                     # line 5's from id is no bus: NaN flows, a NaN gradient row
        sc_raw('case14 solved_case line 5 not between buses', (buses, bad, gens), slack, base.v.detach().contiguous(),
               base.theta.detach().contiguous(), lines)
        two = gens.clone()
        other = int((two[0, :, 0] != slack).nonzero()[0])
        two[:, other, 0] = float(slack)                              # a second unit on the slack
        sc('case14 solved_case two units on the slack', (buses, lines, two), slack, v.to(dev), theta.to(dev))

        b118 = synth.solvable_grids(118, 2, seed=0, device=dev)      # N = 118 > 64: the lane loops make a second trip
        res = nr('case118 newton_raphson', b118[:3], b118[3])
        sc('case118 solved_case', b118[:3], b118[3], res.v.detach(), res.theta.detach(), 0.5 + weights((b118[1].shape[1],), 26).abs())

        mixed = synth.solvable_contingency_grids(14, 6, [4, 13], seed=11, device=dev, shuffle=True)
        nr('case14 x 6 newton_raphson mixed topologies', mixed[:3], mixed[3], mixed_topologies=True)

        g1 = powerflow.ac_generator_contingency_screen_differentiable
        ac_run('case14 ac g1 default pickup=None', g1, grids, slack)
        ac_run('case14 ac g1 default pmax rating=BtE', g1, grids, slack, pickup='pmax', rating=0.5 + weights((Bt, E), 22).abs())

    def ac_calls():
        run = ac_run

        def n1(bu, li, ge, **kw):
            return powerflow.ac_contingency_screen(bu, li, ge, differentiable=True, **kw)

        n2 = powerflow.ac_n2_contingency_screen_differentiable

        def special_pairs(case, E):
            """Pairs in both orders, pairs that share a bus, every pair of parallel lines of the topology"""
            f, t, _ = synth.case_topology(case)
            ends = [frozenset((int(a), int(b))) for a, b in zip(f, t)]
            share = [[j, k] for j in range(E) for k in range(j + 1, E) if len(ends[j] & ends[k]) == 1][:6]
            parallel = [[j, k] for j in range(E) for k in range(j + 1, E) if ends[j] == ends[k]]
            some = share[:3] + parallel + [[0, E - 1], [1, E // 2]]
            return some + [[k, j] for j, k in some] + share[3:], len(parallel)

        buses, lines, gens, slack, _, _ = synth.solvable_grids(14, 3, seed=0, device=dev)
        grids = (buses, lines, gens)
        Bt, E = lines.shape[0], lines.shape[1]
        rng = np.random.default_rng(7)
        ratings = {'none': None, 'E': 0.5 + weights((E,), 21).abs(), 'BtE': 0.5 + weights((Bt, E), 22).abs()}
        all_pairs = powerflow._pair_list(None, E).tolist()
        both = ((True, True), (False, False))
        for rname, rating in ratings.items():
            run(f'case14 n1 default rating={rname}', n1, grids, slack, rating=rating)
            run(f'case14 n2 every pair rating={rname}', n2, grids, slack, rating=rating)
        for n in (33, 257):
            run(f'case14 n1 rows={n}', n1, grids, slack, modes=both, outages=rng.integers(0, E, n).tolist())
        for n in (64, 65):
            run(f'case14 n2 rows={n}', n2, grids, slack, modes=both, pairs=[all_pairs[i] for i in rng.choice(len(all_pairs), n, replace=False)])
        special, n_parallel = special_pairs(14, E)
        run(f'case14 n2 both orders, shared buses, {n_parallel} parallel', n2, grids, slack, modes=both, pairs=special,
            rating=ratings['BtE'])
        bad = lines.clone()
        bad[2, 7, 3] = float('nan')                                  # grid 2 has no base solution
        for name, also in (('zero gradients into it', None), ('gradients into it', 2)):
            run(f'case14 n1 failed grid, {name}', n1, (buses, bad, gens), slack, modes=both, also_grid=also)
            run(f'case14 n2 failed grid, {name}', n2, (buses, bad, gens), slack, modes=both, also_grid=also,
                pairs=[all_pairs[i] for i in rng.choice(len(all_pairs), 70, replace=False)])

        # case118: two trips of the lane loops over the buses, three over the lines
        buses, lines, gens, slack, _, _ = synth.solvable_grids(118, 2, seed=0, device=dev)
        grids = (buses, lines, gens)
        E = lines.shape[1]
        special, n_parallel = special_pairs(118, E)
        every = powerflow._pair_list(None, E)
        pairs = special + every[rng.choice(every.shape[0], 40 - len(special), replace=False)].tolist()
        rating = 0.5 + weights((E,), 26).abs()
        run('case118 n1 40 outages', n1, grids, slack, modes=both, outages=rng.choice(E, 40, replace=False).tolist(), rating=rating)
        run(f'case118 n2 40 pairs, {n_parallel} parallel', n2, grids, slack, modes=both, pairs=pairs, rating=rating)

    def gns_calls():
        import opf_graph_neural_solver_amd as amd
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
        import helpers                                           # the goldens and topologies of the tool's own tree, for both builds

        DEFAULTS = {k: amd.get_option(k) for k in ('fwd_mapping', 'train_mapping', 'bwd_variant', 'bwds_mode', 'dw_mfma', 'team', 'gw_pack')}

        def run(name, m, grids, igrad=False, **opts):
            """One training step under ``opts`` (the other options at their defaults)"""
            for k, v in {**DEFAULTS, **opts}.items():
                amd.set_option(k, v)
            bu, li, ge = (x.detach().clone().to(dev).requires_grad_(igrad) for x in grids)
            m.zero_grad()
            v, th, tot, last = m(bu, li, ge)
            loss = (tot * weights(tot.shape, 41).float()).sum() + (last * weights(last.shape, 42).float()).sum() \
                + (v * weights(v.shape, 43).float()).sum() + (th * weights(th.shape, 44).float()).sum()
            loss.backward()
            m.check_status()
            for label, x in (('v', v), ('theta', th), ('total', tot), ('last', last)):
                out[f'{name} {label}'] = x.detach().cpu()
            out[f'{name} grad_params'] = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).cpu()
            if igrad:
                for label, x in (('grad_buses', bu), ('grad_lines', li), ('grad_generators', ge)):
                    out[f'{name} {label}'] = x.grad.detach().cpu()
            return th.detach(), li.detach()

        def model(d, h, K, multi, seed=7):
            torch.manual_seed(seed)
            return amd.GNS(d, h, K, 0.9, multi).to(dev)

        def golden(name):
            g = helpers.load_golden(name)
            c = helpers.cfg_of(g)
            m = model(c['latent_dim'], c['hidden_dim'], c['K'], c['multiple_phi'])
            return m, tuple(torch.as_tensor(g[k]) for k in ('buses', 'lines', 'generators'))

        for name in ('odd_hub_indegree_40_b2_K3_d10_multi', 'odd_hub_all_gens_b2_K4_d10_single', 'odd_random_40_one_gen_b2_K4_d20_multi',
                     'odd_chain_one_way_b2_K2_d20_single', 'c14_b3_K4_d20_multi_lowload'):
            m, grids = golden(name)
            run(f'{name} split', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=4)
            run(f'{name} persistent', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=2 if 'multi' in name else 1)

        grids = amd.synth.synth_grids(118, 130, seed=13)
        m = model(20, 10, 4, True)
        for var in (1, 2, 3):
            run(f'case118 x 130 bwd_variant={var}', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=var)
        for mode in (0, 1, 2):
            run(f'case118 x 130 bwds_mode={mode}', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=4, bwds_mode=mode)
        run('case118 x 130 bwd_variant=4 dw_mfma=0', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=4, dw_mfma=0)
        g14 = amd.synth.synth_grids(14, 3, seed=13)
        m14 = model(20, 10, 4, True)
        for team in (1, 2, 4):
            run(f'case14 x 3 team={team}', m14, g14, fwd_mapping=1, train_mapping=1, bwd_variant=2, team=team)
        grids = amd.synth.synth_grids(300, 70, seed=13)
        for mode in (0, 1, 2):
            run(f'case300 x 70 bwds_mode={mode}', m, grids, fwd_mapping=1, train_mapping=1, bwd_variant=4, bwds_mode=mode)
        n, f, t_, gb = helpers.ring_with_chords_320()
        grids = helpers.grids_on_topology(n, f, t_, gb, 3, 320)
        m320 = model(10, 10, 2, True)
        for mode in (0, 1, 2):
            run(f'ring320 x 3 bwds_mode={mode}', m320, grids, fwd_mapping=1, train_mapping=1, bwd_variant=4, bwds_mode=mode)

        run('case30 x 70 input gradients', model(20, 10, 3, True), amd.synth.synth_grids(30, 70, seed=13), igrad=True)
        m, grids = golden('odd_random_33_many_gens_b2_K4_d20_single')
        run('odd_random_33_many_gens input gradients', m, grids, igrad=True)

        def trig_paths(th, li):
            """Grids whose line angles at the returned state (what reverse step K-1 reads) pass / fail the grid-per-workgroup backward's pi / 4 vote"""
            src, dst, sh = li[0, :, 0].long() - 1, li[0, :, 1].long() - 1, li[:, :, 6]
            ds = th[:, src[src]] - th[:, dst[src]]                   # the reference gathers per-line arrays with bus ids (main.py:41)
            dt = th[:, dst[dst]] - th[:, src[dst]]
            dth = th[:, src] - th[:, dst]
            amax = torch.stack([(dth - ds - sh[:, src]).abs(), (-dth - ds + sh[:, src]).abs(), (-dth - dt - sh[:, dst]).abs(), ds.abs(), dt.abs()]).amax(dim=(0, 2))
            return int((amax <= 0.785).sum()), int((amax > 0.785).sum())

        g30 = amd.synth.synth_grids(30, 77, seed=13)
        shifted = tuple(x.clone() for x in g30)
        shifted[1][:20, :, 6] += 1.0
        m30 = model(10, 10, 3, False)
        for pack in (1, 4):
            for tag, grids in (('', g30), (' 1 rad shift in 20 grids', shifted)):
                th, li = run(f'case30 x 77 train_mapping=2 gw_pack={pack}{tag}', m30, grids, train_mapping=2, gw_pack=pack)
                small, lib = trig_paths(th, li)
                print(f'case30 x 77 gw_pack={pack}{tag}: reverse step k = K-1 (estimate from the returned theta): {small} grids on the small-angle path, {lib} on the library path', flush=True)

        mg = model(20, 10, 3, True)
        mg.topology_check = 'group'
        run('case14 x 150 two topologies grouped', mg, amd.synth.contingency_grids(14, 150, [4, 13], seed=11, shuffle=True)[:3])
        for k, v in DEFAULTS.items():
            amd.set_option(k, v)

    {'dc': dc_calls, 'ac': ac_calls, 'pf': pf_calls, 'gns': gns_calls}[which]()
    torch.cuda.synchronize()
    torch.save(out, out_path)
    print(f'{root}: {len(out)} tensors of the {which} set from {powerflow.__file__}', flush=True)


def compare(which, root_a, root_b):
    import torch

    tmp = tempfile.mkdtemp()
    files = []
    for tag, root in (('a', root_a), ('b', root_b)):
        files.append(os.path.join(tmp, f'{tag}.pt'))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), 'dump', which, root, files[-1]], timeout=600)
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
    if len(sys.argv) == 5 and sys.argv[1] == 'dump' and sys.argv[2] in ('dc', 'ac', 'pf', 'gns'):
        dump(*sys.argv[2:])
    elif len(sys.argv) == 5 and sys.argv[1] == 'compare' and sys.argv[2] in ('dc', 'ac', 'pf', 'gns'):
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
