"""Every kernel configuration against a float64 oracle (-m gpu), with the path that actually ran read back from the library.

Each row sets library options, runs the forward (evaluation) or the forward and backward (training) on a data set and asserts
  1. the read-only "last.*" record (include/gns_hip.h) names the path the row is about - the library falls back quietly
     (waves halved for a team, planes that do not fit, teams cancelled, widths without a persistent backward), so an option alone
     proves nothing;
  2. v, theta, total, last and the parameter gradient (plus the input gradients on split-backward rows) of the sampled grids are
     within the error budget of helpers.assert_budget: 4x the float32 oracle's own error against float64, plus 8 fp32 ulps;
  3. a bitwise result where the design promises one (input routes, poisoned workspaces, parameter gradient with and without input
     gradients).
The loss weights all grids outside the sample with 0, so those grids - and the dead lanes of a ragged last group - must add
exactly nothing.  The oracle results depend on the data set, the parameters and the sample only: computed once per data set."""
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import ROOT, assert_budget, cfg_of, load_golden, loss_weights, options, oracle64, t, weighted_loss

OUTS = ('v', 'theta', 'total', 'last')
IGRADS = ('grad_buses', 'grad_lines', 'grad_gens')
LAST = ('fwd_kernel', 'fwd_waves', 'fwd_plane', 'team', 'gw_pack', 'bwd_kernel', 'dw_mfma', 'bwds_mode', 'bwds_chunks', 'bwds_R',
        'bwd_gw_pack')

# name: case, batch, (latent_dim, hidden_dim), K, multiple_phi, seed, sampled grids
DATASETS = {
    'c118x229': (118, 229, (20, 10), 4, True, 21, [0, 1, 63, 64, 127, 128, 191, 192, 228]),
    'c14x229': (14, 229, (20, 10), 4, True, 22, [0, 1, 63, 64, 191, 192, 228]),
    'c30x229': (30, 229, (10, 10), 10, False, 23, [0, 1, 63, 64, 191, 192, 228]),
    'c200x229': (200, 229, (20, 14), 4, True, 24, [0, 63, 64, 192, 228]),
    'c300x8192': (300, 8192, (20, 10), 10, True, 25, [0, 63, 64, 4095, 4096, 8127, 8128, 8191]),
    'c14x4133_K30': (14, 4133, (6, 7), 30, False, 26, [0, 1, 63, 64, 2047, 2048, 4095, 4096, 4132]),
    'c30x4133_K1': (30, 4133, (10, 10), 1, False, 27, [0, 1, 63, 64, 4095, 4096, 4132]),
    # 625 groups: R > 1 and groups % R != 0 for every chunk count; grids at the R-block edges of C = 8, 12, 16, 24, 32 (R = 2, 3, 4, 7, 9)
    'c30x40000': (30, 40000, (20, 10), 3, True, 13, [0, 1, 63, 64, 127, 128, 191, 192, 255, 256, 447, 448, 575, 576, 39935, 39936, 39999]),
    # the benchmark's operating point: grids 0, 1, 63, 64, group and half-batch edges, the last group and the last grid
    'c118x16384': (118, 16384, (20, 10), 4, True, 31, [0, 1, 63, 64, 127, 128, 4097, 8191, 8192, 16319, 16320, 16383]),
}
DEEP_GOLDENS = ['c14_b2_K15_d10_multi', 'c14_b2_K30_d10_single']

REPORT = {}


# ---- CPU: the record reads -1 before any launch and cannot be set ----------------------------------------------------------------
def test_last_path_record_is_read_only_and_unset_before_any_launch():
    code = ('import ctypes, opf_graph_neural_solver_amd as amd\n'
            'lib = amd.load_library()\n'
            f'names = {list(LAST)!r}\n'
            'v = ctypes.c_int(7)\n'
            'for n in names:\n'
            '    assert lib.gns_get_option(("last." + n).encode(), ctypes.byref(v)) == 0, n\n'
            '    assert v.value == -1, (n, v.value)\n'
            '    assert lib.gns_set_option(("last." + n).encode(), 1) == 1, n\n'
            '    assert amd.get_option("last." + n) == -1, n\n'
            'assert lib.gns_get_option(b"last.nothing", ctypes.byref(v)) == 1\n'
            'print("ok")\n')
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, GNS_NO_AUTOBUILD='1'))
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr


def test_last_path_record_is_documented_in_the_c_abi():
    with open(os.path.join(ROOT, 'include', 'gns_hip.h')) as f:
        text = f.read()
    for n in LAST:
        assert f'"last.{n}"' in text or f'last.{n}"' in text, n


# ---- on the device ---------------------------------------------------------------------------------------------------------------
class Data:
    pass


@pytest.fixture(scope='module')
def store(request):
    cache = {}
    yield cache
    path = os.environ.get('GNS_CONFIG_REPORT')
    if path and REPORT:
        with open(path, 'w') as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dataset(store, name):
    if name in store:
        return store[name]
    import opf_graph_neural_solver_amd as amd
    D = Data()
    if name in DATASETS:
        case, bt, (d, h), K, multi, seed, sample = DATASETS[name]
        torch.manual_seed(seed)
        D.model = amd.GNS(d, h, K, 0.9, multi).cuda()
        D.x = amd.synth.synth_grids(case, bt, seed=seed, device='cuda')
        D.cfg = dict(latent_dim=d, hidden_dim=h, K=K, gamma=0.9, multiple_phi=multi)
    elif name.startswith('route'):                     # slices of one bound case118 set of 256 grids
        full = _route_set(store)
        lo, hi = (64, 164) if name == 'route_ragged' else (128, 256)
        D.model, D.cfg = full.model, full.cfg
        D.x = tuple(x[lo:hi] for x in full.x)
        D.full = full.x
        bt, sample = hi - lo, ([0, 1, 35, 36, 63, 64, 99] if name == 'route_ragged' else [0, 63, 64, 127])
    else:                                              # a deep golden of the reference
        g = load_golden(name)
        c = cfg_of(g)
        D.model = amd.GNS(c['latent_dim'], c['hidden_dim'], c['K'], c['gamma'], c['multiple_phi'])
        flat, off, sd = t(g['params']), 0, {}
        for n, p in D.model.named_parameters():
            sd[n] = flat[off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
        D.model.load_state_dict(sd)
        D.model = D.model.cuda()
        D.x = tuple(t(g[k]).cuda().contiguous() for k in ('buses', 'lines', 'generators'))
        D.cfg = c
        bt = D.x[0].shape[0]
        sample = list(range(bt))
    D.model.topology_check = 'first'
    D.Bt, D.sample = bt, sample
    D.w = loss_weights(bt, D.x[0].shape[1], sample, seed=len(name) * 7 + bt)
    D.o32, D.o64 = oracle64(D.model.flat_parameters(), *D.x, D.cfg, sample, D.w)
    store[name] = D
    return D


def _route_set(store):
    if 'route_set' not in store:
        import opf_graph_neural_solver_amd as amd
        S = Data()
        torch.manual_seed(41)
        S.model = amd.GNS(20, 10, 4, 0.9, True).cuda()
        S.x = amd.synth.synth_grids(118, 256, seed=41, device='cuda')
        S.cfg = dict(latent_dim=20, hidden_dim=10, K=4, gamma=0.9, multiple_phi=True)
        store['route_set'] = S
    return store['route_set']


def _run(D, train, inputs=False):
    """One call: outputs (and gradients) of the whole batch on the device, plus the record of the path that ran."""
    import opf_graph_neural_solver_amd as amd
    m, x = D.model, D.x
    m.zero_grad()
    if inputs:
        x = [a.clone().requires_grad_(True) for a in x]
    if not train:
        with torch.no_grad():
            out = m(*x)
    else:
        out = m(*x)
        weighted_loss(out, D.w).backward()
    torch.cuda.synchronize()
    r = {k: o.detach() for k, o in zip(OUTS, out)}
    if train and any(p.grad is not None for p in m.parameters()):
        r['grad_params'] = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    if inputs:
        for k, a in zip(IGRADS, x):
            r[k] = a.grad.detach()
    r['path'] = {n: amd.get_option('last.' + n) for n in LAST}
    return r


def _check(D, r, row):
    """Budget of every output and gradient of the sampled grids; grids outside the sample get exactly zero input gradient."""
    ratios = {}
    s = torch.as_tensor(D.sample, device='cuda')
    for k in OUTS + ('grad_params',) + IGRADS:
        if k not in r:
            continue
        mine = r[k] if k == 'grad_params' else r[k][s]
        ratios[k] = round(assert_budget(mine, D.o32[k], D.o64[k], f'{row}: {k}'), 3)
        if k in IGRADS:
            rest = torch.ones(D.Bt, dtype=torch.bool, device='cuda')
            rest[s] = False
            assert torch.count_nonzero(r[k][rest]) == 0, f'{row}: {k} of grids outside the sample is not exactly zero'
    REPORT[row] = dict(path={k: v for k, v in r['path'].items() if v != -1}, ratios=ratios)
    return ratios


def _expect(r, **want):
    got = {k: r['path'][k] for k in want}
    assert got == want, f'path {got} != {want}'


def _split_layout(groups, chunks):
    """C and R of the split backward (gns_bwds_layout): 8 one-wave sweep workgroups per CU; 8 chunks per group when there is a group
    per CU, finer chunks for smaller batches; an explicit chunk count wins; R groups per workgroup."""
    slots = 8 * _ncu()
    C = chunks or (8 if groups * 8 >= slots else (16 if groups * 16 >= slots else 32))
    return C, max(1, groups * C // slots)


def _equal(a, b, keys, row):
    for k in keys:
        assert torch.equal(a[k], b[k]), f'{row}: {k} differs bitwise'


# ---- evaluation, lane-per-grid ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('team', [1, 2, 4])
@pytest.mark.parametrize('plane', [0, 1, 2])
@pytest.mark.parametrize('waves', [1, 2, 4, 8, 16])
def test_eval_lane_waves_planes_teams(store, waves, plane, team):
    """229 case118 grids = 4 groups: teams of up to 4 are resident; waves x team <= 32 (a team halves its waves), the second plane
    needs one workgroup per group, the (v, theta) plane fits at every team size."""
    D = _dataset(store, 'c118x229')
    with options(fwd_mapping=1, fwd_waves=waves, fwd_plane=plane, team=team):
        r = _run(D, train=False)
    w = waves
    while w * team > 32:
        w //= 2
    _expect(r, fwd_kernel=1, fwd_waves=w, team=team, fwd_plane=plane if team == 1 else min(plane, 1))
    _check(D, r, f'eval lane waves={waves} plane={plane} team={team} c118x229')


@pytest.mark.gpu
@pytest.mark.parametrize('plane', [0, 1, 2])
def test_eval_lane_planes_case200(store, plane):
    """case200: the (v, theta) plane fits in LDS, the second one does not (2 x 200 x 64 x 8 B + the reduction > 160 KB)."""
    D = _dataset(store, 'c200x229')
    with options(fwd_mapping=1, fwd_plane=plane, team=1):
        r = _run(D, train=False)
    _expect(r, fwd_kernel=1, fwd_waves=16, team=1, fwd_plane=min(plane, 1))
    _check(D, r, f'eval lane plane={plane} c200x229 (20,14)')


@pytest.mark.gpu
@pytest.mark.parametrize('plane', [0, 1, 2])
def test_eval_lane_planes_case300_x_8192(store, plane):
    """case300 x 8192 = 128 groups on teams of two: the (v, theta) plane fits only because a team keeps its reduction in HBM."""
    D = _dataset(store, 'c300x8192')
    with options(fwd_mapping=1, fwd_plane=plane):
        r = _run(D, train=False)
    _expect(r, fwd_kernel=1, fwd_waves=16, team=2, fwd_plane=min(plane, 1))
    _check(D, r, f'eval lane plane={plane} c300x8192 K10')


# ---- grid-per-workgroup: every pack, evaluation and training ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('pack', list(range(1, 17)))
@pytest.mark.parametrize('name', ['c14x229', 'c30x229', 'c118x229'])
def test_grid_per_workgroup_packs(store, name, pack):
    """Every gw_pack 1..16 (229 grids: no pack > 1 divides the batch).  A pack the kernels accept runs on them; one they do not
    (more than 16 waves per workgroup, or LDS) falls back to the lane-per-grid kernels.  Either way the values are the oracle's."""
    D = _dataset(store, name)
    wpg = (max(D.x[0].shape[1], D.x[1].shape[1]) + 63) // 64
    with options(fwd_mapping=2, gw_pack=pack):
        r = _run(D, train=False)
    if r['path']['fwd_kernel'] == 2:
        _expect(r, gw_pack=pack)
        assert wpg * pack <= 16
    else:
        _expect(r, fwd_kernel=1, gw_pack=-1)
        assert pack > 1, 'gw_pack 1 must run on the grid-per-workgroup kernel'
    _check(D, r, f'eval gw pack={pack} {name}')
    with options(train_mapping=2, gw_pack=pack):
        r = _run(D, train=True)
    if r['path']['fwd_kernel'] == 2:
        _expect(r, gw_pack=pack, bwd_kernel=0, bwd_gw_pack=pack)
        assert wpg * pack <= 16
    else:
        _expect(r, fwd_kernel=1, bwd_gw_pack=-1)
        assert pack > 1, 'gw_pack 1 must train on the grid-per-workgroup pair'
    _check(D, r, f'train gw pack={pack} {name}')


# ---- training, lane-per-grid ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('variant', [1, 2, 3])
def test_persistent_backward_variants(store, variant):
    D = _dataset(store, 'c118x229')
    with options(train_mapping=1, bwd_variant=variant, dw_mfma=1):
        r = _run(D, train=True)
    _expect(r, fwd_kernel=1, bwd_kernel=variant, dw_mfma=1, bwds_chunks=-1)
    _check(D, r, f'train lane variant={variant} c118x229')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [1, 2, 3])
def test_persistent_variants_reroute(store, variant):
    """(20, 14) has no persistent backward: every variant runs the split one.  A single-phi model has no variant 2 or 3: it runs 1."""
    D = _dataset(store, 'c200x229')
    with options(train_mapping=1, bwd_variant=variant):
        r = _run(D, train=True)
    _expect(r, fwd_kernel=1, bwd_kernel=4, bwds_mode=1)
    _check(D, r, f'train lane variant={variant} c200x229 (20,14) -> split')
    D = _dataset(store, 'c30x229')
    with options(train_mapping=1, bwd_variant=variant):
        r = _run(D, train=True)
    _expect(r, fwd_kernel=1, bwd_kernel=1, dw_mfma=1)
    _check(D, r, f'train lane variant={variant} c30x229 single phi')


def _split_row(D, name, row_opts, chunks, mode):
    """A split-backward row: the parameter-gradient run, then the same with input gradients (gns_backward_inputs): bitwise the same
    parameter gradient, input gradients within the budget."""
    with options(train_mapping=1, bwd_variant=4, dw_mfma=1, **row_opts):
        r = _run(D, train=True)
        C, R = _split_layout((D.Bt + 63) // 64, chunks)
        _expect(r, fwd_kernel=1, bwd_kernel=4, dw_mfma=1, bwds_mode=mode, bwds_chunks=C, bwds_R=R)
        ri = _run(D, train=True, inputs=True)
        _expect(ri, fwd_kernel=1, bwd_kernel=4, bwds_mode=mode, bwds_chunks=C, bwds_R=R)
    _equal(r, ri, ('grad_params',) + OUTS, f'{name}: with input gradients')
    ri['path'] = r['path']
    _check(D, ri, f'train split mode={mode} chunks={chunks} {name}')
    return C, R


@pytest.mark.gpu
@pytest.mark.parametrize('mfma', [1, 0])
@pytest.mark.parametrize('chunks', [0, 8, 12, 16, 24, 32])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_split_backward_modes_chunks_engines(store, mode, chunks, mfma):
    D = _dataset(store, 'c118x229')
    if mfma:
        _split_row(D, 'c118x229', dict(bwds_mode=mode, bwds_chunks=chunks), chunks, mode)
        return
    with options(train_mapping=1, bwd_variant=4, bwds_mode=mode, bwds_chunks=chunks, dw_mfma=0):
        r = _run(D, train=True)
    _expect(r, fwd_kernel=1, bwd_kernel=1, dw_mfma=0, bwds_chunks=-1)     # the packed-FMA engine lives in the persistent kernel
    _check(D, r, f'train lane variant=4 dw_mfma=0 mode={mode} chunks={chunks} c118x229')


@pytest.mark.gpu
@pytest.mark.parametrize('chunks', [0, 8, 12, 16, 24, 32])
def test_split_backward_chunks_on_many_groups(store, chunks):
    """40 000 case30 grids = 625 groups: several groups per sweep workgroup (R > 1) and a last block of fewer than R groups."""
    D = _dataset(store, 'c30x40000')
    mode = chunks // 4 % 3
    C, R = _split_row(D, 'c30x40000', dict(bwds_mode=mode, bwds_chunks=chunks), chunks, mode)
    assert R > 1 and 625 % R != 0, (C, R)


@pytest.mark.gpu
@pytest.mark.parametrize('chunks', [12, 24])
def test_split_backward_chunks_single_phi_k1(store, chunks):
    D = _dataset(store, 'c30x4133_K1')
    _split_row(D, 'c30x4133_K1', dict(bwds_chunks=chunks), chunks, 2)     # a single phi is always reversed bus-major (mode 2)


# ---- the operating point, and shapes with no options set -------------------------------------------------------------------------
@pytest.mark.gpu
def test_operating_point_with_no_options_set(store):
    """case118 x 16 384, (20, 10), three phis, K = 4: the benchmark's pair (lane forward, split backward mode 1)."""
    D = _dataset(store, 'c118x16384')
    C, R = _split_layout(256, 0)
    r = _run(D, train=True)
    _expect(r, fwd_kernel=1, fwd_waves=16, fwd_plane=2, team=1, bwd_kernel=4, dw_mfma=1, bwds_mode=1, bwds_chunks=C, bwds_R=R)
    ri = _run(D, train=True, inputs=True)
    _equal(r, ri, ('grad_params',) + OUTS, 'operating point: with input gradients')
    ri['path'] = r['path']
    _check(D, ri, 'train default c118x16384 (operating point)')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['c200x229', 'c300x8192', 'c14x4133_K30', 'c30x4133_K1', 'c14x229', 'c30x229'])
def test_default_training_shapes(store, name):
    D = _dataset(store, name)
    r = _run(D, train=True)
    assert r['path']['fwd_kernel'] in (1, 2) and r['path']['bwd_kernel'] in (0, 4)
    assert (r['path']['fwd_kernel'] == 2) == (r['path']['bwd_kernel'] == 0)
    _check(D, r, f'train default {name}')
    with torch.no_grad():
        e = _run(D, train=False)
    _check(D, e, f'eval default {name}')


@pytest.mark.gpu
@pytest.mark.parametrize('mapping', [1, 2])
@pytest.mark.parametrize('name', DEEP_GOLDENS)
def test_deep_goldens_under_the_budget(store, name, mapping):
    D = _dataset(store, name)
    with options(train_mapping=mapping):
        r = _run(D, train=True)
    _expect(r, fwd_kernel=mapping, bwd_kernel=4 if mapping == 1 else 0)
    _check(D, r, f'train golden {name} mapping={mapping}')


# ---- input routes on the default training pair ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['route_ragged', 'route_aligned'])
def test_input_routes_are_bitwise_per_call_packing(store, name):
    """Per-call packing, the packed-input cache and a slice of a bound data set.  The ragged slice bu[64:164] leaves real grids of
    the set in the dead lanes of its last group (per-call packing puts copies of grid 163 there): only the live-lane mask keeps
    them out of the weight gradient."""
    D = _dataset(store, name)
    m = D.model
    keys = OUTS + ('grad_params',)
    with options(train_mapping=1):
        m.unbind_dataset()
        m.cache_packed_inputs = False
        ref = _run(D, train=True)
        _expect(ref, fwd_kernel=1, bwd_kernel=4)
        m.cache_packed_inputs = True
        try:
            for _ in range(2):                                   # packs, then reads the cache
                _equal(_run(D, train=True), ref, keys, f'{name}: cache_packed_inputs')
        finally:
            m.cache_packed_inputs = False
        m.bind_dataset(*D.full)
        try:
            hits = m._resident['hits']
            b = _run(D, train=True)
            assert m._resident['hits'] == hits + 1, 'the batch was not read from the bound set'
            _equal(b, ref, keys, f'{name}: bound slice')
        finally:
            m.unbind_dataset()
    _check(D, ref, f'train default pair {name}')


# ---- poisoned workspaces: a kernel that reads a word nothing wrote shows up -----------------------------------------------------
POISON_ROWS = {
    'eval lane': (False, False, dict(fwd_mapping=1)),
    'eval gw': (False, False, dict(fwd_mapping=2, gw_pack=2)),
    'train gw': (True, False, dict(train_mapping=2, gw_pack=1)),
    'train variant 1': (True, False, dict(train_mapping=1, bwd_variant=1)),
    'train variant 2': (True, False, dict(train_mapping=1, bwd_variant=2)),
    'train variant 3': (True, False, dict(train_mapping=1, bwd_variant=3)),
    'train variant 4 fma': (True, False, dict(train_mapping=1, bwd_variant=4, dw_mfma=0)),
    'train split mode 0': (True, False, dict(train_mapping=1, bwd_variant=4, bwds_mode=0, bwds_chunks=12)),
    'train split mode 1': (True, False, dict(train_mapping=1, bwd_variant=4, bwds_mode=1)),
    'train split mode 2': (True, False, dict(train_mapping=1, bwd_variant=4, bwds_mode=2, bwds_chunks=24)),
    'train split inputs': (True, True, dict(train_mapping=1, bwd_variant=4)),
}


@pytest.mark.gpu
@pytest.mark.parametrize('row', list(POISON_ROWS))
def test_poisoned_workspaces_are_bit_identical(store, row, monkeypatch):
    import opf_graph_neural_solver_amd as amd
    D = _dataset(store, 'c118x229')
    train, inputs, opts = POISON_ROWS[row]
    with options(**opts):
        clean = _run(D, train, inputs)
        monkeypatch.setattr(amd.gns, 'POISON_WORKSPACES', True)
        dirty = _run(D, train, inputs)
    assert clean['path'] == dirty['path']
    _equal(dirty, clean, [k for k in OUTS + ('grad_params',) + IGRADS if k in clean], f'poisoned {row}')
    _check(D, clean, f'poison {row} c118x229')
