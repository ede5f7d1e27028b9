"""The GNS C-ABI's argument checking and option table, pinned on a process that sees no device.

Every exported GNS call is made with a null ``cfg``, each required pointer null, ``Bt <= 0``, malformed configs, unsupported
widths, ``K = 65``, short workspaces, the grouped limits, and pairs of violations (so that the precedence between ``GNS_EINVAL``,
``GNS_EUNSUPPORTED`` and ``GNS_ESIZE`` is pinned); every option is set, read, pushed past its range and seeded from the
environment.  The expected values were written down from the library's behaviour before its host layer was folded; where the
header's prose and the behaviour disagree the behaviour is what is pinned (``gns_workspace_bytes`` and the team-status calls accept
``K = 65``, which the launches refuse).

All calls return before the first kernel launch: no workspace handed in is ever large enough to pass a size check, and the pointers
are the address of one small host buffer that the host code never reads.  Without a device the per-device state reports "nothing
ready", so the checks behind it are reached on their ``GNS_EUNSUPPORTED`` side only.  The calls run in child processes with every
device hidden (this file, run as a script, is the child), so the answers are the same on a machine with a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED, ESIZE = 0, 1, 2, 4
NO_DEVICE = dict(HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', GNS_NO_AUTOBUILD='1')

# case118, d = 20, h = 10, K = 4, three phi
GOOD = dict(n_bus=118, n_line=186, n_gen=54, K=4, latent_dim=20, hidden_dim=10, multiple_phi=1, gamma=0.9)
CFGS = {'good': {}, 'null': None, 'K0': dict(K=0), 'phi2': dict(multiple_phi=2), 'd24': dict(latent_dim=24), 'h15': dict(hidden_dim=15),
        'K65': dict(K=65), 'K0+d24': dict(K=0, latent_dim=24), 'd7h5': dict(latent_dim=7, hidden_dim=5), 'h14': dict(hidden_dim=14),
        'nbus0': dict(n_bus=0), 'd0': dict(latent_dim=0)}
BT = 16384
P = 'P'        # a non-null pointer (inputs: never read by the host; outputs: a few bytes are written)
# the arguments after cfg, by name, with a value that passes every check except the workspace sizes (16 bytes: always short)
SPECS = {
    'gns_param_count': [('count', P)],
    'gns_config_supported': [],
    'gns_workspace_bytes': [('Bt', BT), ('save', 1), ('fwd', P), ('bwd', P)],
    'gns_uses_packed_inputs': [('Bt', BT), ('save', 1)],
    'gns_team_status_offset': [('Bt', BT), ('save', 1), ('offset', P)],
    'gns_team_status': [('Bt', BT), ('ws', P), ('ws_bytes', 16), ('save', 1), ('status', P), ('stream', None)],
    'gns_prepack_bytes': [('Bt', BT), ('bytes', P)],
    'gns_prepack': [('topo', P), ('buses', P), ('lines', P), ('gens', P), ('Bt', BT), ('packed', P), ('packed_bytes', 16), ('stream', None)],
    'gns_forward': [('topo', P), ('params', P), ('buses', P), ('lines', P), ('gens', P), ('Bt', BT), ('packed', None), ('v', P),
                    ('theta', P), ('total', P), ('last', P), ('ws', P), ('ws_bytes', 16), ('save', 1), ('stream', None)],
    'gns_backward': [('topo', P), ('params', P), ('buses', P), ('lines', P), ('gens', P), ('Bt', BT), ('packed', None), ('fws', P),
                     ('fws_bytes', 16), ('g_total', P), ('g_last', P), ('g_v', P), ('g_theta', P), ('grad', P), ('bws', P),
                     ('bws_bytes', 16), ('stream', None)],
    'gns_backward_inputs': [('topo', P), ('params', P), ('buses', P), ('lines', P), ('gens', P), ('Bt', BT), ('packed', None), ('fws', P),
                            ('fws_bytes', 16), ('g_total', P), ('g_last', P), ('g_v', P), ('g_theta', P), ('grad', P), ('g_buses', P),
                            ('g_lines', P), ('g_gens', P), ('bws', P), ('bws_bytes', 16), ('stream', None)],
    'gns_workspace_bytes_grouped': [('G', 256), ('save', 1), ('fwd', P), ('bwd', P)],
    'gns_forward_grouped': [('topo', P), ('group_topo', P), ('slot_grid', P), ('G', 256), ('params', P), ('buses', P), ('lines', P),
                            ('gens', P), ('Bt', BT), ('v', P), ('theta', P), ('total', P), ('last', P), ('ws', P), ('ws_bytes', 16),
                            ('save', 1), ('stream', None)],
    'gns_backward_grouped': [('topo', P), ('group_topo', P), ('slot_grid', P), ('G', 256), ('params', P), ('buses', P), ('lines', P),
                             ('gens', P), ('Bt', BT), ('fws', P), ('fws_bytes', 16), ('g_total', P), ('g_last', P), ('g_v', P),
                             ('g_theta', P), ('grad', P), ('bws', P), ('bws_bytes', 16), ('stream', None)],
    'gns_team_status_offset_grouped': [('G', 256), ('save', 1), ('offset', P)],
    'gns_team_status_grouped': [('G', 256), ('ws', P), ('ws_bytes', 16), ('save', 1), ('status', P), ('stream', None)],
}
GROUPED = ('gns_workspace_bytes_grouped', 'gns_forward_grouped', 'gns_backward_grouped', 'gns_team_status_offset_grouped',
           'gns_team_status_grouped')
# pointers a call accepts as NULL (everything else that is a pointer is required)
OPTIONAL = {'gns_workspace_bytes': ('fwd', 'bwd'), 'gns_workspace_bytes_grouped': ('fwd', 'bwd'),
            'gns_backward': ('buses', 'lines', 'gens', 'g_total', 'g_last', 'g_v', 'g_theta'),
            'gns_backward_inputs': ('g_total', 'g_last', 'g_v', 'g_theta', 'grad', 'g_buses', 'g_lines', 'g_gens'),
            'gns_backward_grouped': ('buses', 'lines', 'gens', 'g_total', 'g_last', 'g_v', 'g_theta')}


def _cases():
    """(function, config key, {argument: value}) of every pinned call."""
    out = []
    for fn, spec in SPECS.items():
        for key in CFGS:
            out.append((fn, key, {}))
        for name, default in spec:
            if default == P:
                out.append((fn, 'good', {name: None}))
                out.append((fn, 'd24', {name: None}))          # two violations: which one answers
                out.append((fn, 'K0', {name: None}))
        names = [n for n, _ in spec]
        for count in ('Bt', 'G'):
            if count in names:
                for bad in (0, -1):
                    out.append((fn, 'good', {count: bad}))
                out.append((fn, 'd24', {count: 0}))
                out.append((fn, 'K65', {count: 0}))
                out.append((fn, 'null', {count: 0}))
        if 'save' in names:
            for save in (0, 2):
                for key in ('good', 'K65', 'd24', 'h14', 'd7h5'):
                    out.append((fn, key, {'save': save}))
            out.append((fn, 'good', {'save': 2, 'Bt' if 'Bt' in names else 'G': 0}))
        if 'Bt' in names:
            for bt in (1, 64, 1024, 2048, 4096, 8192):
                out.append((fn, 'good', {'Bt': bt}))
    for fn in GROUPED:
        out += [(fn, 'good', {'G': (1 << 24) + 1}), (fn, 'good', {'G': 1 << 24}), (fn, 'd24', {'G': (1 << 24) + 1})]
    for fn in ('gns_forward_grouped', 'gns_backward_grouped'):
        out += [(fn, 'good', {'Bt': 64 * 256 + 1}), (fn, 'good', {'Bt': 64 * 256 + 1, 'G': 0}), (fn, 'good', {'Bt': 0, 'topo': None})]
    return out


def _case_id(fn, key, over):
    return ' '.join([fn, key] + [f'{k}={"NULL" if v is None else v}' for k, v in over.items()])


def _call(lib, amd, scratch, fn, key, over):
    cfg = None if CFGS[key] is None else ctypes.byref(amd._lib.GnsConfig(**dict(GOOD, **CFGS[key])))
    f = getattr(lib, fn)
    args = []
    for (name, default), ctype in zip(SPECS[fn], f.argtypes[1:]):
        v = over.get(name, default)
        args.append(ctypes.cast(scratch, ctype) if v == P else v)
    return f(cfg, *args)


def _short_workspaces(lib, amd, scratch):
    """gns_forward / gns_backward with workspaces one byte short of what gns_workspace_bytes asks for (and the forward saved for input
    gradients at exactly the lane-per-grid layout: its mark does not fit)."""
    out = {}
    fwd_b, bwd_b = ctypes.c_size_t(), ctypes.c_size_t()
    for key in ('good', 'h14', 'd7h5'):
        cfg = ctypes.byref(amd._lib.GnsConfig(**dict(GOOD, **CFGS[key])))
        for save in (0, 1):
            rc = lib.gns_workspace_bytes(cfg, BT, save, ctypes.byref(fwd_b), ctypes.byref(bwd_b))
            out[f'sizes {key} save={save}'] = [rc, fwd_b.value, bwd_b.value]
            out[f'gns_forward {key} save={save} ws=fwd-1'] = _call(lib, amd, scratch, 'gns_forward', key, dict(save=save, ws_bytes=fwd_b.value - 1))
            out[f'gns_forward {key} save={save} ws=fwd-1 topo=NULL'] = _call(lib, amd, scratch, 'gns_forward', key,
                                                                           dict(save=save, ws_bytes=fwd_b.value - 1, topo=None))
        # (save = 1 sizes from here on)
        out[f'gns_forward {key} save=2 ws=fwd(save=1)'] = _call(lib, amd, scratch, 'gns_forward', key, dict(save=2, ws_bytes=fwd_b.value))
        out[f'gns_forward {key} save=2 ws=fwd(save=1)+256'] = _call(lib, amd, scratch, 'gns_forward', key, dict(save=2, ws_bytes=fwd_b.value + 256))
        out[f'gns_backward {key} fws=fwd-1'] = _call(lib, amd, scratch, 'gns_backward', key, dict(fws_bytes=fwd_b.value - 1, bws_bytes=bwd_b.value))
        out[f'gns_backward {key} bws=bwd-1'] = _call(lib, amd, scratch, 'gns_backward', key, dict(fws_bytes=fwd_b.value, bws_bytes=bwd_b.value - 1))
        out[f'gns_backward {key} bws=bwd-1 grad=NULL'] = _call(lib, amd, scratch, 'gns_backward', key,
                                                             dict(fws_bytes=fwd_b.value, bws_bytes=bwd_b.value - 1, grad=None))
        out[f'gns_backward_inputs {key} fws=fwd+256'] = _call(lib, amd, scratch, 'gns_backward_inputs', key,
                                                            dict(fws_bytes=fwd_b.value + 256, bws_bytes=bwd_b.value))
    nbytes = ctypes.c_size_t()
    cfg = ctypes.byref(amd._lib.GnsConfig(**GOOD))
    out['sizes prepack'] = [lib.gns_prepack_bytes(cfg, BT, ctypes.byref(nbytes)), nbytes.value]
    out['gns_prepack good packed=bytes-1'] = _call(lib, amd, scratch, 'gns_prepack', 'good', dict(packed_bytes=nbytes.value - 1))
    out['gns_prepack good packed=bytes-1 topo=NULL'] = _call(lib, amd, scratch, 'gns_prepack', 'good', dict(packed_bytes=nbytes.value - 1, topo=None))
    return out


def _misc(lib, scratch):
    """The calls without a config: Adam and the profiling switches (argument checks only)."""
    p = ctypes.addressof(scratch)
    out = {}
    for i in range(4):
        a = [p] * 4
        a[i] = None
        out[f'gns_adam_step null[{i}]'] = lib.gns_adam_step(*a, 10, 1e-3, 0.9, 0.999, 1e-8, 1, None)
        out[f'gns_adam_step_dev null[{i}]'] = lib.gns_adam_step_dev(*a, 10, 1e-3, 0.9, 0.999, 1e-8, p, None)
    out['gns_adam_step n=0'] = lib.gns_adam_step(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 1, None)
    out['gns_adam_step step=0'] = lib.gns_adam_step(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, 0, None)
    out['gns_adam_step_dev n=0'] = lib.gns_adam_step_dev(p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, p, None)
    out['gns_adam_step_dev state=NULL'] = lib.gns_adam_step_dev(p, p, p, p, 10, 1e-3, 0.9, 0.999, 1e-8, None, None)
    out['gns_profile_enable -1'] = lib.gns_profile_enable(-1)
    out['gns_profile_enable 0'] = lib.gns_profile_enable(0)
    out['gns_profile_read ms=NULL'] = lib.gns_profile_read(0, None, ctypes.cast(p, ctypes.POINTER(ctypes.c_int)))
    out['gns_profile_read launches=NULL'] = lib.gns_profile_read(1, ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), None)
    return out


# ---- options ---------------------------------------------------------------------------------------------------------------------
# name: (default, values accepted, values refused); what is stored is what was set, except dw_mfma (any integer, stored as 0 / 1)
OPTIONS = {
    'fwd_mapping': (0, (0, 1, 2), (-1, 3)),
    'train_mapping': (0, (0, 1, 2), (-1, 3)),
    'bwd_variant': (4, (1, 2, 3, 4), (0, 5)),
    'gw_pack': (0, (0, 1, 16), (-1, 17)),
    'fwd_waves': (16, (1, 2, 4, 8, 16), (0, -1, 3, 12, 32)),
    'fwd_plane': (2, (0, 1, 2), (-1, 3)),
    'dw_mfma': (1, (0, 1, 5, -3), ()),
    'team': (0, (0, 1, 2, 3, 4), (-1, 5)),
    'bwds_mode': (1, (0, 1, 2), (-1, 3)),
    'bwds_chunks': (0, (0, 1, 2, 4, 8, 12, 16, 24, 32), (-1, 3, 6, 48, 64)),
}
LAST = ('fwd_kernel', 'fwd_waves', 'fwd_plane', 'team', 'gw_pack', 'bwd_kernel', 'dw_mfma', 'bwds_mode', 'bwds_chunks', 'bwds_R', 'bwd_gw_pack')
# environment spellings: {variable: value} -> the options that differ from their defaults afterwards
ENVIRONMENTS = [
    (dict(GNS_TEAM='3', GNS_FWD_MAPPING='lane', GNS_GW_PACK='16', GNS_FWD_WAVES='8', GNS_FWD_PLANE='1', GNS_DW_MFMA='0', GNS_BWD_VARIANT='2',
          GNS_BWDS_MODE='2', GNS_BWDS_CHUNKS='12', GNS_TRAIN_MAPPING='lds'),
     dict(team=3, fwd_mapping=1, gw_pack=16, fwd_waves=8, fwd_plane=1, dw_mfma=0, bwd_variant=2, bwds_mode=2, bwds_chunks=12, train_mapping=2)),
    # out of range: ignored, the defaults stay
    (dict(GNS_TEAM='5', GNS_FWD_MAPPING='2', GNS_GW_PACK='17', GNS_FWD_WAVES='3', GNS_BWD_VARIANT='5', GNS_BWDS_MODE='3', GNS_BWDS_CHUNKS='3',
          GNS_TRAIN_MAPPING='1'), {}),
    (dict(GNS_TEAM='-1', GNS_GW_PACK='0', GNS_FWD_WAVES='32', GNS_BWD_VARIANT='0', GNS_BWDS_MODE='-1', GNS_BWDS_CHUNKS='64'), {}),
    # the two mappings by word only, the plane and the engine by their first character
    (dict(GNS_FWD_MAPPING='lds', GNS_TRAIN_MAPPING='lane', GNS_FWD_PLANE='0x', GNS_DW_MFMA='no'), dict(fwd_mapping=2, train_mapping=1, fwd_plane=0)),
    (dict(GNS_FWD_MAPPING='LDS', GNS_TRAIN_MAPPING='auto', GNS_FWD_PLANE='12', GNS_DW_MFMA='00', GNS_TEAM='4', GNS_BWDS_CHUNKS='0'),
     dict(fwd_plane=1, dw_mfma=0, team=4)),
    (dict(GNS_FWD_PLANE='plane', GNS_DW_MFMA='1', GNS_FWD_WAVES='1', GNS_BWD_VARIANT='1', GNS_BWDS_MODE='0', GNS_GW_PACK='1'),
     dict(fwd_waves=1, bwd_variant=1, bwds_mode=0, gw_pack=1)),
]


def _options(lib):
    v = ctypes.c_int()

    def get(name):
        rc = lib.gns_get_option(name.encode(), ctypes.byref(v))
        return [rc, v.value]

    out = {'defaults': {n: get(n) for n in OPTIONS}, 'last': {n: get('last.' + n) for n in LAST}}
    out['set last'] = {n: lib.gns_set_option(('last.' + n).encode(), 1) for n in LAST}
    out['last after set'] = {n: get('last.' + n) for n in LAST}
    for name, (default, good, bad) in OPTIONS.items():
        rows = []
        for val in good + bad:
            rows.append([val, lib.gns_set_option(name.encode(), val)] + get(name))
        lib.gns_set_option(name.encode(), default)
        out['set ' + name] = rows
    out['others untouched'] = {n: get(n) for n in OPTIONS}
    out['unknown'] = [lib.gns_set_option(b'nothing', 1), get('nothing')[0], get('last.nothing')[0], get('')[0], lib.gns_set_option(b'', 0),
                      lib.gns_set_option(b'Team', 1), lib.gns_set_option(b'team ', 1)]
    out['null'] = [lib.gns_set_option(None, 1), lib.gns_get_option(None, ctypes.byref(v)), lib.gns_get_option(b'team', None)]
    return out


def _child(what):
    sys.path.insert(0, ROOT)
    import opf_graph_neural_solver_amd as amd
    lib = amd.load_library()
    scratch = ctypes.create_string_buffer(64)
    if what == 'calls':
        out = {_case_id(*c): _call(lib, amd, scratch, *c) for c in _cases()}
        out.update(_short_workspaces(lib, amd, scratch))
        out.update(_misc(lib, scratch))
    elif what == 'options':
        out = _options(lib)
    else:                                  # the options as the environment seeded them
        out = {n: amd.get_option(n) for n in OPTIONS}
    print('RESULT ' + json.dumps(out))


def _run_child(what, env=None):
    keep = {k: v for k, v in os.environ.items() if not k.startswith('GNS_') or k == 'GNS_LIB'}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(keep, **NO_DEVICE, **(env or {})))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    assert r.returncode == 0 and len(lines) == 1, r.stdout + r.stderr
    return json.loads(lines[0][len('RESULT '):])


@pytest.fixture(scope='module')
def calls():
    return _run_child('calls')


@pytest.fixture(scope='module')
def options():
    return _run_child('options')


def _expected(fn, key, over):
    """The code the library returns for a pinned call on a process without a device, as a rule per entry point (in the order the
    library checks) - written down from its behaviour, see the module docstring."""
    spec = dict(SPECS[fn])
    a = dict(spec, **over)
    cfg = None if CFGS[key] is None else dict(GOOD, **CFGS[key])
    null = [n for n, d in spec.items() if d == P and a[n] is None and n not in OPTIONAL.get(fn, ())]
    if fn == 'gns_param_count':                      # (no range checks on the counts, none on multiple_phi)
        return EINVAL if cfg is None or null or cfg['K'] <= 0 or cfg['latent_dim'] <= 0 or cfg['hidden_dim'] <= 0 else OK
    bad_cfg = cfg is None or min(cfg['n_bus'], cfg['n_line'], cfg['K'], cfg['latent_dim'], cfg['hidden_dim']) <= 0 or cfg['n_gen'] < 0 \
        or cfg['multiple_phi'] not in (0, 1)
    wide = cfg is not None and (cfg['latent_dim'] > 20 or cfg['hidden_dim'] > 14)
    deep = cfg is not None and cfg['K'] > 64
    if fn == 'gns_config_supported':
        return 0 if bad_cfg or wide or deep else 1
    if fn == 'gns_uses_packed_inputs':               # (without a device nothing runs on the grid-per-workgroup kernels)
        return 0 if bad_cfg or a['Bt'] <= 0 or wide else 1
    if fn in GROUPED:                                # the config, the group count, the widths and K, then the split backward: not ready
        if bad_cfg or a['G'] <= 0 or a['G'] > 1 << 24:
            return EINVAL
        return EUNSUPPORTED
    if bad_cfg:
        return EINVAL
    if fn in ('gns_prepack_bytes', 'gns_prepack'):   # (any width: the input layout does not depend on it)
        if a['Bt'] <= 0 or 'bytes' in null:
            return EINVAL
        if fn == 'gns_prepack_bytes':
            return OK
        return EINVAL if null else ESIZE
    if null or a['Bt'] <= 0:
        return EINVAL
    if wide:
        return EUNSUPPORTED
    if fn == 'gns_workspace_bytes':                  # K is not capped here; save_state 2 needs the split backward
        return EUNSUPPORTED if a['save'] == 2 else OK
    if fn in ('gns_team_status_offset', 'gns_team_status'):      # K is not capped here either; no CUs, no teams: nothing to read
        return OK
    if deep:
        return EUNSUPPORTED
    if fn == 'gns_backward_inputs':
        return EUNSUPPORTED
    return ESIZE                                     # gns_forward, gns_backward: 16-byte workspaces


@pytest.mark.parametrize('case', _cases(), ids=lambda c: _case_id(*c))
def test_return_code(case, calls):
    assert calls[_case_id(*case)] == _expected(*case)


def test_the_rules_reproduce_the_figures_checked_by_hand():
    """The cases the issue lists (case118, d = 20, h = 10, K = 4, three phi, 16 384 grids), as literals."""
    assert [_expected('gns_forward', 'good', {'save': s}) for s in (0, 1, 2)] == [ESIZE] * 3
    assert _expected('gns_forward', 'good', {'topo': None}) == EINVAL
    assert _expected('gns_forward', 'K65', {}) == EUNSUPPORTED and _expected('gns_forward', 'd24', {}) == EUNSUPPORTED
    assert _expected('gns_backward', 'good', {}) == ESIZE
    assert _expected('gns_backward_inputs', 'good', {}) == EUNSUPPORTED and _expected('gns_workspace_bytes_grouped', 'good', {}) == EUNSUPPORTED
    assert _expected('gns_workspace_bytes', 'good', {'save': 2}) == EUNSUPPORTED
    assert _expected('gns_workspace_bytes', 'K65', {}) == OK and _expected('gns_team_status', 'K65', {}) == OK
    assert _expected('gns_forward', 'd24', {'topo': None}) == EINVAL and _expected('gns_forward_grouped', 'd24', {'G': 0}) == EINVAL
    assert _expected('gns_forward_grouped', 'good', {'Bt': 64 * 256 + 1}) == EUNSUPPORTED


def test_short_workspaces_and_precedence_of_the_size_checks(calls):
    for key in ('good', 'h14', 'd7h5'):
        for save in (0, 1):
            rc, fwd, bwd = calls[f'sizes {key} save={save}']
            assert rc == OK and fwd > 16 and bwd > 16
            assert calls[f'gns_forward {key} save={save} ws=fwd-1'] == ESIZE
            assert calls[f'gns_forward {key} save={save} ws=fwd-1 topo=NULL'] == EINVAL
        # saved for input gradients: the size is compared (twice: the layout, then the mark behind it) before the split backward is looked for
        assert calls[f'gns_forward {key} save=2 ws=fwd(save=1)'] == ESIZE
        assert calls[f'gns_forward {key} save=2 ws=fwd(save=1)+256'] == EUNSUPPORTED
        assert calls[f'gns_backward {key} fws=fwd-1'] == ESIZE
        assert calls[f'gns_backward {key} bws=bwd-1'] == ESIZE
        assert calls[f'gns_backward {key} bws=bwd-1 grad=NULL'] == EINVAL
        assert calls[f'gns_backward_inputs {key} fws=fwd+256'] == EUNSUPPORTED
    # the sizes themselves (lane-per-grid forward, persistent backward without teams: what a process without a device is told)
    assert calls['sizes good save=0'] == [OK, 659932928, 383249664]
    assert calls['sizes good save=1'] == [OK, 2330314496, 383249664]
    assert calls['sizes h14 save=1'] == [OK, 2701574144, 437342464]
    assert calls['sizes d7h5 save=1'] == [OK, 2020954112, 297582848]        # (a narrow model is sized as the (10, 10) kernel it runs on)
    rc, nbytes = calls['sizes prepack']
    assert rc == OK and nbytes > 16
    assert calls['gns_prepack good packed=bytes-1'] == ESIZE
    assert calls['gns_prepack good packed=bytes-1 topo=NULL'] == EINVAL


def test_calls_without_a_config(calls):
    for name, rc in calls.items():
        if name.startswith(('gns_adam_step', 'gns_profile_read')) or name == 'gns_profile_enable -1':
            assert rc == EINVAL, name
    assert calls['gns_profile_enable 0'] == OK


def test_every_option_round_trips_and_refuses_one_beyond_its_range(options):
    assert options['defaults'] == {n: [OK, d] for n, (d, _, _) in OPTIONS.items()}
    for name, (default, good, bad) in OPTIONS.items():
        rows = options['set ' + name]
        stored = default
        for (val, rc, get_rc, got), accept in zip(rows, [True] * len(good) + [False] * len(bad)):
            assert val in (good if accept else bad) and get_rc == OK
            assert rc == (OK if accept else EINVAL), (name, val)
            if accept:
                stored = (1 if val else 0) if name == 'dw_mfma' else val
            assert got == stored, (name, val)                     # a refused value leaves the option as it was
    assert options['others untouched'] == options['defaults']
    assert options['unknown'] == [EINVAL] * 7
    assert options['null'] == [EINVAL] * 3


def test_last_names_read_and_refuse_writes(options):
    assert options['last'] == {n: [OK, -1] for n in LAST}
    assert options['set last'] == {n: EINVAL for n in LAST}
    assert options['last after set'] == options['last']


@pytest.mark.parametrize('env,changed', ENVIRONMENTS, ids=[' '.join(f'{k[4:]}={v}' for k, v in e.items()) for e, _ in ENVIRONMENTS])
def test_environment_spellings(env, changed):
    want = {n: d for n, (d, _, _) in OPTIONS.items()}
    want.update(changed)
    assert _run_child('environment', env) == want


if __name__ == '__main__':
    _child(sys.argv[1])
