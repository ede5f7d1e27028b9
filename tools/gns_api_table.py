"""The decisions of the GNS host layer (csrc/gns_api.hip) as one deterministic text table, so that two builds can be diffed.

For a fixed list of (case, grids, latent_dim, hidden_dim, K, multiple_phi, save_state) and of option settings: the return code,
forward and backward workspace bytes, gns_uses_packed_inputs and the team-status offset, plain and grouped, one line per model and
batch with a column per save_state.  On a process that
sees a GPU also the "last.*" record after a real forward and backward through the module for each path (without one, those lines
are left out and the sizing lines show what a process without a device is told).

usage: python tools/gns_api_table.py [> table.txt]      (GNS_LIB selects another build of the library)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import opf_graph_neural_solver_amd as amd  # noqa: E402

lib = amd.load_library()
GPU = torch.cuda.is_available()
NCU = torch.cuda.get_device_properties(0).multi_processor_count if GPU else 256
NONE = ctypes.c_size_t(-1).value
OPTIONS = ('train_mapping', 'fwd_mapping', 'gw_pack', 'team', 'bwd_variant', 'dw_mfma', 'bwds_chunks', 'bwds_mode', 'bwds_save', 'fwd_waves', 'fwd_plane')
LAST = ('fwd_kernel', 'fwd_waves', 'fwd_plane', 'team', 'gw_pack', 'bwd_kernel', 'dw_mfma', 'bwds_mode', 'bwds_chunks', 'bwds_R', 'bwd_gw_pack', 'bwds_save')
DEFAULTS = {n: amd.get_option(n) for n in OPTIONS}
# Grids on both sides of every automatic threshold of gw_train_pack (32 groups; 16 for case300), gw_eval_pack (NCU groups; NCU / 4 for
# a case that does not pack) and lane_team (NCU / 4, NCU / 2 and 128 groups), for the CU count of the device
BATCHES = sorted({64, 1024, 1088, 2048, 2112, 4096 - 64, 4096, 16 * NCU, 16 * NCU + 64, 8192, 32 * NCU, 32 * NCU + 64, 64 * NCU - 64,
                  64 * NCU, 16384, 130})
POINTS = ((30, 4096), (118, 1024), (118, 8192), (300, 1088))       # (case, grids) of the lines beyond the main model and the defaults
MODELS = ((20, 10, 4, 1), (10, 10, 4, 1), (20, 14, 4, 1), (7, 5, 4, 1), (20, 10, 4, 0), (10, 10, 30, 0))
SETTINGS = [{}] + [{n: v} for n, vals in (('train_mapping', (1, 2)), ('fwd_mapping', (1, 2)), ('gw_pack', (1, 4)), ('team', (1, 2, 4)),
                                          ('bwd_variant', (1, 2, 3)), ('dw_mfma', (0,)), ('bwds_chunks', (8, 32))) for v in vals]


def use(setting):
    for n, v in dict(DEFAULTS, **setting).items():
        amd.set_option(n, v)


def sizing(case, Bt, d, h, K, multi):
    """One line: for save_state 0, 1 and 2 the plain and the grouped answers."""
    N, E, Gn = amd.synth.CASE_SHAPES[case]
    cfg = amd._lib.GnsConfig(N, E, Gn, K, d, h, multi, 0.9)
    G = (Bt + 63) // 64

    def show(rc, *vals):
        return f'{rc}:' + ','.join('-' if rc else ('none' if v == NONE else str(v)) for v in vals)

    cols = []
    for save in (0, 1, 2):
        fwd, bwd, off = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        rc = lib.gns_workspace_bytes(ctypes.byref(cfg), Bt, save, ctypes.byref(fwd), ctypes.byref(bwd))
        packed = lib.gns_uses_packed_inputs(ctypes.byref(cfg), Bt, save)
        rc_off = lib.gns_team_status_offset(ctypes.byref(cfg), Bt, save, ctypes.byref(off))
        gf, gb, goff = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        grc = lib.gns_workspace_bytes_grouped(ctypes.byref(cfg), G, save, ctypes.byref(gf), ctypes.byref(gb))
        grc_off = lib.gns_team_status_offset_grouped(ctypes.byref(cfg), G, save, ctypes.byref(goff))
        cols.append(f'save{save} {show(rc, fwd.value, bwd.value)} packed={packed} off {show(rc_off, off.value)} '
                    f'grouped {show(grc, gf.value, gb.value)} off {show(grc_off, goff.value)}')
    return f'case{case} Bt={Bt} d={d} h={h} K={K} phi={multi} | ' + ' | '.join(cols)


def last_record():
    return ' '.join(f'{n}={amd.get_option("last." + n)}' for n in LAST)


def real_run(case, Bt, d, h, K, multi, kind):
    """One real call through the module and the path it took.  kind: train, eval, igrad, grouped."""
    torch.manual_seed(0)
    m = amd.GNS(d, h, K, 0.9, bool(multi)).cuda()
    if kind == 'grouped':
        m.topology_check = 'group'
        bu, li, ge, _ = amd.synth.contingency_grids(case, Bt, [1, 4, 9], seed=2, shuffle=True, device='cuda')
    else:
        bu, li, ge = amd.synth.synth_grids(case, Bt, seed=1, device='cuda')
    if kind == 'eval':
        with torch.no_grad():
            out = m(bu, li, ge)
    else:
        if kind == 'igrad':
            bu.requires_grad_(True)
        out = m(bu, li, ge)
        out[2].mean().backward()
    torch.cuda.synchronize()
    m.check_status()
    return f'finite={int(bool(torch.isfinite(out[2]).all()))} {last_record()}'


def main():
    print(f'# device: {"gpu" if GPU else "none"} ncu={NCU if GPU else 0} defaults: ' + ' '.join(f'{n}={v}' for n, v in DEFAULTS.items()))
    print('# sizing (rc:forward bytes,backward bytes; packed inputs; rc:team status offset; the same of the grouped calls), default options')
    for case in (14, 30, 118, 300):
        for Bt in BATCHES:
            print(sizing(case, Bt, *MODELS[0]))
    for model in MODELS[1:]:
        for case, Bt in POINTS:
            print(sizing(case, Bt, *model))
    print('# sizing, one option changed')
    for setting in SETTINGS[1:]:
        use(setting)
        for case, Bt in POINTS:
            print(' '.join(f'{n}={v}' for n, v in setting.items()) + ' | ' + sizing(case, Bt, *MODELS[0]))
    use({})
    if not GPU:
        return
    print('# the path real calls took (last.*)')
    for case in (14, 30, 118, 300):
        for Bt in (130, 2048, 2112, 16384):
            for kind in ('train', 'eval'):
                print(f'case{case} Bt={Bt} d=20 h=10 K=4 phi=1 {kind} | {real_run(case, Bt, 20, 10, 4, 1, kind)}')
    for (d, h, K, multi) in MODELS[1:]:
        for kind in ('train', 'eval'):
            print(f'case30 Bt=4096 d={d} h={h} K={K} phi={multi} {kind} | {real_run(30, 4096, d, h, K, multi, kind)}')
    for case, Bt in ((14, 130), (118, 4096)):
        print(f'case{case} Bt={Bt} d=20 h=10 K=4 phi=1 igrad | {real_run(case, Bt, 20, 10, 4, 1, "igrad")}')
        print(f'case{case} Bt={Bt} d=20 h=10 K=4 phi=1 grouped | {real_run(case, Bt, 20, 10, 4, 1, "grouped")}')
    for setting in SETTINGS[1:] + [{'bwd_variant': 2, 'team': 2}, {'bwds_mode': 0}, {'bwds_mode': 2}]:
        use(setting)
        for case, Bt in ((30, 4096), (118, 1024)):
            for kind in ('train', 'eval'):
                print(' '.join(f'{n}={v}' for n, v in setting.items()) + f' | case{case} Bt={Bt} d=20 h=10 K=4 phi=1 {kind} | '
                      + real_run(case, Bt, 20, 10, 4, 1, kind))
    use({})


if __name__ == '__main__':
    main()
