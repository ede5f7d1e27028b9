"""ctypes binding of libgns_hip.so (include/gns_hip.h).  Fails loudly when the library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

GNS_ERRORS = {1: 'GNS_EINVAL (bad argument)', 2: 'GNS_EUNSUPPORTED (no compiled kernel holds this model: latent_dim <= 20, hidden_dim <= 14, K <= 64; narrower models run zero-padded on the next wider kernel)',
              3: 'GNS_ETOPOLOGY (bus id out of range or not a valid line index)', 4: 'GNS_ESIZE (buffer too small)',
              5: 'GNS_ELAUNCH (HIP launch error)'}
GNS_EUNSUPPORTED, GNS_ETOPOLOGY = 2, 3     # the codes callers tell apart (include/gns_hip.h)


class GnsConfig(ctypes.Structure):
    _fields_ = [('n_bus', ctypes.c_int32), ('n_line', ctypes.c_int32), ('n_gen', ctypes.c_int32), ('K', ctypes.c_int32),
                ('latent_dim', ctypes.c_int32), ('hidden_dim', ctypes.c_int32), ('multiple_phi', ctypes.c_int32),
                ('gamma', ctypes.c_float)]


class PfConfig(ctypes.Structure):
    _fields_ = [('n_bus', ctypes.c_int32), ('n_line', ctypes.c_int32), ('n_gen', ctypes.c_int32), ('max_iter', ctypes.c_int32),
                ('tol', ctypes.c_double)]


class FdConfig(ctypes.Structure):
    _fields_ = [('pf', PfConfig), ('alg', ctypes.c_int32)]


class PfInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_bus', 'n_line', 'n_gen', 'slack', 'n_pv', 'n_pq', 'dim', 'nnz_jac', 'nnz_lu',
                                              'nnz_ybus', 'n_ops', 'n_steps')] + [('lds_bytes', ctypes.c_int64)] + \
                [(n, ctypes.c_int32) for n in ('n_adj_ops', 'n_adj_steps', 'n_factor_steps')]


class FdInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_bus', 'n_line', 'n_gen', 'slack', 'n_pv', 'n_pq', 'nnz_ybus', 'dim_p', 'nnz_lu_p',
                                              'dim_pp', 'nnz_lu_pp', 'factor_p_ops', 'factor_p_steps', 'solve_p_ops',
                                              'solve_p_steps', 'factor_pp_ops', 'factor_pp_steps', 'solve_pp_ops',
                                              'solve_pp_steps')] + [('lds_bytes', ctypes.c_int64)]


def library_path():
    # GNS_LIB selects an alternative build (ablation / A-B timing runs); the default is the shipped library
    return os.environ.get('GNS_LIB') or os.path.join(_HERE, 'libgns_hip.so')


def load_library():
    """Load (once) and type the C-ABI.  Raises OSError with build instructions if the .so is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path) and not os.environ.get('GNS_LIB') and os.environ.get('GNS_NO_AUTOBUILD') != '1':
        # a source-only checkout: build in-tree once (hipcc cross-compiles for gfx950; ~1 minute); never a fallback path
        import shutil
        import subprocess
        if shutil.which('make') and (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
            env = dict(os.environ, PATH=os.environ.get('PATH', '') + ':/opt/rocm/bin')
            subprocess.run(['make', '-C', os.path.join(_HERE, 'csrc'), '-j4'], check=False, env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(path):
        raise OSError(f'{path} not found: build it with `make -C {os.path.join(_HERE, "csrc")}` '
                      '(hipcc --offload-arch=gfx950) or `python -c "import __graft_entry__ as g; g.build()"`. '
                      'There is no CPU fallback for the GNS hot path.')
    lib = ctypes.CDLL(path)
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    cfgp = ctypes.POINTER(GnsConfig)
    lib.gns_version.restype = ctypes.c_char_p
    lib.gns_version.argtypes = []
    lib.gns_param_count.argtypes = [cfgp, ctypes.POINTER(i64)]
    lib.gns_config_supported.argtypes = [cfgp]
    lib.gns_topology_bytes.argtypes = [i32, i32, i32, ctypes.POINTER(sz)]
    lib.gns_prepare_topology.argtypes = [i32, i32, i32, vp, vp, vp, vp, sz]
    lib.gns_workspace_bytes.argtypes = [cfgp, i64, ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.gns_forward.argtypes = [cfgp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, sz, ctypes.c_int, vp]
    lib.gns_uses_packed_inputs.argtypes = [cfgp, i64, ctypes.c_int]
    lib.gns_prepack_bytes.argtypes = [cfgp, i64, ctypes.POINTER(sz)]
    lib.gns_prepack.argtypes = [cfgp, vp, vp, vp, vp, i64, vp, sz, vp]
    lib.gns_backward.argtypes = [cfgp, vp, vp, vp, vp, vp, i64, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_backward_inputs.argtypes = [cfgp, vp, vp, vp, vp, vp, i64, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_adam_step.argtypes = [vp, vp, vp, vp, i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, i64, vp]
    lib.gns_adam_step_dev.argtypes = [vp, vp, vp, vp, i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp]
    lib.gns_team_status_offset.argtypes = [cfgp, i64, ctypes.c_int, ctypes.POINTER(sz)]
    lib.gns_team_status.argtypes = [cfgp, i64, vp, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), vp]
    lib.gns_workspace_bytes_grouped.argtypes = [cfgp, i64, ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.gns_forward_grouped.argtypes = [cfgp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, sz, ctypes.c_int, vp]
    lib.gns_backward_grouped.argtypes = [cfgp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_team_status_offset_grouped.argtypes = [cfgp, i64, ctypes.c_int, ctypes.POINTER(sz)]
    lib.gns_team_status_grouped.argtypes = [cfgp, i64, vp, sz, ctypes.c_int, ctypes.POINTER(ctypes.c_int), vp]
    lib.gns_profile_enable.argtypes = [ctypes.c_int]
    lib.gns_profile_read.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    lib.gns_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.gns_get_option.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    pfcp = ctypes.POINTER(PfConfig)
    lib.gns_pf_topology_bytes.argtypes = [i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(sz)]
    lib.gns_pf_prepare_topology.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, sz]
    lib.gns_pf_topology_info.argtypes = [vp, ctypes.POINTER(PfInfo)]
    lib.gns_pf_topology_slots.argtypes = [i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(i64)]
    lib.gns_pf_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_pf_solve.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_pf_workspace_bytes_set.argtypes = [pfcp, vp, sz, vp, i32, i64, ctypes.POINTER(sz)]
    lib.gns_pf_solve_set.argtypes = [pfcp, vp, vp, sz, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_pf_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_pf_adjoint_set.argtypes = [pfcp, vp, vp, sz, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    fdcp = ctypes.POINTER(FdConfig)
    lib.gns_fd_topology_bytes.argtypes = [i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(sz)]
    lib.gns_fd_prepare_topology.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, sz]
    lib.gns_fd_topology_info.argtypes = [vp, ctypes.POINTER(FdInfo)]
    lib.gns_fd_topology_slots.argtypes = [i32, i32, i32, vp, vp, vp, i32, ctypes.POINTER(i64)]
    lib.gns_fd_workspace_bytes.argtypes = [fdcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_fd_solve.argtypes = [fdcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_fd_workspace_bytes_set.argtypes = [fdcp, vp, sz, vp, i32, i64, ctypes.POINTER(sz)]
    lib.gns_fd_solve_set.argtypes = [fdcp, vp, vp, sz, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dc_lds_bytes.argtypes = [vp, ctypes.POINTER(i64)]
    lib.gns_dc_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_dc_solve.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dc_workspace_bytes_set.argtypes = [pfcp, vp, sz, vp, i32, i64, ctypes.POINTER(sz)]
    lib.gns_dc_solve_set.argtypes = [pfcp, vp, vp, sz, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dc_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dc_adjoint_set.argtypes = [pfcp, vp, vp, sz, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dcn1_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcn1_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_dcn1_screen.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dcn1_adjoint_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcn1_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_dcn1_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dcn2_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcn2_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_dcn2_screen.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_dcn2_adjoint_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcn2_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, i32, i32, ctypes.POINTER(sz)]
    lib.gns_dcn2_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz,
                                     vp]
    lib.gns_dcg1_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcg1_workspace_bytes.argtypes = [pfcp, vp, i64, i32, i32, ctypes.POINTER(sz)]
    lib.gns_dcg1_screen.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp,
                                    vp, vp, sz, vp]
    lib.gns_dcg1_adjoint_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcg1_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, i32, i32, i32, ctypes.POINTER(sz)]
    lib.gns_dcg1_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp,
                                     vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gns_acn1_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acn1_screen.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32] + [vp] * 18 + [vp, sz, vp]
    lib.gns_acn1_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acn1_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32] + [vp] * 19 + [vp, sz, vp]
    lib.gns_acn2_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acn2_screen.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32] + [vp] * 18 + [vp, sz, vp]
    lib.gns_acn2_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acn2_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, i32] + [vp] * 19 + [vp, sz, vp]
    lib.gns_pf_topology_bytes_out_gen.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, ctypes.POINTER(sz)]
    lib.gns_pf_prepare_topology_out_gen.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, vp, sz]
    lib.gns_pf_topology_slots_out_gen.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, ctypes.POINTER(i64)]
    lib.gns_acg1_workspace_bytes.argtypes = [pfcp, vp, sz, vp, i32, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acg1_screen.argtypes = [pfcp, vp, vp, sz, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, i32] + \
        [vp] * 18 + [vp, sz, vp]
    lib.gns_acg1_adjoint_workspace_bytes.argtypes = [pfcp, vp, sz, vp, i32, i64, i32, ctypes.POINTER(sz)]
    lib.gns_acg1_adjoint.argtypes = [pfcp, vp, vp, sz, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, i32] + \
        [vp] * 20 + [vp, sz, vp]
    lib.gns_pfs_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_pfs_evaluate.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i32] + [vp] * 16 + [vp, sz, vp]
    lib.gns_pfs_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_pfs_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, vp, vp, i32] + [vp] * 20 + [vp, sz, vp]
    lib.gns_dcopf_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcopf_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_dcopf_solve.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32] + [vp] * 10 + [vp, sz, vp]
    lib.gns_dcopf_adjoint_lds_bytes.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcopf_adjoint_workspace_bytes.argtypes = [pfcp, vp, i64, ctypes.POINTER(sz)]
    lib.gns_dcopf_adjoint.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32] + [vp] * 22 + [vp, sz, vp]
    lib.gns_dcscopf_lds_bytes.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.gns_dcscopf_workspace_bytes.argtypes = [pfcp, vp, i64, i32, ctypes.POINTER(sz)]
    lib.gns_dcscopf_solve.argtypes = [pfcp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, vp, i32, i32, vp, i32, vp] + [vp] * 12 + [vp, sz, vp]
    for f in (PF_EXPORTS + FD_EXPORTS + DC_EXPORTS + DCN1_EXPORTS + DCN2_EXPORTS + DCN2_ADJOINT_EXPORTS + ACN1_EXPORTS + ACN1_ADJOINT_EXPORTS +
              ACN2_EXPORTS + ACN2_ADJOINT_EXPORTS + DCG1_EXPORTS + DCG1_ADJOINT_EXPORTS + ACG1_EXPORTS + ACG1_ADJOINT_EXPORTS +
              PFS_EXPORTS + DCOPF_EXPORTS + DCOPF_GRAD_EXPORTS + DCSCOPF_EXPORTS):
        getattr(lib, f).restype = ctypes.c_int
    for f in ('gns_profile_enable', 'gns_profile_read', 'gns_param_count', 'gns_config_supported', 'gns_topology_bytes', 'gns_prepare_topology',
              'gns_workspace_bytes', 'gns_forward', 'gns_backward', 'gns_backward_inputs', 'gns_profile_enable', 'gns_profile_read',
              'gns_set_option', 'gns_get_option', 'gns_prepack_bytes', 'gns_prepack', 'gns_uses_packed_inputs', 'gns_adam_step',
              'gns_adam_step_dev', 'gns_team_status', 'gns_team_status_offset', 'gns_workspace_bytes_grouped', 'gns_forward_grouped',
              'gns_backward_grouped', 'gns_team_status_grouped', 'gns_team_status_offset_grouped'):
        getattr(lib, f).restype = ctypes.c_int
    _LIB = lib
    return lib


EXPORTS = ('gns_version', 'gns_param_count', 'gns_config_supported', 'gns_topology_bytes', 'gns_prepare_topology',
           'gns_workspace_bytes', 'gns_forward', 'gns_backward', 'gns_backward_inputs', 'gns_profile_enable', 'gns_profile_read',
           'gns_set_option', 'gns_get_option', 'gns_prepack_bytes', 'gns_prepack', 'gns_uses_packed_inputs', 'gns_adam_step',
           'gns_adam_step_dev', 'gns_team_status', 'gns_team_status_offset', 'gns_workspace_bytes_grouped', 'gns_forward_grouped',
           'gns_backward_grouped', 'gns_team_status_grouped', 'gns_team_status_offset_grouped')


# the power-flow solver's C-ABI (include/gns_powerflow.h)
PF_EXPORTS = ('gns_pf_topology_bytes', 'gns_pf_prepare_topology', 'gns_pf_topology_info', 'gns_pf_workspace_bytes', 'gns_pf_solve',
              'gns_pf_workspace_bytes_set', 'gns_pf_solve_set', 'gns_pf_adjoint', 'gns_pf_adjoint_set', 'gns_pf_topology_slots',
              'gns_pf_topology_bytes_out_gen', 'gns_pf_prepare_topology_out_gen', 'gns_pf_topology_slots_out_gen')
# the fast-decoupled solver's C-ABI (include/gns_powerflow.h, "Fast-decoupled")
FD_EXPORTS = ('gns_fd_topology_bytes', 'gns_fd_prepare_topology', 'gns_fd_topology_info', 'gns_fd_topology_slots',
              'gns_fd_workspace_bytes', 'gns_fd_solve', 'gns_fd_workspace_bytes_set', 'gns_fd_solve_set')
# the DC power flow's C-ABI (include/gns_powerflow.h, "DC power flow"): it runs on the fast-decoupled blob
DC_EXPORTS = ('gns_dc_lds_bytes', 'gns_dc_workspace_bytes', 'gns_dc_solve', 'gns_dc_workspace_bytes_set', 'gns_dc_solve_set',
              'gns_dc_adjoint', 'gns_dc_adjoint_set')
# the DC contingency screen's C-ABI (include/gns_powerflow.h, "DC contingency screening"): on the fast-decoupled blob too
DCN1_EXPORTS = ('gns_dcn1_lds_bytes', 'gns_dcn1_workspace_bytes', 'gns_dcn1_screen', 'gns_dcn1_adjoint_lds_bytes',
                'gns_dcn1_adjoint_workspace_bytes', 'gns_dcn1_adjoint')
# the DC N-2 contingency screen's C-ABI (include/gns_powerflow.h, "DC N-2 contingency screening"): on the fast-decoupled blob too
DCN2_EXPORTS = ('gns_dcn2_lds_bytes', 'gns_dcn2_workspace_bytes', 'gns_dcn2_screen')
# the gradients of the DC N-2 screen (the same section, "Gradients of the N-2 screen")
DCN2_ADJOINT_EXPORTS = ('gns_dcn2_adjoint_lds_bytes', 'gns_dcn2_adjoint_workspace_bytes', 'gns_dcn2_adjoint')
# the AC contingency screen's C-ABI (include/gns_powerflow.h, "AC contingency screening"): on the Newton-Raphson blob
ACN1_EXPORTS = ('gns_acn1_workspace_bytes', 'gns_acn1_screen')
# the gradients of the AC screen (the same section, "Gradients of the AC screen")
ACN1_ADJOINT_EXPORTS = ('gns_acn1_adjoint_workspace_bytes', 'gns_acn1_adjoint')
# the AC N-2 contingency screen's C-ABI (include/gns_powerflow.h, "AC N-2 contingency screening"): on the Newton-Raphson blob too
ACN2_EXPORTS = ('gns_acn2_workspace_bytes', 'gns_acn2_screen')
# the gradients of the AC N-2 screen (include/gns_powerflow.h, "Gradients of the AC N-2 screen")
ACN2_ADJOINT_EXPORTS = ('gns_acn2_adjoint_workspace_bytes', 'gns_acn2_adjoint')
# the DC generator contingency screen's C-ABI (include/gns_powerflow.h, "DC generator contingency screening"): on the fast-decoupled
# blob too
DCG1_EXPORTS = ('gns_dcg1_lds_bytes', 'gns_dcg1_workspace_bytes', 'gns_dcg1_screen')
# the gradients of the DC generator screen (include/gns_powerflow.h, "Gradients of the DC generator screen")
DCG1_ADJOINT_EXPORTS = ('gns_dcg1_adjoint_lds_bytes', 'gns_dcg1_adjoint_workspace_bytes', 'gns_dcg1_adjoint')
# the AC generator contingency screen's C-ABI (include/gns_powerflow.h, "AC generator contingency screening"): on a set of
# Newton-Raphson blobs, each the analysis without one generator row (gns_pf_prepare_topology_out_gen)
ACG1_EXPORTS = ('gns_acg1_workspace_bytes', 'gns_acg1_screen')
# the gradients of the AC generator screen (include/gns_powerflow.h, "Gradients of the AC generator screen")
ACG1_ADJOINT_EXPORTS = ('gns_acg1_adjoint_workspace_bytes', 'gns_acg1_adjoint')
# the solved case of an AC power flow and its gradients (include/gns_powerflow.h, "The solved case"): on the Newton-Raphson blob
PFS_EXPORTS = ('gns_pfs_workspace_bytes', 'gns_pfs_evaluate', 'gns_pfs_adjoint_workspace_bytes', 'gns_pfs_adjoint')
# the DC optimal power flow's C-ABI (include/gns_powerflow.h, "DC optimal power flow"): on the fast-decoupled blob too
DCOPF_EXPORTS = ('gns_dcopf_lds_bytes', 'gns_dcopf_workspace_bytes', 'gns_dcopf_solve')
# the gradients of the DC optimal power flow (include/gns_powerflow.h, "DC optimal power flow: adjoint")
DCOPF_GRAD_EXPORTS = ('gns_dcopf_adjoint_lds_bytes', 'gns_dcopf_adjoint_workspace_bytes', 'gns_dcopf_adjoint')
# the security-constrained DC optimal power flow (include/gns_powerflow.h, "Security-constrained DC optimal power flow")
DCSCOPF_EXPORTS = ('gns_dcscopf_lds_bytes', 'gns_dcscopf_workspace_bytes', 'gns_dcscopf_solve')
# the limits of include/gns_powerflow.h
PF_LDS_MAX_BYTES = 163840
PF_MAX_SLOTS = 65535


def set_option(name: str, value: int) -> None:
    """Process-wide tuning knob of the library (include/gns_hip.h, "configuration")."""
    rc = load_library().gns_set_option(name.encode(), int(value))
    if rc != 0:
        raise ValueError(f'gns_set_option({name!r}, {value}) rejected: {GNS_ERRORS.get(rc, rc)}')


def get_option(name: str) -> int:
    v = ctypes.c_int()
    rc = load_library().gns_get_option(name.encode(), ctypes.byref(v))
    if rc != 0:
        raise ValueError(f'unknown option {name!r}')
    return v.value
