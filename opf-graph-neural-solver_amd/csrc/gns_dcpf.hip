// Batched DC power flow and its adjoint (include/gns_powerflow.h, "DC power flow"): one wave per grid on the fast-decoupled blob.
// Bbus (makeBdc) has the pattern of B', so it is built from the line rows straight into the B' factor slots, factored once by the
// blob's B' factorisation program and solved once by its B' solve program.  The factor, the right-hand side and one bus vector
// live in LDS; there is no Y-bus and no workspace.  The matrix is symmetric, so the adjoint is a second solve with the same programs.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"

namespace {

__device__ inline double dc_wave_sum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// The not-solved outputs of grid g
__device__ __forceinline__ void dc_not_solved(const int g, const int N, const int E, double* th_out, double* fl_out, double* sp_out,
                                              uint8_t* conv_out) {
  const double nan = __builtin_nan("");
  for (int i = threadIdx.x; i < N; i += PF_THREADS) th_out[(size_t)g * N + i] = nan;
  for (int e = threadIdx.x; e < E; e += PF_THREADS) fl_out[(size_t)g * E + e] = nan;
  if (threadIdx.x == 0) { sp_out[g] = nan; conv_out[g] = 0; }
}

// The solve of grid g on the FD blob at topo: the body of both solve kernels
__device__ __forceinline__ void dc_solve_grid(const int32_t* topo, const int g, const float* buses, const float* lines,
                                              const float* gens, double* th_out, double* fl_out, double* sp_out, uint8_t* conv_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], slack = topo[FH_SLACK], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[FH_Y_PTR];
  const int32_t* y_col = topo + topo[FH_Y_COL];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int32_t* bslot = topo + topo[FH_BSLOT];

  double* F = lds;                       // [nnz1] factor of Bbus[r, r], then [d1] right-hand side / theta_r
  double* rhs = F + nnz1;
  double* th = rhs + d1;                 // [N] theta by bus
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;

  for (int s = lane; s < nnz1; s += PF_THREADS) F[s] = 0.0;
  __syncthreads();
  dc_matrix(N, y_ptr, st_ptr, st, bslot, line, F, lane);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_F1], topo + topo[FH_STEP_F1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_F1]), F, lane);
  bool bad = pf_bad_pivot(d1, topo + topo[FH_PIVOT1], F, lane);

  for (int i = lane; i < N; i += PF_THREADS)
    if (p_idx[i] >= 0) rhs[p_idx[i]] = dc_injection(i, y_diag, st_ptr, st, gen_ptr, gen_idx, bus, line, gen);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), F, lane);
  for (int i = lane; i < N; i += PF_THREADS) {
    const double x = p_idx[i] >= 0 ? rhs[p_idx[i]] : 0.0;
    th[i] = x;
    bad |= !pf_finite(x);
  }
  __syncthreads();
  if (__ballot(bad)) { dc_not_solved(g, N, E, th_out, fl_out, sp_out, conv_out); return; }

  for (int i = lane; i < N; i += PF_THREADS) th_out[(size_t)g * N + i] = th[i];
  for (int e = lane; e < E; e += PF_THREADS) {
    int f, t;
    double flow = __builtin_nan("");
    if (pf_line_ends(line, e, N, f, t)) {
      const double b = dc_line_b(line, e);
      flow = b * (th[f] - th[t]) + (0.0 - b * (double)line[e * 7 + 6]);
    }
    fl_out[(size_t)g * E + e] = flow;
  }
  // slack_p = Bbus[slack, :] theta - P_slack: the lanes share the slack's row, summed in a fixed order
  double acc = 0.0;
  for (int p = y_ptr[slack] + lane; p < y_ptr[slack + 1]; p += PF_THREADS) acc += dc_b_entry(p, st_ptr, st, line) * th[y_col[p]];
  acc = dc_wave_sum(acc);
  if (lane == 0) {
    sp_out[g] = acc - dc_injection(slack, y_diag, st_ptr, st, gen_ptr, gen_idx, bus, line, gen);
    conv_out[g] = 1;
  }
}

__global__ __launch_bounds__(PF_THREADS) void gns_dc_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                            const float* __restrict__ lines, const float* __restrict__ gens,
                                                            double* __restrict__ th_out, double* __restrict__ fl_out,
                                                            double* __restrict__ sp_out, uint8_t* __restrict__ conv_out) {
  dc_solve_grid(topo, blockIdx.x, buses, lines, gens, th_out, fl_out, sp_out, conv_out);
}

// A batch over a set of FD blobs (gns_dc_solve_set): the grid, order and blob checks of gns_fd_set_kernel, with DC's LDS image
__global__ __launch_bounds__(PF_THREADS) void gns_dc_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                const int32_t* __restrict__ grid_off, const int32_t* __restrict__ order,
                                                                int64_t Bt, int N, int E, int Gn, int64_t lds_bytes,
                                                                const float* __restrict__ buses, const float* __restrict__ lines,
                                                                const float* __restrict__ gens, double* __restrict__ th_out,
                                                                double* __restrict__ fl_out, double* __restrict__ sp_out,
                                                                uint8_t* __restrict__ conv_out) {
  const int64_t g64 = pf_set_grid(order);
  if (g64 < 0 || g64 >= Bt) return;                             // not a grid of this batch: nothing to write
  const int g = (int)g64;
  const int32_t* topo;
  if (!pf_set_member<DcBlobKind>(set, set_words, grid_off[g], N, E, Gn, lds_bytes, INT32_MAX, topo)) {
    dc_not_solved(g, N, E, th_out, fl_out, sp_out, conv_out);
    return;
  }
  dc_solve_grid(topo, g, buses, lines, gens, th_out, fl_out, sp_out, conv_out);
}

// ---- the adjoint (gns_dc_adjoint): theta_r = Bbus[r, r]^-1 P_r with a symmetric matrix, so lambda_r = Bbus[r, r]^-1 g_r on the same
// factor with the same solve program (include/gns_powerflow.h, "DC power flow", gradients).

// Whether grid g's incoming gradients are all exactly zero (a NULL one counts as zero)
__device__ __forceinline__ bool dc_zero_incoming(const int g, const int N, const int E, const double* gth, const double* gfl,
                                                 const double* gsp) {
  bool nz = gsp && gsp[g] != 0.0;
  if (gth) for (int i = threadIdx.x; i < N; i += PF_THREADS) nz |= gth[(size_t)g * N + i] != 0.0;
  if (gfl) for (int e = threadIdx.x; e < E; e += PF_THREADS) nz |= gfl[(size_t)g * E + e] != 0.0;
  return __ballot(nz) == 0;
}

// The adjoint of grid g (solved, with a non-zero incoming gradient) on the FD blob at topo: the body of both adjoint kernels.
// LDS: the solve's image, lambda by bus where the solve keeps theta.
__device__ __forceinline__ void dc_adjoint_grid(const int32_t* topo, const int g, const float* lines, const double* th_in,
                                                const double* gth, const double* gfl, const double* gsp, float* gb_out,
                                                float* gl_out, float* gg_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[FH_Y_PTR];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int32_t* bslot = topo + topo[FH_BSLOT];

  double* F = lds;                       // [nnz1] factor, then [d1] right-hand side / lambda_r
  double* rhs = F + nnz1;
  double* lam = rhs + d1;                // [N] lambda by bus, 0 at the slack
  const float* line = lines + (size_t)g * E * 7;
  const double* theta = th_in + (size_t)g * N;
  const double* gf = gfl ? gfl + (size_t)g * E : nullptr;
  const double gs = gsp ? gsp[g] : 0.0;

  for (int s = lane; s < nnz1; s += PF_THREADS) F[s] = 0.0;
  __syncthreads();
  dc_matrix(N, y_ptr, st_ptr, st, bslot, line, F, lane);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_F1], topo + topo[FH_STEP_F1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_F1]), F, lane);
  if (__ballot(pf_bad_pivot(d1, topo + topo[FH_PIVOT1], F, lane))) {
    pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out);
    return;
  }

  // g_i = grad_theta_i + sum_l grad_flow_l b_l (e_f - e_t)_i: +b_l at the line's from bus (ff stamp), -b_l at its to bus (tt stamp)
  for (int i = lane; i < N; i += PF_THREADS) {
    if (p_idx[i] < 0) continue;                             // the slack's theta is constant
    double x = gth ? gth[(size_t)g * N + i] : 0.0;
    const int d = y_diag[i];
    if (gf)
      for (int q = st_ptr[d]; q < st_ptr[d + 1]; ++q) {
        const int e = st[q] >> 2, kind = st[q] & 3;
        if (kind >= 2) continue;
        const double w = gf[e] * dc_line_b(line, e);
        x += kind == 0 ? w : 0.0 - w;
      }
    rhs[p_idx[i]] = x;
  }
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), F, lane);
  for (int i = lane; i < N; i += PF_THREADS) lam[i] = p_idx[i] >= 0 ? rhs[p_idx[i]] : 0.0;
  __syncthreads();

  // dl/dP_i = lambda_i - grad_slack_p at every bus (slack_p = -sum_i P_i: Bbus has zero column sums).  (0.0 - x rather than -x: an
  // exact zero stays +0.)
  if (gb_out)
    for (int i = lane; i < N; i += PF_THREADS) {
      float* row = gb_out + ((size_t)g * N + i) * 6;
      const float d = (float)(0.0 - (lam[i] - gs));
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = d;                              // Pd
      row[3] = 0.0f;
      row[4] = d;                              // Gs
      row[5] = 0.0f;
    }
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {      // a lane per generator, in the blob's by-bus order
      const int b = pf_slot_bus(gen_ptr, N, q);
      float* row = gg_out + ((size_t)g * Gn + gen_idx[q]) * 7;
      for (int c = 0; c < 6; ++c) row[c] = 0.0f;
      row[6] = (float)(lam[b] - gs);                   // Pg
    }
  if (gl_out)
    for (int e = lane; e < E; e += PF_THREADS) {
      float* row = gl_out + ((size_t)g * E + e) * 7;
      int f, t;
      if (!pf_line_ends(line, e, N, f, t)) {
        for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
        continue;
      }
      const double x = line[e * 7 + 3], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
      const double b = dc_line_b(line, e);
      const double w = (gf ? gf[e] : 0.0) - (lam[f] - lam[t]);   // dl/dPfinj_l: through the flow and through P_f, P_t
      const double d_b = w * (theta[f] - theta[t] - sh);         // through the flow, Bbus and Pfinj_l = -b_l shift_l
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f;
      row[3] = (float)(0.0 - d_b * b / x);                       // x: db/dx = -b / x
      row[4] = 0.0f;
      row[5] = (float)(0.0 - d_b * b / tau);                     // tau: db/dtau = -b / tau
      row[6] = (float)(0.0 - b * w);                             // shift
    }
}

__global__ __launch_bounds__(PF_THREADS) void gns_dc_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ lines,
                                                                    const double* __restrict__ th_in,
                                                                    const uint8_t* __restrict__ conv_in,
                                                                    const double* __restrict__ gth, const double* __restrict__ gfl,
                                                                    const double* __restrict__ gsp, float* __restrict__ gb_out,
                                                                    float* __restrict__ gl_out, float* __restrict__ gg_out) {
  const int g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  if (dc_zero_incoming(g, N, E, gth, gfl, gsp)) { pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out); return; }
  if (!conv_in[g]) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }
  dc_adjoint_grid(topo, g, lines, th_in, gth, gfl, gsp, gb_out, gl_out, gg_out);
}

// The adjoint over a set of FD blobs (gns_dc_adjoint_set): a grid without a usable blob gets NaN rows (zero rows when its
// incoming gradient is zero) and never indexes the set
__global__ __launch_bounds__(PF_THREADS) void gns_dc_adjoint_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                        const int32_t* __restrict__ grid_off,
                                                                        const int32_t* __restrict__ order, int64_t Bt, int N, int E,
                                                                        int Gn, int64_t lds_bytes, const float* __restrict__ lines,
                                                                        const double* __restrict__ th_in,
                                                                        const uint8_t* __restrict__ conv_in,
                                                                        const double* __restrict__ gth, const double* __restrict__ gfl,
                                                                        const double* __restrict__ gsp, float* __restrict__ gb_out,
                                                                        float* __restrict__ gl_out, float* __restrict__ gg_out) {
  const int64_t g64 = pf_set_grid(order);
  if (g64 < 0 || g64 >= Bt) return;
  const int g = (int)g64;
  if (dc_zero_incoming(g, N, E, gth, gfl, gsp)) { pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out); return; }
  const int32_t* topo;
  const bool ok = pf_set_member<DcBlobKind>(set, set_words, grid_off[g], N, E, Gn, lds_bytes, INT32_MAX, topo);
  if (!ok || !conv_in[g]) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }
  dc_adjoint_grid(topo, g, lines, th_in, gth, gfl, gsp, gb_out, gl_out, gg_out);
}

// ---- host: the checks of a DC call.  Its configuration gives the shape only (max_iter and tol are not read); there is no workspace.

bool dc_batch_ok(const void* blob_dev, const float* buses, const float* lines, const float* gens, int64_t Bt) {
  return blob_dev && buses && lines && gens && Bt > 0 && Bt <= 0x7FFFFFFF;
}

// One blob: GNS_EINVAL unless it is an FD blob of cfg's shape, GNS_EUNSUPPORTED for a DC LDS image above the limit
int dc_check_topology(const gns_pf_config* cfg, const void* topo_host, int64_t* lds) {
  if (!cfg || !topo_host) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  *lds = dc_lds_bytes(h);
  return *lds > GNS_PF_LDS_MAX_BYTES ? GNS_EUNSUPPORTED : GNS_OK;
}

int dc_check_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off, int32_t n_member,
                 int64_t* lds) {
  int32_t nnzy = 0;
  return pf_scan_set<DcBlobKind>(cfg, set_host, set_words, member_off, n_member, &nnzy, lds);
}

}  // namespace

extern "C" int gns_dc_lds_bytes(const void* topo_host, int64_t* bytes) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  *bytes = dc_lds_bytes(h);
  return GNS_OK;
}

extern "C" int gns_dc_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  if (!pf_header_ok<DcBlobKind>(cfg, static_cast<const int32_t*>(topo_host))) return GNS_EINVAL;
  *bytes = 0;
  return GNS_OK;
}

extern "C" int gns_dc_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                            const float* buses, const float* lines, const float* generators, int64_t Bt,
                            double* theta, double* line_flow, double* slack_p, uint8_t* converged,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!dc_batch_ok(topo_dev, buses, lines, generators, Bt) || !theta || !line_flow || !slack_p || !converged) return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = dc_check_topology(cfg, topo_host, &lds);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_dc_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, theta, line_flow,
                                  slack_p, converged);
}

extern "C" int gns_dc_workspace_bytes_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                          int32_t n_member, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = dc_check_set(cfg, set_host, set_words, member_off, n_member, &lds);
  if (rc != GNS_OK) return rc;
  *bytes = 0;
  return GNS_OK;
}

extern "C" int gns_dc_solve_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                double* theta, double* line_flow, double* slack_p, uint8_t* converged,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!grid_off || !dc_batch_ok(set_dev, buses, lines, generators, Bt) || !theta || !line_flow || !slack_p || !converged)
    return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = dc_check_set(cfg, set_host, set_words, member_off, n_member, &lds);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_dc_set_kernel>(Bt, lds, stream, static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off, order, Bt,
                                      cfg->n_bus, cfg->n_line, cfg->n_gen, lds, buses, lines, generators, theta, line_flow, slack_p,
                                      converged);
}

// With no gradient output asked for the adjoint calls return GNS_OK without a launch, after every other check.
extern "C" int gns_dc_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                              const float* buses, const float* lines, const float* generators, int64_t Bt,
                              const double* theta, const uint8_t* converged,
                              const double* grad_theta, const double* grad_line_flow, const double* grad_slack_p,
                              float* grad_buses, float* grad_lines, float* grad_generators,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!dc_batch_ok(topo_dev, buses, lines, generators, Bt) || !theta || !converged) return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = dc_check_topology(cfg, topo_host, &lds);
  if (rc != GNS_OK) return rc;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  return pf_launch<gns_dc_adjoint_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), lines, theta, converged, grad_theta,
                                          grad_line_flow, grad_slack_p, grad_buses, grad_lines, grad_generators);
}

extern "C" int gns_dc_adjoint_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                  const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                                  const float* buses, const float* lines, const float* generators, int64_t Bt,
                                  const double* theta, const uint8_t* converged,
                                  const double* grad_theta, const double* grad_line_flow, const double* grad_slack_p,
                                  float* grad_buses, float* grad_lines, float* grad_generators,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!grid_off || !dc_batch_ok(set_dev, buses, lines, generators, Bt) || !theta || !converged) return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = dc_check_set(cfg, set_host, set_words, member_off, n_member, &lds);
  if (rc != GNS_OK) return rc;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  return pf_launch<gns_dc_adjoint_set_kernel>(Bt, lds, stream, static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off,
                                              order, Bt, cfg->n_bus, cfg->n_line, cfg->n_gen, lds, lines, theta, converged,
                                              grad_theta, grad_line_flow, grad_slack_p, grad_buses, grad_lines, grad_generators);
}
