// Batched DC optimal power flow (include/gns_powerflow.h, "DC optimal power flow") on the fast-decoupled blob: the cheapest dispatch
// within the units' bounds and the lines' ratings, with the multipliers and the locational marginal prices.  The problem is reduced
// to the dispatch p by generator shift factors: one solve z_g = A^-1 e_bus(g) per unit on the base factor gives the row
// S_g[l] = b_l (z_g[f_l] - z_g[t_l]), the flows are f0 + S p with f0 the flows without generation, and the one equality left is the
// balance sum p = sum (Pd + Gs).  A primal-dual interior point with PIPS's steps then works on a Gn x Gn normal matrix per grid.
//
// Three launches:
//   gns_dcopf_factor_kernel  a wave per (grid, chunk of W units) on the DC screens' image: the base case without generation, a lane
//                            per unit for its solve, S into the workspace as [E][Gn] per grid (a line's row contiguous: that is how
//                            the normal matrix reads it), f0, the units' finite flags and the grid's status
//   gns_dcopf_ipm_kernel     a wave per grid: the iteration, everything but S in LDS (dcopf_lds_bytes); its body, dcopf_ipm, is in
//                            gns_dcopf_device.h, where the security-constrained call (gns_dcscopf.hip) runs it with its rows
//   gns_dcopf_finish_kernel  a wave per grid on the DC image again: theta and the flows from the optimal injections in fp64, and the
//                            prices from one more solve on the symmetric factor
// No atomics, every sum in a fixed order (a lane's terms in index order, then the wave's xor tree).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"
#include "gns_dcopf_device.h"

namespace {

// The largest image of the three kernels (the finish runs on the factor kernel's image at width 1)
int64_t dcopf_call_lds(const int32_t* h, int lanes) {
  const int64_t a = dcopf_factor_lds(h, lanes), b = dcopf_lds_bytes(h);
  return a > b ? a : b;
}

// ---- the factor kernel
__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_factor_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const int Bt, const int W, const int nchunks,
                                                                      double* __restrict__ ws) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, Gn - k0);
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  const DcopfWorkspace w = dcopf_workspace(ws, Bt, Gn, E);
  const float* gen = gens + (size_t)g * Gn * 7;
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * ld, Gn, lane);

  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, zero, m, lane)) {
    if (k0 == 0 && lane == 0) w.status[g] = 0.0;
    return;
  }

  // lane j: z = A^-1 e_bus on the base factor for unit k0 + j (nothing at the slack: its column of S is zero)
  bool fin = false;
  if (lane < nk) {
    const float fb = gen[(k0 + lane) * 7];
    const int bus = (int)fb - 1;
    if (fb == (float)(bus + 1) && bus >= 0 && bus < N) {
      double* zc = m.Z + lane;
      for (int s = 0; s < d1; ++s) zc[s * ld] = 0.0;
      if (p_idx[bus] >= 0) zc[p_idx[bus] * ld] = 1.0;
      dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, zc, ld);
      fin = true;
      for (int s = 0; s < d1; ++s) fin &= pf_finite(zc[s * ld]);
    }
  }
  __syncthreads();

  // the chunk's units in order, a line per lane: S_g[l] = b_l (z_g[f_l] - z_g[t_l]), z = 0 at the slack
  double* S = w.S + (size_t)g * E * Gn;
  for (int j = 0; j < nk; ++j) {
    const int ok = __shfl((int)fin, j);
    for (int l = lane; l < E; l += PF_THREADS) {
      const int2 en = m.ends[l];
      const double zf = en.x >= 0 ? m.Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? m.Z[en.y * ld + j] : 0.0;
      S[(size_t)l * Gn + k0 + j] = ok ? m.lb[l] * (zf - zt) : __builtin_nan("");
    }
    if (lane == 0) w.fin[(size_t)g * Gn + k0 + j] = ok ? 1.0 : 0.0;
  }
  if (k0 == 0) {
    for (int l = lane; l < E; l += PF_THREADS) w.f0[(size_t)g * E + l] = m.lF[l];
    if (lane == 0) w.status[g] = 1.0;
  }
}

// ---- the interior point: the body both this kernel and gns_dcscopf_ipm_kernel run is dcopf_ipm (gns_dcopf_device.h)
__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_ipm_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                   const float* __restrict__ gens, const double* __restrict__ cost,
                                                                   const int cost_per_grid, const double* __restrict__ rating,
                                                                   const int rating_per_grid, const int Bt, const double tol,
                                                                   const int max_iter, double* __restrict__ ws,
                                                                   double* __restrict__ pg_out, double* __restrict__ mu_line_out,
                                                                   double* __restrict__ mu_pmax_out, double* __restrict__ mu_pmin_out,
                                                                   double* __restrict__ objective_out, uint8_t* __restrict__ conv_out,
                                                                   int32_t* __restrict__ iter_out) {
  extern __shared__ double lds[];
  dcopf_ipm<false>(lds, topo, buses, gens, cost, cost_per_grid, rating, rating_per_grid, Bt, tol, max_iter, ws, DcopfRows{}, pg_out,
                   mu_line_out, mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
}

// ---- the finish: theta and the flows at the returned dispatch as gns_dc_kernel defines them, the injections in fp64; then
// lmp = -lambda - A^-1 sum_l b_l mu_line_l (e_f - e_t) on the same factor (0 at the slack), a bus walking its diagonal's stamps
__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_finish_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const int Bt,
                                                                      const double* __restrict__ ws, const double* __restrict__ pg,
                                                                      const double* __restrict__ mu_line, double* __restrict__ theta_out,
                                                                      double* __restrict__ flow_out, double* __restrict__ lmp_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int2* ops_s = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);
  const DcopfWorkspace w = dcopf_workspace(const_cast<double*>(ws), Bt, Gn, E);
  const Dcn1Image m = dcn1_image(topo, lds);
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const double* p = pg + (size_t)g * Gn;
  const double* ml = mu_line + (size_t)g * E;
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * 2, Gn, lane);

  if (w.status[g] == 0.0 || w.solved[g] == 0.0 || !dcn1_base_case(topo, bus, line, zero, m, lane)) {
    const double nan = __builtin_nan("");
    for (int i = lane; i < N; i += PF_THREADS) { theta_out[(size_t)g * N + i] = nan; lmp_out[(size_t)g * N + i] = nan; }
    for (int l = lane; l < E; l += PF_THREADS) flow_out[(size_t)g * E + l] = nan;
    return;
  }
  for (int i = lane; i < N; i += PF_THREADS) {
    if (p_idx[i] < 0) continue;
    double inj = dc_injection(i, y_diag, st_ptr, st, gen_ptr, gen_idx, bus, line, zero);
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) inj += p[gen_idx[q]];
    m.rhs[p_idx[i]] = inj;
  }
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
  for (int i = lane; i < N; i += PF_THREADS) {
    const double x = p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0;
    m.th[i] = x;
    theta_out[(size_t)g * N + i] = x;
  }
  __syncthreads();
  for (int e = lane; e < E; e += PF_THREADS) {
    int f, t;
    const bool ok = pf_line_ends(line, e, N, f, t);
    const double b = m.lb[e];
    flow_out[(size_t)g * E + e] = ok ? b * (m.th[f] - m.th[t]) + (0.0 - b * (double)line[e * 7 + 6]) : __builtin_nan("");
  }
  for (int i = lane; i < N; i += PF_THREADS) {
    if (p_idx[i] < 0) continue;
    double r = 0.0;
    const int d = y_diag[i];
    for (int q = st_ptr[d]; q < st_ptr[d + 1]; ++q) {
      const int e = st[q] >> 2, kind = st[q] & 3;
      if (kind >= 2) continue;
      const double x = m.lb[e] * ml[e];
      r += kind == 0 ? x : 0.0 - x;
    }
    m.rhs[p_idx[i]] = r;
  }
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
  const double lam = w.lam[g];
  for (int i = lane; i < N; i += PF_THREADS) lmp_out[(size_t)g * N + i] = 0.0 - lam - (p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0);
}

}  // namespace

int gns_dcopf_launch_factor(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, const float* generators,
                            int64_t Bt, double* ws, void* stream) {
  const int lanes = dcopf_lanes(h);
  const int64_t nchunks = (h[FH_GN] + lanes - 1) / lanes;
  return pf_launch<gns_dcopf_factor_kernel>(Bt * nchunks, dcopf_factor_lds(h, lanes), stream, static_cast<const int32_t*>(topo_dev), buses,
                                            lines, generators, (int)Bt, lanes, (int)nchunks, ws);
}

int gns_dcopf_launch_finish(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, int64_t Bt, const double* ws,
                            const double* pg, const double* mu, double* theta, double* line_flow, double* lmp, void* stream) {
  return pf_launch<gns_dcopf_finish_kernel>(Bt, dcopf_factor_lds(h, 1), stream, static_cast<const int32_t*>(topo_dev), buses, lines, (int)Bt,
                                            ws, pg, mu, theta, line_flow, lmp);
}

extern "C" int gns_dcopf_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int w = dcopf_lanes(h);
  *bytes = dcopf_call_lds(h, w);
  if (lanes) *lanes = w;
  return GNS_OK;
}

extern "C" int gns_dcopf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  *bytes = dcopf_ws_bytes(static_cast<const int32_t*>(topo_host), Bt);
  return GNS_OK;
}

extern "C" int gns_dcopf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                               double* pg, double* theta, double* line_flow, double* lmp, double* mu_line, double* mu_pmax,
                               double* mu_pmin, double* objective, uint8_t* converged, int32_t* iterations,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cost || (cost_per_grid != 0 && cost_per_grid != 1) ||
      (rating_per_grid != 0 && rating_per_grid != 1) || !pg || !theta || !line_flow || !lmp || !mu_line || !mu_pmax || !mu_pmin ||
      !objective || !converged || !iterations || !workspace)
    return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int lanes = dcopf_lanes(h);
  int64_t nchunks = 0;
  if (!pf_chunks(h[FH_GN], lanes, Bt, &nchunks)) return GNS_EINVAL;
  if (workspace_bytes < dcopf_ws_bytes(h, Bt)) return GNS_ESIZE;
  if (dcopf_call_lds(h, lanes) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double* ws = static_cast<double*>(workspace);
  int rl = gns_dcopf_launch_factor(h, topo_dev, buses, lines, generators, Bt, ws, stream);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcopf_ipm_kernel>(Bt, dcopf_lds_bytes(h), stream, topo, buses, generators, cost, (int)cost_per_grid, rating,
                                       (int)rating_per_grid, (int)Bt, cfg->tol, (int)cfg->max_iter, ws, pg, mu_line, mu_pmax, mu_pmin,
                                       objective, converged, iterations);
  if (rl != GNS_OK) return rl;
  return gns_dcopf_launch_finish(h, topo_dev, buses, lines, Bt, ws, pg, mu_line, theta, line_flow, lmp, stream);
}
