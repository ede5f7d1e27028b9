// Batched security-constrained DC optimal power flow (include/gns_powerflow.h, "Security-constrained DC optimal power flow"): the
// problem of gns_dcopf_solve plus, per listed row (l, k), the limit on line l's flow after the outage of line k.  A post-outage flow
// is F_l + L_r F_k with L_r = b_l (z_k[f_l] - z_k[t_l]) / (1 - b_k d_k), the DC N-1 screen's line-outage factor, so a row is a
// combination of two rows of S and the normal matrix stays Gn x Gn however many rows are listed.
//
// Five launches, a wave per workgroup:
//   gns_dcopf_factor_kernel   gns_dcopf.hip's, unchanged, into this call's workspace
//   gns_dcscopf_rows_kernel   a wave per (grid, chunk of W row slots) on the same image: the base factor, lane j its own solve z_k for
//                             slot j (a solve per slot, duplicates of k included: per-grid lists need no host work), L_r and the
//                             slot's status into the workspace
//   gns_dcscopf_ipm_kernel    a wave per grid: dcopf_ipm (gns_dcopf_device.h) with the rows' state in LDS behind the iterate
//   gns_dcopf_finish_kernel   gns_dcopf.hip's, unchanged, on the per-line multipliers the iteration left: mu_line_l + sum_r mu_r at l,
//                             L_r mu_r at k
//   gns_dcscopf_row_flow_kernel  a thread per slot: line_flow_l + L_r line_flow_k
// No atomics, every sum in a fixed order (a lane's terms in index order, the rows in list order, then the wave's xor tree).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"
#include "gns_dcopf_device.h"

namespace {

// The rows' part of the workspace behind gns_dcopf_solve's: L_r [Bt][R], the slots' status [Bt][R], the finish's multipliers [Bt][E]
struct DcscopfWorkspace {
  double* L;
  double* st;
  double* mu_eff;
};

__host__ __device__ inline DcscopfWorkspace dcscopf_workspace(double* rows_ws, const int64_t Bt, const int64_t R) {
  DcscopfWorkspace w;
  w.L = rows_ws;
  w.st = w.L + Bt * R;
  w.mu_eff = w.st + Bt * R;
  return w;
}

size_t dcscopf_ws_bytes(const int32_t* h, int64_t Bt, int64_t R) {
  return dcopf_ws_bytes(h, Bt) + (((size_t)Bt * (size_t)(2 * R + h[FH_E]) * sizeof(double) + 255) & ~(size_t)255);
}

// The interior point's image with R row slots: gns_dcopf_solve's, ten doubles per slot and an int32 per line
int64_t dcscopf_ipm_lds(const int32_t* h, int64_t R) { return dcopf_lds_bytes(h) + 8 * (10 * R + ((int64_t)h[FH_E] + 1) / 2); }

int64_t dcscopf_call_lds(const int32_t* h, int lanes, int64_t R) {
  const int64_t a = dcopf_factor_lds(h, lanes), b = dcscopf_ipm_lds(h, R);
  return a > b ? a : b;
}

// ---- the row-factor kernel
__global__ __launch_bounds__(PF_THREADS) void gns_dcscopf_rows_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines,
                                                                      const int32_t* __restrict__ rows, const int rows_per_grid,
                                                                      const int R, const double* __restrict__ rating_c,
                                                                      const int rating_c_per_grid, const uint8_t* __restrict__ bridge,
                                                                      const int Bt, const int W, const int nchunks,
                                                                      double* __restrict__ rows_ws) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1];
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, R - k0);
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  const DcscopfWorkspace w = dcscopf_workspace(rows_ws, Bt, R);
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * ld, Gn, lane);
  const int32_t* ids = rows + (rows_per_grid ? (size_t)g * R * 2 : 0);
  const double* rc = rating_c ? rating_c + (rating_c_per_grid ? (size_t)g * E : 0) : nullptr;
  const size_t at = (size_t)g * R + k0 + lane;

  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, zero, m, lane)) {
    if (lane < nk) { w.L[at] = __builtin_nan(""); w.st[at] = DCSCOPF_ROW_FAILED; }
    return;
  }
  if (lane >= nk) return;                              // (no barrier follows)

  // lane j: the slot's kind, then z_k on the base factor, the screen's denominator and L_r
  const int l = ids[2 * (k0 + lane)], k = ids[2 * (k0 + lane) + 1];
  const bool listed = l != -1 || k != -1;
  const bool lines_ok = l >= 0 && l < E && k >= 0 && k < E && l != k;
  double L = 0.0, st = DCSCOPF_ROW_EMPTY;
  if (listed && !lines_ok) {
    st = DCSCOPF_ROW_FAILED;
  } else if (!listed || !rc || rc[l] == __builtin_inf()) {
    // an empty slot, or a monitored line without a rating: it constrains nothing
  } else if (bridge[k]) {
    st = DCSCOPF_ROW_FAILED;
  } else {
    double* zc = m.Z + lane;
    int2 en;
    const bool fin = dcn1_lane_z(topo, m, k, zc, ld, en);
    const double d = (en.x >= 0 ? zc[en.x * ld] : 0.0) - (en.y >= 0 ? zc[en.y * ld] : 0.0);
    const double den = 1.0 - m.lb[k] * d;
    const int2 el = m.ends[l];
    const double zf = el.x >= 0 ? zc[el.x * ld] : 0.0, zt = el.y >= 0 ? zc[el.y * ld] : 0.0;
    L = m.lb[l] * (zf - zt) / den;
    st = fin && pf_finite(den) && den != 0.0 && pf_finite(L) ? DCSCOPF_ROW_OK : DCSCOPF_ROW_FAILED;
  }
  w.L[at] = st == DCSCOPF_ROW_OK ? L : __builtin_nan("");
  w.st[at] = st;
}

// ---- the interior point with the rows
__global__ __launch_bounds__(PF_THREADS) void gns_dcscopf_ipm_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                     const float* __restrict__ gens, const double* __restrict__ cost,
                                                                     const int cost_per_grid, const double* __restrict__ rating,
                                                                     const int rating_per_grid, const int32_t* __restrict__ rows,
                                                                     const int rows_per_grid, const int R,
                                                                     const double* __restrict__ rating_c, const int rating_c_per_grid,
                                                                     const int Bt, const double tol, const int max_iter,
                                                                     double* __restrict__ ws, double* __restrict__ rows_ws,
                                                                     double* __restrict__ pg_out, double* __restrict__ mu_line_out,
                                                                     double* __restrict__ mu_pmax_out, double* __restrict__ mu_pmin_out,
                                                                     double* __restrict__ objective_out, uint8_t* __restrict__ conv_out,
                                                                     int32_t* __restrict__ iter_out, double* __restrict__ mu_row_out) {
  extern __shared__ double lds[];
  const int g = blockIdx.x, E = topo[FH_E];
  const DcscopfWorkspace w = dcscopf_workspace(rows_ws, Bt, R);
  DcopfRows r;
  r.R = R;
  r.ids = rows + (rows_per_grid ? (size_t)g * R * 2 : 0);
  r.rc = rating_c ? rating_c + (rating_c_per_grid ? (size_t)g * E : 0) : nullptr;
  r.L = w.L + (size_t)g * R;
  r.st = w.st + (size_t)g * R;
  r.mu_row = mu_row_out + (size_t)g * R;
  r.mu_eff = w.mu_eff + (size_t)g * E;
  dcopf_ipm<true>(lds, topo, buses, gens, cost, cost_per_grid, rating, rating_per_grid, Bt, tol, max_iter, ws, r, pg_out, mu_line_out,
                  mu_pmax_out, mu_pmin_out, objective_out, conv_out, iter_out);
}

// ---- row_flow [Bt][R] at the returned dispatch: NaN in an empty slot (and in every slot of a grid without a dispatch)
__global__ __launch_bounds__(PF_THREADS) void gns_dcscopf_row_flow_kernel(const int32_t* __restrict__ topo, const int32_t* __restrict__ rows,
                                                                          const int rows_per_grid, const int R, const int Bt,
                                                                          const double* __restrict__ rows_ws,
                                                                          const double* __restrict__ line_flow,
                                                                          double* __restrict__ row_flow) {
  const int E = topo[FH_E];
  const DcscopfWorkspace w = dcscopf_workspace(const_cast<double*>(rows_ws), Bt, R);
  const int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
  if (i >= (int64_t)Bt * R) return;
  const int64_t g = i / R, r = i % R;
  double v = __builtin_nan("");
  if (w.st[i] == DCSCOPF_ROW_OK) {
    const int32_t* id = rows + (rows_per_grid ? i * 2 : r * 2);
    v = line_flow[g * E + id[0]] + w.L[i] * line_flow[g * E + id[1]];
  }
  row_flow[i] = v;
}

}  // namespace

extern "C" int gns_dcscopf_lds_bytes(const void* topo_host, int32_t n_row, int64_t* bytes, int32_t* lanes) {
  if (!topo_host || !bytes || n_row <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int w = dcopf_lanes(h);
  *bytes = dcscopf_call_lds(h, w, n_row);
  if (lanes) *lanes = w;
  return GNS_OK;
}

extern "C" int gns_dcscopf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_row, size_t* bytes) {
  if (!bytes || Bt <= 0 || n_row <= 0) return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  *bytes = dcscopf_ws_bytes(static_cast<const int32_t*>(topo_host), Bt, n_row);
  return GNS_OK;
}

extern "C" int gns_dcscopf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                 const float* buses, const float* lines, const float* generators, int64_t Bt,
                                 const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                                 const int32_t* rows, int32_t rows_per_grid, int32_t n_row,
                                 const double* rating_c, int32_t rating_c_per_grid, const uint8_t* bridge,
                                 double* pg, double* theta, double* line_flow, double* lmp, double* mu_line, double* mu_pmax,
                                 double* mu_pmin, double* objective, uint8_t* converged, int32_t* iterations,
                                 double* mu_row, double* row_flow,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cost || (cost_per_grid != 0 && cost_per_grid != 1) ||
      (rating_per_grid != 0 && rating_per_grid != 1) || !pg || !theta || !line_flow || !lmp || !mu_line || !mu_pmax || !mu_pmin ||
      !objective || !converged || !iterations || !workspace)
    return GNS_EINVAL;
  if (!rows || !bridge || !mu_row || !row_flow || n_row <= 0 || (rows_per_grid != 0 && rows_per_grid != 1) ||
      (rating_c_per_grid != 0 && rating_c_per_grid != 1))
    return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int lanes = dcopf_lanes(h);
  int64_t nchunks = 0, nrchunks = 0, nflow = 0;
  if (!pf_chunks(h[FH_GN], lanes, Bt, &nchunks) || !pf_chunks(n_row, lanes, Bt, &nrchunks) || !pf_chunks(n_row, PF_THREADS, Bt, &nflow))
    return GNS_EINVAL;
  if (workspace_bytes < dcscopf_ws_bytes(h, Bt, n_row)) return GNS_ESIZE;
  if (dcscopf_call_lds(h, lanes, n_row) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double* ws = static_cast<double*>(workspace);
  double* rows_ws = ws + dcopf_ws_bytes(h, Bt) / sizeof(double);
  if (!rating_c) { rating_c = rating; rating_c_per_grid = rating_per_grid; }
  int rl = gns_dcopf_launch_factor(h, topo_dev, buses, lines, generators, Bt, ws, stream);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcscopf_rows_kernel>(Bt * nrchunks, dcopf_factor_lds(h, lanes), stream, topo, buses, lines, rows, (int)rows_per_grid,
                                          (int)n_row, rating_c, (int)rating_c_per_grid, bridge, (int)Bt, lanes, (int)nrchunks, rows_ws);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcscopf_ipm_kernel>(Bt, dcscopf_ipm_lds(h, n_row), stream, topo, buses, generators, cost, (int)cost_per_grid, rating,
                                         (int)rating_per_grid, rows, (int)rows_per_grid, (int)n_row, rating_c, (int)rating_c_per_grid,
                                         (int)Bt, cfg->tol, (int)cfg->max_iter, ws, rows_ws, pg, mu_line, mu_pmax, mu_pmin, objective,
                                         converged, iterations, mu_row);
  if (rl != GNS_OK) return rl;
  rl = gns_dcopf_launch_finish(h, topo_dev, buses, lines, Bt, ws, pg, dcscopf_workspace(rows_ws, Bt, n_row).mu_eff, theta, line_flow, lmp,
                               stream);
  if (rl != GNS_OK) return rl;
  return pf_launch<gns_dcscopf_row_flow_kernel>((Bt * n_row + PF_THREADS - 1) / PF_THREADS, 0, stream, topo, rows, (int)rows_per_grid,
                                                (int)n_row, (int)Bt, (const double*)rows_ws, (const double*)line_flow, row_flow);
}
