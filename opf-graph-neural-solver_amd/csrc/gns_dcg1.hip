// Batched DC generator contingency screening (include/gns_powerflow.h, "DC generator contingency screening") on the fast-decoupled
// blob: the post-outage DC flows of a list of rows (generator g out, with line k out as well or no line).  A generator outage changes
// the injections alone, so it is one more solve u_g on the base factor; the line on top of it is the rank-1 update of the N-1
// screen, from the single-line solve z_k that screen makes.  Per grid that is one solve per distinct generator and per distinct
// line of the list, not one factorisation per row.
//
// Two kernels, no atomics, the shape of gns_dcn2.hip:
//   factor  one wave per (grid, chunk of W candidates), the candidates being the list's lines followed by its generators, with the
//           N-1 screen's prologue, image and lane solve (gns_dcn1_device.h): a line lane solves z_k as that screen does, bit for bit; a
//           generator lane writes the change of the injections dP into its column and runs the same solve program.  A pass with a
//           line per lane then stores z[f_l] - z[t_l] of every candidate contiguously into the workspace (H_k for a line, D_g for a
//           generator), with a finite flag per candidate; chunk 0 also stores the base flows F_l, b_l and the grid's status.
//   row     one wave per (grid, chunk of Q consecutive rows): F, b and the rating sit in LDS (24 E bytes); per row den and alpha are
//           computed identically on every lane, a line per lane forms F'_l from the two contiguous rows D_g and H_k (an optional
//           contiguous store), and the wave reduction of gns_dcn1_kernel finishes the row.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"

namespace {

// Lane j's own solve for generator gi out: u = A^-1 dP on the base factor into column uc of Z.  dP is -Pg at the generator's bus
// first, then the shares Pg (w_h / W) of the other generators h at their buses in generator-index order, W the sum of w_h over
// h != gi in that order; with w NULL or W not positive nothing is shared and the slack picks the loss up.  The slack's own entry
// is not in the system.  Returns whether every entry of u is finite.
__device__ __forceinline__ bool dcg1_lane_u(const int32_t* topo, const Dcn1Image& m, const float* gen, const double* w, const int gi,
                                            double* uc, const int ld) {
  const int N = topo[FH_N], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  for (int s = 0; s < d1; ++s) uc[s * ld] = 0.0;
  const double pg = (double)gen[gi * 7 + 6];
  double W = 0.0;
  if (w)
    for (int h = 0; h < Gn; ++h)
      if (h != gi) W += w[h];
  const bool shared = W > 0.0;
  for (int i = 0; i < N; ++i) {                       // the generators of a bus are listed in generator-index order
    const int q0 = gen_ptr[i], q1 = gen_ptr[i + 1], p = p_idx[i];
    if (q0 == q1 || p < 0) continue;
    double dp = 0.0;
    bool any = false;
    for (int q = q0; q < q1; ++q)
      if (gen_idx[q] == gi) { dp = 0.0 - pg; any = true; }
    if (shared)
      for (int q = q0; q < q1; ++q) {
        const int h = gen_idx[q];
        if (h != gi) { dp += pg * (w[h] / W); any = true; }
      }
    if (any) uc[p * ld] = dp;
  }
  dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, uc, ld);
  bool fin = true;
  for (int s = 0; s < d1; ++s) fin &= pf_finite(uc[s * ld]);
  return fin;
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_factor_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                     const float* __restrict__ lines, const float* __restrict__ gens,
                                                                     const int32_t* __restrict__ line_list, const int n_line,
                                                                     const int32_t* __restrict__ gen_list, const int n_gen,
                                                                     const double* __restrict__ pickup, const int pickup_per_grid,
                                                                     const int Bt, const int W, const int nchunks,
                                                                     double* __restrict__ ws, uint8_t* __restrict__ conv_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int n_cand = n_line + n_gen;
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, n_cand - k0);
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  const Dcn2Workspace w = dcn2_workspace(ws, Bt, n_cand, E);
  const float* gen = gens + (size_t)g * Gn * 7;

  // a grid whose base solve fails: the status alone; the row kernel reads nothing else of it
  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, gen, m, lane)) {
    if (k0 == 0 && lane == 0) { w.status[g] = 0.0; conv_out[g] = 0; }
    return;
  }

  // lane j: candidate k0 + j on the base factor, a line as the N-1 screen solves it, a generator from its change of the injections
  bool fin = false;
  if (lane < nk) {
    const int c = k0 + lane;
    if (c < n_line) {
      const int e = line_list[c];
      int2 en;
      if (e >= 0 && e < E) fin = dcn1_lane_z(topo, m, e, m.Z + lane, ld, en);
    } else {
      const int gi = gen_list[c - n_line];
      const double* wg = pickup ? pickup + (pickup_per_grid ? (size_t)g * Gn : 0) : nullptr;
      if (gi >= 0 && gi < Gn) fin = dcg1_lane_u(topo, m, gen, wg, gi, m.Z + lane, ld);
    }
  }
  __syncthreads();

  // the chunk's candidates in order, a line per lane: z_c[f_l] - z_c[t_l], z = 0 at the slack
  for (int j = 0; j < nk; ++j) {
    const size_t row = (size_t)g * n_cand + k0 + j;
    const int ok = __shfl((int)fin, j);
    for (int l = lane; l < E; l += PF_THREADS) {
      const int2 en = m.ends[l];
      const double zf = en.x >= 0 ? m.Z[en.x * ld + j] : 0.0, zt = en.y >= 0 ? m.Z[en.y * ld + j] : 0.0;
      w.H[row * E + l] = ok ? zf - zt : __builtin_nan("");
    }
    if (lane == 0) w.fin[row] = ok ? 1.0 : 0.0;
  }
  if (k0 == 0) {
    for (int l = lane; l < E; l += PF_THREADS) {
      w.F[(size_t)g * E + l] = m.lF[l];
      w.b[(size_t)g * E + l] = m.lb[l];
    }
    if (lane == 0) { w.status[g] = 1.0; conv_out[g] = 1; }
  }
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_row_kernel(const int32_t* __restrict__ line_list, const int n_line, const int n_gen,
                                                                  const int32_t* __restrict__ row_cols, const int P,
                                                                  const uint8_t* __restrict__ islanding,
                                                                  const double* __restrict__ rating, const int rating_per_grid,
                                                                  const int E, const int Bt, const int Q, const int nchunks,
                                                                  const double* __restrict__ ws, double* __restrict__ fl_out,
                                                                  double* __restrict__ wl_out, int32_t* __restrict__ wi_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int n_cand = n_line + n_gen;
  const int g = blockIdx.x / nchunks, p0 = (blockIdx.x % nchunks) * Q;
  const int np = min(Q, P - p0);
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);

  if (w.status[g] == 0.0) {                      // the base solve failed: every row of the grid is NaN / -1
    dcn1_rows_not_solved(g, P, E, p0, np, fl_out, wl_out, wi_out);
    return;
  }
  double* F = lds;                               // [E] base flow
  double* b = F + E;                             // [E] b_l
  double* rt = b + E;                            // [E] rating (1 without one)
  const double* rt_in = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  for (int l = lane; l < E; l += PF_THREADS) {
    F[l] = w.F[(size_t)g * E + l];
    b[l] = w.b[(size_t)g * E + l];
    rt[l] = rt_in ? rt_in[l] : 1.0;
  }
  __syncthreads();

  const double* Hg = w.H + (size_t)g * n_cand * E;
  const double* fin = w.fin + (size_t)g * n_cand;
  for (int q = 0; q < np; ++q) {
    const int p = p0 + q;
    const int cg = row_cols[2 * (size_t)p], ck = row_cols[2 * (size_t)p + 1];     // the generator's and the line's position, -1: no line
    bool ok = cg >= 0 && cg < n_gen && ck >= -1 && ck < n_line && !islanding[p];
    int ek = -1;
    double alpha = 0.0;
    const double* Dg = Hg;
    const double* Hk = Hg;
    if (ok) {
      Dg += (size_t)(n_line + cg) * E;
      ok = fin[n_line + cg] != 0.0;
    }
    if (ok && ck >= 0) {
      ek = line_list[ck];
      Hk += (size_t)ck * E;
      // the same scalars on every lane: the flow of line k with the generator out, then the N-1 screen's den and alpha
      const double fgk = F[ek] + b[ek] * Dg[ek];
      const double den = 1.0 - b[ek] * Hk[ek];
      alpha = fgk / den;
      ok = fin[ck] != 0.0 && pf_finite(den) && den != 0.0 && pf_finite(alpha);
    }
    if (!ok) { dcn1_rows_not_solved(g, P, E, p, 1, fl_out, wl_out, wi_out); continue; }
    const size_t row = (size_t)g * P + p;
    double best = -1.0;
    int bi = INT32_MAX;
    for (int l = lane; l < E; l += PF_THREADS) {
      const double fg = F[l] + b[l] * Dg[l];
      const double fl = ek < 0 ? fg : l == ek ? 0.0 : fg + (b[l] * Hk[l]) * alpha;
      if (fl_out) fl_out[row * E + l] = fl;
      const double v = fabs(fl) / rt[l];
      if (dcn1_worse(v, l, best, bi)) { best = v; bi = l; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (dcn1_worse(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { wl_out[row] = best; wi_out[row] = bi; }
  }
}

// Whether the n entries of list are indices below bound, ascending and distinct
bool dcg1_list_ok(const int32_t* list, int32_t n, int32_t bound) {
  for (int32_t c = 0; c < n; ++c)
    if (list[c] < 0 || list[c] >= bound || (c > 0 && list[c] <= list[c - 1])) return false;
  return true;
}

// One blob, the two candidate lists and one row list: GNS_EINVAL unless it is an FD blob of cfg's shape, the lines and the generators
// are indices of it, ascending and distinct (the line list may be empty), and every row holds a position into the generators and a
// position into the lines or -1; lanes and lds are the chunk width and the LDS image of the factor kernel's launch (the N-1 screen's)
int dcg1_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* line_host, int32_t n_line, const int32_t* gen_host,
               int32_t n_gen, const int32_t* row_cols_host, int32_t n_row, int* lanes, int64_t* lds) {
  if (!cfg || !topo_host || n_line < 0 || (n_line > 0 && !line_host) || !gen_host || n_gen <= 0 || !row_cols_host || n_row <= 0)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_line > h[FH_E] || n_gen > h[FH_GN]) return GNS_EINVAL;
  if (!dcg1_list_ok(line_host, n_line, h[FH_E]) || !dcg1_list_ok(gen_host, n_gen, h[FH_GN])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_row; ++p) {
    const int32_t a = row_cols_host[2 * p], b = row_cols_host[2 * p + 1];
    if (a < 0 || a >= n_gen || b < -1 || b >= n_line) return GNS_EINVAL;
  }
  *lanes = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  *lds = dcn1_lds_bytes(h, *lanes);
  return GNS_OK;
}

}  // namespace

extern "C" int gns_dcg1_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return gns_dcn1_lds_bytes(topo_host, bytes, lanes);
}

extern "C" int gns_dcg1_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line, int32_t n_gen,
                                        size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_line < 0 || n_gen <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_line > h[FH_E] || n_gen > h[FH_GN]) return GNS_EINVAL;
  *bytes = dcn2_ws_bytes(h, Bt, (int64_t)n_line + n_gen);
  return GNS_OK;
}

extern "C" int gns_dcg1_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                               const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                               const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                               double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || (n_line > 0 && !line_dev) || !gen_dev ||
      !row_cols_dev || !islanding || !worst_loading || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1) ||
      (pickup_per_grid != 0 && pickup_per_grid != 1))
    return GNS_EINVAL;
  int lanes = 0;
  int64_t lds = 0;
  const int rc = dcg1_check(cfg, topo_host, line_host, n_line, gen_host, n_gen, row_cols_host, n_row, &lanes, &lds);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int64_t n_cand = (int64_t)n_line + n_gen;
  const int Q = dcn2_pairs_per_wave(n_row);
  int64_t nchunks_c = 0, nchunks_p = 0;
  if (!pf_chunks(n_cand, lanes, Bt, &nchunks_c) || !pf_chunks(n_row, Q, Bt, &nchunks_p)) return GNS_EINVAL;
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcn2_ws_bytes(h, Bt, n_cand)) return GNS_ESIZE;
  double* ws = static_cast<double*>(workspace);
  const int rc1 = pf_launch<gns_dcg1_factor_kernel>(Bt * nchunks_c, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines,
                                                    generators, line_dev, (int)n_line, gen_dev, (int)n_gen, pickup, (int)pickup_per_grid,
                                                    (int)Bt, lanes, (int)nchunks_c, ws, converged);
  if (rc1 != GNS_OK) return rc1;
  return pf_launch<gns_dcg1_row_kernel>(Bt * nchunks_p, 24 * (int64_t)h[FH_E], stream, line_dev, (int)n_line, (int)n_gen, row_cols_dev,
                                        (int)n_row, islanding, rating, (int)rating_per_grid, (int)h[FH_E], (int)Bt, Q, (int)nchunks_p,
                                        (const double*)ws, line_flow, worst_loading, worst_line);
}
