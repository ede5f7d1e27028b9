// Batched DC N-2 contingency screening (include/gns_powerflow.h, "DC N-2 contingency screening") on the fast-decoupled blob.  A
// double-line outage is a rank-2 change of Bbus[r, r], so the post-outage flows of the pair (j, k) come from the two single-line
// solves z_j, z_k on the base factor (what gns_dcn1.hip makes per outage) and a 2x2 system per pair.  Per grid that is one solve per
// distinct line of the pair list, not one factorisation per pair.
//
// Two kernels, no atomics:
//   factor  one wave per (grid, chunk of W candidate lines) with the N-1 screen's prologue, image and lane solve (gns_dcn1_device.h),
//           so z_c is that screen's bit for bit.  A pass with a line per lane then stores H_c[l] = z_c[f_l] - z_c[t_l] for every line
//           contiguously into the workspace, with a finite flag per candidate; chunk 0 also stores the base flows F_l, b_l and the
//           grid's status.
//   pair    one wave per (grid, chunk of Q consecutive pairs): F, b and the rating sit in LDS (24 E bytes); per pair the six scalars
//           of the 2x2 system are computed identically on every lane, a line per lane forms F'_l from the two H rows (contiguous
//           loads, an optional contiguous store), and the wave reduction of gns_dcn1_kernel finishes the row.  The kernel orders
//           the two lines of a pair itself, so (k, j) gives the bits of (j, k).
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"

namespace {

// The workspace of one call: H [Bt][n_cand][E], then F [Bt][E], b [Bt][E], the candidates' finite flags [Bt][n_cand] and the grids'
// status [Bt] (1: the base case is solved), all doubles
struct Dcn2Workspace {
  double* H;
  double* F;
  double* b;
  double* fin;
  double* status;
};

__host__ __device__ inline Dcn2Workspace dcn2_workspace(double* ws, const int64_t Bt, const int64_t n_cand, const int64_t E) {
  Dcn2Workspace w;
  w.H = ws;
  w.F = w.H + Bt * n_cand * E;
  w.b = w.F + Bt * E;
  w.fin = w.b + Bt * E;
  w.status = w.fin + Bt * n_cand;
  return w;
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcn2_factor_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                     const float* __restrict__ lines, const float* __restrict__ gens,
                                                                     const int32_t* __restrict__ cand, const int n_cand, const int Bt,
                                                                     const int W, const int nchunks, double* __restrict__ ws,
                                                                     uint8_t* __restrict__ conv_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, n_cand - k0);
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  const Dcn2Workspace w = dcn2_workspace(ws, Bt, n_cand, E);

  // a grid whose base solve fails: the status alone; the pair kernel reads nothing else of it
  if (!dcn1_base_case(topo, buses + (size_t)g * N * 6, lines + (size_t)g * E * 7, gens + (size_t)g * Gn * 7, m, lane)) {
    if (k0 == 0 && lane == 0) { w.status[g] = 0.0; conv_out[g] = 0; }
    return;
  }

  // lane j: z of candidate k0 + j on the base factor, as the N-1 screen solves it
  bool fin = false;
  if (lane < nk) {
    const int e = cand[k0 + lane];
    int2 en;
    if (e >= 0 && e < E) fin = dcn1_lane_z(topo, m, e, m.Z + lane, ld, en);
  }
  __syncthreads();

  // the chunk's candidates in order, a line per lane: H_c[l] = z_c[f_l] - z_c[t_l], z = 0 at the slack
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

__global__ __launch_bounds__(PF_THREADS) void gns_dcn2_pair_kernel(const int32_t* __restrict__ cand, const int n_cand,
                                                                   const int32_t* __restrict__ pair_cols, const int P,
                                                                   const uint8_t* __restrict__ islanding,
                                                                   const double* __restrict__ rating, const int rating_per_grid,
                                                                   const int E, const int Bt, const int Q, const int nchunks,
                                                                   const double* __restrict__ ws, double* __restrict__ fl_out,
                                                                   double* __restrict__ wl_out, int32_t* __restrict__ wi_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
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
    int cj = pair_cols[2 * (size_t)p], ck = pair_cols[2 * (size_t)p + 1];
    if (cj > ck) { const int c = cj; cj = ck; ck = c; }          // cand ascends: the lower line first, whatever the pair's order
    const bool in_range = cj >= 0 && ck < n_cand && cj != ck;
    bool ok = in_range && !islanding[p];
    int ej = -1, ek = -1;
    double a_j = 0.0, a_k = 0.0;
    const double* Hj = Hg;
    const double* Hk = Hg;
    if (ok) {
      ej = cand[cj];
      ek = cand[ck];
      Hj += (size_t)cj * E;
      Hk += (size_t)ck * E;
      // (I - diag(b) M^T Z) a = F_S: the same six scalars on every lane
      const double m11 = 1.0 - b[ej] * Hj[ej], m12 = 0.0 - b[ej] * Hk[ej];
      const double m21 = 0.0 - b[ek] * Hj[ek], m22 = 1.0 - b[ek] * Hk[ek];
      const double det = m11 * m22 - m12 * m21;
      a_j = (F[ej] * m22 - m12 * F[ek]) / det;
      a_k = (m11 * F[ek] - m21 * F[ej]) / det;
      ok = fin[cj] != 0.0 && fin[ck] != 0.0 && pf_finite(det) && det != 0.0 && pf_finite(a_j) && pf_finite(a_k);
    }
    if (!ok) { dcn1_rows_not_solved(g, P, E, p, 1, fl_out, wl_out, wi_out); continue; }
    const size_t row = (size_t)g * P + p;
    double best = -1.0;
    int bi = INT32_MAX;
    for (int l = lane; l < E; l += PF_THREADS) {
      const double fl = l == ej || l == ek ? 0.0 : F[l] + b[l] * (Hj[l] * a_j + Hk[l] * a_k);
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

// Pairs a workgroup of the pair kernel takes one after the other: from the length of the pair list alone
int dcn2_pairs_per_wave(int64_t n_pair) { return n_pair >= 8192 ? 32 : 8; }

// One blob, one candidate list and one pair list: GNS_EINVAL unless it is an FD blob of cfg's shape, the candidates are lines of it,
// ascending and distinct, and every pair holds two different positions into them; lanes and lds are the chunk width and the LDS
// image of the factor kernel's launch (the N-1 screen's)
int dcn2_check(const gns_pf_config* cfg, const void* topo_host, const int32_t* cand_host, int32_t n_cand,
               const int32_t* pair_cols_host, int32_t n_pair, int* lanes, int64_t* lds) {
  if (!cfg || !topo_host || !cand_host || n_cand <= 0 || !pair_cols_host || n_pair <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  for (int32_t c = 0; c < n_cand; ++c)
    if (cand_host[c] < 0 || cand_host[c] >= h[FH_E] || (c > 0 && cand_host[c] <= cand_host[c - 1])) return GNS_EINVAL;
  for (int64_t p = 0; p < n_pair; ++p) {
    const int32_t a = pair_cols_host[2 * p], b = pair_cols_host[2 * p + 1];
    if (a < 0 || a >= n_cand || b < 0 || b >= n_cand || a == b) return GNS_EINVAL;
  }
  *lanes = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  *lds = dcn1_lds_bytes(h, *lanes);
  return GNS_OK;
}

size_t dcn2_ws_bytes(const int32_t* h, int64_t Bt, int64_t n_cand) {
  const int64_t E = h[FH_E];
  return ((size_t)Bt * (size_t)(n_cand * E + 2 * E + n_cand + 1) * sizeof(double) + 255) & ~(size_t)255;
}

}  // namespace

extern "C" int gns_dcn2_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return gns_dcn1_lds_bytes(topo_host, bytes, lanes);
}

extern "C" int gns_dcn2_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_cand <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_cand > h[FH_E]) return GNS_EINVAL;
  *bytes = dcn2_ws_bytes(h, Bt, n_cand);
  return GNS_OK;
}

extern "C" int gns_dcn2_screen(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                               const float* buses, const float* lines, const float* generators, int64_t Bt,
                               const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                               const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                               const double* rating, int32_t rating_per_grid,
                               double* line_flow, double* worst_loading, int32_t* worst_line, uint8_t* converged,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cand_dev || !pair_cols_dev || !islanding || !worst_loading || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  int lanes = 0;
  int64_t lds = 0;
  const int rc = dcn2_check(cfg, topo_host, cand_host, n_cand, pair_cols_host, n_pair, &lanes, &lds);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int Q = dcn2_pairs_per_wave(n_pair);
  const int64_t nchunks_c = ((int64_t)n_cand + lanes - 1) / lanes, nchunks_p = ((int64_t)n_pair + Q - 1) / Q;
  if (Bt > 0x7FFFFFFF / nchunks_c || Bt > 0x7FFFFFFF / nchunks_p) return GNS_EINVAL;   // a workgroup per (grid, chunk) in one launch
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcn2_ws_bytes(h, Bt, n_cand)) return GNS_ESIZE;
  double* ws = static_cast<double*>(workspace);
  const int rc1 = pf_launch<gns_dcn2_factor_kernel>(Bt * nchunks_c, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines,
                                                    generators, cand_dev, (int)n_cand, (int)Bt, lanes, (int)nchunks_c, ws, converged);
  if (rc1 != GNS_OK) return rc1;
  return pf_launch<gns_dcn2_pair_kernel>(Bt * nchunks_p, 24 * (int64_t)h[FH_E], stream, cand_dev, (int)n_cand, pair_cols_dev, (int)n_pair,
                                         islanding, rating, (int)rating_per_grid, (int)h[FH_E], (int)Bt, Q, (int)nchunks_p,
                                         (const double*)ws, line_flow, worst_loading, worst_line);
}
