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
// The adjoint (gns_dcn2_adjoint) follows the forward's host code below.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"

namespace {

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

// ---- the adjoint (gns_dcn2_adjoint; include/gns_powerflow.h, "DC N-2 contingency screening", gradients)
//
// Five launches, no atomics, every sum in a fixed order:
//   factor   gns_dcn2_factor_kernel again, into the adjoint's own workspace: H, F, b, the flags and the status are the forward's bits
//   pair     one wave per (grid, chunk of Q consecutive pairs), the forward's chunks: per pair M and a as the forward computes them,
//            G from the incoming gradients, ga by the wave's shuffle tree (a line per lane with grad_line_flow, one term without),
//            v = M^-T ga; a record per (grid, pair) and the chunk's partial of gF, each line's sum owned by lane l mod 64
//   gather   one wave per (grid, candidate): it scans the pair list 64 pairs at a time, takes the pairs that hold its candidate in
//            list order and sums T'_c[l] = sum_p G_pl a_pc, plus v_r a_pc at the two outaged lines (the 2x2 terms), a line per lane
//   solve    (gns_dcn1_device.h, shared with gns_dcg1_adjoint) one wave per (grid, chunk of W columns) on the N-1 adjoint's image: column 0 is q_0 = sum_l gF_l b_l m_l, column c + 1
//            is sum_l b_l T'_c[l] m_l; lane j solves its column on the base factor, then a line per lane forms the chunk's partial
//   reduce   gns_dcn1_adjoint_reduce_kernel: the chunks in order, the contract, every element written

constexpr int DCN2_REC = 6;   // doubles of a (grid, pair) record: a_j, a_k, v_j, v_k, the worst-line term, (contributes, worst line)

// The adjoint's workspace after the forward's block (dcn2_ws_bytes, itself a multiple of 256 bytes), all doubles but the last:
// T' [Bt][n_cand][E], the records [Bt][n_pair][6], the pair chunks' partials of gF [Bt][chunks_p][E + 1] (the last one the chunk's
// status), gF [Bt][E], per candidate the number of contributing pairs that do not hold it [Bt][n_cand], the solve kernel's partials
// [Bt][chunks_a][N + 2 E + 1] and the factor kernel's converged bytes [Bt]
struct Dcn2AdjointWorkspace {
  double* T;
  double* rec;
  double* gf_part;
  double* gf;
  double* others;
  double* part;
  uint8_t* conv;
};

__host__ __device__ inline int64_t dcn2_adjoint_doubles(const int32_t* h, const int64_t Bt, const int64_t n_cand, const int64_t n_pair,
                                                        const int64_t chunks_p, const int64_t chunks_a) {
  const int64_t E = h[FH_E];
  return Bt * (n_cand * E + n_pair * DCN2_REC + chunks_p * (E + 1) + E + n_cand + chunks_a * dcn1_adjoint_partial(h));
}

__host__ __device__ inline Dcn2AdjointWorkspace dcn2_adjoint_workspace(double* ws, const int32_t* h, const int64_t Bt,
                                                                       const int64_t n_cand, const int64_t n_pair,
                                                                       const int64_t chunks_p, const int64_t chunks_a) {
  const int64_t E = h[FH_E];
  Dcn2AdjointWorkspace w;
  w.T = ws;
  w.rec = w.T + Bt * n_cand * E;
  w.gf_part = w.rec + Bt * n_pair * DCN2_REC;
  w.gf = w.gf_part + Bt * chunks_p * (E + 1);
  w.others = w.gf + Bt * E;
  w.part = w.others + Bt * n_cand;
  w.conv = reinterpret_cast<uint8_t*>(w.part + Bt * chunks_a * dcn1_adjoint_partial(h));
  return w;
}

// The two candidates of pair p, the lower first, as the forward orders them
__device__ __forceinline__ int2 dcn2_pair(const int32_t* pair_cols, const int p) {
  const int cj = pair_cols[2 * (size_t)p], ck = pair_cols[2 * (size_t)p + 1];
  return cj > ck ? make_int2(ck, cj) : make_int2(cj, ck);
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcn2_adjoint_pair_kernel(const int32_t* __restrict__ cand, const int n_cand,
                                                                           const int32_t* __restrict__ pair_cols, const int P,
                                                                           const uint8_t* __restrict__ islanding,
                                                                           const double* __restrict__ rating, const int rating_per_grid,
                                                                           const int32_t* __restrict__ wi_in,
                                                                           const uint8_t* __restrict__ conv_in,
                                                                           const double* __restrict__ gfl, const double* __restrict__ gwl,
                                                                           const int E, const int Bt, const int Q, const int nchunks,
                                                                           const double* __restrict__ ws, double* __restrict__ rec_out,
                                                                           double* __restrict__ gf_part) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / nchunks, p0 = (blockIdx.x % nchunks) * Q;
  const int np = min(Q, P - p0);
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);
  double* part = gf_part + (size_t)blockIdx.x * (E + 1);
  const size_t row0 = (size_t)g * P + p0;

  // a grid that is not solved: nothing to add; its gradient is NaN unless every incoming gradient of the chunk is zero
  if (!conv_in[g] || w.status[g] == 0.0) {
    const bool nz = dcn1_rows_nonzero(np >= 64 ? ~0ull : (1ull << np) - 1, row0, E, gfl, gwl);
    dcn1_partial_none(part, E + 1, nz ? DCN1_PART_NAN : DCN1_PART_UNSOLVED_ZERO);
    return;
  }
  double* F = lds;                               // [E] base flow
  double* b = F + E;                             // [E] b_l
  double* rt = b + E;                            // [E] rating (1 without one)
  double* gF = rt + E;                           // [E] the chunk's sum of dl/dF_l; lane l mod 64 alone touches entry l
  const double* rt_in = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  for (int l = lane; l < E; l += PF_THREADS) {
    F[l] = w.F[(size_t)g * E + l];
    b[l] = w.b[(size_t)g * E + l];
    rt[l] = rt_in ? rt_in[l] : 1.0;
    gF[l] = 0.0;
  }
  __syncthreads();

  const double* Hg = w.H + (size_t)g * n_cand * E;
  const double* fin = w.fin + (size_t)g * n_cand;
  unsigned long long unsolved = 0;               // the chunk's rows the forward left NaN / -1
  for (int q = 0; q < np; ++q) {
    const int p = p0 + q;
    const size_t row = (size_t)g * P + p;
    double* rec = rec_out + row * DCN2_REC;
    const int2 c = dcn2_pair(pair_cols, p);
    bool ok = c.x >= 0 && c.y < n_cand && c.x != c.y && !islanding[p];
    int ej = -1, ek = -1;
    double m11 = 0.0, m12 = 0.0, m21 = 0.0, m22 = 0.0, det = 0.0, a_j = 0.0, a_k = 0.0;
    const double* Hj = Hg;
    const double* Hk = Hg;
    if (ok) {                                    // the forward's 2x2 system, expression for expression
      ej = cand[c.x];
      ek = cand[c.y];
      Hj += (size_t)c.x * E;
      Hk += (size_t)c.y * E;
      m11 = 1.0 - b[ej] * Hj[ej]; m12 = 0.0 - b[ej] * Hk[ej];
      m21 = 0.0 - b[ek] * Hj[ek]; m22 = 1.0 - b[ek] * Hk[ek];
      det = m11 * m22 - m12 * m21;
      a_j = (F[ej] * m22 - m12 * F[ek]) / det;
      a_k = (m11 * F[ek] - m21 * F[ej]) / det;
      ok = fin[c.x] != 0.0 && fin[c.y] != 0.0 && pf_finite(det) && det != 0.0 && pf_finite(a_j) && pf_finite(a_k);
    }
    if (!ok) {                                   // skipped, never multiplied by zero
      unsolved |= 1ull << q;
      if (lane == 0) reinterpret_cast<int2*>(rec)[DCN2_REC - 1] = make_int2(0, -1);
      continue;
    }
    // d|F'_w| / rating_w at the line the forward found worst: the sign of its flow
    const double gw = gwl ? gwl[row] : 0.0;
    const int wl_in = wi_in[row];
    int wl = -1;
    double gterm = 0.0;
    if (gw != 0.0 && wl_in >= 0 && wl_in < E && wl_in != ej && wl_in != ek) {
      const double fw = F[wl_in] + b[wl_in] * (Hj[wl_in] * a_j + Hk[wl_in] * a_k);
      gterm = gw * (fw > 0.0 ? 1.0 : fw < 0.0 ? -1.0 : 0.0) / rt[wl_in];
      wl = wl_in;
    }
    // ga = sum_l G_l b_l (H_j[l], H_k[l]) over the lines that stay, and gF_l += G_l
    double ga_j = 0.0, ga_k = 0.0;
    bool has = false;
    if (gfl) {
      const double* grow = gfl + row * E;
      for (int l = lane; l < E; l += PF_THREADS) {
        if (l == ej || l == ek) continue;
        const double G = l == wl ? grow[l] + gterm : grow[l];
        if (G == 0.0) continue;
        has = true;
        gF[l] += G;
        const double x = G * b[l];
        ga_j += x * Hj[l];
        ga_k += x * Hk[l];
      }
      for (int o = 32; o > 0; o >>= 1) {
        ga_j += __shfl_xor(ga_j, o);
        ga_k += __shfl_xor(ga_k, o);
      }
      has = __ballot(has) != 0;
    } else if (wl >= 0 && gterm != 0.0) {
      has = true;
      if ((wl & (PF_THREADS - 1)) == lane) gF[wl] += gterm;
      const double x = gterm * b[wl];
      ga_j = x * Hj[wl];
      ga_k = x * Hk[wl];
    }
    if (!has) {                                  // a zero incoming gradient: the row adds nothing
      if (lane == 0) reinterpret_cast<int2*>(rec)[DCN2_REC - 1] = make_int2(0, -1);
      continue;
    }
    // v = M^-T ga; dl/dF at the two outaged lines
    const double v_j = (ga_j * m22 - m21 * ga_k) / det, v_k = (m11 * ga_k - m12 * ga_j) / det;
    if ((ej & (PF_THREADS - 1)) == lane) gF[ej] += v_j;
    if ((ek & (PF_THREADS - 1)) == lane) gF[ek] += v_k;
    if (lane == 0) {
      rec[0] = a_j; rec[1] = a_k; rec[2] = v_j; rec[3] = v_k; rec[4] = gterm;
      reinterpret_cast<int2*>(rec)[DCN2_REC - 1] = make_int2(1, wl);
    }
  }
  // an unsolved row with a non-zero incoming gradient: the grid's gradient is NaN
  const bool nan = dcn1_rows_nonzero(unsolved, row0, E, gfl, gwl);
  for (int l = lane; l < E; l += PF_THREADS) part[l] = gF[l];
  if (lane == 0) part[E] = nan ? DCN1_PART_NAN : DCN1_PART_OK;
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcn2_adjoint_gather_kernel(const int32_t* __restrict__ cand, const int n_cand,
                                                                             const int32_t* __restrict__ pair_cols, const int P,
                                                                             const uint8_t* __restrict__ conv_in,
                                                                             const double* __restrict__ gfl, const int E, const int Bt,
                                                                             const double* __restrict__ ws,
                                                                             const double* __restrict__ rec_in, double* __restrict__ T_out,
                                                                             double* __restrict__ others_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / n_cand, c = blockIdx.x % n_cand;
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);
  if (!conv_in[g] || w.status[g] == 0.0) return;            // no records, and nothing reads T' of this grid
  double* T = lds;                                          // [E]; lane l mod 64 alone touches entry l
  for (int l = lane; l < E; l += PF_THREADS) T[l] = 0.0;

  int others = 0;                                           // contributing pairs of the grid that do not hold c
  for (int p0 = 0; p0 < P; p0 += PF_THREADS) {
    const int pm = p0 + lane;
    bool mine = false, other = false;
    if (pm < P) {
      mine = pair_cols[2 * (size_t)pm] == c || pair_cols[2 * (size_t)pm + 1] == c;
      other = !mine && reinterpret_cast<const int2*>(rec_in + ((size_t)g * P + pm) * DCN2_REC)[DCN2_REC - 1].x != 0;
    }
    others += __popcll(__ballot(other));
    for (unsigned long long todo = __ballot(mine); todo; todo &= todo - 1) {   // the pairs that hold c, in list order
      const int p = p0 + __ffsll((long long)todo) - 1;
      const size_t row = (size_t)g * P + p;
      const double* rec = rec_in + row * DCN2_REC;
      const int2 st = reinterpret_cast<const int2*>(rec)[DCN2_REC - 1];
      if (!st.x) continue;
      const int2 cc = dcn2_pair(pair_cols, p);
      const int ej = cand[cc.x], ek = cand[cc.y];
      const double a_c = cc.x == c ? rec[0] : rec[1];
      const double gterm = rec[4];
      if (gfl) {
        const double* grow = gfl + row * E;
        for (int l = lane; l < E; l += PF_THREADS) {
          if (l == ej || l == ek) continue;
          const double G = l == st.y ? grow[l] + gterm : grow[l];
          if (G != 0.0) T[l] += G * a_c;
        }
      } else if (st.y >= 0 && (st.y & (PF_THREADS - 1)) == lane) {
        T[st.y] += gterm * a_c;
      }
      // the 2x2 terms: -gM[r][c] = v_r a_c at the two outaged lines
      if ((ej & (PF_THREADS - 1)) == lane) T[ej] += rec[2] * a_c;
      if ((ek & (PF_THREADS - 1)) == lane) T[ek] += rec[3] * a_c;
    }
  }
  double* out = T_out + ((size_t)g * n_cand + c) * E;
  for (int l = lane; l < E; l += PF_THREADS) out[l] = T[l];
  if (lane == 0) others_out[(size_t)g * n_cand + c] = (double)others;
}

// The launch shape of the adjoint: the forward's pair chunks, the N-1 adjoint's width over n_cand + 1 columns, and the largest LDS
// image of its kernels
struct Dcn2AdjointShape {
  int Q, lanes;
  int64_t chunks_c, chunks_p, chunks_a, lds_factor, lds_solve, lds;
};

Dcn2AdjointShape dcn2_adjoint_shape(const int32_t* h, int64_t n_cand, int64_t n_pair) {
  Dcn2AdjointShape s;
  s.Q = dcn2_pairs_per_wave(n_pair);
  s.lanes = dcn1_adjoint_lanes(h, GNS_PF_LDS_MAX_BYTES);
  const int lanes_f = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  s.chunks_c = (n_cand + lanes_f - 1) / lanes_f;
  s.chunks_p = (n_pair + s.Q - 1) / s.Q;
  s.chunks_a = (n_cand + 1 + s.lanes - 1) / s.lanes;
  s.lds_factor = dcn1_lds_bytes(h, lanes_f);
  s.lds_solve = dcn1_adjoint_lds_bytes(h, s.lanes);
  s.lds = s.lds_solve > 32 * (int64_t)h[FH_E] ? s.lds_solve : 32 * (int64_t)h[FH_E];
  return s;
}

size_t dcn2_adjoint_ws_bytes(const int32_t* h, int64_t Bt, int64_t n_cand, int64_t n_pair, const Dcn2AdjointShape& s) {
  const size_t own = (size_t)dcn2_adjoint_doubles(h, Bt, n_cand, n_pair, s.chunks_p, s.chunks_a) * sizeof(double) + (size_t)Bt;
  return dcn2_ws_bytes(h, Bt, n_cand) + ((own + 255) & ~(size_t)255);
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
  int64_t nchunks_c = 0, nchunks_p = 0;
  if (!pf_chunks(n_cand, lanes, Bt, &nchunks_c) || !pf_chunks(n_pair, Q, Bt, &nchunks_p)) return GNS_EINVAL;
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

extern "C" int gns_dcn2_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  // the shape of the shortest lists: the width and the image depend on the blob alone
  return pf_fd_lds_query(topo_host, bytes, lanes, dcn1_adjoint_lanes, [](const int32_t* h, int) { return dcn2_adjoint_shape(h, 1, 1).lds; });
}

extern "C" int gns_dcn2_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_cand,
                                                int32_t n_pair, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_cand <= 0 || n_pair <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_cand > h[FH_E]) return GNS_EINVAL;
  const Dcn2AdjointShape s = dcn2_adjoint_shape(h, n_cand, n_pair);
  if (Bt > 0x7FFFFFFF / s.chunks_c || Bt > 0x7FFFFFFF / s.chunks_p || Bt > 0x7FFFFFFF / s.chunks_a || Bt > 0x7FFFFFFF / n_cand)
    return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = dcn2_adjoint_ws_bytes(h, Bt, n_cand, n_pair, s);
  return GNS_OK;
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_dcn2_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* cand_host, const int32_t* cand_dev, int32_t n_cand,
                                const int32_t* pair_cols_host, const int32_t* pair_cols_dev, int32_t n_pair, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid,
                                const int32_t* worst_line, const uint8_t* converged,
                                const double* grad_line_flow, const double* grad_worst_loading,
                                float* grad_buses, float* grad_lines, float* grad_generators,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cand_dev || !pair_cols_dev || !islanding ||
      !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  int lanes_f = 0;
  int64_t lds_f = 0;
  const int rc = dcn2_check(cfg, topo_host, cand_host, n_cand, pair_cols_host, n_pair, &lanes_f, &lds_f);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const Dcn2AdjointShape s = dcn2_adjoint_shape(h, n_cand, n_pair);
  // a workgroup per (grid, chunk) or (grid, candidate) in one launch
  if (Bt > 0x7FFFFFFF / s.chunks_c || Bt > 0x7FFFFFFF / s.chunks_p || Bt > 0x7FFFFFFF / s.chunks_a || Bt > 0x7FFFFFFF / n_cand)
    return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcn2_adjoint_ws_bytes(h, Bt, n_cand, n_pair, s)) return GNS_ESIZE;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  const int E = h[FH_E];
  double* ws = static_cast<double*>(workspace);
  const Dcn2AdjointWorkspace a = dcn2_adjoint_workspace(ws + dcn2_ws_bytes(h, Bt, n_cand) / sizeof(double), h, Bt, n_cand, n_pair,
                                                        s.chunks_p, s.chunks_a);
  int rl = pf_launch<gns_dcn2_factor_kernel>(Bt * s.chunks_c, s.lds_factor, stream, topo, buses, lines, generators, cand_dev, (int)n_cand,
                                             (int)Bt, lanes_f, (int)s.chunks_c, ws, a.conv);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcn2_adjoint_pair_kernel>(Bt * s.chunks_p, 32 * (int64_t)E, stream, cand_dev, (int)n_cand, pair_cols_dev, (int)n_pair,
                                               islanding, rating, (int)rating_per_grid, worst_line, converged, grad_line_flow,
                                               grad_worst_loading, E, (int)Bt, s.Q, (int)s.chunks_p, (const double*)ws, a.rec, a.gf_part);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcn2_adjoint_gather_kernel>(Bt * n_cand, 8 * (int64_t)E, stream, cand_dev, (int)n_cand, pair_cols_dev, (int)n_pair,
                                                 converged, grad_line_flow, E, (int)Bt, (const double*)ws, (const double*)a.rec, a.T, a.others);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcn2_adjoint_solve_kernel>(Bt * s.chunks_a, s.lds_solve, stream, topo, buses, lines, generators, cand_dev, (int)n_cand, (int)n_cand,
                                                (double*)nullptr, converged,
                                                (int)Bt, s.lanes, (int)s.chunks_a, (int)s.chunks_p, (const double*)ws, (const double*)a.T,
                                                (const double*)a.gf_part, (const double*)a.others, a.gf, a.part);
  if (rl != GNS_OK) return rl;
  return pf_launch<gns_dcn1_adjoint_reduce_kernel>(Bt, 0, stream, topo, lines, (int)s.chunks_a, (const double*)a.part, grad_buses,
                                                   grad_lines, grad_generators);
}
