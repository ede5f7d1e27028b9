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
// The adjoint (gns_dcg1_adjoint) follows the forward's host code below.
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

// ---- the adjoint (gns_dcg1_adjoint; include/gns_powerflow.h, "Gradients of the DC generator screen")
//
// Five launches, no atomics, every sum in a fixed order, the shape of gns_dcn2_adjoint:
//   factor   gns_dcg1_factor_kernel again, into the adjoint's own workspace: H, D, F, b, the flags and the status are the forward's bits
//   row      one wave per (grid, chunk of Q consecutive rows), the forward's chunks: per row den and alpha as the forward computes
//            them, G from the incoming gradients, ga by the wave's shuffle tree (a line per lane with grad_line_flow, one term
//            without), v = ga / den; a record per (grid, row) and the chunk's partial of gF, each line's sum owned by lane l mod 64
//   gather   one wave per (grid, candidate): it scans the row list 64 rows at a time, takes the rows that hold its candidate in list
//            order and sums T_k[l] = sum G_l alpha (+ v alpha at l = k) for a line, S_g[l] = sum G_l (+ v at the row's line) for a
//            generator, a line per lane
//   solve    gns_dcn2_adjoint_solve_kernel (gns_dcn1_device.h): column 0 is y_0, then a column per line and per generator; the
//            generators' y go by bus into the workspace
//   reduce   the chunks in order, the contract, every element written; a lane per listed generator forms W_g, the shared mean of
//            y_g and c_g^T y_g, then a lane per generator adds the Pg term and sums the gradient of the weights in list order

constexpr int DCG1_REC = 4;   // doubles of a (grid, row) record: alpha, v, the worst-line term, (contributes, worst line)
constexpr int DCG1_GEN = 3;   // doubles the reduce kernel keeps per listed generator: Pg_g / W_g (0: nothing shared), s_g, c_g^T y_g

// The adjoint's workspace after the forward's block (dcn2_ws_bytes, itself a multiple of 256 bytes), all doubles but the last:
// T / S [Bt][n_cand][E], the records [Bt][n_row][4], the row chunks' partials of gF [Bt][chunks_p][E + 1] (the last one the chunk's
// status), gF [Bt][E], per candidate the number of contributing rows that do not hold it [Bt][n_cand], the solve kernel's partials
// [Bt][chunks_a][N + 2 E + 1], the generators' y by bus [Bt][n_gen][N], three doubles per listed generator [Bt][n_gen][3] and the
// factor kernel's converged bytes [Bt]
struct Dcg1AdjointWorkspace {
  double* T;
  double* rec;
  double* gf_part;
  double* gf;
  double* others;
  double* part;
  double* ycols;
  double* gen;
  uint8_t* conv;
};

// The launch shape of the adjoint: the forward's row chunks, the N-1 adjoint's width over n_cand + 1 columns, and the largest LDS
// image of its kernels
struct Dcg1AdjointShape {
  int Q, lanes, lanes_f;
  int64_t n_cand, chunks_c, chunks_p, chunks_a, lds_factor, lds_solve, lds;
};

Dcg1AdjointShape dcg1_adjoint_shape(const int32_t* h, int64_t n_line, int64_t n_gen, int64_t n_row) {
  Dcg1AdjointShape s;
  s.n_cand = n_line + n_gen;
  s.Q = dcn2_pairs_per_wave(n_row);
  s.lanes = dcn1_adjoint_lanes(h, GNS_PF_LDS_MAX_BYTES);
  s.lanes_f = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  s.chunks_c = (s.n_cand + s.lanes_f - 1) / s.lanes_f;
  s.chunks_p = (n_row + s.Q - 1) / s.Q;
  s.chunks_a = (s.n_cand + 1 + s.lanes - 1) / s.lanes;
  s.lds_factor = dcn1_lds_bytes(h, s.lanes_f);
  s.lds_solve = dcn1_adjoint_lds_bytes(h, s.lanes);
  s.lds = s.lds_solve > 32 * (int64_t)h[FH_E] ? s.lds_solve : 32 * (int64_t)h[FH_E];
  return s;
}

int64_t dcg1_adjoint_doubles(const int32_t* h, int64_t Bt, int64_t n_gen, int64_t n_row, const Dcg1AdjointShape& s) {
  const int64_t N = h[FH_N], E = h[FH_E];
  return Bt * (s.n_cand * E + n_row * DCG1_REC + s.chunks_p * (E + 1) + E + s.n_cand + s.chunks_a * dcn1_adjoint_partial(h) +
               n_gen * N + n_gen * DCG1_GEN);
}

Dcg1AdjointWorkspace dcg1_adjoint_workspace(double* ws, const int32_t* h, int64_t Bt, int64_t n_gen, int64_t n_row,
                                            const Dcg1AdjointShape& s) {
  const int64_t N = h[FH_N], E = h[FH_E];
  Dcg1AdjointWorkspace w;
  w.T = ws;
  w.rec = w.T + Bt * s.n_cand * E;
  w.gf_part = w.rec + Bt * n_row * DCG1_REC;
  w.gf = w.gf_part + Bt * s.chunks_p * (E + 1);
  w.others = w.gf + Bt * E;
  w.part = w.others + Bt * s.n_cand;
  w.ycols = w.part + Bt * s.chunks_a * dcn1_adjoint_partial(h);
  w.gen = w.ycols + Bt * n_gen * N;
  w.conv = reinterpret_cast<uint8_t*>(w.gen + Bt * n_gen * DCG1_GEN);
  return w;
}

size_t dcg1_adjoint_ws_bytes(const int32_t* h, int64_t Bt, int64_t n_gen, int64_t n_row, const Dcg1AdjointShape& s) {
  const size_t own = (size_t)dcg1_adjoint_doubles(h, Bt, n_gen, n_row, s) * sizeof(double) + (size_t)Bt;
  return dcn2_ws_bytes(h, Bt, s.n_cand) + ((own + 255) & ~(size_t)255);
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_adjoint_row_kernel(const int32_t* __restrict__ line_list, const int n_line,
                                                                          const int n_gen, const int32_t* __restrict__ row_cols,
                                                                          const int P, const uint8_t* __restrict__ islanding,
                                                                          const double* __restrict__ rating, const int rating_per_grid,
                                                                          const int32_t* __restrict__ wi_in,
                                                                          const uint8_t* __restrict__ conv_in,
                                                                          const double* __restrict__ gfl, const double* __restrict__ gwl,
                                                                          const int E, const int Bt, const int Q, const int nchunks,
                                                                          const double* __restrict__ ws, double* __restrict__ rec_out,
                                                                          double* __restrict__ gf_part) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int n_cand = n_line + n_gen;
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
  double* gF = rt + E;                           // [E] the chunk's sum of dl/dFg_l; lane l mod 64 alone touches entry l
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
    double* rec = rec_out + row * DCG1_REC;
    const int cg = row_cols[2 * (size_t)p], ck = row_cols[2 * (size_t)p + 1];
    bool ok = cg >= 0 && cg < n_gen && ck >= -1 && ck < n_line && !islanding[p];
    int ek = -1;
    double den = 1.0, alpha = 0.0;
    const double* Dg = Hg;
    const double* Hk = Hg;
    if (ok) {                                    // the forward's row, expression for expression
      Dg += (size_t)(n_line + cg) * E;
      ok = fin[n_line + cg] != 0.0;
    }
    if (ok && ck >= 0) {
      ek = line_list[ck];
      Hk += (size_t)ck * E;
      const double fgk = F[ek] + b[ek] * Dg[ek];
      den = 1.0 - b[ek] * Hk[ek];
      alpha = fgk / den;
      ok = fin[ck] != 0.0 && pf_finite(den) && den != 0.0 && pf_finite(alpha);
    }
    if (!ok) {                                   // skipped, never multiplied by zero
      unsolved |= 1ull << q;
      if (lane == 0) reinterpret_cast<int2*>(rec)[DCG1_REC - 1] = make_int2(0, -1);
      continue;
    }
    // d|F'_w| / rating_w at the line the forward found worst: the sign of its flow
    const double gw = gwl ? gwl[row] : 0.0;
    const int wl_in = wi_in[row];
    int wl = -1;
    double gterm = 0.0;
    if (gw != 0.0 && wl_in >= 0 && wl_in < E && wl_in != ek) {
      const double fg = F[wl_in] + b[wl_in] * Dg[wl_in];
      const double fw = ek < 0 ? fg : fg + (b[wl_in] * Hk[wl_in]) * alpha;
      gterm = gw * (fw > 0.0 ? 1.0 : fw < 0.0 ? -1.0 : 0.0) / rt[wl_in];
      wl = wl_in;
    }
    // ga = sum_l G_l b_l H_k[l] over the lines that stay, and gF_l += G_l
    double ga = 0.0;
    bool has = false;
    if (gfl) {
      const double* grow = gfl + row * E;
      for (int l = lane; l < E; l += PF_THREADS) {
        if (l == ek) continue;
        const double G = l == wl ? grow[l] + gterm : grow[l];
        if (G == 0.0) continue;
        has = true;
        gF[l] += G;
        if (ek >= 0) ga += (G * b[l]) * Hk[l];
      }
      for (int o = 32; o > 0; o >>= 1) ga += __shfl_xor(ga, o);
      has = __ballot(has) != 0;
    } else if (wl >= 0 && gterm != 0.0) {
      has = true;
      if ((wl & (PF_THREADS - 1)) == lane) gF[wl] += gterm;
      if (ek >= 0) ga = (gterm * b[wl]) * Hk[wl];
    }
    if (!has) {                                  // a zero incoming gradient: the row adds nothing
      if (lane == 0) reinterpret_cast<int2*>(rec)[DCG1_REC - 1] = make_int2(0, -1);
      continue;
    }
    // v = ga / den: dl/dFg at the outaged line
    const double v = ek >= 0 ? ga / den : 0.0;
    if (ek >= 0 && (ek & (PF_THREADS - 1)) == lane) gF[ek] += v;
    if (lane == 0) {
      rec[0] = alpha; rec[1] = v; rec[2] = gterm;
      reinterpret_cast<int2*>(rec)[DCG1_REC - 1] = make_int2(1, wl);
    }
  }
  // an unsolved row with a non-zero incoming gradient: the grid's gradient is NaN
  const bool nan = dcn1_rows_nonzero(unsolved, row0, E, gfl, gwl);
  for (int l = lane; l < E; l += PF_THREADS) part[l] = gF[l];
  if (lane == 0) part[E] = nan ? DCN1_PART_NAN : DCN1_PART_OK;
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_adjoint_gather_kernel(const int32_t* __restrict__ line_list, const int n_line,
                                                                             const int n_gen, const int32_t* __restrict__ row_cols,
                                                                             const int P, const uint8_t* __restrict__ conv_in,
                                                                             const double* __restrict__ gfl, const int E, const int Bt,
                                                                             const double* __restrict__ ws,
                                                                             const double* __restrict__ rec_in, double* __restrict__ T_out,
                                                                             double* __restrict__ others_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int n_cand = n_line + n_gen;
  const int g = blockIdx.x / n_cand, c = blockIdx.x % n_cand;
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);
  if (!conv_in[g] || w.status[g] == 0.0) return;            // no records, and nothing reads T of this grid
  double* T = lds;                                          // [E]; lane l mod 64 alone touches entry l
  for (int l = lane; l < E; l += PF_THREADS) T[l] = 0.0;
  const bool is_line = c < n_line;
  const int col = is_line ? 1 : 0, want = is_line ? c : c - n_line;

  int others = 0;                                           // contributing rows of the grid that do not hold c
  for (int p0 = 0; p0 < P; p0 += PF_THREADS) {
    const int pm = p0 + lane;
    bool mine = false, other = false;
    if (pm < P) {
      mine = row_cols[2 * (size_t)pm + col] == want;
      other = !mine && reinterpret_cast<const int2*>(rec_in + ((size_t)g * P + pm) * DCG1_REC)[DCG1_REC - 1].x != 0;
    }
    others += __popcll(__ballot(other));
    for (unsigned long long todo = __ballot(mine); todo; todo &= todo - 1) {   // the rows that hold c, in list order
      const int p = p0 + __ffsll((long long)todo) - 1;
      const size_t row = (size_t)g * P + p;
      const double* rec = rec_in + row * DCG1_REC;
      const int2 st = reinterpret_cast<const int2*>(rec)[DCG1_REC - 1];
      if (!st.x) continue;
      const int ck = row_cols[2 * (size_t)p + 1];
      const int ek = ck >= 0 ? line_list[ck] : -1;
      const double a_c = is_line ? rec[0] : 1.0;            // T_k takes G alpha, S_g takes G
      const double gterm = rec[2];
      if (gfl) {
        const double* grow = gfl + row * E;
        for (int l = lane; l < E; l += PF_THREADS) {
          if (l == ek) continue;
          const double G = l == st.y ? grow[l] + gterm : grow[l];
          if (G != 0.0) T[l] += G * a_c;
        }
      } else if (st.y >= 0 && (st.y & (PF_THREADS - 1)) == lane) {
        T[st.y] += gterm * a_c;
      }
      // the outaged line's own entry: v alpha (the derivative of den) for T_k, v for S_g
      if (ek >= 0 && (ek & (PF_THREADS - 1)) == lane) T[ek] += rec[1] * a_c;
    }
  }
  double* out = T_out + ((size_t)g * n_cand + c) * E;
  for (int l = lane; l < E; l += PF_THREADS) out[l] = T[l];
  if (lane == 0) others_out[(size_t)g * n_cand + c] = (double)others;
}

// A wave per grid: gns_dcn1_adjoint_reduce_kernel's sums and contract, with the generators' own terms.  y_g by bus is the solve
// kernel's; dl/dPg_g += c_g^T y_g, and dl/dw_h sums (Pg_g / W_g) (y_g[m_h] - s_g) over the listed g != h that share, s_g the
// shared mean sum_{h != g} (w_h / W_g) y_g[m_h].
__global__ __launch_bounds__(PF_THREADS) void gns_dcg1_adjoint_reduce_kernel(const int32_t* __restrict__ topo, const float* __restrict__ lines,
                                                                             const float* __restrict__ gens,
                                                                             const int32_t* __restrict__ gen_list, const int n_gen,
                                                                             const double* __restrict__ pickup, const int pickup_per_grid,
                                                                             const int nchunks, const double* __restrict__ partials,
                                                                             const double* __restrict__ ycols, double* __restrict__ gen_ws,
                                                                             float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                             float* __restrict__ gg_out, double* __restrict__ gp_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int np = (int)dcn1_adjoint_partial(topo);
  const double* part = partials + (size_t)g * nchunks * np;

  const double status = dcn1_reduce_status(part, nchunks, np);
  if (status != DCN1_PART_OK) {
    const bool nan = status == DCN1_PART_NAN;
    dc_adjoint_fill(g, N, E, Gn, nan ? __builtin_nanf("") : 0.0f, gb_out, gl_out, gg_out);
    if (gp_out) for (int h = lane; h < Gn; h += PF_THREADS) gp_out[(size_t)g * Gn + h] = nan ? __builtin_nan("") : 0.0;
    return;
  }
  dcn1_reduce_buses_lines(topo, lines + (size_t)g * E * 7, nchunks, part, g, gb_out, gl_out);
  if (!gg_out && !gp_out) return;

  // a lane per listed generator: W_g in generator-index order as the forward sums it, then s_g and y_g at its own bus in the blob's
  // by-bus order
  const float* gen = gens + (size_t)g * Gn * 7;
  const double* wg = pickup ? pickup + (pickup_per_grid ? (size_t)g * Gn : 0) : nullptr;
  const double* yg = ycols + (size_t)g * n_gen * N;
  double* gw = gen_ws + (size_t)g * n_gen * DCG1_GEN;
  for (int c = lane; c < n_gen; c += PF_THREADS) {
    const int gi = gen_list[c];
    const double* y = yg + (size_t)c * N;
    double W = 0.0;
    if (wg)
      for (int h = 0; h < Gn; ++h)
        if (h != gi) W += wg[h];
    const bool shared = W > 0.0;
    double s = 0.0, own = 0.0;
    for (int i = 0; i < N; ++i)
      for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) {
        const int h = gen_idx[q];
        if (h == gi) own = y[i];
        else if (shared) s += (wg[h] / W) * y[i];
      }
    gw[c * DCG1_GEN] = shared ? (double)gen[gi * 7 + 6] / W : 0.0;
    gw[c * DCG1_GEN + 1] = s;
    gw[c * DCG1_GEN + 2] = s - own;
  }
  __threadfence_block();
  __syncthreads();

  for (int q = lane; q < Gn; q += PF_THREADS) {        // a lane per generator, in the blob's by-bus order
    const int bus = dcn1_slot_bus(gen_ptr, N, q), h = gen_idx[q];
    double dpg = dcn1_reduce_dp(part, nchunks, np, bus), dw = 0.0;
    for (int c = 0; c < n_gen; ++c) {                  // the listed generators in list order
      const double coef = gw[c * DCG1_GEN];
      if (gen_list[c] == h) dpg += gw[c * DCG1_GEN + 2];
      else if (coef != 0.0) dw += coef * (yg[(size_t)c * N + bus] - gw[c * DCG1_GEN + 1]);
    }
    if (gg_out) {
      float* row = gg_out + ((size_t)g * Gn + h) * 7;
      for (int c = 0; c < 6; ++c) row[c] = 0.0f;
      row[6] = (float)dpg;                             // Pg
    }
    if (gp_out) gp_out[(size_t)g * Gn + h] = dw;
  }
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

extern "C" int gns_dcg1_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  // the shape of the shortest lists: the width and the image depend on the blob alone
  return pf_fd_lds_query(topo_host, bytes, lanes, dcn1_adjoint_lanes, [](const int32_t* h, int) { return dcg1_adjoint_shape(h, 0, 1, 1).lds; });
}

// Whether a workgroup per (grid, chunk) or (grid, candidate) fits one launch
static bool dcg1_adjoint_launches(int64_t Bt, const Dcg1AdjointShape& s) {
  return Bt <= 0x7FFFFFFF / s.chunks_c && Bt <= 0x7FFFFFFF / s.chunks_p && Bt <= 0x7FFFFFFF / s.chunks_a && Bt <= 0x7FFFFFFF / s.n_cand;
}

extern "C" int gns_dcg1_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_line,
                                                int32_t n_gen, int32_t n_row, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_line < 0 || n_gen <= 0 || n_row <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_line > h[FH_E] || n_gen > h[FH_GN]) return GNS_EINVAL;
  const Dcg1AdjointShape s = dcg1_adjoint_shape(h, n_line, n_gen, n_row);
  if (!dcg1_adjoint_launches(Bt, s)) return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = dcg1_adjoint_ws_bytes(h, Bt, n_gen, n_row, s);
  return GNS_OK;
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_dcg1_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const int32_t* line_host, const int32_t* line_dev, int32_t n_line,
                                const int32_t* gen_host, const int32_t* gen_dev, int32_t n_gen,
                                const int32_t* row_cols_host, const int32_t* row_cols_dev, int32_t n_row, const uint8_t* islanding,
                                const double* rating, int32_t rating_per_grid, const double* pickup, int32_t pickup_per_grid,
                                const int32_t* worst_line, const uint8_t* converged,
                                const double* grad_line_flow, const double* grad_worst_loading,
                                float* grad_buses, float* grad_lines, float* grad_generators, double* grad_pickup,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || (n_line > 0 && !line_dev) || !gen_dev ||
      !row_cols_dev || !islanding || !worst_line || !converged || (rating_per_grid != 0 && rating_per_grid != 1) ||
      (pickup_per_grid != 0 && pickup_per_grid != 1))
    return GNS_EINVAL;
  int lanes_f = 0;
  int64_t lds_f = 0;
  const int rc = dcg1_check(cfg, topo_host, line_host, n_line, gen_host, n_gen, row_cols_host, n_row, &lanes_f, &lds_f);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const Dcg1AdjointShape s = dcg1_adjoint_shape(h, n_line, n_gen, n_row);
  if (!dcg1_adjoint_launches(Bt, s)) return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_buses && !grad_lines && !grad_generators && !grad_pickup) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcg1_adjoint_ws_bytes(h, Bt, n_gen, n_row, s)) return GNS_ESIZE;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  const int E = h[FH_E], n_cand = (int)s.n_cand;
  double* ws = static_cast<double*>(workspace);
  const Dcg1AdjointWorkspace a = dcg1_adjoint_workspace(ws + dcn2_ws_bytes(h, Bt, n_cand) / sizeof(double), h, Bt, n_gen, n_row, s);
  int rl = pf_launch<gns_dcg1_factor_kernel>(Bt * s.chunks_c, s.lds_factor, stream, topo, buses, lines, generators, line_dev, (int)n_line,
                                             gen_dev, (int)n_gen, pickup, (int)pickup_per_grid, (int)Bt, s.lanes_f, (int)s.chunks_c, ws,
                                             a.conv);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcg1_adjoint_row_kernel>(Bt * s.chunks_p, 32 * (int64_t)E, stream, line_dev, (int)n_line, (int)n_gen, row_cols_dev,
                                              (int)n_row, islanding, rating, (int)rating_per_grid, worst_line, converged, grad_line_flow,
                                              grad_worst_loading, E, (int)Bt, s.Q, (int)s.chunks_p, (const double*)ws, a.rec, a.gf_part);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcg1_adjoint_gather_kernel>(Bt * n_cand, 8 * (int64_t)E, stream, line_dev, (int)n_line, (int)n_gen, row_cols_dev,
                                                 (int)n_row, converged, grad_line_flow, E, (int)Bt, (const double*)ws,
                                                 (const double*)a.rec, a.T, a.others);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcn2_adjoint_solve_kernel>(Bt * s.chunks_a, s.lds_solve, stream, topo, buses, lines, generators, line_dev, (int)n_line,
                                                n_cand, a.ycols, converged, (int)Bt, s.lanes, (int)s.chunks_a, (int)s.chunks_p,
                                                (const double*)ws, (const double*)a.T, (const double*)a.gf_part,
                                                (const double*)a.others, a.gf, a.part);
  if (rl != GNS_OK) return rl;
  return pf_launch<gns_dcg1_adjoint_reduce_kernel>(Bt, 0, stream, topo, lines, generators, gen_dev, (int)n_gen, pickup,
                                                   (int)pickup_per_grid, (int)s.chunks_a, (const double*)a.part, (const double*)a.ycols,
                                                   a.gen, grad_buses, grad_lines, grad_generators, grad_pickup);
}
