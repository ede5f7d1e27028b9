// What the DC screens that run a factor kernel and then a streaming row kernel share (gns_dcn2.hip: double outages; gns_dcg1.hip:
// generator and generator-plus-line outages), on top of gns_dcn1_device.h.  A screen of this shape has candidates (lines, then
// generators), each with one solve on the base factor, and rows that each combine two of them.  Here: the workspace, the factor
// kernel, the skeletons of the row kernel, the adjoint's row kernel and its gather kernel, the kernel that solves the adjoint's
// columns on the base factor, and the host code of the entry points after their own argument and list checks.  A screen brings its
// row model, the type Rows (Dcn2Pairs, Dcg1Rows): the lists of the call {line_list, n_line, n_gen, cols} (the candidate lines, the
// numbers of candidate lines and generators, the rows' two columns), which a kernel takes as __restrict__ parameters, with
//   NOUT, REC      the lines a row takes out at most; the doubles of a row's record in the adjoint's workspace: the row's own
//                  REC - 2 first, then the worst-line term and (contributes, worst line) as two ints
//   n_cand()       the candidates of the call
//   Row            the state of one row, a DcrowOut<NOUT> (the lines that are out, -1 for none, and in the adjoint dl/dF there):
//                    place(s, p)         whether row p of the list is well formed; keeps its candidate positions
//                    solve(s, base)      the row's scalars from the grid's base case, the same on every lane; whether the row is solved
//                    flow(base, l)       the post-outage flow of a line that stays
//                    Sums, ga_term(base, x, l)   what x = G_l b_l of a line that stays adds to the row's sums ga
//                    close(ga)           v, dl/dF at the lines that are out, from the wave's ga
//                    record(rec)         the row's own doubles of its record
//   holds(p, c)    whether row p holds candidate c
//   held(p, c, rec)  for the gather of candidate c over a contributing row p: a_c, the factor of G_l in the candidate's sum, and the
//                  lines that are out with v from the record (a DcrowHeld<NOUT>)
// Everything else is written once below: the grid's status, the LDS image, the NaN / -1 rows, the worst-loading reduction, the
// record of a row that adds nothing, the ownership of the LDS sums by lane l mod 64, the scan of the list 64 rows at a time and the
// chunk's status.
#pragma once
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

size_t dcn2_ws_bytes(const int32_t* h, int64_t Bt, int64_t n_cand) {
  const int64_t E = h[FH_E];
  return ((size_t)Bt * (size_t)(n_cand * E + 2 * E + n_cand + 1) * sizeof(double) + 255) & ~(size_t)255;
}

// Rows (pairs) a workgroup of the row kernel takes one after the other: from the length of the list alone
int dcn2_pairs_per_wave(int64_t n_pair) { return n_pair >= 8192 ? 32 : 8; }

// The candidates of a call: n_line lines (ascending), then n_gen generators (ascending; none in the N-2 screen) with the pickup
// weights [Gn] or [Bt][Gn] that share a lost unit's output (NULL: the slack picks it up)
struct DcrowCands {
  const int32_t* line;
  int n_line;
  const int32_t* gen;
  int n_gen;
  const double* pickup;
  int pickup_per_grid;
  __host__ __device__ int count() const { return n_line + n_gen; }
};

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

// One wave per (grid, chunk of W candidates) with the N-1 screen's prologue, image and lane solve: a line lane solves z_k as that
// screen does, bit for bit; a generator lane writes the change of the injections into its column and runs the same solve program.
// A pass with a line per lane then stores z[f_l] - z[t_l] of every candidate contiguously into the workspace, with a finite flag
// per candidate; chunk 0 also stores the base flows F_l, b_l and the grid's status.
__global__ __launch_bounds__(PF_THREADS) void gns_dcrow_factor_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                      const float* __restrict__ lines, const float* __restrict__ gens,
                                                                      const DcrowCands cands, const int Bt, const int W,
                                                                      const int nchunks, double* __restrict__ ws,
                                                                      uint8_t* __restrict__ conv_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int n_line = cands.n_line, n_cand = cands.count();
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
      const int e = cands.line[c];
      int2 en;
      if (e >= 0 && e < E) fin = dcn1_lane_z(topo, m, e, m.Z + lane, ld, en);
    } else {
      const int gi = cands.gen[c - n_line];
      const double* wg = cands.pickup ? cands.pickup + (cands.pickup_per_grid ? (size_t)g * Gn : 0) : nullptr;
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

// ---- the row models' parts

// A grid's base case as a row reads it: F_l and b_l (in LDS), the candidates' rows of H and their finite flags (in the workspace)
struct DcrowBase {
  const double* F;
  const double* b;
  const double* H;
  const double* fin;
  int E;
};

// The lines a row takes out (-1: none there) and, in the adjoint, dl/dF at each of them
template <int NOUT>
struct DcrowOut {
  int e[NOUT];
  double v[NOUT];
  __device__ __forceinline__ bool out(const int l) const {
    bool o = false;
#pragma unroll
    for (int i = 0; i < NOUT; ++i) o |= l == e[i];
    return o;
  }
};

// What the gather of a candidate takes from a contributing row: the factor of G_l, and the lines that are out with v
template <int NOUT>
struct DcrowHeld : DcrowOut<NOUT> {
  double a_c;
};

// The sums ga of a row, each over the lines that stay: per lane, then over the wave by the shuffle tree, the sums side by side
template <int NA>
struct DcrowSums {
  double s[NA];
  __device__ __forceinline__ void operator+=(const DcrowSums& o) {
#pragma unroll
    for (int a = 0; a < NA; ++a) s[a] += o.s[a];
  }
  __device__ __forceinline__ void wave_sum() {
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int a = 0; a < NA; ++a) s[a] += __shfl_xor(s[a], o);
    }
  }
};

// (contributes, worst line) of a row's record
__device__ __forceinline__ int2& dcrow_rec_status(double* rec, const int REC) { return reinterpret_cast<int2*>(rec)[REC - 1]; }
__device__ __forceinline__ int2 dcrow_rec_status(const double* rec, const int REC) { return reinterpret_cast<const int2*>(rec)[REC - 1]; }

// The LDS image of a row workgroup: the grid's F, b and the rating (1 without one), [E] each, and in the adjoint the chunk's sum of
// dl/dF_l, zeroed; lane l mod 64 alone touches entry l of that
struct DcrowImage {
  double* F;
  double* b;
  double* rt;
  double* gF;
};

template <bool ADJOINT>
__device__ __forceinline__ DcrowImage dcrow_image(double* lds, const Dcn2Workspace& w, const int g, const int E, const double* rating,
                                                  const int rating_per_grid) {
  DcrowImage m;
  m.F = lds;
  m.b = m.F + E;
  m.rt = m.b + E;
  m.gF = m.rt + E;
  const double* rt_in = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  for (int l = threadIdx.x; l < E; l += PF_THREADS) {
    m.F[l] = w.F[(size_t)g * E + l];
    m.b[l] = w.b[(size_t)g * E + l];
    m.rt[l] = rt_in ? rt_in[l] : 1.0;
    if (ADJOINT) m.gF[l] = 0.0;
  }
  __syncthreads();
  return m;
}

// ---- the forward's row kernel: one wave per (grid, chunk of Q consecutive rows).  F, b and the rating sit in LDS (24 E bytes); per
// row the scalars are computed identically on every lane, a line per lane forms F'_l from the candidates' contiguous rows of H (an
// optional contiguous store), and the wave reduction of gns_dcn1_kernel finishes the row.
template <class Rows>
__global__ __launch_bounds__(PF_THREADS) void gns_dcrow_kernel(const int32_t* __restrict__ line_list, const int n_line, const int n_gen,
                                                               const int32_t* __restrict__ cols, const int P, const uint8_t* __restrict__ islanding,
                                                               const double* __restrict__ rating, const int rating_per_grid,
                                                               const int E, const int Bt, const int Q, const int nchunks,
                                                               const double* __restrict__ ws, double* __restrict__ fl_out,
                                                               double* __restrict__ wl_out, int32_t* __restrict__ wi_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const Rows s = {line_list, n_line, n_gen, cols};
  const int n_cand = s.n_cand();
  const int g = blockIdx.x / nchunks, p0 = (blockIdx.x % nchunks) * Q;
  const int np = min(Q, P - p0);
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);

  if (w.status[g] == 0.0) {                      // the base solve failed: every row of the grid is NaN / -1
    dcn1_rows_not_solved(g, P, E, p0, np, fl_out, wl_out, wi_out);
    return;
  }
  const DcrowImage m = dcrow_image<false>(lds, w, g, E, rating, rating_per_grid);
  const DcrowBase base = {m.F, m.b, w.H + (size_t)g * n_cand * E, w.fin + (size_t)g * n_cand, E};
  for (int q = 0; q < np; ++q) {
    const int p = p0 + q;
    typename Rows::Row r;
    if (!(r.place(s, p) && !islanding[p] && r.solve(s, base))) { dcn1_rows_not_solved(g, P, E, p, 1, fl_out, wl_out, wi_out); continue; }
    const size_t row = (size_t)g * P + p;
    double best = -1.0;
    int bi = INT32_MAX;
    for (int l = lane; l < E; l += PF_THREADS) {
      const double fl = r.out(l) ? 0.0 : r.flow(base, l);
      if (fl_out) fl_out[row * E + l] = fl;
      const double v = fabs(fl) / m.rt[l];
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

// ---- the adjoint's row kernel: one wave per (grid, chunk of Q consecutive rows), the forward's chunks.  Per row the forward's
// scalars again, G from the incoming gradients, ga by the wave's shuffle tree (a line per lane with grad_line_flow, one term
// without), v from ga; a record per (grid, row) and the chunk's partial of gF [E + 1], the last entry the chunk's status.
template <class Rows>
__global__ __launch_bounds__(PF_THREADS) void gns_dcrow_adjoint_kernel(const int32_t* __restrict__ line_list, const int n_line, const int n_gen,
                                                                       const int32_t* __restrict__ cols, const int P,
                                                                       const uint8_t* __restrict__ islanding,
                                                                       const double* __restrict__ rating, const int rating_per_grid,
                                                                       const int32_t* __restrict__ wi_in,
                                                                       const uint8_t* __restrict__ conv_in,
                                                                       const double* __restrict__ gfl, const double* __restrict__ gwl,
                                                                       const int E, const int Bt, const int Q, const int nchunks,
                                                                       const double* __restrict__ ws, double* __restrict__ rec_out,
                                                                       double* __restrict__ gf_part) {
  constexpr int NOUT = Rows::NOUT, REC = Rows::REC;
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const Rows s = {line_list, n_line, n_gen, cols};
  const int n_cand = s.n_cand();
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
  const DcrowImage m = dcrow_image<true>(lds, w, g, E, rating, rating_per_grid);
  const DcrowBase base = {m.F, m.b, w.H + (size_t)g * n_cand * E, w.fin + (size_t)g * n_cand, E};
  double* gF = m.gF;
  unsigned long long unsolved = 0;               // the chunk's rows the forward left NaN / -1
  for (int q = 0; q < np; ++q) {
    const int p = p0 + q;
    const size_t row = (size_t)g * P + p;
    double* rec = rec_out + row * REC;
    typename Rows::Row r;
    if (!(r.place(s, p) && !islanding[p] && r.solve(s, base))) {   // the forward's row, expression for expression: skipped, never
      unsolved |= 1ull << q;                                       // multiplied by zero
      if (lane == 0) dcrow_rec_status(rec, REC) = make_int2(0, -1);
      continue;
    }
    // d|F'_w| / rating_w at the line the forward found worst: the sign of its flow
    const double gw = gwl ? gwl[row] : 0.0;
    const int wl_in = wi_in[row];
    int wl = -1;
    double gterm = 0.0;
    if (gw != 0.0 && wl_in >= 0 && wl_in < E && !r.out(wl_in)) {
      gterm = dcn1_worst_term(gw, r.flow(base, wl_in), m.rt[wl_in]);
      wl = wl_in;
    }
    // ga: the sums of G_l b_l H[l] over the lines that stay, and gF_l += G_l
    typename Rows::Row::Sums ga = {};
    bool has = false;
    if (gfl) {
      const double* grow = gfl + row * E;
      for (int l = lane; l < E; l += PF_THREADS) {
        if (r.out(l)) continue;
        const double G = l == wl ? grow[l] + gterm : grow[l];
        if (G == 0.0) continue;
        has = true;
        gF[l] += G;
        ga += r.ga_term(base, G * m.b[l], l);
      }
      ga.wave_sum();
      has = __ballot(has) != 0;
    } else if (wl >= 0 && gterm != 0.0) {
      has = true;
      if ((wl & (PF_THREADS - 1)) == lane) gF[wl] += gterm;
      ga = r.ga_term(base, gterm * m.b[wl], wl);
    }
    if (!has) {                                  // a zero incoming gradient: the row adds nothing
      if (lane == 0) dcrow_rec_status(rec, REC) = make_int2(0, -1);
      continue;
    }
    r.close(ga);                                 // v: dl/dF at the lines that are out
#pragma unroll
    for (int i = 0; i < NOUT; ++i)
      if (r.e[i] >= 0 && (r.e[i] & (PF_THREADS - 1)) == lane) gF[r.e[i]] += r.v[i];
    if (lane == 0) {
      r.record(rec);
      rec[REC - 2] = gterm;
      dcrow_rec_status(rec, REC) = make_int2(1, wl);
    }
  }
  // an unsolved row with a non-zero incoming gradient: the grid's gradient is NaN
  const bool nan = dcn1_rows_nonzero(unsolved, row0, E, gfl, gwl);
  for (int l = lane; l < E; l += PF_THREADS) part[l] = gF[l];
  if (lane == 0) part[E] = nan ? DCN1_PART_NAN : DCN1_PART_OK;
}

// ---- the adjoint's gather kernel: one wave per (grid, candidate).  It scans the row list 64 rows at a time, takes the rows that
// hold its candidate in list order and sums T_c[l] = sum_p G_pl a_pc, plus v a_pc at the lines that are out, a line per lane; and
// it counts the contributing rows of the grid that do not hold the candidate.
template <class Rows>
__global__ __launch_bounds__(PF_THREADS) void gns_dcrow_adjoint_gather_kernel(const int32_t* __restrict__ line_list, const int n_line, const int n_gen,
                                                                              const int32_t* __restrict__ cols, const int P,
                                                                              const uint8_t* __restrict__ conv_in,
                                                                              const double* __restrict__ gfl, const int E, const int Bt,
                                                                              const double* __restrict__ ws,
                                                                              const double* __restrict__ rec_in, double* __restrict__ T_out,
                                                                              double* __restrict__ others_out) {
  constexpr int NOUT = Rows::NOUT, REC = Rows::REC;
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const Rows s = {line_list, n_line, n_gen, cols};
  const int n_cand = s.n_cand();
  const int g = blockIdx.x / n_cand, c = blockIdx.x % n_cand;
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);
  if (!conv_in[g] || w.status[g] == 0.0) return;            // no records, and nothing reads T of this grid
  double* T = lds;                                          // [E]; lane l mod 64 alone touches entry l
  for (int l = lane; l < E; l += PF_THREADS) T[l] = 0.0;

  int others = 0;                                           // contributing rows of the grid that do not hold c
  for (int p0 = 0; p0 < P; p0 += PF_THREADS) {
    const int pm = p0 + lane;
    bool mine = false, other = false;
    if (pm < P) {
      mine = s.holds(pm, c);
      other = !mine && dcrow_rec_status(rec_in + ((size_t)g * P + pm) * REC, REC).x != 0;
    }
    others += __popcll(__ballot(other));
    for (unsigned long long todo = __ballot(mine); todo; todo &= todo - 1) {   // the rows that hold c, in list order
      const int p = p0 + __ffsll((long long)todo) - 1;
      const size_t row = (size_t)g * P + p;
      const double* rec = rec_in + row * REC;
      const int2 st = dcrow_rec_status(rec, REC);
      if (!st.x) continue;
      const DcrowHeld<NOUT> h = s.held(p, c, rec);
      const double a_c = h.a_c, gterm = rec[REC - 2];
      if (gfl) {
        const double* grow = gfl + row * E;
        for (int l = lane; l < E; l += PF_THREADS) {
          if (h.out(l)) continue;
          const double G = l == st.y ? grow[l] + gterm : grow[l];
          if (G != 0.0) T[l] += G * a_c;
        }
      } else if (st.y >= 0 && (st.y & (PF_THREADS - 1)) == lane) {
        T[st.y] += gterm * a_c;
      }
      // the lines that are out: v a_c
#pragma unroll
      for (int i = 0; i < NOUT; ++i)
        if (h.e[i] >= 0 && (h.e[i] & (PF_THREADS - 1)) == lane) T[h.e[i]] += h.v[i] * a_c;
    }
  }
  double* out = T_out + ((size_t)g * n_cand + c) * E;
  for (int l = lane; l < E; l += PF_THREADS) out[l] = T[l];
  if (lane == 0) others_out[(size_t)g * n_cand + c] = (double)others;
}

// ---- what the adjoints of the screens with a factor kernel share (gns_dcn2_adjoint, gns_dcg1_adjoint): the solves on the base factor

// Lane j's own right-hand side sum_l x_l b_l m_l of the row x [E] into column uc, a few entries fetched ahead; whether any x_l is
// not exactly zero
__device__ __forceinline__ bool dcn2_lane_rhs(const Dcn1Image& m, const int E, const int d1, const double* x, double* uc, const int ld) {
  for (int s = 0; s < d1; ++s) uc[s * ld] = 0.0;
  bool has = false;
  for (int l0 = 0; l0 < E; l0 += DCN1_PREFETCH) {
    double xv[DCN1_PREFETCH];
#pragma unroll
    for (int u = 0; u < DCN1_PREFETCH; ++u) xv[u] = x[min(l0 + u, E - 1)];
#pragma unroll
    for (int u = 0; u < DCN1_PREFETCH; ++u) {
      const int l = l0 + u;
      if (l >= E || xv[u] == 0.0) continue;
      has = true;
      const int2 en = m.ends[l];
      if (en.x == en.y) continue;                             // m_l = 0
      const double y = xv[u] * m.lb[l];
      if (en.x >= 0) uc[en.x * ld] += y;
      if (en.y >= 0) uc[en.y * ld] -= y;
    }
  }
  return has;
}

// One wave per (grid, chunk of W columns): column 0 is y_0 from gF, column c + 1 is y_c from row c of T_in, each solved by its own
// lane on the base factor; then a line per lane forms the chunk's partial.  The first n_own of the n_cand candidates are the lines
// cand lists (ascending); the rest (the generator screen's generators) have rows of H and T_in like them but no own line, and their
// y goes by bus into ycols [Bt][n_cand - n_own][N] for the reduce kernel.
__global__ __launch_bounds__(PF_THREADS) void gns_dcn2_adjoint_solve_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                            const float* __restrict__ lines, const float* __restrict__ gens,
                                                                            const int32_t* __restrict__ cand, const int n_own, const int n_cand,
                                                                            double* __restrict__ ycols,
                                                                            const uint8_t* __restrict__ conv_in,
                                                                            const int Bt, const int W, const int nchunks,
                                                                            const int nchunks_p, const double* __restrict__ ws,
                                                                            const double* __restrict__ T_in,
                                                                            const double* __restrict__ gf_part,
                                                                            const double* __restrict__ others, double* __restrict__ gf,
                                                                            double* __restrict__ partials) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / nchunks, k0 = (blockIdx.x % nchunks) * W;
  const int nk = min(W, n_cand + 1 - k0);                    // column 0 is y_0, column c + 1 candidate c
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const Dcn1Image m = dcn1_image(topo, lds);
  const int ld = W + 1;
  double* U = m.Z + d1 * ld;                                 // [d1][ld] the columns' right-hand sides, then y
  int* o_has = reinterpret_cast<int*>(U + d1 * ld);          // [W] whether the column holds anything
  const int np = (int)dcn1_adjoint_partial(topo);
  double* part = partials + (size_t)blockIdx.x * np;         // [N] dl/dP, [E] dl/db, [E] sum of w, the status
  const float* line = lines + (size_t)g * E * 7;
  const Dcn2Workspace w = dcn2_workspace(const_cast<double*>(ws), Bt, n_cand, E);

  // the pair chunks' statuses: one that is NaN makes the grid's gradient NaN
  bool nan = false;
  for (int q = lane; q < nchunks_p; q += PF_THREADS) nan |= gf_part[((size_t)g * nchunks_p + q) * (E + 1) + E] == DCN1_PART_NAN;
  nan = __ballot(nan) != 0;
  if (!conv_in[g] || w.status[g] == 0.0 ||
      !dcn1_base_case(topo, buses + (size_t)g * N * 6, line, gens + (size_t)g * Gn * 7, m, lane)) {
    dcn1_partial_none(part, np, nan ? DCN1_PART_NAN : DCN1_PART_UNSOLVED_ZERO);
    return;
  }
  if (nan) { dcn1_partial_none(part, np, DCN1_PART_NAN); return; }

  // chunk 0: gF_l, the pair chunks' partials summed in order, for lane 0's right-hand side and the pass below
  double* gfg = gf + (size_t)g * E;
  if (k0 == 0) {
    for (int l = lane; l < E; l += PF_THREADS) {
      double s = 0.0;
      for (int q = 0; q < nchunks_p; ++q) s += gf_part[((size_t)g * nchunks_p + q) * (E + 1) + l];
      gfg[l] = s;
    }
    __syncthreads();
  }

  // lane j: the right-hand side of column k0 + j and its solve on the base factor
  const double* Tg = T_in + (size_t)g * n_cand * E;
  bool has = false, bad = false;
  if (lane < nk) {
    const int col = k0 + lane;
    double* uc = U + lane;
    has = dcn2_lane_rhs(m, E, d1, col == 0 ? gfg : Tg + (size_t)(col - 1) * E, uc, ld);
    if (has) {
      dcn1_lane_solve(topo[FH_NOPS_S1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]), m.F, nnz1, uc, ld);
      bool fin = true;
      for (int s = 0; s < d1; ++s) fin &= pf_finite(uc[s * ld]);
      bad = !fin;
    }
  }
  if (lane < W) o_has[lane] = has;
  __syncthreads();
  if (__ballot(bad)) { dcn1_partial_none(part, np, DCN1_PART_NAN); return; }

  // a line per lane over the chunk's columns in order.  Column 0: w = gF - (y0_f - y0_t), dl/db += w (theta_f - theta_t - shift), the
  // sum of w gives dl/dshift = -b sum w.  Column c + 1: dl/db += H_c[l] (T'_c[l] - (y_f - y_t)).
  // A pair gives nothing to its own two lines: through the shared solves that zero is reached to rounding only, so a candidate line
  // that every contributing pair of the grid holds (an empty sum over the others) gets the exact zero.
  const double* Hg = w.H + (size_t)g * n_cand * E;
  for (int l = lane; l < E; l += PF_THREADS) {
    int c = 0, hi = n_own;                                   // the candidate of line l, if it is one: cand ascends
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (cand[mid] <= l) c = mid;
      else hi = mid;
    }
    if (n_own > 0 && cand[c] == l && others[(size_t)g * n_cand + c] == 0.0) {
      part[N + l] = 0.0;
      part[N + E + l] = 0.0;
      continue;
    }
    const int2 en = m.ends[l];
    const double thf = en.x >= 0 ? m.rhs[en.x] : 0.0, tht = en.y >= 0 ? m.rhs[en.y] : 0.0;
    const double sh = (double)line[l * 7 + 6];
    double d_b = 0.0, sw = 0.0;
    for (int j = 0; j < nk; ++j) {
      if (!o_has[j]) continue;
      const double yf = en.x >= 0 ? U[en.x * ld + j] : 0.0, yt = en.y >= 0 ? U[en.y * ld + j] : 0.0;
      if (k0 + j == 0) {
        const double x = gfg[l] - (yf - yt);
        d_b += x * ((thf - tht) - sh);
        sw += x;
      } else {
        const size_t at = (size_t)(k0 + j - 1) * E + l;
        d_b += Hg[at] * (Tg[at] - (yf - yt));
      }
    }
    part[N + l] = d_b;
    part[N + E + l] = sw;
  }
  // a bus per lane: dl/dP_i = y0[i], 0 at the slack
  for (int i = lane; i < N; i += PF_THREADS) {
    const int p = p_idx[i];
    part[i] = k0 == 0 && p >= 0 && o_has[0] ? U[p * ld] : 0.0;
  }
  // the columns without an own line: y by bus, 0 at the slack and for a column that holds nothing
  for (int j = max(n_own + 1 - k0, 0); j < nk; ++j) {
    double* y = ycols + ((size_t)g * (n_cand - n_own) + (k0 + j - 1 - n_own)) * N;
    for (int i = lane; i < N; i += PF_THREADS) {
      const int p = p_idx[i];
      y[i] = p >= 0 && o_has[j] ? U[p * ld + j] : 0.0;
    }
  }
  if (lane == 0) part[np - 1] = DCN1_PART_OK;
}
// ---- host: what the entry points of the two screens share after their own argument and list checks

// What a call passes to its launches whatever the screen
struct DcrowCall {
  const int32_t* topo;
  const float* buses;
  const float* lines;
  const float* gens;
  int64_t Bt;
  const uint8_t* islanding;
  const double* rating;
  int rating_per_grid;
  void* stream;
};

inline int dcrow_launch_factor(const DcrowCall& c, const DcrowCands& cands, int64_t nchunks, int lanes, int64_t lds, double* ws,
                               uint8_t* conv) {
  return pf_launch<gns_dcrow_factor_kernel>(c.Bt * nchunks, lds, c.stream, c.topo, c.buses, c.lines, c.gens, cands, (int)c.Bt, lanes,
                                            (int)nchunks, ws, conv);
}

// The head of a *_workspace_bytes query: GNS_EINVAL unless the call's own arguments are in order (args_ok), the blob is an FD blob of
// cfg's shape and it has that many lines and generators
inline int dcrow_counts_check(const gns_pf_config* cfg, const void* topo_host, bool args_ok, int64_t n_line, int64_t n_gen) {
  if (!cfg || !topo_host || !args_ok) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h)) return GNS_EINVAL;
  if (n_line > h[FH_E] || n_gen > h[FH_GN]) return GNS_EINVAL;
  return GNS_OK;
}

// gns_dcn2_workspace_bytes / gns_dcg1_workspace_bytes
inline int dcrow_ws_query(const gns_pf_config* cfg, const void* topo_host, bool args_ok, int64_t Bt, int64_t n_line, int64_t n_gen,
                          size_t* bytes) {
  const int rc = dcrow_counts_check(cfg, topo_host, args_ok, n_line, n_gen);
  if (rc != GNS_OK) return rc;
  *bytes = dcn2_ws_bytes(static_cast<const int32_t*>(topo_host), Bt, n_line + n_gen);
  return GNS_OK;
}

// gns_dcn2_screen / gns_dcg1_screen: the chunks, the LDS image of the factor kernel (the N-1 screen's), the workspace, two launches
template <class Rows>
int dcrow_screen(const int32_t* h, const DcrowCall& c, const DcrowCands& cands, const Rows& rows, int64_t n_row, double* line_flow,
                 double* worst_loading, int32_t* worst_line, uint8_t* converged, void* workspace, size_t workspace_bytes) {
  const int64_t n_cand = cands.count();
  const int lanes = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES), Q = dcn2_pairs_per_wave(n_row);
  int64_t nchunks_c = 0, nchunks_p = 0;
  if (!pf_chunks(n_cand, lanes, c.Bt, &nchunks_c) || !pf_chunks(n_row, Q, c.Bt, &nchunks_p)) return GNS_EINVAL;
  const int64_t lds = dcn1_lds_bytes(h, lanes);
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcn2_ws_bytes(h, c.Bt, n_cand)) return GNS_ESIZE;
  double* ws = static_cast<double*>(workspace);
  const int rc = dcrow_launch_factor(c, cands, nchunks_c, lanes, lds, ws, converged);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_dcrow_kernel<Rows>>(c.Bt * nchunks_p, 24 * (int64_t)h[FH_E], c.stream, rows.line_list, rows.n_line, rows.n_gen,
                                           rows.cols, (int)n_row, c.islanding, c.rating, c.rating_per_grid, (int)h[FH_E], (int)c.Bt, Q,
                                           (int)nchunks_p, (const double*)ws, line_flow, worst_loading, worst_line);
}

// The launch shape of an adjoint: the forward's row chunks, the N-1 adjoint's width over n_cand + 1 columns, and the largest LDS
// image of its kernels
struct DcrowAdjointShape {
  int Q, lanes, lanes_f;
  int64_t n_cand, chunks_c, chunks_p, chunks_a, lds_factor, lds_solve, lds;
};

inline DcrowAdjointShape dcrow_adjoint_shape(const int32_t* h, int64_t n_cand, int64_t n_row) {
  DcrowAdjointShape s;
  s.n_cand = n_cand;
  s.Q = dcn2_pairs_per_wave(n_row);
  s.lanes = dcn1_adjoint_lanes(h, GNS_PF_LDS_MAX_BYTES);
  s.lanes_f = dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES);
  s.chunks_c = (n_cand + s.lanes_f - 1) / s.lanes_f;
  s.chunks_p = (n_row + s.Q - 1) / s.Q;
  s.chunks_a = (n_cand + 1 + s.lanes - 1) / s.lanes;
  s.lds_factor = dcn1_lds_bytes(h, s.lanes_f);
  s.lds_solve = dcn1_adjoint_lds_bytes(h, s.lanes);
  s.lds = s.lds_solve > 32 * (int64_t)h[FH_E] ? s.lds_solve : 32 * (int64_t)h[FH_E];
  return s;
}

// Whether a workgroup per (grid, chunk) or (grid, candidate) fits one launch
inline bool dcrow_adjoint_launches(int64_t Bt, const DcrowAdjointShape& s) {
  return Bt <= 0x7FFFFFFF / s.chunks_c && Bt <= 0x7FFFFFFF / s.chunks_p && Bt <= 0x7FFFFFFF / s.chunks_a && Bt <= 0x7FFFFFFF / s.n_cand;
}

// gns_dcn2_adjoint_lds_bytes / gns_dcg1_adjoint_lds_bytes: the shape of the shortest lists, for the width and the image depend on
// the blob alone
inline int dcrow_adjoint_lds_query(const void* topo_host, int64_t* bytes, int32_t* lanes) {
  return pf_fd_lds_query(topo_host, bytes, lanes, dcn1_adjoint_lanes, [](const int32_t* h, int) { return dcrow_adjoint_shape(h, 1, 1).lds; });
}

// An adjoint's workspace after the forward's block (dcn2_ws_bytes, itself a multiple of 256 bytes), all doubles but the last: T
// [Bt][n_cand][E], the records [Bt][n_row][rec], the row chunks' partials of gF [Bt][chunks_p][E + 1] (the last one the chunk's
// status), gF [Bt][E], per candidate the number of contributing rows that do not hold it [Bt][n_cand], the solve kernel's partials
// [Bt][chunks_a][N + 2 E + 1], then the screen's own blocks (own doubles in all; none in the N-2 screen) and the factor kernel's
// converged bytes [Bt]
struct DcrowAdjointWorkspace {
  double* T;
  double* rec;
  double* gf_part;
  double* gf;
  double* others;
  double* part;
  double* own;
  uint8_t* conv;
};

inline int64_t dcrow_adjoint_doubles(const int32_t* h, int64_t Bt, int64_t rec, int64_t n_row, const DcrowAdjointShape& s) {
  const int64_t E = h[FH_E];
  return Bt * (s.n_cand * E + n_row * rec + s.chunks_p * (E + 1) + E + s.n_cand + s.chunks_a * dcn1_adjoint_partial(h));
}

inline DcrowAdjointWorkspace dcrow_adjoint_workspace(double* ws, const int32_t* h, int64_t Bt, int64_t rec, int64_t n_row,
                                                     const DcrowAdjointShape& s, int64_t own) {
  const int64_t E = h[FH_E];
  DcrowAdjointWorkspace w;
  w.T = ws;
  w.rec = w.T + Bt * s.n_cand * E;
  w.gf_part = w.rec + Bt * n_row * rec;
  w.gf = w.gf_part + Bt * s.chunks_p * (E + 1);
  w.others = w.gf + Bt * E;
  w.part = w.others + Bt * s.n_cand;
  w.own = w.part + Bt * s.chunks_a * dcn1_adjoint_partial(h);
  w.conv = reinterpret_cast<uint8_t*>(w.own + own);
  return w;
}

inline size_t dcrow_adjoint_ws_bytes(const int32_t* h, int64_t Bt, int64_t rec, int64_t n_row, const DcrowAdjointShape& s, int64_t own) {
  const size_t after = (size_t)(dcrow_adjoint_doubles(h, Bt, rec, n_row, s) + own) * sizeof(double) + (size_t)Bt;
  return dcn2_ws_bytes(h, Bt, s.n_cand) + ((after + 255) & ~(size_t)255);
}

// gns_dcn2_adjoint_workspace_bytes / gns_dcg1_adjoint_workspace_bytes; own_per_grid: the doubles of the screen's own blocks per grid
inline int dcrow_adjoint_ws_query(const gns_pf_config* cfg, const void* topo_host, bool args_ok, int64_t Bt, int64_t n_line,
                                  int64_t n_gen, int64_t n_row, int64_t rec, int64_t own_per_grid, size_t* bytes) {
  const int rc = dcrow_counts_check(cfg, topo_host, args_ok, n_line, n_gen);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const DcrowAdjointShape s = dcrow_adjoint_shape(h, n_line + n_gen, n_row);
  if (!dcrow_adjoint_launches(Bt, s)) return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = dcrow_adjoint_ws_bytes(h, Bt, rec, n_row, s, Bt * own_per_grid);
  return GNS_OK;
}

// gns_dcn2_adjoint / gns_dcg1_adjoint up to their own reduce launch: the shape, the launch limit, the LDS image, "nothing asked
// for" (GNS_OK without a launch, after every other check; a->T stays NULL then), the workspace, and the first four launches:
//   factor   gns_dcrow_factor_kernel again, into the adjoint's own workspace: H, F, b, the flags and the status are the forward's bits
//   row      gns_dcrow_adjoint_kernel: a record per (grid, row) and the chunks' partials of gF
//   gather   gns_dcrow_adjoint_gather_kernel: T per (grid, candidate)
//   solve    gns_dcn2_adjoint_solve_kernel: the chunks' partials for the reduce kernel, and the generators' y by bus into the first
//            of the screen's own blocks
// No atomics, every sum in a fixed order.
template <class Rows>
int dcrow_adjoint_launch(const int32_t* h, const DcrowCall& c, const DcrowCands& cands, const Rows& rows, int64_t n_row,
                         int64_t own_per_grid, bool asked, const int32_t* worst_line, const uint8_t* converged,
                         const double* grad_line_flow, const double* grad_worst_loading, void* workspace, size_t workspace_bytes,
                         DcrowAdjointShape* shape, DcrowAdjointWorkspace* a) {
  const int64_t Bt = c.Bt, own = Bt * own_per_grid;
  const int n_cand = cands.count(), E = h[FH_E];
  const DcrowAdjointShape s = dcrow_adjoint_shape(h, n_cand, n_row);
  *shape = s;
  a->T = nullptr;
  if (!dcrow_adjoint_launches(Bt, s)) return GNS_EINVAL;
  if (s.lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!asked) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  if (workspace_bytes < dcrow_adjoint_ws_bytes(h, Bt, Rows::REC, n_row, s, own)) return GNS_ESIZE;
  double* ws = static_cast<double*>(workspace);
  const DcrowAdjointWorkspace w = dcrow_adjoint_workspace(ws + dcn2_ws_bytes(h, Bt, n_cand) / sizeof(double), h, Bt, Rows::REC, n_row, s, own);
  int rl = dcrow_launch_factor(c, cands, s.chunks_c, s.lanes_f, s.lds_factor, ws, w.conv);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcrow_adjoint_kernel<Rows>>(Bt * s.chunks_p, 32 * (int64_t)E, c.stream, rows.line_list, rows.n_line, rows.n_gen,
                                                 rows.cols, (int)n_row, c.islanding, c.rating, c.rating_per_grid, worst_line, converged,
                                                 grad_line_flow, grad_worst_loading, E, (int)Bt, s.Q, (int)s.chunks_p, (const double*)ws,
                                                 w.rec, w.gf_part);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcrow_adjoint_gather_kernel<Rows>>(Bt * n_cand, 8 * (int64_t)E, c.stream, rows.line_list, rows.n_line, rows.n_gen,
                                                        rows.cols, (int)n_row, converged, grad_line_flow, E, (int)Bt, (const double*)ws,
                                                        (const double*)w.rec, w.T, w.others);
  if (rl != GNS_OK) return rl;
  rl = pf_launch<gns_dcn2_adjoint_solve_kernel>(Bt * s.chunks_a, s.lds_solve, c.stream, c.topo, c.buses, c.lines, c.gens, cands.line,
                                                cands.n_line, n_cand, cands.n_gen ? w.own : (double*)nullptr, converged, (int)Bt, s.lanes,
                                                (int)s.chunks_a, (int)s.chunks_p, (const double*)ws, (const double*)w.T,
                                                (const double*)w.gf_part, (const double*)w.others, w.gf, w.part);
  if (rl != GNS_OK) return rl;
  *a = w;
  return GNS_OK;
}

}  // namespace
