// What the adjoints of the two AC contingency screens share, gns_acn1_adjoint (gns_acn1.hip) and gns_acn2_adjoint (gns_acn2.hip).
// Device: the incoming gradients of a call, a row's effective flow cotangents, the layout and the status of a (grid, chunk) partial, the routine of a solved row (acn_adjoint_row: the implicit function theorem on the grid without
// the row's line or lines, templated on the Y-bus view as acn_solve_row is), the row kernel (gns_acn_adjoint_kernel<M>: acn_view,
// the forward's prologue, then acn_adjoint_row, over a chunk's rows) and the kernel that sums a grid's partials.  Host: the workspace
// query and an adjoint call (acn_adjoint_call<Rows>), on the screen's trait.  Both adjoints are this code at M = 1 and M = 2.
// gns_acg1_adjoint (gns_acg1.hip: generator outages) has a row kernel, a reduce kernel and an entry point of its own on a set of
// blobs; its rows run acn_adjoint_row from here with the generator part of a partial laid out by generator row (the Gen hook), and
// its reduce kernel sums the buses and the lines with the pieces of the reduce kernel here.
// The algebra of a row is gns_ac_device.h's, shared with gns_pf_adjoint and the solved case: the Jacobian row, the worst-loading
// cotangent, the gather of the flow cotangents to the buses, dl/dvg's column sum and the cotangents of a line row; the bus of a
// generator slot and the fill of a grid's gradient rows are gns_pf_device.h's.
#pragma once
#include "gns_acn1_device.h"

namespace {

// The status of a chunk's partial: gns_dcn1.hip's (valid sums; the grid's gradient is NaN; the grid has no base solution and the
// chunk's incoming gradients are zero)
constexpr double ACN1_PART_OK = 0.0, ACN1_PART_NAN = 1.0, ACN1_PART_UNSOLVED_ZERO = 2.0;

// The incoming gradients of a call (each may be NULL: zero), in the layout of Acn1Out's rows
struct Acn1Grad {
  const double* v;        // [Bt,K,N]
  const double* theta;
  const double* p_from;   // [Bt,K,E]
  const double* q_from;
  const double* p_to;
  const double* q_to;
  const double* worst;    // [Bt,K]
  const double* v_min;
  const double* v_max;
};

// Whether any incoming gradient of row `row` is not exactly zero (a NaN counts); the same answer in every lane
__device__ __forceinline__ bool acn1_row_nonzero(const Acn1Grad& gr, const size_t row, const int N, const int E) {
  bool nz = false;
  if (threadIdx.x == 0)
    nz = (gr.worst && gr.worst[row] != 0.0) || (gr.v_min && gr.v_min[row] != 0.0) || (gr.v_max && gr.v_max[row] != 0.0);
  for (int i = threadIdx.x; i < N; i += PF_THREADS) {
    if (gr.v) nz |= gr.v[row * N + i] != 0.0;
    if (gr.theta) nz |= gr.theta[row * N + i] != 0.0;
  }
  for (int l = threadIdx.x; l < E; l += PF_THREADS) {
    if (gr.p_from) nz |= gr.p_from[row * E + l] != 0.0;
    if (gr.q_from) nz |= gr.q_from[row * E + l] != 0.0;
    if (gr.p_to) nz |= gr.p_to[row * E + l] != 0.0;
    if (gr.q_to) nz |= gr.q_to[row * E + l] != 0.0;
  }
  return __ballot(nz) != 0;
}

// The effective flow cotangents of one row: W_f = grad_p_from + j grad_q_from and W_t likewise, with what grad_worst_loading adds
// at line w's from end (wf) or to end (wt); zero at the outaged line(s) of the row's Y-bus view.  The same in every lane.  at()
// has the signature ac_flow_cot_bus and ac_worst_cot ask for (gns_ac_device.h); these cotangents do not depend on the line's ends.
template <class YB>   // an AcnYbus<M>
struct Acn1Cot {
  const double* gpf;   // the row's [E] incoming gradients, NULL: zero
  const double* gqf;
  const double* gpt;
  const double* gqt;
  const YB& Y;
  int w;
  double2 wf, wt;
  __device__ __forceinline__ void at(const int l, const int, const int, double2& Wf, double2& Wt) const {
    Wf = make_double2(0.0, 0.0); Wt = Wf;
    if (Y.out(l)) return;
    if (gpf) Wf.x = gpf[l];
    if (gqf) Wf.y = gqf[l];
    if (gpt) Wt.x = gpt[l];
    if (gqt) Wt.y = gqt[l];
    if (l == w) { Wf.x += wf.x; Wf.y += wf.y; Wt.x += wt.x; Wt.y += wt.y; }
  }
};

// The generator part of a partial as the line screens lay it out: a double per generator slot (the blob's by-bus order), dl/dvg.
// Every row of those screens runs on the one base blob, so the slots mean the same in every row, and Pg is read off the bus sums.
struct AcnSlotPartial {
  static constexpr int GEN = 1;            // doubles per generator
};

// Doubles of one (grid, chunk) partial: per bus the sums of lambda_P, lambda_Q, |V|^2 lambda_P, |V|^2 lambda_Q; per line its five
// columns; the generator part, Layout::GEN doubles per generator; the chunk's status
template <class Layout = AcnSlotPartial>
__device__ __host__ inline int64_t acn1_adjoint_partial(const int32_t* h) {
  return 4 * (int64_t)h[PH_N] + 5 * (int64_t)h[PH_E] + Layout::GEN * (int64_t)h[PH_GN] + 1;
}

// acn_adjoint_row's one hook, the generator part of a row.  The line screens' (this one, which compiles to nothing): dl/dvg of the
// first generator of a PV / slack bus into that generator's slot.  gns_acg1.hip's Acg1Gen, for rows whose blobs differ: the slots
// that are the blob's (gen_ptr[N] of them), dl/dvg into the unit's original generator row, and a call per remaining unit
// (unit: its row and its bus's lambda_P) and one after them (lost), for what Pg and the pickup weights get.
struct AcnSlotGen {};

// The wave's exit with the chunk's status alone (its sums are not read then)
__device__ __forceinline__ void acn1_partial_status(double* part, const int np, const double status) {
  if (threadIdx.x == 0) part[np - 1] = status;
}

// A solved row of either adjoint after its kernel's prologue (the row decode, the skip of a row nobody asks for, the decision that
// the row has a solution, the Y-bus view Y of the grid without the row's line or lines): the forward's state of row `row` (read,
// not solved again), I = Y V, the Jacobian on Y factored on Newton-Raphson's LDS image, the row's cotangents, one transposed
// solve, and the bus, generator and line sums added into the chunk's partial `part`, every lane into the addresses it alone owns.
// False when the row gives the grid a NaN gradient (a zero or non-finite pivot, a non-finite lambda); the same in every lane.
// Flows and flow cotangents are skipped at every line Y.out names, and the row adds exactly 0 to those lines' own columns.
template <class YB, class Gen = AcnSlotGen>   // an AcnYbus<M>; AcnSlotGen, or a hook with unit() and lost() (Acg1Gen)
__device__ __forceinline__ bool acn_adjoint_row(const int32_t* __restrict__ topo, const float* line, const size_t row, const YB& Y,
                                                const double* rt, const Acn1Grad& gr, const double* __restrict__ v_in,
                                                const double* __restrict__ th_in, const int32_t* __restrict__ wl_in,
                                                const int32_t* __restrict__ lo_in, const int32_t* __restrict__ hi_in, double* part,
                                                const Gen& gen = Gen()) {
  constexpr bool by_row = !std::is_same_v<Gen, AcnSlotGen>;   // the generator part by original generator row, not by slot
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK], dim = topo[PH_DIM];
  const int nnzLU = topo[PH_NNZLU], t_nsteps = topo[PH_T_NSTEPS];
  const int32_t* role = topo + topo[PH_ROLE];
  const int32_t* th_idx = topo + topo[PH_TH_IDX];
  const int32_t* vm_idx = topo + topo[PH_VM_IDX];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];
  const int32_t* jslot = topo + topo[PH_JSLOT];
  const int32_t* pivot = topo + topo[PH_PIVOT];
  const int32_t* step_ptr = topo + topo[PH_STEP_PTR];
  const int2* ops = reinterpret_cast<const int2*>(topo + topo[PH_OPS]);
  const int32_t* t_step_ptr = topo + topo[PH_T_STEP_PTR];
  const int2* t_ops = reinterpret_cast<const int2*>(topo + topo[PH_T_OPS]);
  double* part_bus = part;                 // [N][4]
  double* part_line = part + 4 * N;        // [E][5]
  double* part_gen = part_line + 5 * E;    // [Gn], or the hook's layout

  double* F = lds;                         // Newton-Raphson's image: [nnzLU] factor, then [dim] right-hand side / lambda
  double* rhs = lds + nnzLU;
  double* Vm = rhs + dim;
  double* dV = Vm + N;                     // the solve's Va: the total direct dl/d|V_i| of the row (vg reads it at PV / slack buses)
  double* Vr = dV + N;
  double* Vi = Vr + N;
  double* Ir = Vi + N;
  double* Ii = Ir + N;
  double* lamP = Ii + N;                   // the solve's Psp / Qsp: lambda of each bus's P and Q mismatch (0 where there is none)
  double* lamQ = lamP + N;

  // the forward's state of the row (read, not solved again) and I = Y V there
  __syncthreads();                         // the row before has read its last LDS value
  for (int i = lane; i < N; i += PF_THREADS) {
    const double vm = v_in[row * N + i], va = th_in[row * N + i];
    Vm[i] = vm;
    Vr[i] = vm * cos(va); Vi[i] = vm * sin(va);
  }
  for (int s = lane; s < nnzLU + dim; s += PF_THREADS) F[s] = 0.0;
  __syncthreads();
  for (int i = lane; i < N; i += PF_THREADS) {
    double ir = 0.0, ii = 0.0;
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int c = y_col[p];
      const double2 y = Y.at(p);
      ir += y.x * Vr[c] - y.y * Vi[c];
      ii += y.x * Vi[c] + y.y * Vr[c];
    }
    Ir[i] = ir; Ii[i] = ii;
  }
  __syncthreads();

  // the Jacobian at that state, factored by the leading steps of the solve program (its solve operations there see a zero
  // right-hand side)
  for (int i = lane; i < N; i += PF_THREADS)
    if (i != slack) ac_jacobian_row(i, slack, y_ptr, y_col, jslot, Y, Vm, Vr, Vi, Ir, Ii, F);
  __syncthreads();
  pf_run_program(t_step_ptr[t_nsteps + 1], step_ptr, ops, F, lane);
  if (__ballot(pf_bad_pivot(dim, pivot, F, lane))) return false;

  // the row's effective cotangents.  grad_worst_loading goes to worst_line by ac_worst_cot's rule, unless that line is out in this
  // row; grad_v_min and grad_v_max go to the buses the forward reported.
  Acn1Cot<YB> cot = {gr.p_from ? gr.p_from + row * E : nullptr, gr.q_from ? gr.q_from + row * E : nullptr,
                     gr.p_to ? gr.p_to + row * E : nullptr, gr.q_to ? gr.q_to + row * E : nullptr, Y, -1,
                     make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
  const int w = wl_in[row];
  if (!Y.out(w)) ac_worst_cot(cot, gr.worst ? gr.worst[row] : 0.0, w, N, E, rt, line, Vm, Vr, Vi);
  const double g_lo = gr.v_min ? gr.v_min[row] : 0.0, g_hi = gr.v_max ? gr.v_max[row] : 0.0;
  const int i_lo = lo_in[row], i_hi = hi_in[row];

  // J^T lambda = dl/dx: the theta and |V| cotangents at the unknowns plus the flows' derivatives, a bus per lane (the slack's
  // theta is the constant 0)
  for (int i = lane; i < N; i += PF_THREADS) {
    double dth = gr.theta ? gr.theta[row * N + i] : 0.0;
    double dvm = gr.v ? gr.v[row * N + i] : 0.0;
    if (i == i_lo) dvm += g_lo;
    if (i == i_hi) dvm += g_hi;
    ac_flow_cot_bus(i, N, y_diag, st_ptr, st, line, cot, Vm, Vr, Vi, dth, dvm);
    dV[i] = dvm;
    if (th_idx[i] >= 0) rhs[th_idx[i]] = dth;
    if (vm_idx[i] >= 0) rhs[vm_idx[i]] = dvm;
  }
  __syncthreads();
  pf_run_program(t_nsteps, t_step_ptr, t_ops, F, lane);
  bool bad = false;
  for (int i = lane; i < N; i += PF_THREADS) {
    const double lp = th_idx[i] >= 0 ? rhs[th_idx[i]] : 0.0, lq = vm_idx[i] >= 0 ? rhs[vm_idx[i]] : 0.0;
    lamP[i] = lp; lamQ[i] = lq;
    bad |= !pf_finite(lp) || !pf_finite(lq);
  }
  if (__ballot(bad)) return false;
  __syncthreads();

  // dl/dp = direct - lambda^T dF/dp, gns_pf_adjoint's algebra (pf_adjoint_grid) on the row's Y-bus, added to the chunk's sums
  for (int i = lane; i < N; i += PF_THREADS) {
    const double m2 = Vm[i] * Vm[i], lp = lamP[i], lq = lamQ[i];
    double* pb = part_bus + 4 * i;
    pb[0] += lp; pb[1] += lq; pb[2] += m2 * lp; pb[3] += m2 * lq;
  }
  const int n_slot = by_row ? gen_ptr[N] : Gn;       // a blob without a generator row lists one slot fewer
  for (int q = lane; q < n_slot; q += PF_THREADS) {  // a lane per generator slot, in the blob's by-bus order
    const int b = pf_slot_bus(gen_ptr, N, q);
    if constexpr (by_row) gen.unit(part_gen, gen_idx[q], lamP[b]);
    if (q != gen_ptr[b] || role[b] == 0) continue;   // the first generator of a PV / slack bus sets |V_b|
    const double acc = ac_vg_column(b, Vr[b] / Vm[b], Vi[b] / Vm[b], y_ptr, y_col, Y, Vr, Vi, Ir, Ii, lamP, lamQ);
    part_gen[by_row ? gen_idx[q] : q] += dV[b] - acc;
  }
  if constexpr (by_row) gen.lost(part_gen);
  for (int e = lane; e < E; e += PF_THREADS) {      // a line per lane, over its four stamps; the row adds nothing to a line that is out
    int a, b2;
    if (Y.out(e) || !pf_line_ends(line, e, N, a, b2)) continue;
    double2 Wf, Wt;
    cot.at(e, a, b2, Wf, Wt);
    // Lambda_f - W_f and Lambda_t - W_t: the flow term is +Re(conj(W) S) on the line's own stamps, the mismatch term -Re(conj(Lambda) S)
    const AcLineCot d = ac_line_row_cot(line, e, a, b2, Vm, Vr, Vi, lamP[a] - Wf.x, lamQ[a] - Wf.y, lamP[b2] - Wt.x, lamQ[b2] - Wt.y);
    double* pl = part_line + 5 * e;
    pl[0] += d.r; pl[1] += d.x; pl[2] += d.b; pl[3] += d.tau; pl[4] += d.sh;
  }
  return true;
}

// The row kernel of both adjoints, M lines out per row: workgroup blockIdx.x = grid * nchunks + chunk walks rows k0 .. k0 + C of the
// grid's list in order, each lane adding into the addresses of the chunk's partial it alone owns (a bus, a line or a generator
// slot per lane)
template <int M>
__global__ __launch_bounds__(PF_THREADS) void gns_acn_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                     const float* __restrict__ lines, const float* __restrict__ gens,
                                                                     const int32_t* __restrict__ list, const int K,
                                                                     const uint8_t* __restrict__ islanding,
                                                                     const double* __restrict__ rating, const int rating_per_grid,
                                                                     const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                                     const uint8_t* __restrict__ conv_in,
                                                                     const int32_t* __restrict__ wl_in, const int32_t* __restrict__ lo_in,
                                                                     const int32_t* __restrict__ hi_in,
                                                                     const uint8_t* __restrict__ conv0, const Acn1Grad gr,
                                                                     const double2* __restrict__ ybus_ws, const int C, const int nchunks,
                                                                     double* __restrict__ partials) {
  const int lane = threadIdx.x;
  const int g = (int)(blockIdx.x / (unsigned)nchunks), k0 = (int)(blockIdx.x % (unsigned)nchunks) * C;
  const int nk = min(C, K - k0);
  const int N = topo[PH_N], E = topo[PH_E], nnzY = topo[PH_NNZY];
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  const int np = (int)acn1_adjoint_partial(topo);
  double* part = partials + (size_t)blockIdx.x * np;

  for (int q = lane; q < np - 1; q += PF_THREADS) part[q] = 0.0;   // bus i's, line l's and slot q's doubles all sit at lane + 64 m
  bool solved_row = false;

  for (int j = 0; j < nk; ++j) {
    const size_t row = (size_t)g * K + k0 + j;
    // a row whose incoming gradients are all exactly zero or NULL is skipped, never multiplied by zero
    if (!acn1_row_nonzero(gr, row, N, E)) continue;
    // a row without a solution (no base solution, an islanding row, a stopped or unconverged iteration, what acn_view refuses): the
    // grid's gradient is NaN.  The view is the forward's: the same builder on the same row.
    AcnYbus<M> Y;
    if (!acn_view(conv0[g] != 0 && conv_in[row] != 0 && !islanding[k0 + j], topo, bus, line, list, k0 + j,
                  ybus_ws + (size_t)g * nnzY, Y) ||
        !acn_adjoint_row(topo, line, row, Y, rt, gr, v_in, th_in, wl_in, lo_in, hi_in, part)) {
      acn1_partial_status(part, np, ACN1_PART_NAN);
      return;
    }
    solved_row = true;
  }
  // a grid without a base solution whose chunk asked for nothing: zero rows when every chunk says so
  acn1_partial_status(part, np, !solved_row && conv0[g] == 0 ? ACN1_PART_UNSOLVED_ZERO : ACN1_PART_OK);
}

// The pieces of a reduce kernel (a wave per grid g; part: the grid's first partial, np doubles each), shared with gns_acg1.hip.

// Whether a chunk of the grid says NaN (bad) and whether any holds sums (solved); the same in every lane
__device__ __forceinline__ void acn1_reduce_status(const double* part, const int nchunks, const int np, bool& bad, bool& solved) {
  bool b = false, s = false;
  for (int c = threadIdx.x; c < nchunks; c += PF_THREADS) {
    const double status = part[(size_t)c * np + np - 1];
    b |= status != ACN1_PART_OK && status != ACN1_PART_UNSOLVED_ZERO;
    s |= status != ACN1_PART_UNSOLVED_ZERO;
  }
  bad = __ballot(b) != 0;
  solved = __ballot(s) != 0;
}

// The grid's bus rows: the chunks in order, the contract (0.0 - x rather than -x: an exact zero stays +0)
__device__ __forceinline__ void acn1_reduce_buses(const int g, const int N, const int nchunks, const int np, const double* part,
                                                  float* gb_out) {
  for (int i = threadIdx.x; i < N; i += PF_THREADS) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; ++c)
      for (int u = 0; u < 4; ++u) s[u] += part[(size_t)c * np + 4 * i + u];
    float* row = gb_out + ((size_t)g * N + i) * 6;
    row[0] = 0.0f; row[1] = 0.0f;
    row[2] = (float)(0.0 - s[0]);          // Pd
    row[3] = (float)(0.0 - s[1]);          // Qd
    row[4] = (float)(0.0 - s[2]);          // Gs
    row[5] = (float)s[3];                  // Bs
  }
}

// The grid's line rows: the chunks in order; a line whose id columns are not buses of the grid gets a NaN row
__device__ __forceinline__ void acn1_reduce_lines(const int g, const int N, const int E, const float* line, const int nchunks,
                                                  const int np, const double* part, float* gl_out) {
  for (int e = threadIdx.x; e < E; e += PF_THREADS) {
    float* row = gl_out + ((size_t)g * E + e) * 7;
    int f, t;
    if (!pf_line_ends(line, e, N, f, t)) {
      for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
      continue;
    }
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; ++c)
      for (int u = 0; u < 5; ++u) s[u] += part[(size_t)c * np + 4 * N + 5 * e + u];
    row[0] = 0.0f; row[1] = 0.0f;
    for (int u = 0; u < 5; ++u) row[2 + u] = (float)s[u];
  }
}

// A wave per grid: the chunks' partials summed in order, the contract applied, every element of the three gradient rows written
__global__ __launch_bounds__(PF_THREADS) void gns_acn1_adjoint_reduce_kernel(const int32_t* __restrict__ topo,
                                                                             const float* __restrict__ lines, const int nchunks,
                                                                             const double* __restrict__ partials,
                                                                             float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                             float* __restrict__ gg_out) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int np = (int)acn1_adjoint_partial(topo);
  const double* part = partials + (size_t)g * nchunks * np;
  const float* line = lines + (size_t)g * E * 7;

  bool bad, solved;
  acn1_reduce_status(part, nchunks, np, bad, solved);
  if (bad || !solved) {
    pf_adjoint_fill(g, N, E, Gn, bad ? __builtin_nanf("") : 0.0f, gb_out, gl_out, gg_out);
    return;
  }

  if (gb_out) acn1_reduce_buses(g, N, nchunks, np, part, gb_out);
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = pf_slot_bus(gen_ptr, N, q);
      double dp = 0.0, dvg = 0.0;
      for (int c = 0; c < nchunks; ++c) {
        dp += part[(size_t)c * np + 4 * b];
        dvg += part[(size_t)c * np + 4 * N + 5 * E + q];
      }
      float* row = gg_out + ((size_t)g * Gn + gen_idx[q]) * 7;
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f;
      row[4] = (float)dvg;                   // vg
      row[5] = 0.0f;
      row[6] = (float)dp;                    // Pg: S_spec += Pg
    }
  if (gl_out) acn1_reduce_lines(g, N, E, line, nchunks, np, part, gl_out);
}

// ---- host: what gns_acn1_adjoint and gns_acn2_adjoint (and their workspace queries) do alike

// The partials of a call: one per (grid, chunk), rounded up to 256 bytes
template <class Layout = AcnSlotPartial>
inline size_t acn1_adjoint_partial_bytes(const int32_t* h, int64_t Bt, int64_t nchunks) {
  return ((size_t)Bt * nchunks * acn1_adjoint_partial<Layout>(h) * sizeof(double) + 255) & ~(size_t)255;
}

// The workspace of either adjoint: the base Y-bus of every grid, then a partial per (grid, chunk of Rows::chunk(n_row) rows of the
// list)
template <class Rows>
int acn_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, int32_t n_row, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0 || n_row <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  int64_t nchunks = 0;
  if (!pf_chunks(n_row, Rows::chunk(n_row), Bt, &nchunks)) return GNS_EINVAL;
  if (pf_lds_bytes(h) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt) + acn1_adjoint_partial_bytes(h, Bt, nchunks);
  return GNS_OK;
}

// An adjoint call, in the order the codes win: the arguments, the blob's header, the list (Rows::list_ok, as in acn_screen_call), a
// workgroup per (grid, chunk of C = Rows::chunk(n_row) rows) in one launch, the LDS image; with no gradient output asked for GNS_OK
// without a launch; then the workspace.  Three launches: the base Y-bus of every grid into the workspace, the row kernel at Rows::M
// lines out (a workgroup per (grid, chunk)), the sum of each grid's partials.
template <class Rows>
int acn_adjoint_call(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev, const float* buses, const float* lines,
                     const float* generators, int64_t Bt, const int32_t* list_host, const int32_t* list_dev, int32_t n_row,
                     const uint8_t* islanding, const double* rating, int32_t rating_per_grid, const double* v, const double* theta,
                     const uint8_t* converged, const int32_t* worst_line, const int32_t* v_min_bus, const int32_t* v_max_bus,
                     const uint8_t* base_converged, const Acn1Grad& gr, float* grad_buses, float* grad_lines,
                     float* grad_generators, void* workspace, size_t workspace_bytes, void* stream) {
  const int C = Rows::chunk(n_row);
  if (!pf_config_ok(cfg) || !topo_host || !topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF ||
      !list_host || !list_dev || n_row <= 0 || !islanding || (rating_per_grid != 0 && rating_per_grid != 1) || !v || !theta ||
      !converged || !worst_line || !v_min_bus || !v_max_bus || !base_converged)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h) || !Rows::list_ok(h, list_host, n_row)) return GNS_EINVAL;
  int64_t nchunks = 0;
  if (!pf_chunks(n_row, C, Bt, &nchunks)) return GNS_EINVAL;
  const int64_t lds = pf_lds_bytes(h);
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  if (!workspace) return GNS_EINVAL;
  const size_t ybytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt);
  if (workspace_bytes < ybytes + acn1_adjoint_partial_bytes(h, Bt, nchunks)) return GNS_ESIZE;
  const int32_t* topo = static_cast<const int32_t*>(topo_dev);
  double2* ybus = static_cast<double2*>(workspace);
  double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + ybytes);
  const int rc0 = pf_launch<gns_acn1_ybus_kernel>(Bt, 0, stream, topo, buses, lines, ybus);
  if (rc0 != GNS_OK) return rc0;
  const int rc1 = pf_launch<gns_acn_adjoint_kernel<Rows::M>>(Bt * nchunks, lds, stream, topo, buses, lines, generators, list_dev,
                                                             (int)n_row, islanding, rating, (int)rating_per_grid, v, theta, converged,
                                                             worst_line, v_min_bus, v_max_bus, base_converged, gr,
                                                             (const double2*)ybus, C, (int)nchunks, partials);
  if (rc1 != GNS_OK) return rc1;
  return pf_launch<gns_acn1_adjoint_reduce_kernel>(Bt, 0, stream, topo, lines, (int)nchunks, (const double*)partials, grad_buses,
                                                   grad_lines, grad_generators);
}

}  // namespace
