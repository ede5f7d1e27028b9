// The solved case of an AC power flow (include/gns_powerflow.h, "The solved case"): at a given state (|V|, theta) of every grid of
// a batch, the branch flows at both ends of every line, the bus injections, Newton-Raphson's ||F||_inf, the generators' outputs, the
// slack's balancing power and the screens' summaries (gns_pfs_evaluate), and the gradients of a loss of those with respect to the
// state and the grid inputs (gns_pfs_adjoint).  One wave per grid, on the Newton-Raphson blob; nothing is iterated or solved.
// The arithmetic that other kernels also do is written again here in their expression order (the build has -ffp-contract=off, so
// the same order gives the same bits): the Y-bus row product and the mismatch of pf_solve_grid (gns_powerflow.hip), the flows, the
// extremes and the worst loading of acn_solve_row (gns_acn1_device.h), the line-row stamp algebra of acn_adjoint_row
// (gns_acn_adjoint_device.h).  No atomics; every sum in a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_acn_adjoint_device.h"

namespace {

// LDS image of one grid of either kernel: five bus vectors, in doubles.  It is below Newton-Raphson's image (pf_lds_bytes) on every
// topology, so what gns_pf_solve accepts is accepted here.
inline int64_t pfs_lds_bytes(const int32_t* h) { return 8 * 5 * (int64_t)h[PH_N]; }

// The outputs of gns_pfs_evaluate.  The [Bt,*] ones may be NULL: not written.
struct PfsOut {
  double* p_from;       // [Bt,E]
  double* q_from;
  double* p_to;
  double* q_to;
  double* p_inj;        // [Bt,N]
  double* q_inj;
  double* gen_p;        // [Bt,Gn]
  double* gen_q;
  double* mis;          // [Bt]
  double* slack_p;
  double* worst;
  int32_t* worst_line;
  double* v_min;
  int32_t* v_min_bus;
  double* v_max;
  int32_t* v_max_bus;
};

// The bus of generator slot q of the blob's by-bus lists: gen_ptr[b] <= q < gen_ptr[b + 1]
__device__ __forceinline__ int pfs_slot_bus(const int32_t* gen_ptr, const int N, const int q) {
  int b = 0, hi = N;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (gen_ptr[mid] <= q) b = mid;
    else hi = mid;
  }
  return b;
}

// Grids (waves) of one workgroup of gns_pfs_kernel.  1 is what ships; other values are builds for the packing measurement alone
// (tools/build_variant.sh with SRC=gns_pfs -DPFS_WAVES=4, profiles/solved_case/gpu_time_packing.txt): every wave still works on
// its own grid with its own LDS image, and such a build takes only batches that are a multiple of PFS_WAVES.
#ifndef PFS_WAVES
#define PFS_WAVES 1
#endif

__global__ __launch_bounds__(PF_THREADS * PFS_WAVES) void gns_pfs_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                             const float* __restrict__ lines, const float* __restrict__ gens,
                                                             const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                             const double* __restrict__ rating, const int rating_per_grid,
                                                             double2* __restrict__ ybus_ws, const PfsOut o) {
  extern __shared__ double lds[];
#if PFS_WAVES == 1
  const int lane = threadIdx.x, g = blockIdx.x;
#else
  const int lane = threadIdx.x % PF_THREADS, wave = threadIdx.x / PF_THREADS, g = blockIdx.x * PFS_WAVES + wave;
#endif
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK], nnzY = topo[PH_NNZY];
  const int32_t* th_idx = topo + topo[PH_TH_IDX];
  const int32_t* vm_idx = topo + topo[PH_VM_IDX];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[PH_Y_PTR];
  const int32_t* y_col = topo + topo[PH_Y_COL];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];

#if PFS_WAVES == 1
  double* Vm = lds;
#else
  double* Vm = lds + (size_t)wave * 5 * N;
#endif
  double* Vr = Vm + N;
  double* Vi = Vr + N;
  double* Pi = Vi + N;                   // the injections, which the generator rows read
  double* Qi = Pi + N;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;
  double2* Y = ybus_ws + (size_t)g * nnzY;

  // the Y-bus values (makeYbus) and the state
  for (int i = lane; i < N; i += PF_THREADS) {
    pf_ybus_row(i, y_ptr, y_diag, st_ptr, st, bus, line, Y);
    const double vm = v_in[(size_t)g * N + i], va = th_in[(size_t)g * N + i];
    Vm[i] = vm;
    Vr[i] = vm * cos(va); Vi[i] = vm * sin(va);
  }
  __syncthreads();

  // the injections S_i = V_i conj(sum_k Y_ik V_k), Newton-Raphson's mismatch and its infinity norm (pf_solve_grid's expressions),
  // and the voltage extremes (acn_solve_row's), a bus per lane
  const double inf = __builtin_inf();
  double nrm = 0.0;
  bool bad = false;
  double lo = -inf, hi = -inf;           // lo holds -|V|: the smallest |V| is the first in acn1_before's order of the negated values
  int lo_i = INT32_MAX, hi_i = INT32_MAX;
  for (int i = lane; i < N; i += PF_THREADS) {
    double ir = 0.0, ii = 0.0;
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int k = y_col[p];
      const double2 y = Y[p];
      ir += y.x * Vr[k] - y.y * Vi[k];
      ii += y.x * Vi[k] + y.y * Vr[k];
    }
    const double P = Vr[i] * ir + Vi[i] * ii, Q = Vi[i] * ir - Vr[i] * ii;
    Pi[i] = P; Qi[i] = Q;
    if (o.p_inj) o.p_inj[(size_t)g * N + i] = P;
    if (o.q_inj) o.q_inj[(size_t)g * N + i] = Q;
    double pg = 0.0;
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) pg += (double)gen[gen_idx[q] * 7 + 6];
    const double psp = pg - (double)bus[i * 6 + 2], qsp = -(double)bus[i * 6 + 3];
    if (th_idx[i] >= 0) {
      const double fp = P - psp;
      nrm = fmax(nrm, fabs(fp));
      bad |= !pf_finite(fp);
    }
    if (vm_idx[i] >= 0) {
      const double fq = Q - qsp;
      nrm = fmax(nrm, fabs(fq));
      bad |= !pf_finite(fq);
    }
    const double vm = Vm[i];
    if (acn1_before(-vm, i, lo, lo_i)) { lo = -vm; lo_i = i; }
    if (acn1_before(vm, i, hi, hi_i)) { hi = vm; hi_i = i; }
  }
  nrm = pf_wave_max(nrm);
  const double mis = __ballot(bad) ? __builtin_nan("") : nrm;
  acn1_wave_first(lo, lo_i);
  acn1_wave_first(hi, hi_i);
  __syncthreads();

  // the branch flows on the line's own stamps and the worst loading, a line per lane (acn_solve_row's expressions); NaN at a line
  // whose id columns are not buses of the grid
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  double best = -1.0;
  int bi = INT32_MAX;
  for (int l = lane; l < E; l += PF_THREADS) {
    double pf = 0.0, qf = 0.0, pt = 0.0, qt = 0.0;
    int a, b;
    if (!acn1_line_ends(line, l, N, a, b)) pf = qf = pt = qt = __builtin_nan("");
    else {
      const double2 yff = acn1_stamp(line, l, 0), ytt = acn1_stamp(line, l, 1), yft = acn1_stamp(line, l, 2), ytf = acn1_stamp(line, l, 3);
      const double far = Vr[a], fai = Vi[a], tor = Vr[b], toi = Vi[b];
      const double ifr = (yff.x * far - yff.y * fai) + (yft.x * tor - yft.y * toi);
      const double ifi = (yff.x * fai + yff.y * far) + (yft.x * toi + yft.y * tor);
      const double itr = (ytf.x * far - ytf.y * fai) + (ytt.x * tor - ytt.y * toi);
      const double iti = (ytf.x * fai + ytf.y * far) + (ytt.x * toi + ytt.y * tor);
      pf = far * ifr + fai * ifi; qf = fai * ifr - far * ifi;
      pt = tor * itr + toi * iti; qt = toi * itr - tor * iti;
    }
    if (o.p_from) o.p_from[(size_t)g * E + l] = pf;
    if (o.q_from) o.q_from[(size_t)g * E + l] = qf;
    if (o.p_to) o.p_to[(size_t)g * E + l] = pt;
    if (o.q_to) o.q_to[(size_t)g * E + l] = qt;
    const double sf = sqrt(pf * pf + qf * qf), s_t = sqrt(pt * pt + qt * qt);
    const double s = sf != sf ? sf : s_t != s_t ? s_t : fmax(sf, s_t);   // NaN from either end
    const double load = rt ? s / rt[l] : s;
    if (acn1_before(load, l, best, bi)) { best = load; bi = l; }
  }
  acn1_wave_first(best, bi);

  // the generators, a lane per slot of the by-bus lists: a bus's q_inj + Qd shared equally among its units (pfsoln without limit
  // ranges); Pg as given, but the first unit listed on the slack carries what the slack injects beyond the other units there
  const double ps = Pi[slack] + (double)bus[slack * 6 + 2];
  if (o.gen_p || o.gen_q)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = pfs_slot_bus(gen_ptr, N, q);
      const int j = gen_idx[q];
      if (o.gen_q) o.gen_q[(size_t)g * Gn + j] = (Qi[b] + (double)bus[b * 6 + 3]) / (double)(gen_ptr[b + 1] - gen_ptr[b]);
      if (o.gen_p) {
        double p = (double)gen[j * 7 + 6];
        if (b == slack && q == gen_ptr[slack]) {
          double others = 0.0;
          for (int u = gen_ptr[slack] + 1; u < gen_ptr[slack + 1]; ++u) others += (double)gen[gen_idx[u] * 7 + 6];
          p = ps - others;
        }
        o.gen_p[(size_t)g * Gn + j] = p;
      }
    }

  if (lane == 0) {
    double listed = 0.0;
    for (int u = gen_ptr[slack]; u < gen_ptr[slack + 1]; ++u) listed += (double)gen[gen_idx[u] * 7 + 6];
    o.mis[g] = mis;
    o.slack_p[g] = ps - listed;
    o.worst[g] = best; o.worst_line[g] = bi;
    o.v_min[g] = -lo; o.v_min_bus[g] = lo_i;
    o.v_max[g] = hi; o.v_max_bus[g] = hi_i;
  }
}

// ---- the adjoint

// The incoming gradients of gns_pfs_adjoint (each may be NULL: zero) and the indices the forward reported
struct PfsGrad {
  const double* p_from;   // [Bt,E]
  const double* q_from;
  const double* p_to;
  const double* q_to;
  const double* p_inj;    // [Bt,N]
  const double* q_inj;
  const double* gen_p;    // [Bt,Gn]
  const double* gen_q;
  const double* slack_p;  // [Bt]
  const double* worst;
  const double* v_min;
  const double* v_max;
};

// Whether any incoming gradient of grid g is not exactly zero (a NaN counts); the same answer in every lane
__device__ __forceinline__ bool pfs_grid_nonzero(const PfsGrad& gr, const int g, const int N, const int E, const int Gn) {
  bool nz = false;
  if (threadIdx.x == 0)
    nz = (gr.slack_p && gr.slack_p[g] != 0.0) || (gr.worst && gr.worst[g] != 0.0) || (gr.v_min && gr.v_min[g] != 0.0) ||
         (gr.v_max && gr.v_max[g] != 0.0);
  for (int i = threadIdx.x; i < N; i += PF_THREADS) {
    if (gr.p_inj) nz |= gr.p_inj[(size_t)g * N + i] != 0.0;
    if (gr.q_inj) nz |= gr.q_inj[(size_t)g * N + i] != 0.0;
  }
  for (int l = threadIdx.x; l < E; l += PF_THREADS) {
    if (gr.p_from) nz |= gr.p_from[(size_t)g * E + l] != 0.0;
    if (gr.q_from) nz |= gr.q_from[(size_t)g * E + l] != 0.0;
    if (gr.p_to) nz |= gr.p_to[(size_t)g * E + l] != 0.0;
    if (gr.q_to) nz |= gr.q_to[(size_t)g * E + l] != 0.0;
  }
  for (int q = threadIdx.x; q < Gn; q += PF_THREADS) {
    if (gr.gen_p) nz |= gr.gen_p[(size_t)g * Gn + q] != 0.0;
    if (gr.gen_q) nz |= gr.gen_q[(size_t)g * Gn + q] != 0.0;
  }
  return __ballot(nz) != 0;
}

// The line-end cotangents of one grid: W_f = grad_p_from + j grad_q_from + Lambda_f and W_t likewise (Lambda: the bus cotangents,
// in LDS), with what grad_worst_loading adds at line w's from end (wf) or to end (wt).  The same in every lane.
struct PfsCot {
  const double* gpf;   // the grid's [E] incoming gradients, NULL: zero
  const double* gqf;
  const double* gpt;
  const double* gqt;
  const double* LamR;  // [N]
  const double* LamI;
  int w;
  double2 wf, wt;
  __device__ __forceinline__ void at(const int l, const int a, const int b, double2& Wf, double2& Wt) const {
    Wf = make_double2(LamR[a], LamI[a]); Wt = make_double2(LamR[b], LamI[b]);
    if (gpf) Wf.x += gpf[l];
    if (gqf) Wf.y += gqf[l];
    if (gpt) Wt.x += gpt[l];
    if (gqt) Wt.y += gqt[l];
    if (l == w) { Wf.x += wf.x; Wf.y += wf.y; Wt.x += wt.x; Wt.y += wt.y; }
  }
};

// What the line-end cotangents add to dl/dtheta_i and dl/d|V_i|: acn1_flow_cot_bus's gather (gns_acn_adjoint_device.h) with these W.
// Bus i walks the stamps of its diagonal entry, kind 0 for every line it is the from end of and kind 1 for every line it is the to
// end of; no scatter.
__device__ __forceinline__ void pfs_flow_cot_bus(const int i, const int N, const int32_t* y_diag, const int32_t* st_ptr,
                                                 const int32_t* st, const float* line, const PfsCot& cot, const double* Vm,
                                                 const double* Vr, const double* Vi, double& dth, double& dvm) {
  const int p = y_diag[i];
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const int e = st[q] >> 2, kind = st[q] & 3;
    if (kind > 1) continue;
    int a, b;
    if (!acn1_line_ends(line, e, N, a, b)) continue;       // NaN flows: the line's own gradient row is NaN
    double2 Wf, Wt;
    cot.at(e, a, b, Wf, Wt);
    if (Wf.x == 0.0 && Wf.y == 0.0 && Wt.x == 0.0 && Wt.y == 0.0) continue;
    double2 A, D, B, C;
    acn1_flow_terms(line, e, a, b, Vm, Vr, Vi, A, D, B, C);
    const double tf = Wf.y * A.x - Wf.x * A.y, tt = Wt.y * B.x - Wt.x * B.y;   // Re(conj(W_f) jA), Re(conj(W_t) jB)
    if (kind == 0) {
      dth += tf - tt;
      dvm += ((Wf.x * (2.0 * D.x + A.x) + Wf.y * (2.0 * D.y + A.y)) + (Wt.x * B.x + Wt.y * B.y)) / Vm[a];
    } else {
      dth += tt - tf;
      dvm += ((Wt.x * (2.0 * C.x + B.x) + Wt.y * (2.0 * C.y + B.y)) + (Wf.x * A.x + Wf.y * A.y)) / Vm[b];
    }
  }
}

__global__ __launch_bounds__(PF_THREADS) void gns_pfs_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                     const float* __restrict__ lines,
                                                                     const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                                     const double* __restrict__ rating, const int rating_per_grid,
                                                                     const int32_t* __restrict__ wl_in, const int32_t* __restrict__ lo_in,
                                                                     const int32_t* __restrict__ hi_in, const PfsGrad gr,
                                                                     double* __restrict__ gv_out, double* __restrict__ gth_out,
                                                                     float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                     float* __restrict__ gg_out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK];
  const int32_t* gen_ptr = topo + topo[PH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[PH_GEN_IDX];
  const int32_t* y_diag = topo + topo[PH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[PH_ST_PTR];
  const int32_t* st = topo + topo[PH_ST];

  // a grid whose incoming gradients are all exactly zero or NULL: zero rows, whatever its state (skipped, never multiplied by zero)
  if (!pfs_grid_nonzero(gr, g, N, E, Gn)) {
    acn1_reduce_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out);
    for (int i = lane; i < N; i += PF_THREADS) {
      if (gv_out) gv_out[(size_t)g * N + i] = 0.0;
      if (gth_out) gth_out[(size_t)g * N + i] = 0.0;
    }
    return;
  }

  double* Vm = lds;
  double* Vr = Vm + N;
  double* Vi = Vr + N;
  double* LamR = Vi + N;                 // the bus cotangents Lambda_i = dl/dP_i + j dl/dQ_i
  double* LamI = LamR + N;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const double* ggp = gr.gen_p ? gr.gen_p + (size_t)g * Gn : nullptr;
  const double* ggq = gr.gen_q ? gr.gen_q + (size_t)g * Gn : nullptr;

  // what the slack's P takes besides grad_p_inj: grad_slack_p and the gradient of the first slack unit's gen_p
  const bool slack_unit = gen_ptr[slack + 1] > gen_ptr[slack];
  const double gsp = gr.slack_p ? gr.slack_p[g] : 0.0;
  const double gfirst = slack_unit && ggp ? ggp[gen_idx[gen_ptr[slack]]] : 0.0;
  const double gps = gsp + gfirst;

  // the state, the bus cotangents and the bus rows, a bus per lane
  for (int i = lane; i < N; i += PF_THREADS) {
    const double vm = v_in[(size_t)g * N + i], va = th_in[(size_t)g * N + i];
    Vm[i] = vm;
    Vr[i] = vm * cos(va); Vi[i] = vm * sin(va);
    double lr = gr.p_inj ? gr.p_inj[(size_t)g * N + i] : 0.0;
    double li = gr.q_inj ? gr.q_inj[(size_t)g * N + i] : 0.0;
    if (i == slack) lr += gps;
    double gq = 0.0;                     // dl/dQd_i: the units' grad_gen_q in listing order, shared as gen_q is
    const int n = gen_ptr[i + 1] - gen_ptr[i];
    if (n > 0 && ggq) {
      for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) gq += ggq[gen_idx[q]];
      gq /= (double)n;
    }
    li += gq;
    LamR[i] = lr; LamI[i] = li;
    if (gb_out) {
      float* row = gb_out + ((size_t)g * N + i) * 6;
      const double m2 = vm * vm;
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = (float)(i == slack ? gps : 0.0);   // Pd
      row[3] = (float)gq;                         // Qd
      row[4] = (float)(m2 * lr);                  // Gs: S_i gains |V_i|^2 conj(Gs + j Bs)
      row[5] = (float)(0.0 - m2 * li);            // Bs
    }
  }
  __syncthreads();

  // the line-end cotangents.  grad_worst_loading goes to the end of worst_line that attains the maximum (the from end on equality)
  // as S / |S| / rating, nothing at |S| = 0; grad_v_min and grad_v_max go to the buses the forward reported (acn_adjoint_row's rule).
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  PfsCot cot = {gr.p_from ? gr.p_from + (size_t)g * E : nullptr, gr.q_from ? gr.q_from + (size_t)g * E : nullptr,
                gr.p_to ? gr.p_to + (size_t)g * E : nullptr, gr.q_to ? gr.q_to + (size_t)g * E : nullptr, LamR, LamI, -1,
                make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
  const double gw = gr.worst ? gr.worst[g] : 0.0;
  const int w = wl_in[g];
  int wa = 0, wb = 0;
  if (gw != 0.0 && w >= 0 && w < E && acn1_line_ends(line, w, N, wa, wb)) {
    double2 A, D, B, Cc;
    acn1_flow_terms(line, w, wa, wb, Vm, Vr, Vi, A, D, B, Cc);
    const double pf = D.x + A.x, qf = D.y + A.y, pt = Cc.x + B.x, qt = Cc.y + B.y;
    const double sf = sqrt(pf * pf + qf * qf), s_t = sqrt(pt * pt + qt * qt);
    const double r = rt ? rt[w] : 1.0;
    if (sf >= s_t) { if (sf > 0.0) cot.wf = make_double2(gw * (pf / sf) / r, gw * (qf / sf) / r); }
    else cot.wt = make_double2(gw * (pt / s_t) / r, gw * (qt / s_t) / r);
    cot.w = w;
  }
  const double g_lo = gr.v_min ? gr.v_min[g] : 0.0, g_hi = gr.v_max ? gr.v_max[g] : 0.0;
  const int i_lo = lo_in[g], i_hi = hi_in[g];

  // dl/dtheta and dl/d|V| at every bus, the slack included: the gather of the line ends, the bus's own shunt, the extremes
  if (gv_out || gth_out)
    for (int i = lane; i < N; i += PF_THREADS) {
      double dth = 0.0;
      double dvm = 2.0 * Vm[i] * ((double)bus[i * 6 + 4] * LamR[i] - (double)bus[i * 6 + 5] * LamI[i]);
      if (i == i_lo) dvm += g_lo;
      if (i == i_hi) dvm += g_hi;
      pfs_flow_cot_bus(i, N, y_diag, st_ptr, st, line, cot, Vm, Vr, Vi, dth, dvm);
      if (gth_out) gth_out[(size_t)g * N + i] = dth;
      if (gv_out) gv_out[(size_t)g * N + i] = dvm;
    }

  // the generators' Pg, a lane per slot: gen_p passes Pg through at every unit but the first on the slack; on the slack every listed
  // Pg leaves slack_p, and every one but the first leaves the first unit's gen_p
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = pfs_slot_bus(gen_ptr, N, q);
      const int j = gen_idx[q];
      double gp = ggp ? ggp[j] : 0.0;
      if (b == slack) gp = q == gen_ptr[slack] ? 0.0 - gsp : gp - gsp - gfirst;
      float* row = gg_out + ((size_t)g * Gn + j) * 7;
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f; row[4] = 0.0f; row[5] = 0.0f;
      row[6] = (float)gp;                              // Pg
    }

  // the lines' r, x, b, tau, shift, a line per lane over its four stamps: acn_adjoint_row's algebra with +W where the mismatch
  // term has -Lambda; a line whose id columns are not buses of the grid gets a NaN row
  if (gl_out)
    for (int e = lane; e < E; e += PF_THREADS) {
      float* row = gl_out + ((size_t)g * E + e) * 7;
      int a, b2;
      if (!acn1_line_ends(line, e, N, a, b2)) {
        for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
        continue;
      }
      double2 Wf, Wt;
      cot.at(e, a, b2, Wf, Wt);
      const double lpf = 0.0 - Wf.x, lqf = 0.0 - Wf.y, lpt = 0.0 - Wt.x, lqt = 0.0 - Wt.y;
      const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
      const double den = r * r + x * x;
      const double ysr = r / den, ysi = -x / den, t2 = tau * tau;
      const double cs = cos(sh), sn = sin(sh);
      const double mf = Vm[a] * Vm[a], mt = Vm[b2] * Vm[b2];
      const double gffr = 0.0 - mf * lpf, gffi = mf * lqf;
      const double gttr = 0.0 - mt * lpt, gtti = mt * lqt;
      const double pr = Vr[a] * Vr[b2] + Vi[a] * Vi[b2], pi = Vi[a] * Vr[b2] - Vr[a] * Vi[b2];   // V_f conj(V_t)
      const double gftr = 0.0 - (pr * lpf + pi * lqf), gfti = 0.0 - (pi * lpf - pr * lqf);
      const double gtfr = 0.0 - (pr * lpt - pi * lqt), gtfi = 0.0 - (0.0 - pi * lpt - pr * lqt);
      const double gmr = gffr / t2 + gttr - ((cs * gftr + sn * gfti) + (cs * gtfr - sn * gtfi)) / tau;
      const double gmi = gffi / t2 + gtti - ((cs * gfti - sn * gftr) + (cs * gtfi + sn * gtfr)) / tau;
      const double y2r = ysr * ysr - ysi * ysi, y2i = 2.0 * ysr * ysi;
      const double qr = y2r * gmr + y2i * gmi, qi = y2r * gmi - y2i * gmr;   // conj(y_s^2) Gamma
      const double a0r = ysr / t2, a0i = (ysi + 0.5 * b) / t2;
      const double a2r = -(ysr * cs - ysi * sn) / tau, a2i = -(ysr * sn + ysi * cs) / tau;
      const double a3r = -(ysr * cs + ysi * sn) / tau, a3i = -(ysi * cs - ysr * sn) / tau;
      const double d_tau = 0.0 - (2.0 * (a0r * gffr + a0i * gffi) + (a2r * gftr + a2i * gfti) + (a3r * gtfr + a3i * gtfi)) / tau;
      const double d_sh = (a2r * gfti - a2i * gftr) - (a3r * gtfi - a3i * gtfr);
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = (float)(0.0 - qr);                                  // r
      row[3] = (float)(0.0 - qi);                                  // x
      row[4] = (float)(0.5 * gffi / t2 + 0.5 * gtti);              // b
      row[5] = (float)d_tau;                                       // tau
      row[6] = (float)d_sh;                                        // shift
    }
}

// What both entry points check alike, in the order the codes win: the arguments every call needs, the blob's header
inline int pfs_check(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev, const float* buses, const float* lines,
                     const float* generators, int64_t Bt, const double* v, const double* theta, int32_t rating_per_grid) {
  if (!pf_config_ok(cfg) || !topo_host || !topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !v || !theta ||
      (rating_per_grid != 0 && rating_per_grid != 1))
    return GNS_EINVAL;
  return pf_header_ok<PfBlobKind>(cfg, static_cast<const int32_t*>(topo_host)) ? GNS_OK : GNS_EINVAL;
}

}  // namespace

extern "C" int gns_pfs_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt);
  return GNS_OK;
}

extern "C" int gns_pfs_evaluate(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev, const float* buses,
                                const float* lines, const float* generators, int64_t Bt, const double* v, const double* theta,
                                const double* rating, int32_t rating_per_grid, double* p_from, double* q_from, double* p_to,
                                double* q_to, double* p_inj, double* q_inj, double* gen_p, double* gen_q, double* mismatch,
                                double* slack_p, double* worst_loading, int32_t* worst_line, double* v_min, int32_t* v_min_bus,
                                double* v_max, int32_t* v_max_bus, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = pfs_check(cfg, topo_host, topo_dev, buses, lines, generators, Bt, v, theta, rating_per_grid);
  if (rc != GNS_OK) return rc;
  if (!mismatch || !slack_p || !worst_loading || !worst_line || !v_min || !v_min_bus || !v_max || !v_max_bus || !workspace)
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (workspace_bytes < pf_ws_bytes_nnzy(h[PH_NNZY], Bt)) return GNS_ESIZE;
  const int64_t lds = pfs_lds_bytes(h);
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  const PfsOut out = {p_from, q_from, p_to, q_to, p_inj, q_inj, gen_p, gen_q, mismatch, slack_p, worst_loading, worst_line,
                      v_min, v_min_bus, v_max, v_max_bus};
#if PFS_WAVES == 1
  return pf_launch<gns_pfs_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, v, theta, rating,
                                   (int)rating_per_grid, static_cast<double2*>(workspace), out);
#else   // a measurement build: PFS_WAVES grids per workgroup
  if (Bt % PFS_WAVES != 0) return GNS_EINVAL;
  if (lds * PFS_WAVES > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(gns_pfs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          GNS_PF_LDS_MAX_BYTES) != hipSuccess)
    return GNS_ELAUNCH;
  hipLaunchKernelGGL(gns_pfs_kernel, dim3((unsigned)(Bt / PFS_WAVES)), dim3(PF_THREADS * PFS_WAVES), (size_t)(lds * PFS_WAVES),
                     (hipStream_t)stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, v, theta, rating,
                     (int)rating_per_grid, static_cast<double2*>(workspace), out);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
#endif
}

// The adjoint reads no Y-bus (every term reduces to the line ends and the bus shunts), so it needs no workspace: the query answers 0
// after the checks of the call.
extern "C" int gns_pfs_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  *bytes = 0;
  return GNS_OK;
}

extern "C" int gns_pfs_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev, const float* buses,
                               const float* lines, const float* generators, int64_t Bt, const double* v, const double* theta,
                               const double* rating, int32_t rating_per_grid, const int32_t* worst_line, const int32_t* v_min_bus,
                               const int32_t* v_max_bus, const double* grad_p_from, const double* grad_q_from,
                               const double* grad_p_to, const double* grad_q_to, const double* grad_p_inj, const double* grad_q_inj,
                               const double* grad_gen_p, const double* grad_gen_q, const double* grad_slack_p,
                               const double* grad_worst_loading, const double* grad_v_min, const double* grad_v_max, double* grad_v,
                               double* grad_theta, float* grad_buses, float* grad_lines, float* grad_generators, void* workspace,
                               size_t workspace_bytes, void* stream) {
  (void)workspace; (void)workspace_bytes;
  const int rc = pfs_check(cfg, topo_host, topo_dev, buses, lines, generators, Bt, v, theta, rating_per_grid);
  if (rc != GNS_OK) return rc;
  if (!worst_line || !v_min_bus || !v_max_bus) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  const int64_t lds = pfs_lds_bytes(h);
  if (lds > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_v && !grad_theta && !grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  const PfsGrad gr = {grad_p_from, grad_q_from, grad_p_to, grad_q_to, grad_p_inj, grad_q_inj, grad_gen_p, grad_gen_q, grad_slack_p,
                      grad_worst_loading, grad_v_min, grad_v_max};
  return pf_launch<gns_pfs_adjoint_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, v, theta, rating,
                                           (int)rating_per_grid, worst_line, v_min_bus, v_max_bus, gr, grad_v, grad_theta, grad_buses,
                                           grad_lines, grad_generators);
}
