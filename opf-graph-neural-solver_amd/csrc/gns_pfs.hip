// The solved case of an AC power flow (include/gns_powerflow.h, "The solved case"): at a given state (|V|, theta) of every grid of
// a batch, the branch flows at both ends of every line, the bus injections, Newton-Raphson's ||F||_inf, the generators' outputs, the
// slack's balancing power and the screens' summaries (gns_pfs_evaluate), and the gradients of a loss of those with respect to the
// state and the grid inputs (gns_pfs_adjoint).  One wave per grid, on the Newton-Raphson blob; nothing is iterated or solved.
// What the AC screens and Newton-Raphson's adjoint also compute is gns_ac_device.h's, the one copy they all run: a line's flows and
// loading, the voltage extremes, the worst-loading cotangent, the gather of the line-end cotangents and the cotangent algebra of a
// line row; the Y-bus row and a line's stamp are gns_pf_device.h's.  Only the Y-bus row product and the mismatch stand here in
// pf_solve_grid's expression order (gns_powerflow.hip keeps its own written out; the build has -ffp-contract=off, so the same order
// gives the same bits).  No atomics; every sum in a fixed order.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_ac_device.h"

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
  // and the voltage extremes (the screens' ac_voltage_extremes, this loop's body as its per-bus work), a bus per lane
  double nrm = 0.0;
  bool bad = false;
  const AcExtremes ex = ac_voltage_extremes(N, Vm, lane, [&](const int i, const double) {
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
  });
  nrm = pf_wave_max(nrm);
  const double mis = __ballot(bad) ? __builtin_nan("") : nrm;
  __syncthreads();

  // the branch flows on the line's own stamps and the worst loading, a line per lane (the functions acn_solve_row calls); NaN at a
  // line whose id columns are not buses of the grid
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  double best = -1.0;
  int bi = INT32_MAX;
  for (int l = lane; l < E; l += PF_THREADS) {
    const double nan = __builtin_nan("");
    int a, b;
    const AcFlows s = pf_line_ends(line, l, N, a, b) ? ac_line_flows(line, l, a, b, Vr, Vi) : AcFlows{nan, nan, nan, nan};
    if (o.p_from) o.p_from[(size_t)g * E + l] = s.pf;
    if (o.q_from) o.q_from[(size_t)g * E + l] = s.qf;
    if (o.p_to) o.p_to[(size_t)g * E + l] = s.pt;
    if (o.q_to) o.q_to[(size_t)g * E + l] = s.qt;
    const double load = ac_loading(s, rt, l);
    if (ac_before(load, l, best, bi)) { best = load; bi = l; }
  }
  ac_wave_first(best, bi);

  // the generators, a lane per slot of the by-bus lists: a bus's q_inj + Qd shared equally among its units (pfsoln without limit
  // ranges); Pg as given, but the first unit listed on the slack carries what the slack injects beyond the other units there
  const double ps = Pi[slack] + (double)bus[slack * 6 + 2];
  if (o.gen_p || o.gen_q)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = pf_slot_bus(gen_ptr, N, q);
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
    o.v_min[g] = -ex.lo; o.v_min_bus[g] = ex.lo_i;
    o.v_max[g] = ex.hi; o.v_max_bus[g] = ex.hi_i;
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
    pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out);
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

  // the line-end cotangents.  grad_worst_loading goes to worst_line by ac_worst_cot's rule; grad_v_min and grad_v_max go to the
  // buses the forward reported.
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  PfsCot cot = {gr.p_from ? gr.p_from + (size_t)g * E : nullptr, gr.q_from ? gr.q_from + (size_t)g * E : nullptr,
                gr.p_to ? gr.p_to + (size_t)g * E : nullptr, gr.q_to ? gr.q_to + (size_t)g * E : nullptr, LamR, LamI, -1,
                make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
  ac_worst_cot(cot, gr.worst ? gr.worst[g] : 0.0, wl_in[g], N, E, rt, line, Vm, Vr, Vi);
  const double g_lo = gr.v_min ? gr.v_min[g] : 0.0, g_hi = gr.v_max ? gr.v_max[g] : 0.0;
  const int i_lo = lo_in[g], i_hi = hi_in[g];

  // dl/dtheta and dl/d|V| at every bus, the slack included: the gather of the line ends, the bus's own shunt, the extremes
  if (gv_out || gth_out)
    for (int i = lane; i < N; i += PF_THREADS) {
      double dth = 0.0;
      double dvm = 2.0 * Vm[i] * ((double)bus[i * 6 + 4] * LamR[i] - (double)bus[i * 6 + 5] * LamI[i]);
      if (i == i_lo) dvm += g_lo;
      if (i == i_hi) dvm += g_hi;
      ac_flow_cot_bus(i, N, y_diag, st_ptr, st, line, cot, Vm, Vr, Vi, dth, dvm);
      if (gth_out) gth_out[(size_t)g * N + i] = dth;
      if (gv_out) gv_out[(size_t)g * N + i] = dvm;
    }

  // the generators' Pg, a lane per slot: gen_p passes Pg through at every unit but the first on the slack; on the slack every listed
  // Pg leaves slack_p, and every one but the first leaves the first unit's gen_p
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = pf_slot_bus(gen_ptr, N, q);
      const int j = gen_idx[q];
      double gp = ggp ? ggp[j] : 0.0;
      if (b == slack) gp = q == gen_ptr[slack] ? 0.0 - gsp : gp - gsp - gfirst;
      float* row = gg_out + ((size_t)g * Gn + j) * 7;
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f; row[4] = 0.0f; row[5] = 0.0f;
      row[6] = (float)gp;                              // Pg
    }

  // the lines' r, x, b, tau, shift, a line per lane over its four stamps: ac_line_row_cot with -W where the mismatch
  // term has -Lambda; a line whose id columns are not buses of the grid gets a NaN row
  if (gl_out)
    for (int e = lane; e < E; e += PF_THREADS) {
      float* row = gl_out + ((size_t)g * E + e) * 7;
      int a, b2;
      if (!pf_line_ends(line, e, N, a, b2)) {
        for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
        continue;
      }
      double2 Wf, Wt;
      cot.at(e, a, b2, Wf, Wt);
      const AcLineCot d = ac_line_row_cot(line, e, a, b2, Vm, Vr, Vi, 0.0 - Wf.x, 0.0 - Wf.y, 0.0 - Wt.x, 0.0 - Wt.y);
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = (float)d.r; row[3] = (float)d.x; row[4] = (float)d.b; row[5] = (float)d.tau; row[6] = (float)d.sh;
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
