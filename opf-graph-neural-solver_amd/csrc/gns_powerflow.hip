// Batched Newton-Raphson AC power flow (include/gns_powerflow.h): one wave per grid.  The grid's LU factor, right-hand side and
// bus state live in LDS; the Y-bus values of the grid go to the workspace once and are re-read every iteration.  Every grid runs
// the same elimination program of its topology blob (gns_pf_topology.cpp): steps of independent operations separated by barriers.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_ac_device.h"

namespace {

// The solve of grid g on the blob at topo: the body of both kernels below.  Its Y-bus values go to ybus_ws + g * (the blob's
// nnz(Y)), or with SET to ybus_ws + g * ystride (the largest nnz(Y) of a set).
template <bool SET>
__device__ __forceinline__ void pf_solve_grid(const int32_t* topo, const int g, const float* buses,
                                              const float* lines, const float* gens,
                                              const double* v0, const double* th0,
                                              double* v_out, double* th_out,
                                              uint8_t* conv_out, int32_t* it_out,
                                              double* mis_out, double2* ybus_ws, int ystride, int max_iter,
                                              double tol) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK], dim = topo[PH_DIM];
  const int nnzLU = topo[PH_NNZLU], nnzY = topo[PH_NNZY], nsteps = topo[PH_NSTEPS];
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

  double* F = lds;                       // [nnzLU] factor, then [dim] right-hand side / Newton step
  double* rhs = lds + nnzLU;
  double* Vm = rhs + dim;
  double* Va = Vm + N;
  double* Vr = Va + N;
  double* Vi = Vr + N;
  double* Ir = Vi + N;
  double* Ii = Ir + N;
  double* Psp = Ii + N;
  double* Qsp = Psp + N;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;
  double2* Y = ybus_ws + (size_t)g * (SET ? ystride : nnzY);

  // Y-bus values (makeYbus), specified injections, starting point.  This loop, the row product and the pivot test in the
  // iteration and the result store stay written out in this body although fd_solve_grid has the same loop and store and
  // gns_pf_device.h has pf_row_current and pf_bad_pivot: with any of them behind a shared helper the compiler allocates
  // gns_pf_kernel or gns_pf_set_kernel differently, and those variants (not kept) ran 1.1 to 3.8 % slower
  // (profiles/pf_refactor/gpu_time_helper_variants.txt).  As written both kernels compile to the instructions they had before.
  for (int i = lane; i < N; i += PF_THREADS) {
    pf_ybus_row(i, y_ptr, y_diag, st_ptr, st, bus, line, Y);
    double pg = 0.0;
    for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) pg += (double)gen[gen_idx[q] * 7 + 6];
    Psp[i] = pg - (double)bus[i * 6 + 2];
    Qsp[i] = -(double)bus[i * 6 + 3];
    const int ro = role[i];
    double vm = 1.0, va = 0.0;
    if (ro != 0 && gen_ptr[i + 1] > gen_ptr[i]) vm = (double)gen[gen_idx[gen_ptr[i]] * 7 + 4];
    if (v0 && ro == 0) vm = v0[(size_t)g * N + i];
    if (th0 && ro != 2) va = th0[(size_t)g * N + i] - th0[(size_t)g * N + slack];
    Vm[i] = vm; Va[i] = va;
  }
  __syncthreads();

  int it = 0;
  bool conv = false;
  double mis = 0.0;
  for (;;) {
    for (int i = lane; i < N; i += PF_THREADS) { Vr[i] = Vm[i] * cos(Va[i]); Vi[i] = Vm[i] * sin(Va[i]); }
    __syncthreads();
    // mismatch F = [Re(V conj(YV)) - P ; Im(...) - Q] into the right-hand side, and its infinity norm
    double nrm = 0.0;
    bool bad = false;
    for (int i = lane; i < N; i += PF_THREADS) {
      double ir = 0.0, ii = 0.0;                 // I_i = sum_k Y_ik V_k, pf_row_current's sum (written out: see the set-up loop)
      for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
        const int k = y_col[p];
        const double2 y = Y[p];
        ir += y.x * Vr[k] - y.y * Vi[k];
        ii += y.x * Vi[k] + y.y * Vr[k];
      }
      Ir[i] = ir; Ii[i] = ii;
      if (th_idx[i] >= 0) {
        const double fp = (Vr[i] * ir + Vi[i] * ii) - Psp[i];
        rhs[th_idx[i]] = fp;
        nrm = fmax(nrm, fabs(fp));
        bad |= !pf_finite(fp);
      }
      if (vm_idx[i] >= 0) {
        const double fq = (Vi[i] * ir - Vr[i] * ii) - Qsp[i];
        rhs[vm_idx[i]] = fq;
        nrm = fmax(nrm, fabs(fq));
        bad |= !pf_finite(fq);
      }
    }
    nrm = pf_wave_max(nrm);
    if (__ballot(bad)) { mis = __builtin_nan(""); break; }
    mis = nrm;
    if (nrm < tol) { conv = true; break; }
    if (it >= max_iter) break;

    // Jacobian (MATPOWER dSbus_dV, polar) into its factor slots; fill slots start at zero
    for (int s = lane; s < nnzLU; s += PF_THREADS) F[s] = 0.0;
    __syncthreads();
    for (int i = lane; i < N; i += PF_THREADS)
      if (i != slack) ac_jacobian_row(i, slack, y_ptr, y_col, jslot, AcPlainYbus{Y}, Vm, Vr, Vi, Ir, Ii, F);
    __syncthreads();

    // LU factorisation and both triangular solves: F[dst] -= F[a] F[b] or F[dst] /= F[a], independent within a step
    pf_run_program(nsteps, step_ptr, ops, F, lane);

    // the update, only if every pivot is a finite non-zero and the new iterate is finite
    for (int k = lane; k < dim; k += PF_THREADS) {      // pf_bad_pivot's test (written out: see the set-up loop)
      const double pv = F[pivot[k]];
      bad |= pv == 0.0 || !pf_finite(pv);
    }
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) bad |= !pf_finite(Va[i] - rhs[th_idx[i]]);
      if (vm_idx[i] >= 0) bad |= !pf_finite(Vm[i] - rhs[vm_idx[i]]);
    }
    if (__ballot(bad)) break;
    for (int i = lane; i < N; i += PF_THREADS) {
      if (th_idx[i] >= 0) Va[i] -= rhs[th_idx[i]];
      if (vm_idx[i] >= 0) Vm[i] -= rhs[vm_idx[i]];
    }
    __syncthreads();
    ++it;
  }

  for (int i = lane; i < N; i += PF_THREADS) {
    v_out[(size_t)g * N + i] = Vm[i];
    th_out[(size_t)g * N + i] = Va[i];
  }
  if (lane == 0) { conv_out[g] = conv ? 1 : 0; it_out[g] = it; mis_out[g] = mis; }
}

__global__ __launch_bounds__(PF_THREADS) void gns_pf_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                            const float* __restrict__ lines, const float* __restrict__ gens,
                                                            const double* __restrict__ v0, const double* __restrict__ th0,
                                                            double* __restrict__ v_out, double* __restrict__ th_out,
                                                            uint8_t* __restrict__ conv_out, int32_t* __restrict__ it_out,
                                                            double* __restrict__ mis_out, double2* __restrict__ ybus_ws,
                                                            int max_iter, double tol) {
  const int g = blockIdx.x;
  pf_solve_grid<false>(topo, g, buses, lines, gens, v0, th0, v_out, th_out, conv_out, it_out, mis_out, ybus_ws, 0, max_iter, tol);
}

// A batch over a set of blobs (gns_pf_solve_set): workgroup w solves grid g = order ? order[w] : w on the blob at set + grid_off[g].
// A grid without a usable blob (pf_set_member) gets the not-solved outputs and never indexes the set.
__global__ __launch_bounds__(PF_THREADS) void gns_pf_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                const int32_t* __restrict__ grid_off, const int32_t* __restrict__ order,
                                                                int64_t Bt, int N, int E, int Gn, int64_t lds_bytes, int nnzy_max,
                                                                const float* __restrict__ buses, const float* __restrict__ lines,
                                                                const float* __restrict__ gens, const double* __restrict__ v0,
                                                                const double* __restrict__ th0, double* __restrict__ v_out,
                                                                double* __restrict__ th_out, uint8_t* __restrict__ conv_out,
                                                                int32_t* __restrict__ it_out, double* __restrict__ mis_out,
                                                                double2* __restrict__ ybus_ws, int max_iter, double tol) {
  const int64_t g64 = pf_set_grid(order);
  if (g64 < 0 || g64 >= Bt) return;                             // not a grid of this batch: nothing to write
  const int g = (int)g64;
  const int32_t* topo;
  if (!pf_set_member<PfBlobKind>(set, set_words, grid_off[g], N, E, Gn, lds_bytes, nnzy_max, topo)) {
    // the not-solved outputs.  (Also in gns_fd_set_kernel, inline in both: as a shared helper these stores moved this kernel's
    // scalar register allocation, 56 -> 39 SGPR spills, and it ran 2.4-3.2 % slower: profiles/pf_refactor/gpu_time_helper_variants.txt.)
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < N; i += PF_THREADS) {
      v_out[(size_t)g * N + i] = nan;
      th_out[(size_t)g * N + i] = nan;
    }
    if (threadIdx.x == 0) { conv_out[g] = 0; it_out[g] = -1; mis_out[g] = nan; }
    return;
  }
  pf_solve_grid<true>(topo, g, buses, lines, gens, v0, th0, v_out, th_out, conv_out, it_out, mis_out, ybus_ws, nnzy_max, max_iter,
                      tol);
}

// ---- the adjoint (gns_pf_adjoint): gradients of a loss of (v, theta) at a converged solution, by the implicit function theorem:
// J^T lambda = dl/dx at the solution, dl/dp = -lambda^T dF/dp (include/gns_powerflow.h, "Gradients").

// Whether grid g's incoming gradient rows are all exactly zero (a NULL row counts as zero)
__device__ __forceinline__ bool pf_zero_incoming(const int g, const int N, const double* gv, const double* gth) {
  bool nz = false;
  for (int i = threadIdx.x; i < N; i += PF_THREADS) {
    if (gv) nz |= gv[(size_t)g * N + i] != 0.0;
    if (gth) nz |= gth[(size_t)g * N + i] != 0.0;
  }
  return __ballot(nz) == 0;
}

// The adjoint of grid g (converged, with a non-zero incoming gradient) on the blob at topo: the body of both adjoint kernels.
// LDS: the solve's image, lambda in the Psp / Qsp vectors.  The Y-bus values go to the workspace as in pf_solve_grid.
template <bool SET>
__device__ __forceinline__ void pf_adjoint_grid(const int32_t* topo, const int g, const float* buses, const float* lines,
                                                const double* v_in, const double* th_in, const double* gv,
                                                const double* gth, float* gb_out, float* gl_out, float* gg_out, double2* ybus_ws,
                                                int ystride) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN], slack = topo[PH_SLACK], dim = topo[PH_DIM];
  const int nnzLU = topo[PH_NNZLU], nnzY = topo[PH_NNZY], t_nsteps = topo[PH_T_NSTEPS];
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

  double* F = lds;                       // [nnzLU] factor, then [dim] right-hand side / lambda
  double* rhs = lds + nnzLU;
  double* Vm = rhs + dim;
  double* Va = Vm + N;
  double* Vr = Va + N;
  double* Vi = Vr + N;
  double* Ir = Vi + N;
  double* Ii = Ir + N;
  double* lamP = Ii + N;                 // the solve's Psp / Qsp: lambda of each bus's P and Q mismatch (0 where there is none)
  double* lamQ = lamP + N;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  double2* Y = ybus_ws + (size_t)g * (SET ? ystride : nnzY);

  // the solution, the Y-bus values and I = Y V there
  for (int i = lane; i < N; i += PF_THREADS) {
    pf_ybus_row(i, y_ptr, y_diag, st_ptr, st, bus, line, Y);
    const double vm = v_in[(size_t)g * N + i], va = th_in[(size_t)g * N + i];
    Vm[i] = vm; Va[i] = va;
    Vr[i] = vm * cos(va); Vi[i] = vm * sin(va);
  }
  for (int s = lane; s < nnzLU + dim; s += PF_THREADS) F[s] = 0.0;
  __syncthreads();
  for (int i = lane; i < N; i += PF_THREADS) {
    const double2 cur = pf_row_current(i, y_ptr, y_col, Y, Vr, Vi);
    Ir[i] = cur.x; Ii[i] = cur.y;
  }
  __syncthreads();

  // J at the solution, factored by the leading steps of the solve program (its solve operations there see a zero right-hand side)
  for (int i = lane; i < N; i += PF_THREADS)
    if (i != slack) ac_jacobian_row(i, slack, y_ptr, y_col, jslot, AcPlainYbus{Y}, Vm, Vr, Vi, Ir, Ii, F);
  __syncthreads();
  pf_run_program(t_step_ptr[t_nsteps + 1], step_ptr, ops, F, lane);   // the steps that hold the factorisation
  if (__ballot(pf_bad_pivot(dim, pivot, F, lane))) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }

  // J^T lambda = [dl/dtheta at PV+PQ ; dl/d|V| at PQ] (the slack's theta is constant: its incoming gradient is not used)
  for (int i = lane; i < N; i += PF_THREADS) {
    if (th_idx[i] >= 0) rhs[th_idx[i]] = gth ? gth[(size_t)g * N + i] : 0.0;
    if (vm_idx[i] >= 0) rhs[vm_idx[i]] = gv ? gv[(size_t)g * N + i] : 0.0;
  }
  __syncthreads();
  pf_run_program(t_nsteps, t_step_ptr, t_ops, F, lane);
  for (int i = lane; i < N; i += PF_THREADS) {
    lamP[i] = th_idx[i] >= 0 ? rhs[th_idx[i]] : 0.0;
    lamQ[i] = vm_idx[i] >= 0 ? rhs[vm_idx[i]] : 0.0;
  }
  __syncthreads();

  // dl/dp = -lambda^T dF/dp.  F_P = Re S - (Pg - Pd), F_Q = Im S + Qd with S_i = V_i conj(sum_k Y_ik V_k); a real parameter that
  // moves Y_ik by c moves S_i by V_i conj(V_k) conj(c), so dl/dp = Re(conj(c) G_ik) with G_ik = -V_i conj(V_k) conj(Lambda_i),
  // Lambda = lamP + j lamQ.  (0.0 - x rather than -x: an exact zero stays +0.)
  if (gb_out)
    for (int i = lane; i < N; i += PF_THREADS) {
      float* row = gb_out + ((size_t)g * N + i) * 6;
      const double m2 = Vm[i] * Vm[i], lp = lamP[i], lq = lamQ[i];
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = (float)(0.0 - lp);            // Pd
      row[3] = (float)(0.0 - lq);            // Qd
      row[4] = (float)(0.0 - m2 * lp);       // Gs: c = 1 on Y_ii
      row[5] = (float)(m2 * lq);             // Bs: c = j
    }
  if (gg_out)
    for (int q = lane; q < Gn; q += PF_THREADS) {      // a lane per generator, in the blob's by-bus order
      const int b = pf_slot_bus(gen_ptr, N, q);
      const int j = gen_idx[q];
      double gvg = 0.0;
      if (q == gen_ptr[b] && role[b] != 0) {           // the first generator of a PV / slack bus sets |V_b|
        const double acc = ac_vg_column(b, cos(Va[b]), sin(Va[b]), y_ptr, y_col, AcPlainYbus{Y}, Vr, Vi, Ir, Ii, lamP, lamQ);
        gvg = (gv ? gv[(size_t)g * N + b] : 0.0) - acc;
      }
      float* row = gg_out + ((size_t)g * Gn + j) * 7;
      row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f;
      row[4] = (float)gvg;                             // vg
      row[5] = 0.0f;
      row[6] = (float)lamP[b];                         // Pg: S_spec += Pg
    }
  if (gl_out)
    for (int e = lane; e < E; e += PF_THREADS) {      // a lane per line, over its four stamps
      float* row = gl_out + ((size_t)g * E + e) * 7;
      int f, t;                                        // from the id columns the blob was prepared from (1-based)
      if (!pf_line_ends(line, e, N, f, t)) {
        for (int c = 0; c < 7; ++c) row[c] = __builtin_nanf("");
        continue;
      }
      const AcLineCot d = ac_line_row_cot(line, e, f, t, Vm, Vr, Vi, lamP[f], lamQ[f], lamP[t], lamQ[t]);
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = (float)d.r; row[3] = (float)d.x; row[4] = (float)d.b; row[5] = (float)d.tau; row[6] = (float)d.sh;
    }
}

__global__ __launch_bounds__(PF_THREADS) void gns_pf_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                    const float* __restrict__ lines, const float* __restrict__ gens,
                                                                    const double* __restrict__ v_in, const double* __restrict__ th_in,
                                                                    const uint8_t* __restrict__ conv_in,
                                                                    const double* __restrict__ gv, const double* __restrict__ gth,
                                                                    float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                    float* __restrict__ gg_out, double2* __restrict__ ybus_ws) {
  const int g = blockIdx.x;
  const int N = topo[PH_N], E = topo[PH_E], Gn = topo[PH_GN];
  if (pf_zero_incoming(g, N, gv, gth)) { pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out); return; }
  if (!conv_in[g]) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }
  pf_adjoint_grid<false>(topo, g, buses, lines, v_in, th_in, gv, gth, gb_out, gl_out, gg_out, ybus_ws, 0);
}

// The adjoint over a set of blobs (gns_pf_adjoint_set): the grid, order and blob checks of gns_pf_set_kernel; a grid without a
// usable blob gets NaN rows (zero rows when its incoming gradient is zero) and never indexes the set.
__global__ __launch_bounds__(PF_THREADS) void gns_pf_adjoint_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                        const int32_t* __restrict__ grid_off,
                                                                        const int32_t* __restrict__ order, int64_t Bt, int N, int E,
                                                                        int Gn, int64_t lds_bytes, int nnzy_max,
                                                                        const float* __restrict__ buses,
                                                                        const float* __restrict__ lines,
                                                                        const float* __restrict__ gens,
                                                                        const double* __restrict__ v_in,
                                                                        const double* __restrict__ th_in,
                                                                        const uint8_t* __restrict__ conv_in,
                                                                        const double* __restrict__ gv, const double* __restrict__ gth,
                                                                        float* __restrict__ gb_out, float* __restrict__ gl_out,
                                                                        float* __restrict__ gg_out, double2* __restrict__ ybus_ws) {
  const int64_t g64 = pf_set_grid(order);
  if (g64 < 0 || g64 >= Bt) return;
  const int g = (int)g64;
  if (pf_zero_incoming(g, N, gv, gth)) { pf_adjoint_fill(g, N, E, Gn, 0.0f, gb_out, gl_out, gg_out); return; }
  const int32_t* topo;
  const bool ok = pf_set_member<PfBlobKind>(set, set_words, grid_off[g], N, E, Gn, lds_bytes, nnzy_max, topo);
  if (!ok || !conv_in[g]) { pf_adjoint_fill(g, N, E, Gn, __builtin_nanf(""), gb_out, gl_out, gg_out); return; }
  pf_adjoint_grid<true>(topo, g, buses, lines, v_in, th_in, gv, gth, gb_out, gl_out, gg_out, ybus_ws, nnzy_max);
}

}  // namespace

extern "C" int gns_pf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<PfBlobKind>(cfg, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(h[PH_NNZY], Bt);
  return GNS_OK;
}

extern "C" int gns_pf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                            const float* buses, const float* lines, const float* generators, int64_t Bt,
                            const double* v0, const double* theta0,
                            double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !topo_host ||
      !pf_solve_args_ok(topo_dev, buses, lines, generators, Bt, v0, theta0, v, theta, converged, iterations, mismatch, workspace))
    return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = pf_check_topology<PfBlobKind>(cfg, static_cast<const int32_t*>(topo_host), Bt, workspace_bytes, &lds);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_pf_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, v0, theta0, v,
                                  theta, converged, iterations, mismatch, static_cast<double2*>(workspace), cfg->max_iter, cfg->tol);
}

extern "C" int gns_pf_workspace_bytes_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                          int32_t n_member, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set<PfBlobKind>(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  *bytes = pf_ws_bytes_nnzy(nnzy, Bt);
  return GNS_OK;
}

extern "C" int gns_pf_solve_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const double* v0, const double* theta0,
                                double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !grid_off ||
      !pf_solve_args_ok(set_dev, buses, lines, generators, Bt, v0, theta0, v, theta, converged, iterations, mismatch, workspace))
    return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set<PfBlobKind>(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  if (workspace_bytes < pf_ws_bytes_nnzy(nnzy, Bt)) return GNS_ESIZE;
  return pf_launch<gns_pf_set_kernel>(Bt, lds, stream, static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off, order, Bt,
                                      cfg->n_bus, cfg->n_line, cfg->n_gen, lds, nnzy, buses, lines, generators, v0, theta0, v, theta,
                                      converged, iterations, mismatch, static_cast<double2*>(workspace), cfg->max_iter, cfg->tol);
}

// The adjoint calls check max_iter and tol as the solves do although they use neither: a configuration a solve refuses is
// refused here too.  With no gradient output asked for they return GNS_OK without a launch, after every other check.
extern "C" int gns_pf_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                              const float* buses, const float* lines, const float* generators, int64_t Bt,
                              const double* v, const double* theta, const uint8_t* converged,
                              const double* grad_v, const double* grad_theta,
                              float* grad_buses, float* grad_lines, float* grad_generators,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !topo_host || !pf_adjoint_args_ok(topo_dev, buses, lines, generators, Bt, v, theta, converged, workspace))
    return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = pf_check_topology<PfBlobKind>(cfg, static_cast<const int32_t*>(topo_host), Bt, workspace_bytes, &lds);
  if (rc != GNS_OK) return rc;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  return pf_launch<gns_pf_adjoint_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, v, theta,
                                          converged, grad_v, grad_theta, grad_buses, grad_lines, grad_generators,
                                          static_cast<double2*>(workspace));
}

extern "C" int gns_pf_adjoint_set(const gns_pf_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                  const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                                  const float* buses, const float* lines, const float* generators, int64_t Bt,
                                  const double* v, const double* theta, const uint8_t* converged,
                                  const double* grad_v, const double* grad_theta,
                                  float* grad_buses, float* grad_lines, float* grad_generators,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!pf_config_ok(cfg) || !grid_off || !pf_adjoint_args_ok(set_dev, buses, lines, generators, Bt, v, theta, converged, workspace))
    return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set<PfBlobKind>(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  if (workspace_bytes < pf_ws_bytes_nnzy(nnzy, Bt)) return GNS_ESIZE;
  if (!grad_buses && !grad_lines && !grad_generators) return GNS_OK;
  return pf_launch<gns_pf_adjoint_set_kernel>(Bt, lds, stream, static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off,
                                              order, Bt, cfg->n_bus, cfg->n_line, cfg->n_gen, lds, nnzy, buses, lines, generators, v,
                                              theta, converged, grad_v, grad_theta, grad_buses, grad_lines, grad_generators,
                                              static_cast<double2*>(workspace));
}
