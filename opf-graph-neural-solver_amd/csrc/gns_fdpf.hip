// Batched fast-decoupled AC power flow, XB and BX (include/gns_powerflow.h, "Fast-decoupled"): one wave per grid.  B' and B''
// are built from the line rows straight into their factor slots, factored once by the blob's two factorisation programs, and
// every half-step is one mismatch pass and one triangular-solve program.  Both factors, both right-hand sides and the bus state
// live in LDS; the Y-bus values of the grid go to the workspace once and are re-read by every mismatch pass.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"

namespace {

// Row i of B' and B'' (makeB: -Im(Y) of modified copies of the grid) into their factor slots (FH_BSLOT).  B': Bs = 0, b = 0,
// tau = 1, shift kept, r = 0 with XB; B'': shift = 0, r = 0 with BX, everything else as given.
__device__ __forceinline__ void fd_b_row(const int i, const int32_t* y_ptr, const int32_t* y_diag, const int32_t* st_ptr,
                                         const int32_t* st, const int32_t* bslot, const float* bus, const float* line,
                                         const bool xb, const bool bx, double* F1, double* F2) {
  for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
    const int s1 = bslot[2 * p], s2 = bslot[2 * p + 1];
    if (s1 < 0 && s2 < 0) continue;
    double b1 = 0.0, b2 = 0.0;
    if (p == y_diag[i]) b2 = 0.0 - (double)bus[i * 6 + 5];
    for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
      const int e = st[q] >> 2, kind = st[q] & 3;
      const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
      const double r1 = xb ? 0.0 : r, r2 = bx ? 0.0 : r;
      const double den1 = r1 * r1 + x * x, den2 = r2 * r2 + x * x;
      const double ysr1 = r1 / den1, ysi1 = -x / den1, ysi2 = -x / den2;
      double a1, a2;                                        // Im of the stamp in the B' grid and in the B'' grid
      if (kind == 0) { a1 = ysi1; a2 = (ysi2 + 0.5 * b) / (tau * tau); }
      else if (kind == 1) { a1 = ysi1; a2 = ysi2 + 0.5 * b; }
      else {
        const double c = cos(sh), s = kind == 2 ? sin(sh) : -sin(sh);   // Im(-y_s e^{+-j shift}), tau = 1
        a1 = -(ysr1 * s + ysi1 * c);
        a2 = -ysi2 / tau;                                   // Im(-y_s / tau), shift = 0
      }
      b1 -= a1; b2 -= a2;
    }
    if (s1 >= 0) F1[s1] = b1;
    if (s2 >= 0) F2[s2] = b2;
  }
}

// The scaled mismatch mis = (V conj(YV) - S) / |V| at (Vm, Va): P = Re(mis) into rhs1 at PV+PQ, Q = Im(mis) into rhs2 at PQ.
// Returns max(||P||_inf, ||Q||_inf), or NaN when any of them is not finite (wave-uniform).
__device__ __forceinline__ double fd_mismatch(const int N, const int32_t* y_ptr, const int32_t* y_col, const int32_t* p_idx,
                                              const int32_t* q_idx, const double2* Y, const double* Vm, const double* Va,
                                              double* Vr, double* Vi, const double* Psp, const double* Qsp, double* rhs1,
                                              double* rhs2, const int lane) {
  for (int i = lane; i < N; i += PF_THREADS) { Vr[i] = Vm[i] * cos(Va[i]); Vi[i] = Vm[i] * sin(Va[i]); }
  __syncthreads();
  double nrm = 0.0;
  bool bad = false;
  for (int i = lane; i < N; i += PF_THREADS) {
    const double2 cur = pf_row_current(i, y_ptr, y_col, Y, Vr, Vi);
    const double ir = cur.x, ii = cur.y;
    if (p_idx[i] >= 0) {
      const double fp = ((Vr[i] * ir + Vi[i] * ii) - Psp[i]) / Vm[i];
      rhs1[p_idx[i]] = fp;
      nrm = fmax(nrm, fabs(fp));
      bad |= !pf_finite(fp);
    }
    if (q_idx[i] >= 0) {
      const double fq = ((Vi[i] * ir - Vr[i] * ii) - Qsp[i]) / Vm[i];
      rhs2[q_idx[i]] = fq;
      nrm = fmax(nrm, fabs(fq));
      bad |= !pf_finite(fq);
    }
  }
  nrm = pf_wave_max(nrm);
  __syncthreads();                                          // rhs1 / rhs2 complete before a solve program reads them
  return __ballot(bad) ? __builtin_nan("") : nrm;
}

// One half-step: solve the factor F (rhs at F + nnz) for the step, then x[bus] -= step at the buses idx maps; false (nothing
// updated) when a new value would not be finite.
__device__ __forceinline__ bool fd_half_step(const int N, const int nsteps, const int32_t* step_ptr, const int2* ops, double* F,
                                             const double* rhs, const int32_t* idx, double* x, const int lane) {
  pf_run_program(nsteps, step_ptr, ops, F, lane);
  bool bad = false;
  for (int i = lane; i < N; i += PF_THREADS)
    if (idx[i] >= 0) bad |= !pf_finite(x[i] - rhs[idx[i]]);
  if (__ballot(bad)) return false;
  for (int i = lane; i < N; i += PF_THREADS)
    if (idx[i] >= 0) x[i] -= rhs[idx[i]];
  __syncthreads();
  return true;
}

// The solve of grid g on the FD blob at topo: the body of both kernels below (Y-bus workspace as pf_solve_grid's).
template <bool SET>
__device__ __forceinline__ void fd_solve_grid(const int32_t* topo, const int g, const float* buses, const float* lines,
                                              const float* gens, const double* v0, const double* th0, double* v_out,
                                              double* th_out, uint8_t* conv_out, int32_t* it_out, double* mis_out,
                                              double2* ybus_ws, int ystride, int max_iter, double tol, int alg) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], slack = topo[FH_SLACK], nnzY = topo[FH_NNZY];
  const int d1 = topo[FH_DIM1], nnz1 = topo[FH_NNZLU1], d2 = topo[FH_DIM2], nnz2 = topo[FH_NNZLU2];
  const int32_t* role = topo + topo[FH_ROLE];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* q_idx = topo + topo[FH_Q_IDX];
  const int32_t* gen_ptr = topo + topo[FH_GEN_PTR];
  const int32_t* gen_idx = topo + topo[FH_GEN_IDX];
  const int32_t* y_ptr = topo + topo[FH_Y_PTR];
  const int32_t* y_col = topo + topo[FH_Y_COL];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int32_t* bslot = topo + topo[FH_BSLOT];
  const int32_t* piv1 = topo + topo[FH_PIVOT1];
  const int32_t* piv2 = topo + topo[FH_PIVOT2];

  double* F1 = lds;                      // [nnz1] B' factor, then [d1] right-hand side / step
  double* rhs1 = F1 + nnz1;
  double* F2 = rhs1 + d1;                // [nnz2] B'' factor, then [d2]
  double* rhs2 = F2 + nnz2;
  double* Vm = rhs2 + d2;
  double* Va = Vm + N;
  double* Vr = Va + N;
  double* Vi = Vr + N;
  double* Psp = Vi + N;
  double* Qsp = Psp + N;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;
  double2* Y = ybus_ws + (size_t)g * (SET ? ystride : nnzY);

  // Y-bus values (makeYbus), specified injections, starting point: those of pf_solve_grid, inline here and there, as the result
  // store below (the reason is given there); fill slots of both factors start at 0
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
  for (int s = lane; s < nnz1; s += PF_THREADS) F1[s] = 0.0;
  for (int s = lane; s < nnz2; s += PF_THREADS) F2[s] = 0.0;
  __syncthreads();

  // B' and B'' into their slots, both factored once
  for (int i = lane; i < N; i += PF_THREADS) fd_b_row(i, y_ptr, y_diag, st_ptr, st, bslot, bus, line, alg == 2, alg == 3, F1, F2);
  __syncthreads();
  pf_run_program(topo[FH_NSTEPS_F1], topo + topo[FH_STEP_F1], reinterpret_cast<const int2*>(topo + topo[FH_OPS_F1]), F1, lane);
  pf_run_program(topo[FH_NSTEPS_F2], topo + topo[FH_STEP_F2], reinterpret_cast<const int2*>(topo + topo[FH_OPS_F2]), F2, lane);
  bool bad_pivot = pf_bad_pivot(d1, piv1, F1, lane);
  bad_pivot |= pf_bad_pivot(d2, piv2, F2, lane);
  bad_pivot = __ballot(bad_pivot) != 0;

  const int ns1 = topo[FH_NSTEPS_S1], ns2 = topo[FH_NSTEPS_S2];
  const int32_t* sp1 = topo + topo[FH_STEP_S1];
  const int32_t* sp2 = topo + topo[FH_STEP_S2];
  const int2* ops1 = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);
  const int2* ops2 = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S2]);
  int it = 0;
  bool conv = false;
  double mis = fd_mismatch(N, y_ptr, y_col, p_idx, q_idx, Y, Vm, Va, Vr, Vi, Psp, Qsp, rhs1, rhs2, lane);
  if (mis < tol) conv = true;
  else if (pf_finite(mis) && !bad_pivot) {
    while (it < max_iter) {
      if (!fd_half_step(N, ns1, sp1, ops1, F1, rhs1, p_idx, Va, lane)) break;   // P half-step: theta -= B'^-1 P
      ++it;
      mis = fd_mismatch(N, y_ptr, y_col, p_idx, q_idx, Y, Vm, Va, Vr, Vi, Psp, Qsp, rhs1, rhs2, lane);
      if (!pf_finite(mis)) break;
      if (mis < tol) { conv = true; break; }
      if (!fd_half_step(N, ns2, sp2, ops2, F2, rhs2, q_idx, Vm, lane)) break;   // Q half-step: |V| -= B''^-1 Q
      mis = fd_mismatch(N, y_ptr, y_col, p_idx, q_idx, Y, Vm, Va, Vr, Vi, Psp, Qsp, rhs1, rhs2, lane);
      if (!pf_finite(mis)) break;
      if (mis < tol) { conv = true; break; }
    }
  }

  for (int i = lane; i < N; i += PF_THREADS) {
    v_out[(size_t)g * N + i] = Vm[i];
    th_out[(size_t)g * N + i] = Va[i];
  }
  if (lane == 0) { conv_out[g] = conv ? 1 : 0; it_out[g] = it; mis_out[g] = mis; }
}

__global__ __launch_bounds__(PF_THREADS) void gns_fd_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                            const float* __restrict__ lines, const float* __restrict__ gens,
                                                            const double* __restrict__ v0, const double* __restrict__ th0,
                                                            double* __restrict__ v_out, double* __restrict__ th_out,
                                                            uint8_t* __restrict__ conv_out, int32_t* __restrict__ it_out,
                                                            double* __restrict__ mis_out, double2* __restrict__ ybus_ws,
                                                            int max_iter, double tol, int alg) {
  const int g = blockIdx.x;
  fd_solve_grid<false>(topo, g, buses, lines, gens, v0, th0, v_out, th_out, conv_out, it_out, mis_out, ybus_ws, 0, max_iter, tol,
                       alg);
}

// A batch over a set of FD blobs (gns_fd_solve_set): the grid, order and blob checks of gns_pf_set_kernel, on FD blobs.
__global__ __launch_bounds__(PF_THREADS) void gns_fd_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                const int32_t* __restrict__ grid_off, const int32_t* __restrict__ order,
                                                                int64_t Bt, int N, int E, int Gn, int64_t lds_bytes, int nnzy_max,
                                                                const float* __restrict__ buses, const float* __restrict__ lines,
                                                                const float* __restrict__ gens, const double* __restrict__ v0,
                                                                const double* __restrict__ th0, double* __restrict__ v_out,
                                                                double* __restrict__ th_out, uint8_t* __restrict__ conv_out,
                                                                int32_t* __restrict__ it_out, double* __restrict__ mis_out,
                                                                double2* __restrict__ ybus_ws, int max_iter, double tol, int alg) {
  const int64_t g64 = pf_set_grid(order);
  if (g64 < 0 || g64 >= Bt) return;                             // not a grid of this batch: nothing to write
  const int g = (int)g64;
  const int32_t* topo;
  if (!pf_set_member<FdBlobKind>(set, set_words, grid_off[g], N, E, Gn, lds_bytes, nnzy_max, topo)) {
    // the not-solved outputs, inline as in gns_pf_set_kernel (the reason is given there)
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < N; i += PF_THREADS) {
      v_out[(size_t)g * N + i] = nan;
      th_out[(size_t)g * N + i] = nan;
    }
    if (threadIdx.x == 0) { conv_out[g] = 0; it_out[g] = -1; mis_out[g] = nan; }
    return;
  }
  fd_solve_grid<true>(topo, g, buses, lines, gens, v0, th0, v_out, th_out, conv_out, it_out, mis_out, ybus_ws, nnzy_max, max_iter,
                      tol, alg);
}

bool fd_config_ok(const gns_fd_config* cfg) { return cfg && pf_config_ok(&cfg->pf) && (cfg->alg == 2 || cfg->alg == 3); }

}  // namespace

extern "C" int gns_fd_workspace_bytes(const gns_fd_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<FdBlobKind>(&cfg->pf, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes_nnzy(h[FH_NNZY], Bt);
  return GNS_OK;
}

extern "C" int gns_fd_solve(const gns_fd_config* cfg, const void* topo_host, const void* topo_dev,
                            const float* buses, const float* lines, const float* generators, int64_t Bt,
                            const double* v0, const double* theta0,
                            double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!fd_config_ok(cfg) || !topo_host ||
      !pf_solve_args_ok(topo_dev, buses, lines, generators, Bt, v0, theta0, v, theta, converged, iterations, mismatch, workspace))
    return GNS_EINVAL;
  int64_t lds = 0;
  const int rc = pf_check_topology<FdBlobKind>(&cfg->pf, static_cast<const int32_t*>(topo_host), Bt, workspace_bytes, &lds);
  if (rc != GNS_OK) return rc;
  return pf_launch<gns_fd_kernel>(Bt, lds, stream, static_cast<const int32_t*>(topo_dev), buses, lines, generators, v0, theta0, v,
                                  theta, converged, iterations, mismatch, static_cast<double2*>(workspace), cfg->pf.max_iter,
                                  cfg->pf.tol, cfg->alg);
}

extern "C" int gns_fd_workspace_bytes_set(const gns_fd_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                          int32_t n_member, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set<FdBlobKind>(cfg ? &cfg->pf : nullptr, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  *bytes = pf_ws_bytes_nnzy(nnzy, Bt);
  return GNS_OK;
}

extern "C" int gns_fd_solve_set(const gns_fd_config* cfg, const void* set_host, const void* set_dev, size_t set_words,
                                const int32_t* member_off, int32_t n_member, const int32_t* grid_off, const int32_t* order,
                                const float* buses, const float* lines, const float* generators, int64_t Bt,
                                const double* v0, const double* theta0,
                                double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!fd_config_ok(cfg) || !grid_off ||
      !pf_solve_args_ok(set_dev, buses, lines, generators, Bt, v0, theta0, v, theta, converged, iterations, mismatch, workspace))
    return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set<FdBlobKind>(&cfg->pf, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  if (workspace_bytes < pf_ws_bytes_nnzy(nnzy, Bt)) return GNS_ESIZE;
  return pf_launch<gns_fd_set_kernel>(Bt, lds, stream, static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off, order, Bt,
                                      cfg->pf.n_bus, cfg->pf.n_line, cfg->pf.n_gen, lds, nnzy, buses, lines, generators, v0, theta0,
                                      v, theta, converged, iterations, mismatch, static_cast<double2*>(workspace), cfg->pf.max_iter,
                                      cfg->pf.tol, cfg->alg);
}
