// Batched Newton-Raphson AC power flow (include/gns_powerflow.h): one wave per grid.  The grid's LU factor, right-hand side and
// bus state live in LDS; the Y-bus values of the grid go to the workspace once and are re-read every iteration.  Every grid runs
// the same elimination program of its topology blob (gns_pf_topology.cpp): steps of independent operations separated by barriers.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"

namespace {

constexpr int PF_THREADS = 64;   // one wave

__device__ inline bool pf_finite(double x) { return __builtin_isfinite(x); }

__device__ inline double pf_wave_max(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

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

  // Y-bus values (makeYbus), specified injections, starting point
  for (int i = lane; i < N; i += PF_THREADS) {
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      double yr = 0.0, yi = 0.0;
      if (p == y_diag[i]) { yr = (double)bus[i * 6 + 4]; yi = (double)bus[i * 6 + 5]; }
      for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
        const int e = st[q] >> 2, kind = st[q] & 3;
        const double r = line[e * 7 + 2], x = line[e * 7 + 3], b = line[e * 7 + 4], tau = line[e * 7 + 5], sh = line[e * 7 + 6];
        const double den = r * r + x * x;
        const double ysr = r / den, ysi = -x / den;
        double ar, ai;
        if (kind == 0) { ar = ysr / (tau * tau); ai = (ysi + 0.5 * b) / (tau * tau); }
        else if (kind == 1) { ar = ysr; ai = ysi + 0.5 * b; }
        else {
          const double c = cos(sh), s = kind == 2 ? sin(sh) : -sin(sh);   // -y_s e^{+-j shift} / tau
          ar = -(ysr * c - ysi * s) / tau;
          ai = -(ysr * s + ysi * c) / tau;
        }
        yr += ar; yi += ai;
      }
      Y[p] = make_double2(yr, yi);
    }
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
      double ir = 0.0, ii = 0.0;
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
    for (int i = lane; i < N; i += PF_THREADS) {
      if (i == slack) continue;
      const double vri = Vr[i], vii = Vi[i];
      for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
        const int k = y_col[p];
        if (k == slack) continue;
        const double2 y = Y[p];
        const double a = y.x * Vr[k] - y.y * Vi[k], b = y.x * Vi[k] + y.y * Vr[k];   // Y_ik V_k
        const double cr = vri * a + vii * b, ci = vii * a - vri * b;                 // V_i conj(Y_ik V_k)
        double dar = ci, dai = -cr;                                                  // dS_i / dtheta_k
        double dmr = cr, dmi = ci;                                                   // |V_k| dS_i / d|V_k|
        if (k == i) {
          const double P = vri * Ir[i] + vii * Ii[i], Q = vii * Ir[i] - vri * Ii[i];
          dar -= Q; dai += P;
          dmr += P; dmi += Q;
        }
        dmr /= Vm[k]; dmi /= Vm[k];
        const int s0 = jslot[4 * p], s1 = jslot[4 * p + 1], s2 = jslot[4 * p + 2], s3 = jslot[4 * p + 3];
        if (s0 >= 0) F[s0] = dar;
        if (s1 >= 0) F[s1] = dmr;
        if (s2 >= 0) F[s2] = dai;
        if (s3 >= 0) F[s3] = dmi;
      }
    }
    __syncthreads();

    // LU factorisation and both triangular solves: F[dst] -= F[a] F[b] or F[dst] /= F[a], independent within a step
    for (int s = 0; s < nsteps; ++s) {
      const int q1 = step_ptr[s + 1];
      for (int q = step_ptr[s] + lane; q < q1; q += PF_THREADS) {
        const int2 op = ops[q];
        const int dst = op.x & 0xFFFF, a = (int)((uint32_t)op.x >> 16);
        if (op.y < 0) F[dst] = F[dst] / F[a];
        else F[dst] -= F[a] * F[op.y];
      }
      __syncthreads();
    }

    // the update, only if every pivot is a finite non-zero and the new iterate is finite
    for (int k = lane; k < dim; k += PF_THREADS) {
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
// A grid without a usable blob (grid_off -1, or an offset that is misaligned, outside the set, or not at a blob of this shape
// whose LDS image and Y-bus fit the launch) gets the not-solved outputs and never indexes the set.
__global__ __launch_bounds__(PF_THREADS) void gns_pf_set_kernel(const int32_t* __restrict__ set, int64_t set_words,
                                                                const int32_t* __restrict__ grid_off, const int32_t* __restrict__ order,
                                                                int64_t Bt, int N, int E, int Gn, int64_t lds_bytes, int nnzy_max,
                                                                const float* __restrict__ buses, const float* __restrict__ lines,
                                                                const float* __restrict__ gens, const double* __restrict__ v0,
                                                                const double* __restrict__ th0, double* __restrict__ v_out,
                                                                double* __restrict__ th_out, uint8_t* __restrict__ conv_out,
                                                                int32_t* __restrict__ it_out, double* __restrict__ mis_out,
                                                                double2* __restrict__ ybus_ws, int max_iter, double tol) {
  const int64_t w = blockIdx.x;
  const int64_t g64 = order ? (int64_t)order[w] : w;
  if (g64 < 0 || g64 >= Bt) return;                             // not a grid of this batch: nothing to write
  const int g = (int)g64;
  const int64_t off = grid_off[g];
  bool ok = off >= 0 && off % PF_SET_ALIGN_WORDS == 0 && off + PF_HDR_WORDS <= set_words;
  const int32_t* topo = set + (ok ? off : 0);
  if (ok) {
    ok = topo[PH_MAGIC] == GNS_PF_MAGIC && topo[PH_N] == N && topo[PH_E] == E && topo[PH_GN] == Gn &&
         topo[PH_TOTAL] >= PF_HDR_WORDS && topo[PH_TOTAL] <= set_words - off && topo[PH_NNZY] >= 0 && topo[PH_NNZY] <= nnzy_max &&
         pf_lds_bytes(topo) <= lds_bytes;
  }
  if (!ok) {
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

size_t pf_ws_bytes_nnzy(int64_t nnzy, int64_t Bt) { return (((size_t)Bt * nnzy * sizeof(double2)) + 255) & ~(size_t)255; }
size_t pf_ws_bytes(const int32_t* h, int64_t Bt) { return pf_ws_bytes_nnzy(h[PH_NNZY], Bt); }

bool pf_header_ok(const gns_pf_config* cfg, const int32_t* h) {
  return h[PH_MAGIC] == GNS_PF_MAGIC && h[PH_N] == cfg->n_bus && h[PH_E] == cfg->n_line && h[PH_GN] == cfg->n_gen;
}

// Host check of the members of a set: each at an aligned word offset with its whole blob inside set_words, a blob of cfg's shape.
// Returns GNS_OK with the largest nnz(Y) and LDS image, GNS_EINVAL, or GNS_EUNSUPPORTED when a member's LDS image is too large.
int pf_scan_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off, int32_t n_member,
                int32_t* nnzy_max, int64_t* lds_max) {
  if (!cfg || !set_host || !member_off || n_member <= 0 || set_words > (size_t)INT32_MAX) return GNS_EINVAL;
  const int32_t* set = static_cast<const int32_t*>(set_host);
  int32_t ny = 0;
  int64_t lds = 0;
  bool too_big = false;
  for (int32_t m = 0; m < n_member; ++m) {
    const int64_t off = member_off[m];
    if (off < 0 || off % PF_SET_ALIGN_WORDS != 0 || off + PF_HDR_WORDS > (int64_t)set_words) return GNS_EINVAL;
    const int32_t* h = set + off;
    if (!pf_header_ok(cfg, h) || h[PH_TOTAL] < PF_HDR_WORDS || h[PH_TOTAL] > (int64_t)set_words - off || h[PH_NNZY] < 0)
      return GNS_EINVAL;
    ny = h[PH_NNZY] > ny ? h[PH_NNZY] : ny;
    const int64_t b = pf_lds_bytes(h);
    lds = b > lds ? b : lds;
    too_big |= b > GNS_PF_LDS_MAX_BYTES;
  }
  if (too_big) return GNS_EUNSUPPORTED;
  *nnzy_max = ny;
  *lds_max = lds;
  return GNS_OK;
}

}  // namespace

extern "C" int gns_pf_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!cfg || !topo_host || !bytes || Bt <= 0) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok(cfg, h)) return GNS_EINVAL;
  *bytes = pf_ws_bytes(h, Bt);
  return GNS_OK;
}

extern "C" int gns_pf_solve(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                            const float* buses, const float* lines, const float* generators, int64_t Bt,
                            const double* v0, const double* theta0,
                            double* v, double* theta, uint8_t* converged, int32_t* iterations, double* mismatch,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!cfg || !topo_host || !topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF) return GNS_EINVAL;
  if (!v || !theta || !converged || !iterations || !mismatch || !workspace) return GNS_EINVAL;
  if ((cfg->n_line > 0 && !lines) || cfg->max_iter < 0 || !(cfg->tol >= 0.0) || (v0 == nullptr) != (theta0 == nullptr))
    return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok(cfg, h)) return GNS_EINVAL;
  if (workspace_bytes < pf_ws_bytes(h, Bt)) return GNS_ESIZE;
  gns_pf_info info;
  if (gns_pf_topology_info(topo_host, &info) != GNS_OK) return GNS_EINVAL;
  if (info.lds_bytes > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gns_pf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GNS_PF_LDS_MAX_BYTES) != hipSuccess)
      return GNS_ELAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(gns_pf_kernel, dim3((unsigned)Bt), dim3(PF_THREADS), (size_t)info.lds_bytes, (hipStream_t)stream,
                     static_cast<const int32_t*>(topo_dev), buses, lines, generators, v0, theta0, v, theta, converged, iterations,
                     mismatch, static_cast<double2*>(workspace), cfg->max_iter, cfg->tol);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
}

extern "C" int gns_pf_workspace_bytes_set(const gns_pf_config* cfg, const void* set_host, size_t set_words, const int32_t* member_off,
                                          int32_t n_member, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
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
  if (!cfg || !set_dev || !grid_off || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF) return GNS_EINVAL;
  if (!v || !theta || !converged || !iterations || !mismatch || !workspace) return GNS_EINVAL;
  if (cfg->max_iter < 0 || !(cfg->tol >= 0.0) || (v0 == nullptr) != (theta0 == nullptr)) return GNS_EINVAL;
  int32_t nnzy = 0;
  int64_t lds = 0;
  const int rc = pf_scan_set(cfg, set_host, set_words, member_off, n_member, &nnzy, &lds);
  if (rc != GNS_OK) return rc;
  if (workspace_bytes < pf_ws_bytes_nnzy(nnzy, Bt)) return GNS_ESIZE;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gns_pf_set_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            GNS_PF_LDS_MAX_BYTES) != hipSuccess)
      return GNS_ELAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(gns_pf_set_kernel, dim3((unsigned)Bt), dim3(PF_THREADS), (size_t)lds, (hipStream_t)stream,
                     static_cast<const int32_t*>(set_dev), (int64_t)set_words, grid_off, order, Bt, cfg->n_bus, cfg->n_line,
                     cfg->n_gen, lds, nnzy, buses, lines, generators, v0, theta0, v, theta, converged, iterations, mismatch,
                     static_cast<double2*>(workspace), cfg->max_iter, cfg->tol);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
}
