// The adjoint of the batched DC optimal power flow (include/gns_powerflow.h, "DC optimal power flow: adjoint"): the gradient of a
// loss on the eight outputs of gns_dcopf_solve with respect to Pd and Gs, Pmax and Pmin, the costs and the ratings, by the
// implicit-function theorem on the KKT conditions of the problem reduced to the dispatch p.  The active rows are held as equalities
// and the other multipliers as constants, so the system is the symmetric
//
//     [ diag(2 c2_F)  1    S_aF^T ] [a_p     ]   [g_p     ]
//     [ 1^T           0    0      ] [a_lambda] = [g_lambda]        F: the units inside their bounds, a: the active lines
//     [ S_aF          0    0      ] [a_mu    ]   [g_mu    ]
//
// once the units at a bound are substituted (their a_p is the cotangent of their own multiplier, their a_nu follows from their
// stationarity row).  It is solved dense in LDS by LU with partial pivoting: exact for c2 = 0, never regularised, never squared
// into S Q^-1 S^T.  The forward's normal matrix is not used: it is conditioned 1e14 to 1e20 on linear programs.
//
// Two launches:
//   gns_dcopf_factor_kernel   gns_dcopf.hip's, unchanged, into this call's workspace: S as [E][Gn] per grid
//   gns_dcopf_adjoint_kernel  a wave per grid: the base factor again, the active set from the returned tensors, two network solves
//                             that pull the cotangents of theta, line_flow and lmp back, the KKT solve, a third network solve that
//                             carries a_mu through f0 to the loads, then every gradient row
// No atomics, every sum in a fixed order: a grid's gradient is bit-identical alone, in any batch, in any order and from run to run.
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dc_device.h"
#include "gns_dcn1_device.h"
#include "gns_dcopf_device.h"

namespace {

// What the forward returned and what comes in for it (NULL: zero), by output
struct DcopfAdjointIn {
  const double *pg, *theta, *flow, *lmp, *mu_line, *mu_pmax, *mu_pmin, *objective;
  const uint8_t* converged;
  const int32_t* iterations;
  const double *g_pg, *g_theta, *g_flow, *g_lmp, *g_mu_line, *g_mu_pmax, *g_mu_pmin, *g_objective;
};

// The gradient rows (NULL: not wanted): buses [Bt,N,6] and generators [Bt,Gn,7] fp32, cost [Bt,Gn,2] and rating [Bt,E] fp64
struct DcopfAdjointOut {
  float *buses, *gens;
  double *cost, *rating;
};

// Every element of grid g's gradient rows set to x
__device__ __forceinline__ void dcopf_adjoint_fill(const int g, const int N, const int E, const int Gn, const double x,
                                                   const DcopfAdjointOut& out) {
  pf_adjoint_fill(g, N, E, Gn, (float)x, out.buses, nullptr, out.gens);
  if (out.cost) for (int q = threadIdx.x; q < Gn * 2; q += PF_THREADS) out.cost[(size_t)g * Gn * 2 + q] = x;
  if (out.rating) for (int l = threadIdx.x; l < E; l += PF_THREADS) out.rating[(size_t)g * E + l] = x;
}

// The LDS image behind the network solves' (dcopf_adjoint_lds_bytes)
struct DcopfAdjointImage {
  double *gp, *ap, *nu;     // [Gn] the cotangent of p; a_p; at a unit on a bound the cotangent of its multiplier, then a_nu
  double* gm;               // [E] the cotangent of mu_line at the active lines, then a_mu; 0 at the others
  int *state, *fl;          // [Gn] 0 inside the bounds, 1 at Pmax, 2 at Pmin; the free units in order
  int* al;                  // [E] the active lines in order
  double* K;                // [n][ld] the KKT matrix, the right-hand side in column n
};

__device__ __forceinline__ DcopfAdjointImage dcopf_adjoint_image(double* at, const int Gn, const int E) {
  DcopfAdjointImage a;
  a.gp = at; a.ap = at + Gn; a.nu = at + 2 * Gn;
  a.gm = at + 3 * Gn;
  a.state = reinterpret_cast<int*>(a.gm + E);
  a.fl = a.state + Gn;
  a.al = a.fl + Gn;
  a.K = a.gm + E + (2 * Gn + E + 1) / 2;
  return a;
}

// A line's row as the forward left it: +1 when its upper limit is active (mu_line above the slack rating - flow), -1 when its
// lower one is (-mu_line above rating + flow), 0 otherwise
__device__ __forceinline__ int dcopf_line_row(const double rating, const double flow, const double mu) {
  if (!(rating < __builtin_inf())) return 0;
  if (mu > fmax(rating - flow, 0.0)) return 1;
  if (0.0 - mu > fmax(rating + flow, 0.0)) return -1;
  return 0;
}

// B_f^T x at bus i: +b_l x_l over the lines from i (the ff stamps of its diagonal), -b_l x_l over the lines to it (the tt stamps)
__device__ __forceinline__ double dcopf_bft(const int i, const int32_t* y_diag, const int32_t* st_ptr, const int32_t* st, const double* lb,
                                            const double* x) {
  double r = 0.0;
  const int d = y_diag[i];
  for (int q = st_ptr[d]; q < st_ptr[d + 1]; ++q) {
    const int e = st[q] >> 2, kind = st[q] & 3;
    if (kind >= 2) continue;
    const double v = lb[e] * x[e];
    r += kind == 0 ? v : 0.0 - v;
  }
  return r;
}

// K a = b in place, b and then a in column n of K [n][ld]: LU with partial pivoting (the largest entry of the column, the lowest row
// among equals), a column per lane in the update so that a row is read across the banks.  False (for the whole wave) at a pivot
// that is zero or not finite.
__device__ __forceinline__ bool dcopf_lu_solve(double* K, const int n, const int ld, const int lane) {
  for (int j = 0; j < n; ++j) {
    double best = -1.0;
    int bi = n;
    for (int i = j + lane; i < n; i += PF_THREADS) {
      const double v = fabs(K[i * ld + j]);
      if (v > best) { best = v; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (!(best > 0.0) || !pf_finite(best)) return false;
    __syncthreads();
    if (bi != j)
      for (int c = j + lane; c <= n; c += PF_THREADS) {
        const double a = K[j * ld + c], b = K[bi * ld + c];
        K[j * ld + c] = b;
        K[bi * ld + c] = a;
      }
    __syncthreads();
    const double piv = K[j * ld + j];
    for (int i = j + 1 + lane; i < n; i += PF_THREADS) K[i * ld + j] = K[i * ld + j] / piv;
    __syncthreads();
    for (int c = j + 1 + lane; c <= n; c += PF_THREADS) {
      const double kjc = K[j * ld + c];
      for (int i = j + 1; i < n; ++i) K[i * ld + c] -= K[i * ld + j] * kjc;
    }
    __syncthreads();
  }
  for (int i = n - 1; i >= 0; --i) {
    const double xi = K[i * ld + n] / K[i * ld + i];
    __syncthreads();
    if (lane == 0) K[i * ld + n] = xi;
    for (int r = lane; r < i; r += PF_THREADS) K[r * ld + n] -= K[r * ld + i] * xi;
    __syncthreads();
  }
  return true;
}

__global__ __launch_bounds__(PF_THREADS) void gns_dcopf_adjoint_kernel(const int32_t* __restrict__ topo, const float* __restrict__ buses,
                                                                       const float* __restrict__ lines, const float* __restrict__ gens,
                                                                       const double* __restrict__ cost, const int cost_per_grid,
                                                                       const double* __restrict__ rating, const int rating_per_grid,
                                                                       const int Bt, const int ncap, const double* __restrict__ ws,
                                                                       const DcopfAdjointIn in, const DcopfAdjointOut out) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, g = blockIdx.x;
  const int N = topo[FH_N], E = topo[FH_E], Gn = topo[FH_GN], d1 = topo[FH_DIM1];
  const int32_t* p_idx = topo + topo[FH_P_IDX];
  const int32_t* y_diag = topo + topo[FH_Y_DIAG];
  const int32_t* st_ptr = topo + topo[FH_ST_PTR];
  const int32_t* st = topo + topo[FH_ST];
  const int2* ops_s = reinterpret_cast<const int2*>(topo + topo[FH_OPS_S1]);
  const DcopfWorkspace w = dcopf_workspace(const_cast<double*>(ws), Bt, Gn, E);
  const Dcn1Image m = dcn1_image(topo, lds);
  const DcopfAdjointImage a = dcopf_adjoint_image(m.Z + (size_t)d1 * 2 + 4 * (size_t)Gn, Gn, E);
  const double* __restrict__ S = w.S + (size_t)g * E * Gn;
  const float* bus = buses + (size_t)g * N * 6;
  const float* line = lines + (size_t)g * E * 7;
  const float* gen = gens + (size_t)g * Gn * 7;
  const double* cg = cost + (cost_per_grid ? (size_t)g * Gn * 2 : 0);
  const double* rt = rating ? rating + (rating_per_grid ? (size_t)g * E : 0) : nullptr;
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  const size_t oG = (size_t)g * Gn, oE = (size_t)g * E, oN = (size_t)g * N;
  const double* pg = in.pg + oG;
  const double* flow = in.flow + oE;
  const double* mul = in.mu_line + oE;

  // ---- nothing comes in: zero rows, whatever the grid holds
  {
    bool nz = false;
    for (int q = lane; q < Gn; q += PF_THREADS)
      nz |= (in.g_pg && in.g_pg[oG + q] != 0.0) || (in.g_mu_pmax && in.g_mu_pmax[oG + q] != 0.0) ||
            (in.g_mu_pmin && in.g_mu_pmin[oG + q] != 0.0);
    for (int l = lane; l < E; l += PF_THREADS) nz |= (in.g_flow && in.g_flow[oE + l] != 0.0) || (in.g_mu_line && in.g_mu_line[oE + l] != 0.0);
    for (int i = lane; i < N; i += PF_THREADS) nz |= (in.g_theta && in.g_theta[oN + i] != 0.0) || (in.g_lmp && in.g_lmp[oN + i] != 0.0);
    if (lane == 0) nz |= in.g_objective && in.g_objective[g] != 0.0;
    if (!__ballot(nz)) { dcopf_adjoint_fill(g, N, E, Gn, 0.0, out); return; }
  }

  // ---- a grid the forward did not solve to its tolerance, or whose factor fails: NaN rows
  {
    bool bad = in.iterations[g] < 0 || in.converged[g] == 0 || w.status[g] == 0.0 || !pf_finite(in.objective[g]);
    for (int q = lane; q < Gn; q += PF_THREADS)
      bad |= !pf_finite(pg[q]) || !pf_finite(in.mu_pmax[oG + q]) || !pf_finite(in.mu_pmin[oG + q]) || w.fin[oG + q] == 0.0;
    for (int l = lane; l < E; l += PF_THREADS) bad |= !pf_finite(flow[l]) || !pf_finite(mul[l]);
    for (int i = lane; i < N; i += PF_THREADS) bad |= !pf_finite(in.theta[oN + i]) || !pf_finite(in.lmp[oN + i]);
    if (__ballot(bad)) { dcopf_adjoint_fill(g, N, E, Gn, nan, out); return; }
  }
  const float* zero = dcopf_zero_gens(m.Z + (size_t)d1 * 2, Gn, lane);
  if (!dcn1_base_case(topo, bus, line, zero, m, lane)) { dcopf_adjoint_fill(g, N, E, Gn, nan, out); return; }

  // ---- the active set from the outputs: the free units and the active lines, each list in index order
  int nf = 0, k = 0;
  for (int q0 = 0; q0 < Gn; q0 += PF_THREADS) {
    const int q = q0 + lane;
    int state = -1;
    if (q < Gn) {
      const double p = pg[q], pmax = gen[q * 7 + 1], pmin = gen[q * 7 + 2];
      state = in.mu_pmax[oG + q] > fmax(pmax - p, 0.0) ? 1 : in.mu_pmin[oG + q] > fmax(p - pmin, 0.0) ? 2 : 0;
      a.state[q] = state;
    }
    const unsigned long long mask = __ballot(state == 0);
    if (state == 0) a.fl[nf + __popcll(mask & ((1ull << lane) - 1))] = q;
    nf += __popcll(mask);
  }
  for (int l0 = 0; l0 < E; l0 += PF_THREADS) {
    const int l = l0 + lane;
    const bool act = l < E && dcopf_line_row(rt ? rt[l] : inf, flow[l], mul[l]) != 0;
    const unsigned long long mask = __ballot(act);
    if (act) a.al[k + __popcll(mask & ((1ull << lane) - 1))] = l;
    k += __popcll(mask);
  }
  const int n = nf + 1 + k, ld = (n + 1) | 1;
  if (n > ncap) { dcopf_adjoint_fill(g, N, E, Gn, nan, out); return; }      // the grid's own system does not fit the image
  __syncthreads();

  // ---- the output cotangents pulled back to (p, lambda, mu_line, nu)
  const double gobj = in.g_objective ? in.g_objective[g] : 0.0;
  for (int q = lane; q < Gn; q += PF_THREADS) {
    const double p = pg[q];
    a.gp[q] = (in.g_pg ? in.g_pg[oG + q] : 0.0) + gobj * (2.0 * cg[2 * q] * p + cg[2 * q + 1]);
    const int state = a.state[q];
    a.nu[q] = state == 1 ? (in.g_mu_pmax ? in.g_mu_pmax[oG + q] : 0.0) : state == 2 ? 0.0 - (in.g_mu_pmin ? in.g_mu_pmin[oG + q] : 0.0) : 0.0;
  }
  for (int l = lane; l < E; l += PF_THREADS) a.gm[l] = 0.0;
  __syncthreads();
  if (in.g_mu_line)
    for (int j = lane; j < k; j += PF_THREADS) a.gm[a.al[j]] = in.g_mu_line[oE + a.al[j]];
  // theta and line_flow = B_f theta + Pfinj: t = A^-1 (g_theta_r + B_f,r^T g_flow), then C_g^T t to p; -t goes to the loads at the end
  if (in.g_theta || in.g_flow) {
    for (int i = lane; i < N; i += PF_THREADS) {
      if (p_idx[i] < 0) continue;
      double r = in.g_theta ? in.g_theta[oN + i] : 0.0;
      if (in.g_flow) r += dcopf_bft(i, y_diag, st_ptr, st, m.lb, in.g_flow + oE);
      m.rhs[p_idx[i]] = r;
    }
    __syncthreads();
    pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
    for (int i = lane; i < N; i += PF_THREADS) m.th[i] = p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0;
    __syncthreads();
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const int b = (int)gen[q * 7] - 1;
      if (b >= 0 && b < N) a.gp[q] += m.th[b];
    }
  } else {
    for (int i = lane; i < N; i += PF_THREADS) m.th[i] = 0.0;
  }
  __syncthreads();
  // lmp = -lambda - A^-1 B_f,r^T mu_line: y = A^-1 g_lmp_r, then -sum g_lmp to lambda and -b_l (y_f - y_t) to the active lines
  double glam = 0.0;
  if (in.g_lmp) {
    for (int i = lane; i < N; i += PF_THREADS) {
      const double x = in.g_lmp[oN + i];
      glam += x;
      if (p_idx[i] >= 0) m.rhs[p_idx[i]] = x;
    }
    glam = 0.0 - dcopf_wave_sum(glam);
    __syncthreads();
    pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
    for (int j = lane; j < k; j += PF_THREADS) {
      const int l = a.al[j];
      const int2 en = m.ends[l];
      const double yf = en.x >= 0 ? m.rhs[en.x] : 0.0, yt = en.y >= 0 ? m.rhs[en.y] : 0.0;
      a.gm[l] -= m.lb[l] * (yf - yt);
    }
    __syncthreads();
  }

  // ---- the KKT system: rows of the free units, the balance, the active lines; the units on a bound go to the right-hand side
  double* K = a.K;
  for (int x = lane; x < n * ld; x += PF_THREADS) K[x] = 0.0;
  __syncthreads();
  for (int r = lane; r < nf; r += PF_THREADS) {
    const int q = a.fl[r];
    K[r * ld + r] = 2.0 * cg[2 * q];
    K[r * ld + nf] = 1.0;
    K[nf * ld + r] = 1.0;
    for (int j = 0; j < k; ++j) {
      const double s = S[(size_t)a.al[j] * Gn + q];
      K[r * ld + nf + 1 + j] = s;
      K[(nf + 1 + j) * ld + r] = s;
    }
    K[r * ld + n] = a.gp[q];
  }
  for (int j = lane; j < k; j += PF_THREADS) {
    const double* row = S + (size_t)a.al[j] * Gn;
    double acc = a.gm[a.al[j]];
    for (int q = 0; q < Gn; ++q)
      if (a.state[q] != 0) acc -= row[q] * a.nu[q];
    K[(nf + 1 + j) * ld + n] = acc;
  }
  if (lane == PF_THREADS - 1) {
    double acc = glam;
    for (int q = 0; q < Gn; ++q)
      if (a.state[q] != 0) acc -= a.nu[q];
    K[nf * ld + n] = acc;
  }
  __syncthreads();
  bool bad = !dcopf_lu_solve(K, n, ld, lane);
  if (!bad)
    for (int r = lane; r < n; r += PF_THREADS) bad |= !pf_finite(K[r * ld + n]);
  if (__ballot(bad)) { dcopf_adjoint_fill(g, N, E, Gn, nan, out); return; }

  // ---- a_p, a_mu and, from its stationarity row, a_nu of every unit on a bound
  const double alam = K[nf * ld + n];
  for (int q = lane; q < Gn; q += PF_THREADS) a.ap[q] = a.nu[q];
  for (int l = lane; l < E; l += PF_THREADS) a.gm[l] = 0.0;
  __syncthreads();
  for (int r = lane; r < nf; r += PF_THREADS) a.ap[a.fl[r]] = K[r * ld + n];
  for (int j = lane; j < k; j += PF_THREADS) a.gm[a.al[j]] = K[(nf + 1 + j) * ld + n];
  __syncthreads();
  for (int q = lane; q < Gn; q += PF_THREADS) {
    if (a.state[q] == 0) continue;
    double acc = a.gp[q] - 2.0 * cg[2 * q] * a.nu[q] - alam;
    for (int j = 0; j < k; ++j) acc -= S[(size_t)a.al[j] * Gn + q] * a.gm[a.al[j]];
    a.nu[q] = acc;
  }
  // through f0 = Pfinj - B_f,r A^-1 load_r: v = A^-1 B_f,r^T a_mu goes to the loads
  if (k > 0) {
    for (int i = lane; i < N; i += PF_THREADS)
      if (p_idx[i] >= 0) m.rhs[p_idx[i]] = dcopf_bft(i, y_diag, st_ptr, st, m.lb, a.gm);
    __syncthreads();
    pf_run_program(topo[FH_NSTEPS_S1], topo + topo[FH_STEP_S1], ops_s, m.F, lane);
  }
  __syncthreads();

  // ---- the gradient rows, every element written
  if (out.buses)
    for (int i = lane; i < N; i += PF_THREADS) {
      const double v = k > 0 && p_idx[i] >= 0 ? m.rhs[p_idx[i]] : 0.0;
      const float d = (float)(alam + v - m.th[i]);
      float* row = out.buses + (oN + i) * 6;
      row[0] = 0.0f; row[1] = 0.0f;
      row[2] = d;                              // Pd
      row[3] = 0.0f;
      row[4] = d;                              // Gs
      row[5] = 0.0f;
    }
  if (out.gens)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      float* row = out.gens + (oG + q) * 7;
      const int state = a.state[q];
      row[0] = 0.0f;
      row[1] = state == 1 ? (float)a.nu[q] : 0.0f;       // Pmax
      row[2] = state == 2 ? (float)a.nu[q] : 0.0f;       // Pmin
      row[3] = 0.0f; row[4] = 0.0f; row[5] = 0.0f; row[6] = 0.0f;
    }
  if (out.cost)
    for (int q = lane; q < Gn; q += PF_THREADS) {
      const double p = pg[q];
      out.cost[(oG + q) * 2] = gobj * p * p - 2.0 * p * a.ap[q];
      out.cost[(oG + q) * 2 + 1] = gobj * p - a.ap[q];
    }
  if (out.rating)
    for (int l = lane; l < E; l += PF_THREADS) {
      const int row = dcopf_line_row(rt ? rt[l] : inf, flow[l], mul[l]);
      out.rating[oE + l] = row > 0 ? a.gm[l] : row < 0 ? 0.0 - a.gm[l] : 0.0;
    }
}

}  // namespace

extern "C" int gns_dcopf_adjoint_lds_bytes(const void* topo_host, int64_t* bytes, int32_t* order) {
  if (!topo_host || !bytes) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  const int n = dcopf_adjoint_order(h, GNS_PF_LDS_MAX_BYTES);
  *bytes = dcopf_adjoint_lds_bytes(h, n);
  if (order) *order = n;
  return GNS_OK;
}

extern "C" int gns_dcopf_adjoint_workspace_bytes(const gns_pf_config* cfg, const void* topo_host, int64_t Bt, size_t* bytes) {
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (dcopf_adjoint_lds_bytes(h, 0) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  *bytes = dcopf_ws_bytes(h, Bt);
  return GNS_OK;
}

// With no gradient output asked for the call returns GNS_OK without a launch, after every other check.
extern "C" int gns_dcopf_adjoint(const gns_pf_config* cfg, const void* topo_host, const void* topo_dev,
                                 const float* buses, const float* lines, const float* generators, int64_t Bt,
                                 const double* cost, int32_t cost_per_grid, const double* rating, int32_t rating_per_grid,
                                 const double* pg, const double* theta, const double* line_flow, const double* lmp,
                                 const double* mu_line, const double* mu_pmax, const double* mu_pmin, const double* objective,
                                 const uint8_t* converged, const int32_t* iterations,
                                 const double* grad_pg, const double* grad_theta, const double* grad_line_flow, const double* grad_lmp,
                                 const double* grad_mu_line, const double* grad_mu_pmax, const double* grad_mu_pmin,
                                 const double* grad_objective,
                                 float* grad_buses, float* grad_generators, double* grad_cost, double* grad_rating,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!topo_dev || !buses || !lines || !generators || Bt <= 0 || Bt > 0x7FFFFFFF || !cost || (cost_per_grid != 0 && cost_per_grid != 1) ||
      (rating_per_grid != 0 && rating_per_grid != 1) || !pg || !theta || !line_flow || !lmp || !mu_line || !mu_pmax || !mu_pmin ||
      !objective || !converged || !iterations || !workspace)
    return GNS_EINVAL;
  const int rc = dcopf_check(cfg, topo_host);
  if (rc != GNS_OK) return rc;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  int64_t nchunks = 0;
  if (!pf_chunks(h[FH_GN], dcopf_lanes(h), Bt, &nchunks)) return GNS_EINVAL;
  if (workspace_bytes < dcopf_ws_bytes(h, Bt)) return GNS_ESIZE;
  if (dcopf_adjoint_lds_bytes(h, 0) > GNS_PF_LDS_MAX_BYTES) return GNS_EUNSUPPORTED;
  if (!grad_buses && !grad_generators && !grad_cost && !grad_rating) return GNS_OK;
  const int ncap = dcopf_adjoint_order(h, GNS_PF_LDS_MAX_BYTES);
  double* ws = static_cast<double*>(workspace);
  const int rl = gns_dcopf_launch_factor(h, topo_dev, buses, lines, generators, Bt, ws, stream);
  if (rl != GNS_OK) return rl;
  const DcopfAdjointIn in = {pg, theta, line_flow, lmp, mu_line, mu_pmax, mu_pmin, objective, converged, iterations,
                             grad_pg, grad_theta, grad_line_flow, grad_lmp, grad_mu_line, grad_mu_pmax, grad_mu_pmin, grad_objective};
  const DcopfAdjointOut out = {grad_buses, grad_generators, grad_cost, grad_rating};
  return pf_launch<gns_dcopf_adjoint_kernel>(Bt, dcopf_adjoint_lds_bytes(h, ncap), stream, static_cast<const int32_t*>(topo_dev), buses, lines,
                                             generators, cost, (int)cost_per_grid, rating, (int)rating_per_grid, (int)Bt, ncap,
                                             (const double*)ws, in, out);
}
