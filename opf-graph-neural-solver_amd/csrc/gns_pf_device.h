// Device helpers the power-flow kernels share (gns_powerflow.hip: Newton-Raphson and its adjoint; gns_fdpf.hip: fast-decoupled):
// one wave per grid, the Y-bus of a grid from its line stamps, and the interpreter of the blobs' op programs.
#pragma once
#include <hip/hip_runtime.h>

#include "gns_pf_common.h"

namespace {

constexpr int PF_THREADS = 64;   // one wave

__device__ inline bool pf_finite(double x) { return __builtin_isfinite(x); }

__device__ inline double pf_wave_max(double x) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// Y-bus values of row i (makeYbus) into Y[y_ptr[i] .. y_ptr[i+1]): the line stamps of every entry, Gs + jBs on the diagonal
__device__ __forceinline__ void pf_ybus_row(const int i, const int32_t* y_ptr, const int32_t* y_diag, const int32_t* st_ptr,
                                            const int32_t* st, const float* bus, const float* line, double2* Y) {
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
}

// One op program of the blob (PH_STEP_PTR / PH_OPS, or the transposed PH_T_*): F[dst] -= F[a] F[b] or F[dst] /= F[a],
// independent within a step, a barrier after each step
__device__ __forceinline__ void pf_run_program(const int nsteps, const int32_t* step_ptr, const int2* ops, double* F, const int lane) {
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
}

// Device workspace of Bt grids: their Y-bus values, 16 bytes per entry, rounded up to 256 bytes
inline size_t pf_ws_bytes_nnzy(int64_t nnzy, int64_t Bt) { return (((size_t)Bt * nnzy * sizeof(double2)) + 255) & ~(size_t)255; }

}  // namespace
