// The device helpers of the DC power flow that its kernels (gns_dcpf.hip) and the DC contingency screen (gns_dcn1.hip) share: a line's
// b_l, Bbus from the line rows into the B' factor slots and the injection of a bus.  A line's ends, a generator slot's bus and the
// fill of a grid's gradient rows are gns_pf_device.h's, the same for every kind of kernel.
#pragma once
#include "gns_pf_device.h"

namespace {

// b_l = 1 / (x tau) of line e (makeBdc; tau as given)
__device__ __forceinline__ double dc_line_b(const float* line, const int e) {
  return 1.0 / ((double)line[e * 7 + 3] * (double)line[e * 7 + 5]);
}

// Entry p of Bbus: +b_l for the ff and tt stamps of the entry, -b_l for its ft and tf stamps; parallel lines add
__device__ __forceinline__ double dc_b_entry(const int p, const int32_t* st_ptr, const int32_t* st, const float* line) {
  double bb = 0.0;
  for (int q = st_ptr[p]; q < st_ptr[p + 1]; ++q) {
    const double b = dc_line_b(line, st[q] >> 2);
    bb += (st[q] & 3) < 2 ? b : 0.0 - b;
  }
  return bb;
}

// Bbus[r, r] into the B' factor slots (FH_BSLOT, the first of each pair); the fill slots are zero already
__device__ __forceinline__ void dc_matrix(const int N, const int32_t* y_ptr, const int32_t* st_ptr, const int32_t* st,
                                          const int32_t* bslot, const float* line, double* F, const int lane) {
  for (int i = lane; i < N; i += PF_THREADS)
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int s = bslot[2 * p];
      if (s >= 0) F[s] = dc_b_entry(p, st_ptr, st, line);
    }
}

// P_i = sum Pg - Pd_i - Gs_i - Pbusinj_i, with Pfinj_l = -b_l shift_l added to Pbusinj at the line's from bus (the ff stamp of the
// diagonal) and subtracted at its to bus (the tt stamp)
__device__ __forceinline__ double dc_injection(const int i, const int32_t* y_diag, const int32_t* st_ptr, const int32_t* st,
                                               const int32_t* gen_ptr, const int32_t* gen_idx, const float* bus, const float* line,
                                               const float* gen) {
  double p = 0.0;
  for (int q = gen_ptr[i]; q < gen_ptr[i + 1]; ++q) p += (double)gen[gen_idx[q] * 7 + 6];
  p = p - (double)bus[i * 6 + 2] - (double)bus[i * 6 + 4];
  const int d = y_diag[i];
  for (int q = st_ptr[d]; q < st_ptr[d + 1]; ++q) {
    const int e = st[q] >> 2, kind = st[q] & 3;
    if (kind >= 2) continue;                                // (a line from a bus to itself also stamps ft and tf here)
    const double pfinj = 0.0 - dc_line_b(line, e) * (double)line[e * 7 + 6];
    p -= kind == 0 ? pfinj : 0.0 - pfinj;
  }
  return p;
}

}  // namespace
