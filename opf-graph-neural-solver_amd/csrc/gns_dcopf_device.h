// What the DC optimal power flow (gns_dcopf.hip) and its adjoint (gns_dcopf_adjoint.hip) share: the workspace of a call as the
// factor kernel fills it, the generator block of zeros behind the screens' image, the factor kernel's chunk width and LDS image, the
// wave's sum, the host check of a call's blob, and the launch of the factor kernel, which lives in gns_dcopf.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"
#include "gns_pf_device.h"
#include "gns_dcn1_device.h"

// The factor kernel of gns_dcopf.hip on Bt grids of the blob (h on the host, topo_dev on the device) into the workspace ws, laid out
// by dcopf_workspace: S, f0, the units' finite flags and the grids' status.  The caller has checked the blob, Bt and the chunk count.
int gns_dcopf_launch_factor(const int32_t* h, const void* topo_dev, const float* buses, const float* lines, const float* generators,
                            int64_t Bt, double* ws, void* stream);

namespace {

// The workspace of one call, all doubles: S [Bt][E][Gn], f0 [Bt][E], the units' finite flags [Bt][Gn], the base case's status [Bt]
// (1: solved), then what the iteration leaves for the finish: lambda [Bt] and whether the grid has a dispatch [Bt]
struct DcopfWorkspace {
  double* S;
  double* f0;
  double* fin;
  double* status;
  double* lam;
  double* solved;
};

__host__ __device__ inline DcopfWorkspace dcopf_workspace(double* ws, const int64_t Bt, const int64_t Gn, const int64_t E) {
  DcopfWorkspace w;
  w.S = ws;
  w.f0 = w.S + Bt * E * Gn;
  w.fin = w.f0 + Bt * E;
  w.status = w.fin + Bt * Gn;
  w.lam = w.status + Bt;
  w.solved = w.lam + Bt;
  return w;
}

inline size_t dcopf_ws_bytes(const int32_t* h, int64_t Bt) {
  const int64_t E = h[FH_E], Gn = h[FH_GN];
  return ((size_t)Bt * (size_t)(E * Gn + E + Gn + 3) * sizeof(double) + 255) & ~(size_t)255;
}

// The factor and the finish kernel keep a generator block of zeros behind the screens' image (four doubles per unit hold its seven
// floats): the base case is the one without generation, whatever Pg the rows list
inline int64_t dcopf_zero_gens_bytes(const int32_t* h) { return 32 * (int64_t)h[FH_GN]; }

// Units a workgroup of the factor kernel takes side by side: dcn1_lanes on what the zeros leave
inline int dcopf_lanes(const int32_t* h) { return dcn1_lanes(h, GNS_PF_LDS_MAX_BYTES - dcopf_zero_gens_bytes(h)); }

inline int64_t dcopf_factor_lds(const int32_t* h, int lanes) { return dcn1_lds_bytes(h, lanes) + dcopf_zero_gens_bytes(h); }

__device__ __forceinline__ double dcopf_wave_sum(double x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// The zeros a base case without generation reads as its generator rows
__device__ __forceinline__ const float* dcopf_zero_gens(double* at, const int Gn, const int lane) {
  float* z = reinterpret_cast<float*>(at);
  for (int q = lane; q < Gn * 7; q += PF_THREADS) z[q] = 0.0f;
  __syncthreads();
  return z;
}

// The host checks of a call on the blob at topo_host: GNS_EINVAL unless it is an FD blob of cfg's shape with a unit
inline int dcopf_check(const gns_pf_config* cfg, const void* topo_host) {
  if (!pf_config_ok(cfg) || !topo_host) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (!pf_header_ok<DcBlobKind>(cfg, h) || h[FH_GN] <= 0) return GNS_EINVAL;
  return GNS_OK;
}

}  // namespace
