// C-ABI entry points (include/gns_hip.h).  Host code only: validates, lays out the workspace and enqueues
// kernels on the caller's stream.  No allocation, no synchronisation, no host<->device copies.
// In order: options, device state, profiling, call resolver and path decision, layouts and fillers, launch helpers, entry points, Adam.
#include <atomic>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "gns_kernels.h"
#include "gns_gridwg.h"

namespace {
// ---- process-wide tuning knobs: read from the environment ONCE (first call), never per launch ----------------------
struct GnsTuning {
  int fwd_mapping;   // GNS_FWD_MAPPING: 0 auto, 1 "lane" (lane = grid, state streamed through HBM), 2 "lds" (grid per workgroup, state on chip)
  int gw_pack;       // GNS_GW_PACK: grids per workgroup of the lds mapping (0 = auto)
  int fwd_waves;     // GNS_FWD_WAVES: waves per workgroup of the lane mapping
  int fwd_plane;     // GNS_FWD_PLANE: LDS planes of the lane-mapping forward: 0 none (neighbour (v, theta) from HBM), 1 the (v, theta) plane, 2 (default) also (delta_p, delta_q) between the physics and lambda phases
  int dw_mfma;       // GNS_DW_MFMA=0: packed-FMA weight-gradient engine instead of the matrix pipe
  int train_mapping; // GNS_TRAIN_MAPPING: mapping of the training-mode forward + backward pair: 0 auto, 1 lane, 2 lds
  int bwd_variant;   // GNS_BWD_VARIANT: lane-per-grid backward: 1 wide half-wave records, 2 layer-wise + sub-record windows, 3 = 2 + background chains (one persistent kernel each); 4 split: one kernel sequence per reverse step (gns_backward_split.hip)
  int team;          // GNS_TEAM: workgroups per 64-grid group of the lane mapping when the batch leaves CUs idle: 0 auto, 1 none, 2, 4
  int bwds_mode;     // GNS_BWDS_MODE: sweep kernels per reverse step of the split backward: 0 one per family, 1 {L_m} {L_theta + L_v}, 2 all three families per bus in one kernel
  int bwds_chunks;   // GNS_BWDS_CHUNKS: bus chunks per 64-grid group of the split backward's sweeps (0 = auto: 8, 16 or 32)
  int bwds_save;     // GNS_BWDS_SAVE: 1 (default) a training forward whose backward is the split backward in mode 1 at latent 20, hidden 10 saves L's first-layer activations in place of the hidden sums (saves_first_layer); 0 always the hidden sums
};

// One row per option: its name (gns_set_option / gns_get_option), where it lives, the values it takes (lo..hi, or `check`, which may
// normalise the value) and the environment variable that seeds it, read through `parse`.  A value out of range is refused by
// gns_set_option (GNS_EINVAL) and ignored when it comes from the environment.
bool waves_ok(int& w) { return w > 0 && (w & (w - 1)) == 0 && w * 64 <= GNS_FWD_MAX_THREADS; }
bool chunks_ok(int& c) { return c == 0 || gns_part_index(c) >= 0; }
bool as_flag(int& v) { v = v ? 1 : 0; return true; }                                  // any integer, stored as 0 / 1
int env_int(const char* e) { return std::atoi(e); }
int env_mapping(const char* e) { return !std::strcmp(e, "lane") ? 1 : (!std::strcmp(e, "lds") ? 2 : 0); }   // by word; anything else: auto
int env_plane(const char* e) { return e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2); }     // by first character
int env_flag(const char* e) { return e[0] == '0' ? 0 : 1; }
struct GnsOption {
  const char* name; int GnsTuning::*member; int lo, hi; bool (*check)(int&); const char* env; int (*parse)(const char*);
  bool accepts(int& v) const { return check ? check(v) : (v >= lo && v <= hi); }
};
const GnsOption g_options[] = {
  {"fwd_mapping",   &GnsTuning::fwd_mapping,   0, 2,            nullptr,   "GNS_FWD_MAPPING",   env_mapping},
  {"train_mapping", &GnsTuning::train_mapping, 0, 2,            nullptr,   "GNS_TRAIN_MAPPING", env_mapping},
  {"bwd_variant",   &GnsTuning::bwd_variant,   1, 4,            nullptr,   "GNS_BWD_VARIANT",   env_int},
  {"gw_pack",       &GnsTuning::gw_pack,       0, 16,           nullptr,   "GNS_GW_PACK",       env_int},
  {"fwd_waves",     &GnsTuning::fwd_waves,     0, 0,            waves_ok,  "GNS_FWD_WAVES",     env_int},
  {"fwd_plane",     &GnsTuning::fwd_plane,     0, 2,            nullptr,   "GNS_FWD_PLANE",     env_plane},
  {"dw_mfma",       &GnsTuning::dw_mfma,       0, 0,            as_flag,   "GNS_DW_MFMA",       env_flag},
  {"team",          &GnsTuning::team,          0, GNS_MAX_TEAM, nullptr,   "GNS_TEAM",          env_int},
  {"bwds_mode",     &GnsTuning::bwds_mode,     0, 2,            nullptr,   "GNS_BWDS_MODE",     env_int},
  {"bwds_chunks",   &GnsTuning::bwds_chunks,   0, 0,            chunks_ok, "GNS_BWDS_CHUNKS",   env_int},
  {"bwds_save",     &GnsTuning::bwds_save,     0, 1,            nullptr,   "GNS_BWDS_SAVE",     env_int},
};
GnsTuning make_tuning() {
  GnsTuning t{0, 0, GNS_FWD_THREADS / 64, 2, 1, 0, 4, 0, 1, 0, 1};
  for (const GnsOption& o : g_options)
    if (const char* e = std::getenv(o.env)) { int v = o.parse(e); if (o.accepts(v)) t.*o.member = v; }
  return t;
}
GnsTuning& tuning() {
  static GnsTuning t = make_tuning();            // C++11: thread-safe one-time initialisation
  return t;
}

// ---- the path the last launches took (read-only "last.*" options): the fall-backs below (waves halved for a team, planes that do not
// fit, teams cancelled, widths without a persistent backward) are otherwise invisible to a caller.  Plain host stores at launch time,
// no device work.  -1: not launched yet, or not a property of the path that ran (e.g. last.fwd_plane after a grid-per-workgroup forward).
struct GnsLast {
  int fwd_kernel, fwd_waves, fwd_plane, team, gw_pack;                   // gns_forward / gns_forward_grouped
  int bwd_kernel, dw_mfma, bwds_mode, bwds_chunks, bwds_R, bwd_gw_pack;   // gns_backward / gns_backward_inputs / gns_backward_grouped
  int bwds_save;                                                          // ... 1: it read saved first-layer activations, 0: hidden sums
};
GnsLast g_last{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
struct GnsLastName { const char* name; int GnsLast::*member; };
const GnsLastName g_last_names[] = {                                          // read as "last.<name>"
  {"fwd_kernel", &GnsLast::fwd_kernel}, {"fwd_waves", &GnsLast::fwd_waves}, {"fwd_plane", &GnsLast::fwd_plane}, {"team", &GnsLast::team},
  {"gw_pack", &GnsLast::gw_pack}, {"bwd_kernel", &GnsLast::bwd_kernel}, {"dw_mfma", &GnsLast::dw_mfma}, {"bwds_mode", &GnsLast::bwds_mode},
  {"bwds_chunks", &GnsLast::bwds_chunks}, {"bwds_R", &GnsLast::bwds_R}, {"bwd_gw_pack", &GnsLast::bwd_gw_pack},
  {"bwds_save", &GnsLast::bwds_save},
};
void record_forward(int kernel, int waves, int plane, int team, int pack) {
  g_last.fwd_kernel = kernel; g_last.fwd_waves = waves; g_last.fwd_plane = plane; g_last.team = team; g_last.gw_pack = pack;
}
void record_backward(int kernel, int dw_mfma, int mode, int chunks, int R, int pack, int save = 0) {
  g_last.bwd_kernel = kernel; g_last.dw_mfma = dw_mfma; g_last.bwds_mode = mode; g_last.bwds_chunks = chunks; g_last.bwds_R = R;
  g_last.bwd_gw_pack = pack; g_last.bwds_save = save;
}

// ---- per-device state: kernel attributes (dynamic LDS beyond 64 KB is an opt-in per kernel AND device) and the CU count, set up
// once per device at the first call that finds it current (one process per GPU is the normal deployment; a process that moves a
// model to a second device gets that device initialised the same way).  Never runs inside a stream capture in practice: a capture
// is preceded by eager warm-up calls on the same device.
constexpr int GNS_MAX_DEVICES = 64;
struct GnsDevice {
  int ncu;           // compute units (teams must be resident all at once)
  int gw_ready;      // gns_gw_init_device() and gns_gw_backward_init_device() succeeded
  int split_ready;   // gns_bwds_init_device() succeeded
  int fwd_ready;     // gns_fwd_init_device() succeeded (the lane-per-grid forward may use more than 64 KB of dynamic LDS)
};
const GnsDevice& device() {
  static GnsDevice devs[GNS_MAX_DEVICES];
  static std::atomic<int> done[GNS_MAX_DEVICES];
  static std::mutex mu;
  static const GnsDevice none{0, 0, 0, 0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return none; }     // no ROCm device: the entry points report it
  if (dev < 0 || dev >= GNS_MAX_DEVICES) return none;
  if (!done[dev].load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(mu);
    if (!done[dev].load(std::memory_order_relaxed)) {
      GnsDevice d{0, 0, 0, 0};
      int n = 0;
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) d.ncu = n;
      else (void)hipGetLastError();
      d.gw_ready = (gns_gw_init_device() == GNS_OK && gns_gw_backward_init_device() == GNS_OK) ? 1 : 0;
      d.split_ready = gns_bwds_init_device() == GNS_OK ? 1 : 0;
      d.fwd_ready = gns_fwd_init_device() == GNS_OK ? 1 : 0;
      devs[dev] = d;
      done[dev].store(1, std::memory_order_release);
    }
  }
  return devs[dev];
}

// ---- optional kernel timing (diagnostics) ---------------------------------------------------------------
struct ProfRing { std::vector<hipEvent_t> a, b; int used = 0; };
ProfRing g_prof[2];
int g_prof_cap = 0;
void prof_mark(int which, bool start, hipStream_t st) {
  if (g_prof_cap <= 0) return;
  ProfRing& r = g_prof[which];
  if (r.used >= g_prof_cap) return;
  (void)hipEventRecord(start ? r.a[r.used] : r.b[r.used], st);
  if (!start) ++r.used;
}

// ---- what a call runs on: the compiled kernel pair, and which kernels take it ---------------------------------------------
// The compiled (latent_dim, hidden_dim) pair a model runs on: the smallest one that holds it.  A narrower model runs zero-padded
// (gns_common.h, GnsFamilies): same function, same gradients; only gns_pack_params / gns_unfold know the difference.
bool kernel_dims(int d, int h, int* dk, int* hk) {
  bool found = false;
#define GNS_CASE(DD, HH) if (d <= DD && h <= HH && (!found || DD * HH < *dk * *hk)) { *dk = DD; *hk = HH; found = true; }
  GNS_FOR_EACH_DIMS(GNS_CASE)
#undef GNS_CASE
  return found;
}
// cfg with the kernel's dims in place of the model's (everything but the flat parameter layout is sized by these)
bool kernel_config(const gns_config* model, gns_config* k) {
  *k = *model;
  return kernel_dims(model->latent_dim, model->hidden_dim, &k->latent_dim, &k->hidden_dim);
}

int check_cfg(const gns_config* c) {
  if (!c) return GNS_EINVAL;
  if (c->n_bus <= 0 || c->n_line <= 0 || c->n_gen < 0 || c->K <= 0 || c->latent_dim <= 0 || c->hidden_dim <= 0) return GNS_EINVAL;
  if (c->multiple_phi != 0 && c->multiple_phi != 1) return GNS_EINVAL;
  return GNS_OK;
}

// A validated call: the model's config as the caller gave it (it only lays out the flat parameters and their gradient) and the
// kernel's, which sizes everything else.
struct GnsCall {
  const gns_config* model;
  gns_config k;
  GnsFamilies families() const {         // the parameter families of the model, padded to the kernel's dims
    GnsFamilies f; gns_families_padded(model->latent_dim, model->hidden_dim, k.latent_dim, k.hidden_dim, k.K, k.multiple_phi, &f);
    return f;
  }
};
// The checks every entry point opens with, in the order their codes take precedence: the config (GNS_EINVAL), the entry point's own
// arguments (`args_ok`: GNS_EINVAL), a compiled pair that holds the model and - only where `cap_K` - K <= GNS_MAX_K (GNS_EUNSUPPORTED).
// The launches (gns_forward, gns_backward, gns_backward_inputs, the grouped calls) cap K: their argument structs hold GNS_MAX_K loss
// weights.  The queries (gns_workspace_bytes, gns_uses_packed_inputs, gns_team_status*) never did and still do not.
enum KCap { ANY_K, CAP_K };
int resolve(const gns_config* cfg, bool args_ok, KCap cap_K, GnsCall* c) {
  const int rc = check_cfg(cfg);
  if (rc != GNS_OK) return rc;
  if (!args_ok) return GNS_EINVAL;
  c->model = cfg;
  if (!kernel_config(cfg, &c->k) || (cap_K == CAP_K && cfg->K > GNS_MAX_K)) return GNS_EUNSUPPORTED;
  return GNS_OK;
}

// Workgroups per 64-grid group of the lane-per-grid kernels (gns_device.h, "teams").  Asked by gns_workspace_bytes,
// gns_forward and gns_backward alike.
int lane_team(int64_t Bt) {
  const GnsTuning& T = tuning();
  const int64_t groups = (Bt + GNS_LANES - 1) / GNS_LANES;
  if (groups > GNS_TEAM_MAX_GROUPS) return 1;
  const int ncu = device().ncu < GNS_BWD_MAX_WG ? device().ncu : GNS_BWD_MAX_WG;
  return gns_team_size(groups, ncu, T.team);
}

bool split_available(const gns_config* c) { return device().split_ready && gns_bwds_supported(c->latent_dim, c->hidden_dim, c->multiple_phi); }
// The checks of a grouped call over G 64-grid groups (the model's cfg in, the kernel's out): it always runs the split backward's kernels
int grouped_call(const gns_config* model, int64_t G, GnsCall* c) {
  const int rc = resolve(model, G > 0 && G <= ((int64_t)1 << 24), CAP_K, c);
  if (rc != GNS_OK) return rc;
  return split_available(&c->k) ? GNS_OK : GNS_EUNSUPPORTED;
}
// The split backward (bwd_variant 4) runs the three-phi models on the matrix-pipe engine; everything else keeps the persistent kernel.
bool use_split_backward(const gns_config* c) {
  const GnsTuning& T = tuning();
  if (!split_available(c)) return false;
  if (!gns_backward_persistent_supported(c->latent_dim, c->hidden_dim)) return true;      // the only lane-per-grid backward of this pair
  return T.bwd_variant == 4 && T.dw_mfma;
}

// "This call saves first-layer activations": the training forward stores a1 of every L net where it otherwise stores the hidden sum
// the net read, and the split backward's sweeps start from it (gns_backward_split.hip, BwdsMeasured).  Evaluated identically by
// lane_forward and split_backward - changing an option between a forward and its backward is a caller error (see route()).  True only
// for the shape the saved-activation sweeps are compiled and measured in: a plain training call (save_state 1, one topology, no input
// gradients) of a three-phi model on the (20, 10) kernels, reversed by the split backward in mode 1.
bool saves_first_layer(const gns_config* k, int save_state, bool grouped) {
  const GnsTuning& T = tuning();
  return T.bwds_save == 1 && save_state == 1 && !grouped && k->multiple_phi == 1 && k->latent_dim == 20 && k->hidden_dim == 10 &&
         T.bwds_mode == 1 && use_split_backward(k);
}

// Input gradients (gns_backward_inputs): the input-adjoint buffer behind the split backward's workspace, and the caller's outputs
#define GNS_SAVE_IGRAD 2
#define GNS_IGRAD_MARK 0x49475244u      // written behind a forward workspace saved with save_state = 2
#define GNS_IGRAD_MARK_BYTES 256
size_t igrad_bytes(const gns_config* kcfg, int64_t Bt) {
  return gns_align256((size_t)((Bt + GNS_LANES - 1) / GNS_LANES) * gns_in_rows(kcfg->n_bus, kcfg->n_line) * GNS_LANES * 16);
}
struct IgradOut {
  float* buf; size_t bytes;
  const float *in_buses, *in_lines, *in_gens;
  float *buses, *lines, *gens;
};

// Which mapping runs a training-mode forward and its backward.  Evaluated identically by gns_forward and gns_backward:
// changing "train_mapping" / "gw_pack" between a forward and its backward is a caller error.
int gw_train_pack(const gns_config* c, int64_t Bt) {
  const GnsTuning& T = tuning();
  const int P = T.gw_pack > 0 ? T.gw_pack : 1;
  if (!device().gw_ready || T.train_mapping == 1) return 0;
  if (!gns_gw_supported(c->n_bus, c->n_line, c->latent_dim, c->hidden_dim, c->multiple_phi, P)) return 0;
  if (!gns_gw_backward_supported(c->n_bus, c->n_line, c->latent_dim, c->hidden_dim, c->multiple_phi, P)) return 0;
  if (T.train_mapping == 2) return P;
  // auto: below ~2000 grids per GPU (case118; ~1000 for case300) the grid-per-workgroup pair, one workgroup per grid, is the
  // faster one (measured, case118 x 1024: 0.55 vs 1.20 ms); above, the lane-per-grid pair - teams of workgroups per 64-grid
  // group keep the chip busy down to a quarter of its CUs in groups (case118 x 4096: 1.38 vs 1.96 ms, x 8192: 2.31 vs 3.86).
  const int64_t groups = (Bt + GNS_LANES - 1) / GNS_LANES;
  const int wpg = gns_gw_backward_wpg(c->n_bus);
  return groups <= 32 / (wpg > 2 ? wpg / 2 : 1) ? P : 0;
}
// Grids per workgroup of the evaluation-mode forward when it runs on the grid-per-workgroup kernel, 0 when the lane-per-grid
// kernel runs it.  gns_workspace_bytes, gns_forward and gns_uses_packed_inputs must agree, so they all ask here.
int gw_eval_pack(const gns_config* c, int64_t Bt) {
  const GnsTuning& T = tuning();
  const int N = c->n_bus, E = c->n_line;
  const int wpg = ((N > E ? N : E) + 63) / 64;
  int P = T.gw_pack;
  if (P <= 0) {                                   // auto: one workgroup per CU with as many grids as fit (all waves of a CU in the
    P = 1;                                        // same phase stream the same weights: 73 % scalar-cache hits against 55 %)
    for (int q = 2; q * wpg <= 12; ++q) if (gns_gw_supported(N, E, c->latent_dim, c->hidden_dim, c->multiple_phi, q)) P = q;
  }
  const bool can = device().gw_ready && gns_gw_supported(N, E, c->latent_dim, c->hidden_dim, c->multiple_phi, P);
  bool want = T.fwd_mapping == 2 || (T.fwd_mapping == 0 && N >= 48);
  if (T.fwd_mapping == 0 && want) {
    // auto, by batch: once the lane-per-grid kernel fills the chip with one workgroup per 64-grid group it is the faster one (since it
    // skips the v family on generator buses: case118 x 16384, 256 groups: 0.73 against 0.91 ms); a case too large to pack several
    // grids into a workgroup hands over earlier (case300 x 8192, 128 groups on teams of two: 2.75 against 5.03 ms); small batches
    // stay on chip (case30 x 4096, 64 groups: 0.12 against 0.18 ms).  Measured on MI355X, tools/gpu_time_eval.py.
    const int64_t groups = (Bt + GNS_LANES - 1) / GNS_LANES;
    const int ncu = device().ncu > 0 ? device().ncu : 256;
    if (groups >= ncu || (P == 1 && wpg >= 5 && groups * 4 >= ncu)) want = false;
  }
  return (can && want) ? P : 0;
}

// Which kernels run a call.  The ONE place that decides it: gns_workspace_bytes, gns_uses_packed_inputs, both team-status calls,
// gns_forward and gns_backward (which decides as for save_state = 1) must agree, so they all ask here and nothing else.
enum GnsPath {
  PATH_GW_TRAIN,      // grid-per-workgroup training pair (forward saved for gns_gw_launch_backward)
  PATH_GW_EVAL,       // grid-per-workgroup evaluation: state on chip, inputs read in place
  PATH_LANE,          // lane-per-grid forward (and the split or persistent backward)
  PATH_LANE_IGRAD,    // lane-per-grid forward saved for gns_backward_inputs (save_state 2)
};
struct GnsRoute {
  GnsPath path; int pack;                // pack: grids per workgroup of the grid-per-workgroup kernels, 0 on the lane paths
  bool lane() const { return path == PATH_LANE || path == PATH_LANE_IGRAD; }
};
GnsRoute route(const gns_config* k, int64_t Bt, int save_state) {
  if (save_state == GNS_SAVE_IGRAD) return {PATH_LANE_IGRAD, 0};
  const int P = save_state ? gw_train_pack(k, Bt) : gw_eval_pack(k, Bt);
  if (P > 0) return {save_state ? PATH_GW_TRAIN : PATH_GW_EVAL, P};
  return {PATH_LANE, 0};
}

// ---- workspace layouts and the argument structs' tables --------------------------------------------------------------------
GnsFwdLayout fwd_layout(const gns_config* k, int64_t Bt, int save_state) {
  GnsFwdLayout L;
  gns_fwd_layout(k->n_bus, k->n_line, k->latent_dim, k->hidden_dim, k->K, k->multiple_phi, Bt, save_state, &L);
  return L;
}
GnsBwdsLayout bwds_layout(const gns_config* k, int64_t Bt) {
  GnsBwdsLayout S;
  gns_bwds_layout(k->n_bus, k->n_line, k->latent_dim, k->hidden_dim, k->K, k->multiple_phi, Bt, device().ncu, tuning().bwds_chunks, &S);
  return S;
}
GnsBwdLayout bwd_layout(const gns_config* k, int64_t Bt, int team) {
  GnsBwdLayout B;
  gns_bwd_layout(k->n_bus, k->n_line, k->latent_dim, k->hidden_dim, k->K, k->multiple_phi, Bt, team, &B);
  return B;
}
struct GwTrainLayout { size_t off_pt, off_pn, off_save; GwSaveLayout sv; size_t fwd_total; int blocks, waves; size_t off_slab, off_part, off_tmp, bwd_total; long long slab_floats, nslab; };
GwTrainLayout gw_train_layout(const gns_config* c, int64_t Bt, int P) {
  GwTrainLayout L;
  GnsFamilies f; gns_families(c->latent_dim, c->hidden_dim, c->K, c->multiple_phi, &f);
  size_t o = 0;
  L.off_pt = o; o = gns_align256(o + (size_t)f.t_total * 4);
  L.off_pn = o; o = gns_align256(o + (size_t)f.n_total * 4);
  L.off_save = o;
  L.sv = gw_save_layout(c->n_bus, c->latent_dim, c->hidden_dim, c->K, c->multiple_phi, Bt);
  L.fwd_total = o + L.sv.total;
  const int WPG = gns_gw_backward_wpg(c->n_bus);
  L.blocks = gns_gw_backward_blocks(c->n_bus, c->n_line, c->latent_dim, c->hidden_dim, c->multiple_phi, P, Bt);
  L.waves = P * WPG;
  L.slab_floats = (f.g_total + 63) / 64 * 64;
  L.nslab = (long long)L.blocks * L.waves;
  o = 0;
  L.off_slab = o; o = gns_align256(o + (size_t)L.nslab * L.slab_floats * 4);
  L.off_part = o; o = gns_align256(o + (size_t)GNS_RED_PARTS * L.slab_floats * 4);
  L.off_tmp = o;  o = gns_align256(o + (size_t)L.slab_floats * 4);
  L.bwd_total = o;
  return L;
}

// The family tables of an argument struct: where each family's weights sit in the transposed stream (the forwards), and in the
// natural stream and the gradient slab as well (the backwards)
template <class Args> void fill_forward_families(Args& A, const GnsFamilies& fam) {
  for (int i = 0; i < fam.nfam; ++i) { A.t_off[i] = fam.t_off[i]; A.t_sz[i] = fam.t_sz[i]; }
}
template <class Args> void fill_backward_families(Args& A, const GnsFamilies& fam) {
  fill_forward_families(A, fam);
  for (int i = 0; i < fam.nfam; ++i) { A.n_off[i] = fam.n_off[i]; A.n_sz[i] = fam.n_sz[i]; A.g_off[i] = fam.g_off[i]; A.g_sz[i] = fam.g_sz[i]; }
}
// The loss weight gamma^(K-k) of step k, rounded to fp32 from a double like the reference's python float (main.py:198)
float loss_weight(const gns_config* cfg, int k) {
  const int K = cfg->K;
  return (float)std::pow((double)cfg->gamma, (double)(K - k));
}
template <class Args> void fill_loss_weights(Args& A, const gns_config* cfg) {
  for (int k = 0; k < cfg->K; ++k) A.gw[k] = loss_weight(cfg, k);
}

// Byte offset of the team status word in the forward workspace of a lane-per-grid call over Bt grid slots, (size_t)-1 when it runs
// without teams; *ws_total: the size of that workspace.
size_t team_word_offset(const gns_config* k, int64_t Bt, int save_state, size_t* ws_total = nullptr) {
  if (lane_team(Bt) <= 1) return (size_t)-1;
  const GnsFwdLayout L = fwd_layout(k, Bt, save_state);
  if (ws_total) *ws_total = L.total;
  return L.off_team + GNS_TEAM_STATUS_WORD * 4;
}
// ... and the read of it: waits for `stream` and copies one word
int read_team_word(const void* fwd_workspace, size_t off, void* stream, int* status) {
  unsigned word = 0;
  if (hipMemcpyAsync(&word, (const char*)fwd_workspace + off, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { (void)hipGetLastError(); return GNS_ELAUNCH; }
  *status = word ? 1 : 0;
  return GNS_OK;
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------------
// The grid-per-workgroup forward, P grids per workgroup, on parameters already packed into `pt`.  sv / GL: the save area of a training
// forward and its layout, NULL for an evaluation.
int gw_forward(const gns_config* cfg, const GnsFamilies& fam, const void* topo_dev, const float* pt, const float* buses, const float* lines,
               const float* generators, int64_t Bt, float* v, float* theta, float* total_loss, float* last_loss, int P, char* sv,
               const GwSaveLayout* GL, hipStream_t st) {
  const int N = cfg->n_bus, E = cfg->n_line;
  GnsGwFwdArgs G;
  std::memset(&G, 0, sizeof(G));
  G.topo = (const int*)topo_dev; G.pt = pt; G.buses = buses; G.lines = lines; G.gens = generators;
  G.v_out = v; G.theta_out = theta; G.total_out = total_loss; G.last_out = last_loss;
  if (sv) { G.sv_state = (float*)(sv + GL->off_state); G.sv_S = (float*)(sv + GL->off_S); G.sv_lam = (float*)(sv + GL->off_lam); }
  fill_forward_families(G, fam);
  fill_loss_weights(G, cfg);
  G.Bt = Bt; G.N = N; G.E = E; G.Gn = cfg->n_gen; G.K = cfg->K; G.save = sv ? 1 : 0; G.P = P; G.WPG = ((N > E ? N : E) + 63) / 64;
  record_forward(2, -1, -1, -1, P);
  prof_mark(0, true, st);
  const int rc = gns_gw_launch_forward(cfg->latent_dim, cfg->hidden_dim, cfg->multiple_phi, G, st);
  prof_mark(0, false, st);
  return rc;
}

// The lane-per-grid forward of Bt input grids in L.groups 64-grid groups (parameters and inputs already packed into `ws`).  group_topo /
// slot_grid: NULL for a one-topology batch (lane l of group g computes grid 64 g + l), else the tables of a grouped call.
int lane_forward(const gns_config* cfg, const GnsFamilies& fam, const GnsFwdLayout& L, char* ws, float* pt, float* pin,
                 const int* topo_dev, const int* group_topo, const int* slot_grid, int64_t Bt, float* v, float* theta,
                 float* total_loss, float* last_loss, int save_state, hipStream_t st) {
  const int N = cfg->n_bus, E = cfg->n_line, K = cfg->K, d = cfg->latent_dim, h = cfg->hidden_dim;
  const GnsTuning& T = tuning();
  int rc;
  GnsFwdArgs A;
  std::memset(&A, 0, sizeof(A));
  A.topo = topo_dev; A.group_topo = group_topo; A.slot_grid = slot_grid; A.pt = pt; A.in = pin;
  A.state = (float*)(ws + L.off_state); A.lam = (float*)(ws + L.off_lam); A.msg = (float*)(ws + L.off_msg);
  A.v_out = v; A.theta_out = theta; A.total_out = total_loss; A.last_out = last_loss;
  fill_forward_families(A, fam);
  fill_loss_weights(A, cfg);
  A.Bt = Bt; A.G = L.groups; A.N = N; A.E = E; A.K = K; A.save = save_state ? 1 : 0;
  A.save_a1 = saves_first_layer(cfg, save_state, group_topo != nullptr) ? 1 : 0;
  const int team0 = lane_team(L.groups * GNS_LANES);     // (= lane_team(Bt) for a one-topology batch)
  A.team = team0;
  A.team_ws = (unsigned char*)(ws + L.off_team);
  int waves = T.fwd_waves;
  while (waves * A.team > GNS_MAXP) waves /= 2;
  A.part_idx = gns_part_index(waves * A.team);
  auto pick_planes = [&]() {
    A.plane = (device().fwd_ready && gns_fwd_plane_fits(N, A.team) && T.fwd_plane) ? 1 : 0;
    if (A.plane && gns_fwd_plane2_fits(N, A.team) && T.fwd_plane == 2) A.plane = 2;
  };
  pick_planes();
  if (A.team > 1) {
    // every workgroup of every team must be resident at once: the kernel's own occupancy at this launch configuration says
    // how many a CU holds (not just the CU count); a configuration that does not fit runs one workgroup per group instead
    const int per_cu = gns_fwd_blocks_per_cu(d, h, cfg->multiple_phi, A, waves * 64);
    if ((long long)per_cu * device().ncu < A.G * A.team) {
      A.team = 1;
      waves = T.fwd_waves;
      A.part_idx = gns_part_index(waves);
      pick_planes();
    }
  }
  // (the counters - and the status word gns_team_status reads - are zeroed whenever this batch size is one that may use teams)
  if (team0 > 1 && hipMemsetAsync(A.team_ws, 0, (size_t)L.groups * GNS_TEAM_CTR_BYTES, st) != hipSuccess) return GNS_ELAUNCH;
  record_forward(1, waves, A.plane, A.team, -1);
  prof_mark(0, true, st);
  rc = gns_launch_forward(d, h, cfg->multiple_phi, A, waves * 64, st);
  prof_mark(0, false, st);
  return rc;
}

// The split backward (bwd_variant 4) of a lane-per-grid forward: one phys + sweep kernel sequence per reverse step, then the reduction.
int split_backward(const gns_config* cfg, const GnsFamilies& fam, const GnsFwdLayout& L, const GnsBwdsLayout& S, const char* fw,
                   char* bw, const int* topo_dev, const int* group_topo, const int* slot_grid, const float* params,
                   const void* packed_inputs, int64_t Bt, const float* grad_total, const float* grad_last, const float* grad_v,
                   const float* grad_theta, float* grad_params, hipStream_t st, const IgradOut* ig = nullptr) {
  const int N = cfg->n_bus, E = cfg->n_line, K = cfg->K, d = cfg->latent_dim, h = cfg->hidden_dim;
  int rc;
  GnsBwdsArgs A;
  std::memset(&A, 0, sizeof(A));
  A.topo = topo_dev; A.group_topo = group_topo; A.slot_grid = slot_grid;
  A.pt = (const float*)(fw + L.off_pt); A.pn = (const float*)(fw + L.off_pn);
  A.in = packed_inputs ? (const float*)packed_inputs : (const float*)(fw + L.off_in);
  A.state = (const float*)(fw + L.off_state); A.lam = (const float*)(fw + L.off_lam); A.msg = (const float*)(fw + L.off_msg);
  A.g_total = grad_total; A.g_last = grad_last; A.g_v = grad_v; A.g_theta = grad_theta;
  A.adj = (float*)(bw + S.off_adj); A.slots = (float*)(bw + S.off_slots); A.slab = (float*)(bw + S.off_slab);
  fill_backward_families(A, fam);
  A.Bt = Bt; A.G = S.groups; A.slab_floats = S.slab_floats; A.N = N; A.E = E; A.K = K;
  A.C = S.C; A.part_idx = gns_part_index(S.C); A.R = S.R;
  A.RB = (int)(1 + S.mq); A.RBA = (int)S.adj_rows;
  A.mode = cfg->multiple_phi ? tuning().bwds_mode : 2;          // the single phi is reversed after all three L nets: bus-major
  const size_t lds = gns_bwds_phys_lds(N, &A.use_plane);
  if (ig) {
    A.igrad = ig->buf;
    if (hipMemsetAsync(A.igrad, 0, ig->bytes, st) != hipSuccess) return GNS_ELAUNCH;
  }
  A.save_a1 = saves_first_layer(cfg, ig ? GNS_SAVE_IGRAD : 1, group_topo != nullptr) ? 1 : 0;
  record_backward(4, 1, A.mode, A.C, A.R, -1, A.save_a1);
  prof_mark(1, true, st);
  for (int k = K - 1; k >= 0; --k) {
    A.k = k;
    A.gwk = loss_weight(cfg, k);
    rc = gns_launch_bwds_phys(A, lds, st);
    if (rc != GNS_OK) return rc;
    if (ig) {
      rc = gns_launch_bwds_igrad_phys(A, st);
      if (rc != GNS_OK) return rc;
    }
    rc = gns_launch_bwds_sweep(d, h, cfg->multiple_phi, A, st);
    if (rc != GNS_OK) return rc;
  }
  if (ig && (ig->buses || ig->lines || ig->gens)) {
    rc = gns_launch_bwds_igrad_unpack(A, ig->in_buses, ig->in_lines, ig->in_gens, cfg->n_gen, ig->buses, ig->lines, ig->gens, st);
    if (rc != GNS_OK) return rc;
  }
  prof_mark(1, false, st);
  if (!grad_params) return GNS_OK;
  return gns_launch_reduce(A.slab, (float*)(bw + S.off_part), (float*)(bw + S.off_tmp), params, grad_params, S.nslab, S.slab_floats,
                           fam, K, d, h, st);
}
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------
// Explicit configuration (include/gns_hip.h).  The environment variables of the same meaning only seed the defaults.
extern "C" int gns_set_option(const char* name, int value) {
  if (!name) return GNS_EINVAL;
  for (const GnsOption& o : g_options)
    if (!std::strcmp(name, o.name)) {
      if (!o.accepts(value)) return GNS_EINVAL;
      tuning().*o.member = value;
      return GNS_OK;
    }
  return GNS_EINVAL;                     // (unknown, or one of the read-only "last.*" names)
}
extern "C" int gns_get_option(const char* name, int* value) {
  if (!name || !value) return GNS_EINVAL;
  for (const GnsOption& o : g_options)
    if (!std::strcmp(name, o.name)) { *value = tuning().*o.member; return GNS_OK; }
  if (!std::strncmp(name, "last.", 5))
    for (const GnsLastName& l : g_last_names)
      if (!std::strcmp(name + 5, l.name)) { *value = g_last.*l.member; return GNS_OK; }
  return GNS_EINVAL;
}

extern "C" int gns_profile_enable(int capacity) {
  for (auto& r : g_prof) {
    for (auto e : r.a) (void)hipEventDestroy(e);
    for (auto e : r.b) (void)hipEventDestroy(e);
    r.a.clear(); r.b.clear(); r.used = 0;
  }
  g_prof_cap = 0;
  if (capacity < 0) return GNS_EINVAL;
  for (auto& r : g_prof)
    for (int i = 0; i < capacity; ++i) {
      hipEvent_t x, y;
      if (hipEventCreate(&x) != hipSuccess || hipEventCreate(&y) != hipSuccess) return GNS_ELAUNCH;
      r.a.push_back(x); r.b.push_back(y);
    }
  g_prof_cap = capacity;
  return GNS_OK;
}

extern "C" int gns_profile_read(int backward, float* ms_sum, int* launches) {
  if (!ms_sum || !launches) return GNS_EINVAL;
  ProfRing& r = g_prof[backward ? 1 : 0];
  float tot = 0.f;
  for (int i = 0; i < r.used; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b[i]) != hipSuccess || hipEventElapsedTime(&ms, r.a[i], r.b[i]) != hipSuccess) return GNS_ELAUNCH;
    tot += ms;
  }
  *ms_sum = tot; *launches = r.used; r.used = 0;
  return GNS_OK;
}

extern "C" const char* gns_version(void) { return "gns_hip 0.1 gfx950"; }

extern "C" int gns_param_count(const gns_config* cfg, int64_t* count) {
  if (!cfg || !count || cfg->K <= 0 || cfg->latent_dim <= 0 || cfg->hidden_dim <= 0) return GNS_EINVAL;
  GnsFamilies f; gns_families(cfg->latent_dim, cfg->hidden_dim, cfg->K, cfg->multiple_phi, &f);
  *count = f.flat_total;
  return GNS_OK;
}

extern "C" int gns_config_supported(const gns_config* cfg) {
  GnsCall c;
  return resolve(cfg, true, CAP_K, &c) == GNS_OK ? 1 : 0;
}

extern "C" int gns_workspace_bytes(const gns_config* cfg, int64_t Bt, int save_state, size_t* fwd_bytes, size_t* bwd_bytes) {
  GnsCall c;
  const int rc = resolve(cfg, Bt > 0, ANY_K, &c);
  if (rc != GNS_OK) return rc;
  const gns_config* k = &c.k;
  const GnsRoute R = route(k, Bt, save_state);
  const GnsFwdLayout L = fwd_layout(k, Bt, save_state);
  switch (R.path) {
  case PATH_LANE_IGRAD:                                                // lane-per-grid forward + split backward with input gradients
    if (!split_available(k)) return GNS_EUNSUPPORTED;
    if (fwd_bytes) *fwd_bytes = L.total + GNS_IGRAD_MARK_BYTES;
    if (bwd_bytes) *bwd_bytes = bwds_layout(k, Bt).total + igrad_bytes(k, Bt);
    return GNS_OK;
  case PATH_GW_TRAIN: {
    const GwTrainLayout G = gw_train_layout(k, Bt, R.pack);
    if (fwd_bytes) *fwd_bytes = G.fwd_total;
    if (bwd_bytes) *bwd_bytes = G.bwd_total;
    return GNS_OK;
  }
  case PATH_GW_EVAL:                                                   // state on chip, inputs read in place: only the parameter streams
    if (fwd_bytes) *fwd_bytes = L.off_in;
    if (bwd_bytes) *bwd_bytes = 0;
    return GNS_OK;
  case PATH_LANE:
    break;
  }
  if (fwd_bytes) *fwd_bytes = L.total;
  if (bwd_bytes) {
    *bwd_bytes = bwd_layout(k, Bt, lane_team(Bt)).total;
    if (split_available(k)) {                                          // either variant may be asked for later
      const size_t split = bwds_layout(k, Bt).total;
      if (split > *bwd_bytes) *bwd_bytes = split;
    }
  }
  return GNS_OK;
}

extern "C" int gns_uses_packed_inputs(const gns_config* cfg, int64_t Bt, int save_state) {
  GnsCall c;
  if (resolve(cfg, Bt > 0, ANY_K, &c) != GNS_OK) return 0;
  return route(&c.k, Bt, save_state).lane() ? 1 : 0;
}

// Did a team of workgroups give up at a barrier during the gns_forward that used this workspace?  (Teams: lane-per-grid kernels on a
// batch with fewer 64-grid groups than CUs; a barrier gives up after ~seconds when a partner workgroup never became resident -
// another kernel or process holding its CU.  The losses of that call are NaN; this is how the host learns it without looking at
// them.)  The ONE entry point that synchronises: it waits for `stream` and copies one word.  *status = 0 without touching the
// device when this (cfg, Bt) does not use teams.
// Byte offset of that status word inside the forward workspace, or (size_t)-1 in *offset when this (cfg, Bt, save_state) runs
// without teams.  (Tests inject a failure through it; the host wrapper asks it whether a status has to be checked at all.)
extern "C" int gns_team_status_offset(const gns_config* cfg, int64_t Bt, int save_state, size_t* offset) {
  GnsCall c;
  const int rc = resolve(cfg, offset && Bt > 0, ANY_K, &c);
  if (rc != GNS_OK) return rc;
  *offset = route(&c.k, Bt, save_state).lane() ? team_word_offset(&c.k, Bt, save_state) : (size_t)-1;   // the grid-per-workgroup kernels have no teams
  return GNS_OK;
}

extern "C" int gns_team_status(const gns_config* cfg, int64_t Bt, const void* fwd_workspace, size_t fwd_workspace_bytes, int save_state,
                               int* status, void* stream) {
  GnsCall c;
  const int rc = resolve(cfg, status && fwd_workspace && Bt > 0, ANY_K, &c);
  if (rc != GNS_OK) return rc;
  *status = 0;
  size_t total = 0;
  const size_t off = route(&c.k, Bt, save_state).lane() ? team_word_offset(&c.k, Bt, save_state, &total) : (size_t)-1;
  if (off == (size_t)-1) return GNS_OK;
  if (fwd_workspace_bytes < total) return GNS_ESIZE;
  return read_team_word(fwd_workspace, off, stream, status);
}

extern "C" int gns_prepack_bytes(const gns_config* cfg, int64_t Bt, size_t* bytes) {
  int rc = check_cfg(cfg);
  if (rc != GNS_OK) return rc;
  if (!bytes || Bt <= 0) return GNS_EINVAL;
  const int64_t groups = (Bt + GNS_LANES - 1) / GNS_LANES;
  *bytes = (size_t)groups * gns_in_rows(cfg->n_bus, cfg->n_line) * GNS_LANES * 16;
  return GNS_OK;
}

extern "C" int gns_prepack(const gns_config* cfg, const void* topo_dev, const float* buses, const float* lines,
                           const float* generators, int64_t Bt, void* packed, size_t packed_bytes, void* stream) {
  size_t need = 0;
  int rc = gns_prepack_bytes(cfg, Bt, &need);
  if (rc != GNS_OK) return rc;
  if (!topo_dev || !buses || !lines || !generators || !packed) return GNS_EINVAL;
  if (packed_bytes < need) return GNS_ESIZE;
  return gns_launch_pack_inputs((const int*)topo_dev, buses, lines, generators, (float*)packed, cfg->n_bus, cfg->n_line, cfg->n_gen, Bt,
                                (Bt + GNS_LANES - 1) / GNS_LANES, (hipStream_t)stream);
}

extern "C" int gns_forward(const gns_config* cfg, const void* topo_dev, const float* params, const float* buses,
                           const float* lines, const float* generators, int64_t Bt, const void* packed_inputs, float* v, float* theta,
                           float* total_loss, float* last_loss, void* workspace, size_t workspace_bytes, int save_state,
                           void* stream) {
  GnsCall c;
  int rc = resolve(cfg, topo_dev && params && buses && lines && generators && v && theta && total_loss && last_loss && workspace && Bt > 0,
                   CAP_K, &c);
  if (rc != GNS_OK) return rc;
  cfg = &c.k;                            // the kernel's dims from here on; the model's only lay out the flat parameters
  const int N = cfg->n_bus, E = cfg->n_line, Gn = cfg->n_gen, K = cfg->K, d = cfg->latent_dim, h = cfg->hidden_dim;
  const GnsFamilies fam = c.families();
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const GnsRoute R = route(cfg, Bt, save_state);
  if (R.path == PATH_GW_TRAIN) {                   // training-mode forward of the grid-per-workgroup pair
    const GwTrainLayout GL = gw_train_layout(cfg, Bt, R.pack);
    if (workspace_bytes < GL.fwd_total) return GNS_ESIZE;
    float* gpt = (float*)(ws + GL.off_pt);
    float* gpn = (float*)(ws + GL.off_pn);
    rc = gns_launch_pack_params(params, gpt, gpn, fam, K, d, h, st);
    if (rc != GNS_OK) return rc;
    return gw_forward(cfg, fam, topo_dev, gpt, buses, lines, generators, Bt, v, theta, total_loss, last_loss, R.pack, ws + GL.off_save,
                      &GL.sv, st);
  }
  const GnsFwdLayout L = fwd_layout(cfg, Bt, save_state);
  if (workspace_bytes < (R.path == PATH_GW_EVAL ? L.off_in : L.total)) return GNS_ESIZE;
  if (R.path == PATH_LANE_IGRAD) {                 // saved for gns_backward_inputs: the mark it checks, behind the layout
    if (workspace_bytes < L.total + GNS_IGRAD_MARK_BYTES) return GNS_ESIZE;
    if (!split_available(cfg)) return GNS_EUNSUPPORTED;
    if (hipMemsetD32Async((hipDeviceptr_t)(ws + L.total), GNS_IGRAD_MARK, 1, st) != hipSuccess) return GNS_ELAUNCH;
  }
  float* pt = (float*)(ws + L.off_pt);
  float* pn = (float*)(ws + L.off_pn);
  float* pin = (float*)(ws + L.off_in);
  rc = gns_launch_pack_params(params, pt, pn, fam, K, d, h, st);
  if (rc != GNS_OK) return rc;
  // Evaluation (nothing saved for a backward): the grid-per-workgroup mapping keeps the whole state on chip.
  if (R.path == PATH_GW_EVAL)
    return gw_forward(cfg, fam, topo_dev, pt, buses, lines, generators, Bt, v, theta, total_loss, last_loss, R.pack, nullptr, nullptr, st);
  if (packed_inputs) pin = (float*)packed_inputs;                  // a resident batch packed once by gns_prepack: nothing to redo
  else {
    rc = gns_launch_pack_inputs((const int*)topo_dev, buses, lines, generators, pin, N, E, Gn, Bt, L.groups, st);
    if (rc != GNS_OK) return rc;
  }
  return lane_forward(cfg, fam, L, ws, pt, pin, (const int*)topo_dev, nullptr, nullptr, Bt, v, theta, total_loss, last_loss, save_state, st);
}

extern "C" int gns_backward(const gns_config* cfg, const void* topo_dev, const float* params,
                            const float* buses, const float* lines, const float* generators, int64_t Bt, const void* packed_inputs,
                            const void* fwd_workspace, size_t fwd_workspace_bytes, const float* grad_total,
                            const float* grad_last, const float* grad_v, const float* grad_theta, float* grad_params,
                            void* bwd_workspace, size_t bwd_workspace_bytes, void* stream) {
  GnsCall c;
  int rc = resolve(cfg, topo_dev && params && fwd_workspace && grad_params && bwd_workspace && Bt > 0, CAP_K, &c);
  if (rc != GNS_OK) return rc;
  cfg = &c.k;                            // the kernel's dims from here on; the model's only lay out the flat parameters and their gradient
  const int N = cfg->n_bus, E = cfg->n_line, K = cfg->K, d = cfg->latent_dim, h = cfg->hidden_dim;
  hipStream_t st = (hipStream_t)stream;
  const char* fw = (const char*)fwd_workspace;
  char* bw = (char*)bwd_workspace;
  const GnsRoute R = route(cfg, Bt, 1);            // (no save_state argument: decided as for the forward that saved for this call)
  if (R.path == PATH_GW_TRAIN) {                   // the pair of the grid-per-workgroup training forward
    const int TP = R.pack;
    if (!buses || !lines || !generators) return GNS_EINVAL;
    const GwTrainLayout GL = gw_train_layout(cfg, Bt, TP);
    if (fwd_workspace_bytes < GL.fwd_total || bwd_workspace_bytes < GL.bwd_total) return GNS_ESIZE;
    const GnsFamilies fam = c.families();
    if (hipMemsetAsync(bw + GL.off_slab, 0, (size_t)GL.nslab * GL.slab_floats * 4, st) != hipSuccess) return GNS_ELAUNCH;
    GnsGwBwdArgs G;
    std::memset(&G, 0, sizeof(G));
    G.topo = (const int*)topo_dev;
    G.pt = (const float*)(fw + GL.off_pt); G.pn = (const float*)(fw + GL.off_pn);
    G.buses = buses; G.lines = lines; G.gens = generators;
    const char* sv = fw + GL.off_save;
    G.sv_state = (const float*)(sv + GL.sv.off_state); G.sv_S = (const float*)(sv + GL.sv.off_S); G.sv_lam = (const float*)(sv + GL.sv.off_lam);
    G.g_total = grad_total; G.g_last = grad_last; G.g_v = grad_v; G.g_theta = grad_theta;
    G.slab = (float*)(bw + GL.off_slab);
    fill_backward_families(G, fam);
    fill_loss_weights(G, cfg);
    G.Bt = Bt; G.slab_floats = GL.slab_floats; G.N = N; G.E = E; G.Gn = cfg->n_gen; G.K = K;
    G.P = TP; G.WPG = gns_gw_backward_wpg(N);
    record_backward(0, -1, -1, -1, -1, TP);
    prof_mark(1, true, st);
    rc = gns_gw_launch_backward(d, h, cfg->multiple_phi, G, GL.blocks, st);
    prof_mark(1, false, st);
    if (rc != GNS_OK) return rc;
    return gns_launch_reduce(G.slab, (float*)(bw + GL.off_part), (float*)(bw + GL.off_tmp), params, grad_params, GL.nslab,
                             GL.slab_floats, fam, K, d, h, st);
  }
  const GnsFwdLayout L = fwd_layout(cfg, Bt, 1);
  if (use_split_backward(cfg)) {
    const GnsBwdsLayout S = bwds_layout(cfg, Bt);
    if (fwd_workspace_bytes < L.total || bwd_workspace_bytes < S.total) return GNS_ESIZE;
    return split_backward(cfg, c.families(), L, S, fw, bw, (const int*)topo_dev, nullptr, nullptr, params, packed_inputs, Bt, grad_total,
                          grad_last, grad_v, grad_theta, grad_params, st);
  }
  const int team = lane_team(Bt);
  const GnsBwdLayout B = bwd_layout(cfg, Bt, team);
  if (fwd_workspace_bytes < L.total || bwd_workspace_bytes < B.total) return GNS_ESIZE;
  const GnsFamilies fam = c.families();
  const int blocks = (int)(B.groups * team < GNS_BWD_MAX_WG ? B.groups * team : GNS_BWD_MAX_WG);
  const long long nslab = (long long)blocks * GNS_BWD_WAVES;
  // the V2 sweep writes every slab entry itself on a workgroup's first group: no 90 MB memset in front of it
  const bool v2 = tuning().dw_mfma && tuning().bwd_variant >= 2 && cfg->multiple_phi;
  if (!v2 && hipMemsetAsync(bw + B.off_slab, 0, (size_t)nslab * B.slab_floats * 4, st) != hipSuccess) return GNS_ELAUNCH;
  GnsBwdArgs A;
  std::memset(&A, 0, sizeof(A));
  A.topo = (const int*)topo_dev;
  A.pt = (const float*)(fw + L.off_pt); A.pn = (const float*)(fw + L.off_pn);
  A.in = packed_inputs ? (const float*)packed_inputs : (const float*)(fw + L.off_in);
  A.state = (const float*)(fw + L.off_state); A.lam = (const float*)(fw + L.off_lam); A.msg = (const float*)(fw + L.off_msg);
  A.g_total = grad_total; A.g_last = grad_last; A.g_v = grad_v; A.g_theta = grad_theta;
  A.adj = (float*)(bw + B.off_adj); A.slots = (float*)(bw + B.off_slots); A.slab = (float*)(bw + B.off_slab);
  fill_backward_families(A, fam);
  fill_loss_weights(A, cfg);
  A.Bt = Bt; A.G = B.groups; A.slab_floats = B.slab_floats; A.N = N; A.E = E; A.K = K;
  A.part_idx = gns_part_index(GNS_BWD_WAVES * team);
  A.team = team; A.team_ws = (unsigned char*)(bw + B.off_team);
  if (team > 1 && hipMemsetAsync(A.team_ws, 0, (size_t)B.groups * GNS_TEAM_CTR_BYTES, st) != hipSuccess) return GNS_ELAUNCH;
  A.slab_dirty = v2 ? 1 : 0;
  // (the variant gns_launch_backward dispatches to: 2 and 3 need the matrix pipe and three phi nets, everything else runs 1)
  record_backward(tuning().dw_mfma && cfg->multiple_phi && (tuning().bwd_variant == 2 || tuning().bwd_variant == 3) ? tuning().bwd_variant : 1,
                  tuning().dw_mfma, -1, -1, -1, -1);
  prof_mark(1, true, st);
  // The weight-gradient contraction over the grids runs on the matrix pipe (exact fp32) unless GNS_DW_MFMA=0 asks for
  // the packed-FMA register tiles; both are parity-tested (gns_backward.hip, "weight-gradient engines").
  rc = gns_launch_backward(d, h, cfg->multiple_phi, tuning().dw_mfma, tuning().bwd_variant, A, blocks, st);
  prof_mark(1, false, st);
  if (rc != GNS_OK) return rc;
  // the kernel has summed each workgroup's eight slabs into its first one: one slab per workgroup is left to reduce
  return gns_launch_reduce(A.slab, (float*)(bw + B.off_part), (float*)(bw + B.off_tmp), params, grad_params, blocks, B.slab_floats,
                           fam, K, d, h, st, (long long)GNS_BWD_WAVES * B.slab_floats);
}

extern "C" int gns_backward_inputs(const gns_config* cfg, const void* topo_dev, const float* params,
                                   const float* buses, const float* lines, const float* generators, int64_t Bt, const void* packed_inputs,
                                   const void* fwd_workspace, size_t fwd_workspace_bytes, const float* grad_total,
                                   const float* grad_last, const float* grad_v, const float* grad_theta, float* grad_params,
                                   float* grad_buses, float* grad_lines, float* grad_generators,
                                   void* bwd_workspace, size_t bwd_workspace_bytes, void* stream) {
  GnsCall c;
  const int rc = resolve(cfg, topo_dev && params && buses && lines && generators && fwd_workspace && bwd_workspace && Bt > 0, CAP_K, &c);
  if (rc != GNS_OK) return rc;
  cfg = &c.k;
  if (!split_available(cfg)) return GNS_EUNSUPPORTED;
  const GnsFwdLayout L = fwd_layout(cfg, Bt, 1);
  const GnsBwdsLayout S = bwds_layout(cfg, Bt);
  if (fwd_workspace_bytes < L.total + GNS_IGRAD_MARK_BYTES) return GNS_EINVAL;       // not a save_state = 2 workspace
  const size_t ib = igrad_bytes(cfg, Bt);
  if (bwd_workspace_bytes < S.total + ib) return GNS_ESIZE;
  hipStream_t st = (hipStream_t)stream;
  unsigned mark = 0;                   // (the one synchronisation of this call: a workspace saved without input gradients is refused)
  if (hipMemcpyAsync(&mark, (const char*)fwd_workspace + L.total, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return GNS_ELAUNCH; }
  if (mark != GNS_IGRAD_MARK) return GNS_EINVAL;
  IgradOut ig;
  ig.buf = (float*)((char*)bwd_workspace + S.total); ig.bytes = ib;
  ig.in_buses = buses; ig.in_lines = lines; ig.in_gens = generators;
  ig.buses = grad_buses; ig.lines = grad_lines; ig.gens = grad_generators;
  return split_backward(cfg, c.families(), L, S, (const char*)fwd_workspace, (char*)bwd_workspace, (const int*)topo_dev, nullptr, nullptr, params,
                        packed_inputs, Bt, grad_total, grad_last, grad_v, grad_theta, grad_params, st, &ig);
}

// ---- grouped calls: a batch that mixes topologies, one topology per 64-grid group (include/gns_hip.h) ---------------------------
// Always the lane-per-grid forward and the split backward, whatever "fwd_mapping", "train_mapping" and "gw_pack" say; their workspace
// layouts for Bt = 64 G (grouped_call resolves them).

extern "C" int gns_workspace_bytes_grouped(const gns_config* cfg, int64_t G, int save_state, size_t* fwd_bytes, size_t* bwd_bytes) {
  GnsCall c;
  const int rc = grouped_call(cfg, G, &c);
  if (rc != GNS_OK) return rc;
  if (fwd_bytes) *fwd_bytes = fwd_layout(&c.k, G * GNS_LANES, save_state).total;
  if (bwd_bytes) *bwd_bytes = save_state ? bwds_layout(&c.k, G * GNS_LANES).total : 0;
  return GNS_OK;
}

extern "C" int gns_forward_grouped(const gns_config* cfg, const void* topo_set_dev, const int32_t* group_topo_dev,
                                   const int32_t* slot_grid_dev, int64_t G, const float* params, const float* buses, const float* lines,
                                   const float* generators, int64_t Bt, float* v, float* theta, float* total_loss, float* last_loss,
                                   void* workspace, size_t workspace_bytes, int save_state, void* stream) {
  GnsCall c;
  int rc = grouped_call(cfg, G, &c);
  if (rc != GNS_OK) return rc;
  if (!topo_set_dev || !group_topo_dev || !slot_grid_dev || !params || !buses || !lines || !generators || !v || !theta || !total_loss ||
      !last_loss || !workspace || Bt <= 0 || Bt > G * GNS_LANES)
    return GNS_EINVAL;
  const gns_config& k = c.k;
  const int N = k.n_bus, E = k.n_line, K = k.K, d = k.latent_dim, h = k.hidden_dim;
  const GnsFamilies fam = c.families();
  const GnsFwdLayout L = fwd_layout(&k, G * GNS_LANES, save_state);
  if (workspace_bytes < L.total) return GNS_ESIZE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* pt = (float*)(ws + L.off_pt);
  float* pn = (float*)(ws + L.off_pn);
  float* pin = (float*)(ws + L.off_in);
  rc = gns_launch_pack_params(params, pt, pn, fam, K, d, h, st);
  if (rc != GNS_OK) return rc;
  rc = gns_launch_pack_inputs((const int*)topo_set_dev, buses, lines, generators, pin, N, E, k.n_gen, Bt, L.groups, st, group_topo_dev,
                              slot_grid_dev);
  if (rc != GNS_OK) return rc;
  return lane_forward(&k, fam, L, ws, pt, pin, (const int*)topo_set_dev, group_topo_dev, slot_grid_dev, Bt, v, theta, total_loss,
                      last_loss, save_state, st);
}

extern "C" int gns_backward_grouped(const gns_config* cfg, const void* topo_set_dev, const int32_t* group_topo_dev,
                                    const int32_t* slot_grid_dev, int64_t G, const float* params, const float* buses, const float* lines,
                                    const float* generators, int64_t Bt, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                    const float* grad_total, const float* grad_last, const float* grad_v, const float* grad_theta,
                                    float* grad_params, void* bwd_workspace, size_t bwd_workspace_bytes, void* stream) {
  (void)buses; (void)lines; (void)generators;                    // (the lane-per-grid kernels read the inputs packed by the forward)
  GnsCall c;
  const int rc = grouped_call(cfg, G, &c);
  if (rc != GNS_OK) return rc;
  if (!topo_set_dev || !group_topo_dev || !slot_grid_dev || !params || !fwd_workspace || !grad_params || !bwd_workspace || Bt <= 0 ||
      Bt > G * GNS_LANES)
    return GNS_EINVAL;
  const GnsFwdLayout L = fwd_layout(&c.k, G * GNS_LANES, 1);
  const GnsBwdsLayout S = bwds_layout(&c.k, G * GNS_LANES);
  if (fwd_workspace_bytes < L.total || bwd_workspace_bytes < S.total) return GNS_ESIZE;
  return split_backward(&c.k, c.families(), L, S, (const char*)fwd_workspace, (char*)bwd_workspace, (const int*)topo_set_dev, group_topo_dev,
                        slot_grid_dev, params, nullptr, Bt, grad_total, grad_last, grad_v, grad_theta, grad_params, (hipStream_t)stream);
}

// The team status of a grouped forward.  (gns_team_status answers for the call gns_forward would make for that batch size, which below
// ~2000 grids is the grid-per-workgroup pair, without teams; a grouped call runs the lane-per-grid forward at every size.)
extern "C" int gns_team_status_offset_grouped(const gns_config* cfg, int64_t G, int save_state, size_t* offset) {
  GnsCall c;
  const int rc = grouped_call(cfg, G, &c);
  if (rc != GNS_OK) return rc;
  if (!offset) return GNS_EINVAL;
  *offset = team_word_offset(&c.k, G * GNS_LANES, save_state);
  return GNS_OK;
}

extern "C" int gns_team_status_grouped(const gns_config* cfg, int64_t G, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                       int save_state, int* status, void* stream) {
  size_t off = 0;
  const int rc = gns_team_status_offset_grouped(cfg, G, save_state, &off);
  if (rc != GNS_OK) return rc;
  if (!status || !fwd_workspace) return GNS_EINVAL;
  *status = 0;
  if (off == (size_t)-1) return GNS_OK;
  if (fwd_workspace_bytes < off + 4) return GNS_ESIZE;
  return read_team_word(fwd_workspace, off, stream, status);
}

// ---- Adam on the flat parameter buffer (GNS/main.py:290 with the optimiser of main.py:241-243) ---------------------------
__global__ void gns_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                long long n, float one_minus_b1, float b2, float one_minus_b2, float step_size, float inv_sqrt_bc2, float eps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = m[i] + (gi - m[i]) * one_minus_b1;
  const float vi = b2 * v[i] + one_minus_b2 * gi * gi;
  m[i] = mi; v[i] = vi;
  p[i] -= step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

extern "C" int gns_adam_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             double lr, double beta1, double beta2, double eps, int64_t step, void* stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return GNS_EINVAL;
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  hipLaunchKernelGGL(gns_adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grad, exp_avg,
                     exp_avg_sq, (long long)n, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1),
                     (float)(1.0 / std::sqrt(bc2)), (float)eps);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
}

// The same update with the step counter ON THE DEVICE, so that a whole training step (forward, backward, this) can be captured
// into a HIP graph once and replayed: a captured launch bakes its scalar arguments in, and Adam's bias corrections change every
// step.  state[0] = steps taken so far (a float: exact up to 2^24), state[1..2] = scratch (the step size and 1 / sqrt(1 - beta2^t)
// of the current step).  Two launches: one thread advances the counter and forms the corrections in double like the host
// version, then the element-wise kernel reads them.
__global__ void gns_adam_advance_kernel(float* __restrict__ st, double lr, double b1, double b2) {
  const double step = (double)st[0] + 1.0;
  st[0] = (float)step;
  st[1] = (float)(lr / (1.0 - pow(b1, step)));
  st[2] = (float)(1.0 / sqrt(1.0 - pow(b2, step)));
}
__global__ void gns_adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    long long n, float one_minus_b1, float b2, float one_minus_b2, const float* __restrict__ st, float eps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float step_size = st[1], inv_sqrt_bc2 = st[2];
  const float gi = g[i];
  const float mi = m[i] + (gi - m[i]) * one_minus_b1;
  const float vi = b2 * v[i] + one_minus_b2 * gi * gi;
  m[i] = mi; v[i] = vi;
  p[i] -= step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

extern "C" int gns_adam_step_dev(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 double lr, double beta1, double beta2, double eps, float* step_state, void* stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || !step_state || n <= 0) return GNS_EINVAL;
  hipLaunchKernelGGL(gns_adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_state, lr, beta1, beta2);
  hipLaunchKernelGGL(gns_adam_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grad, exp_avg,
                     exp_avg_sq, (long long)n, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), step_state, (float)eps);
  return hipGetLastError() == hipSuccess ? GNS_OK : GNS_ELAUNCH;
}
