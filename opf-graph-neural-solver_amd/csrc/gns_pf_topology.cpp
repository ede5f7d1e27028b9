// Host analysis of one topology for the Newton-Raphson power-flow kernel (include/gns_powerflow.h): bus roles, Y-bus pattern,
// a minimum-degree ordering, the symbolic LU and the elimination / triangular-solve program, into one relocatable int32 blob
// (layout: gns_pf_common.h).
#include "../../include/gns_powerflow.h"
#include "gns_pf_common.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <vector>

namespace {

struct PfBlob {
  std::vector<int32_t> w;
  PfBlob() : w(PF_HDR_WORDS, 0) {}
  void put(int slot, const std::vector<int32_t>& a) { w[slot] = (int32_t)w.size(); w.insert(w.end(), a.begin(), a.end()); }
};

// Minimum degree on the bus graph without the slack (ties: lowest bus id); the elimination graph is kept as explicit sets.
std::vector<int> min_degree_order(int N, int slack, const std::vector<std::set<int>>& adj0) {
  std::vector<std::set<int>> adj(adj0);
  for (int i = 0; i < N; ++i) adj[i].erase(slack);
  std::vector<char> done(N, 0);
  done[slack] = 1;
  std::vector<int> order;
  for (int it = 0; it < N - 1; ++it) {
    int best = -1;
    size_t bd = 0;
    for (int i = 0; i < N; ++i)
      if (!done[i] && (best < 0 || adj[i].size() < bd)) { best = i; bd = adj[i].size(); }
    order.push_back(best);
    done[best] = 1;
    std::vector<int> nb(adj[best].begin(), adj[best].end());
    for (int a : nb) {
      adj[a].erase(best);
      for (int c : nb) if (c != a) adj[a].insert(c);
    }
    adj[best].clear();
  }
  return order;
}

struct Op { int dst, a, b; };

// List scheduling: an operation goes into the first step after every step that wrote what it reads or that read what it writes;
// within a step no two operations touch a slot one of them writes, so its operations run in any order and on any lane.
// Fills step_ptr [nsteps+1] and ops [2 nops] (layout of PH_STEP_PTR / PH_OPS); returns nsteps.
int schedule(const std::vector<Op>& prog, int nslots, std::vector<int32_t>& step_ptr, std::vector<int32_t>& ops) {
  std::vector<int> lw(nslots, -1), lr(nslots, -1), step(prog.size());
  int nsteps = 0;
  for (size_t o = 0; o < prog.size(); ++o) {
    const Op& op = prog[o];
    int s = std::max(lw[op.dst], lr[op.dst]) + 1;
    s = std::max(s, lw[op.a] + 1);
    if (op.b >= 0) s = std::max(s, lw[op.b] + 1);
    step[o] = s;
    lw[op.dst] = s;
    lr[op.a] = std::max(lr[op.a], s);
    if (op.b >= 0) lr[op.b] = std::max(lr[op.b], s);
    nsteps = std::max(nsteps, s + 1);
  }
  step_ptr.assign(nsteps + 1, 0);
  ops.assign(2 * prog.size(), 0);
  for (size_t o = 0; o < prog.size(); ++o) ++step_ptr[step[o] + 1];
  for (int s = 0; s < nsteps; ++s) step_ptr[s + 1] += step_ptr[s];
  std::vector<int32_t> c(step_ptr.begin(), step_ptr.end() - 1);
  for (size_t o = 0; o < prog.size(); ++o) {
    const int q = c[step[o]]++;
    ops[2 * q] = (int32_t)((uint32_t)prog[o].dst | ((uint32_t)prog[o].a << 16));
    ops[2 * q + 1] = prog[o].b;
  }
  return nsteps;
}

// With slots_out, the factor's slot count nnz(L+U) + dim is written there as soon as it is known, also when it is refused.
int analyse(int N, int E, int Gn, const int32_t* f, const int32_t* t, const int32_t* gb, int slack, std::vector<int32_t>& out,
            int64_t* slots_out = nullptr) {
  if (N <= 0 || E < 0 || Gn < 0 || (E > 0 && (!f || !t)) || (Gn > 0 && !gb)) return GNS_EINVAL;
  if (slack < 0 || slack >= N) return GNS_ETOPOLOGY;
  for (int e = 0; e < E; ++e) if (f[e] < 0 || f[e] >= N || t[e] < 0 || t[e] >= N) return GNS_ETOPOLOGY;
  for (int g = 0; g < Gn; ++g) if (gb[g] < 0 || gb[g] >= N) return GNS_ETOPOLOGY;

  std::vector<std::set<int>> adj(N);
  for (int e = 0; e < E; ++e) if (f[e] != t[e]) { adj[f[e]].insert(t[e]); adj[t[e]].insert(f[e]); }
  {  // every bus must reach the slack through lines
    std::vector<char> seen(N, 0);
    std::vector<int> stack{slack};
    seen[slack] = 1;
    while (!stack.empty()) {
      int i = stack.back(); stack.pop_back();
      for (int k : adj[i]) if (!seen[k]) { seen[k] = 1; stack.push_back(k); }
    }
    for (int i = 0; i < N; ++i) if (!seen[i]) return GNS_ETOPOLOGY;
  }

  std::vector<int32_t> role(N, 0), gen_ptr(N + 1, 0), gen_idx(std::max(Gn, 1), 0);
  for (int g = 0; g < Gn; ++g) { role[gb[g]] = 1; ++gen_ptr[gb[g] + 1]; }
  role[slack] = 2;
  for (int i = 0; i < N; ++i) gen_ptr[i + 1] += gen_ptr[i];
  {
    std::vector<int32_t> c(gen_ptr.begin(), gen_ptr.end() - 1);
    for (int g = 0; g < Gn; ++g) gen_idx[c[gb[g]]++] = g;
  }
  int npv = 0, npq = 0;
  for (int i = 0; i < N; ++i) { npv += role[i] == 1; npq += role[i] == 0; }

  // unknowns in elimination order: each bus's theta, then its |V| if it is a PQ bus
  const std::vector<int> order = min_degree_order(N, slack, adj);
  std::vector<int32_t> th_idx(N, -1), vm_idx(N, -1), var_bus;
  for (int i : order) {
    th_idx[i] = (int32_t)var_bus.size(); var_bus.push_back(i);
    if (role[i] == 0) { vm_idx[i] = (int32_t)var_bus.size(); var_bus.push_back(i); }
  }
  const int dim = (int)var_bus.size();

  // Y-bus pattern (CSR, columns ascending, every diagonal present) and the stamps of every entry
  std::vector<int32_t> y_ptr(N + 1, 0), y_col, y_diag(N);
  std::vector<std::map<int, int>> ypos(N);
  for (int i = 0; i < N; ++i) {
    std::set<int> cols(adj[i]);
    cols.insert(i);
    for (int k : cols) { ypos[i][k] = (int)y_col.size(); y_col.push_back(k); }
    y_diag[i] = ypos[i][i];
    y_ptr[i + 1] = (int32_t)y_col.size();
  }
  const int nnzY = (int)y_col.size();
  std::vector<std::vector<int32_t>> stl(nnzY);
  for (int e = 0; e < E; ++e) {
    stl[ypos[f[e]][f[e]]].push_back(4 * e + 0);
    stl[ypos[t[e]][t[e]]].push_back(4 * e + 1);
    stl[ypos[f[e]][t[e]]].push_back(4 * e + 2);
    stl[ypos[t[e]][f[e]]].push_back(4 * e + 3);
  }
  std::vector<int32_t> st_ptr(nnzY + 1, 0), st;
  for (int p = 0; p < nnzY; ++p) { st.insert(st.end(), stl[p].begin(), stl[p].end()); st_ptr[p + 1] = (int32_t)st.size(); }

  // Jacobian pattern in the ordered unknowns, then the symbolic LU (structurally symmetric, no pivoting)
  std::vector<std::vector<char>> P(dim, std::vector<char>(dim, 0));
  int nnzJ = 0;
  for (int i = 0; i < N; ++i) {
    if (i == slack) continue;
    const int rows[2] = {th_idx[i], vm_idx[i]};
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int k = y_col[p];
      if (k == slack) continue;
      const int cols[2] = {th_idx[k], vm_idx[k]};
      for (int r : rows) for (int c : cols) if (r >= 0 && c >= 0 && !P[r][c]) { P[r][c] = 1; ++nnzJ; }
    }
  }
  std::vector<std::vector<int>> lower(dim), upper(dim);     // rows i > k of column k, columns j > k of row k (after fill)
  for (int k = 0; k < dim; ++k) {
    for (int j = k + 1; j < dim; ++j) {
      if (P[j][k]) lower[k].push_back(j);
      if (P[k][j]) upper[k].push_back(j);
    }
    for (int i : lower[k]) for (int j : upper[k]) P[i][j] = 1;
  }
  std::vector<std::vector<int32_t>> slot(dim, std::vector<int32_t>(dim, -1));
  int nnzLU = 0;
  for (int i = 0; i < dim; ++i) for (int j = 0; j < dim; ++j) if (P[i][j]) slot[i][j] = nnzLU++;
  const int nslots = nnzLU + dim;                             // factor, then the right-hand side / solution
  if (slots_out) *slots_out = nslots;
  if (nslots > GNS_PF_MAX_SLOTS) return GNS_EUNSUPPORTED;     // (16-bit operands; such a factor is far beyond the LDS limit anyway)

  std::vector<int32_t> jslot(4 * (size_t)nnzY, -1), pivot(dim);
  for (int i = 0; i < N; ++i) {
    if (i == slack) continue;
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int k = y_col[p];
      if (k == slack) continue;
      jslot[4 * p + 0] = slot[th_idx[i]][th_idx[k]];
      if (vm_idx[k] >= 0) jslot[4 * p + 1] = slot[th_idx[i]][vm_idx[k]];
      if (vm_idx[i] >= 0) jslot[4 * p + 2] = slot[vm_idx[i]][th_idx[k]];
      if (vm_idx[i] >= 0 && vm_idx[k] >= 0) jslot[4 * p + 3] = slot[vm_idx[i]][vm_idx[k]];
    }
  }
  for (int k = 0; k < dim; ++k) pivot[k] = slot[k][k];

  // the sequential program: right-looking LU, forward solve with unit L, backward solve with U
  std::vector<Op> prog;
  for (int k = 0; k < dim; ++k) {
    for (int i : lower[k]) prog.push_back({slot[i][k], slot[k][k], -1});
    for (int i : lower[k]) for (int j : upper[k]) prog.push_back({slot[i][j], slot[i][k], slot[k][j]});
  }
  for (int k = 0; k < dim; ++k) for (int i : lower[k]) prog.push_back({nnzLU + i, slot[i][k], nnzLU + k});
  for (int k = dim - 1; k >= 0; --k) {
    prog.push_back({nnzLU + k, slot[k][k], -1});
    for (int i = 0; i < k; ++i) if (P[i][k]) prog.push_back({nnzLU + i, slot[i][k], nnzLU + k});
  }
  std::vector<int32_t> step_ptr, ops;
  const int nsteps = schedule(prog, nslots, step_ptr, ops);

  // the transposed solve of the adjoint on the same factor: U^T y = rhs (column k of U^T is row k of U) forward, then
  // L^T x = y (unit diagonal) backward
  std::vector<Op> tprog;
  for (int k = 0; k < dim; ++k) {
    tprog.push_back({nnzLU + k, slot[k][k], -1});
    for (int j : upper[k]) tprog.push_back({nnzLU + j, slot[k][j], nnzLU + k});
  }
  for (int k = dim - 1; k >= 0; --k)
    for (int j = 0; j < k; ++j) if (P[k][j]) tprog.push_back({nnzLU + j, slot[k][j], nnzLU + k});
  std::vector<int32_t> t_step_ptr, t_ops;
  const int t_nsteps = schedule(tprog, nslots, t_step_ptr, t_ops);
  // the adjoint factors J with the solve program's steps up to its last factor operation (the solve ops in them see a zero
  // right-hand side): their count follows the transposed program's step pointers
  int nf = 0;
  for (int s = 0; s < nsteps; ++s)
    for (int q = step_ptr[s]; q < step_ptr[s + 1]; ++q)
      if ((ops[2 * q] & 0xFFFF) < nnzLU) nf = s + 1;
  t_step_ptr.push_back(nf);

  PfBlob b;
  b.w[PH_MAGIC] = GNS_PF_MAGIC; b.w[PH_N] = N; b.w[PH_E] = E; b.w[PH_GN] = Gn; b.w[PH_SLACK] = slack;
  b.w[PH_NPV] = npv; b.w[PH_NPQ] = npq; b.w[PH_DIM] = dim; b.w[PH_NNZJ] = nnzJ; b.w[PH_NNZLU] = nnzLU; b.w[PH_NNZY] = nnzY;
  b.w[PH_NOPS] = (int32_t)prog.size(); b.w[PH_NSTEPS] = nsteps;
  b.put(PH_ROLE, role); b.put(PH_TH_IDX, th_idx); b.put(PH_VM_IDX, vm_idx); b.put(PH_GEN_PTR, gen_ptr); b.put(PH_GEN_IDX, gen_idx);
  b.put(PH_Y_PTR, y_ptr); b.put(PH_Y_COL, y_col); b.put(PH_Y_DIAG, y_diag); b.put(PH_ST_PTR, st_ptr); b.put(PH_ST, st);
  b.put(PH_JSLOT, jslot); b.put(PH_PIVOT, pivot); b.put(PH_STEP_PTR, step_ptr);
  if (b.w.size() % 2) b.w.push_back(0);
  b.put(PH_OPS, ops);
  b.w[PH_T_NOPS] = (int32_t)tprog.size(); b.w[PH_T_NSTEPS] = t_nsteps;
  b.put(PH_T_STEP_PTR, t_step_ptr);
  if (b.w.size() % 2) b.w.push_back(0);
  b.put(PH_T_OPS, t_ops);
  b.w[PH_TOTAL] = (int32_t)b.w.size();
  out.swap(b.w);
  return GNS_OK;
}

int analyse_safe(int N, int E, int Gn, const int32_t* f, const int32_t* t, const int32_t* gb, int slack, std::vector<int32_t>& w,
                 int64_t* slots_out = nullptr) {
  try { return analyse(N, E, Gn, f, t, gb, slack, w, slots_out); } catch (...) { return GNS_EINVAL; }
}

}  // namespace

extern "C" int gns_pf_topology_bytes(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, size_t* bytes) {
  if (!bytes) return GNS_EINVAL;
  std::vector<int32_t> w;
  const int rc = analyse_safe(n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, w);
  if (rc != GNS_OK) return rc;
  *bytes = w.size() * sizeof(int32_t);
  return GNS_OK;
}

extern "C" int gns_pf_topology_slots(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, int64_t* slots) {
  if (!slots) return GNS_EINVAL;
  std::vector<int32_t> w;
  *slots = -1;
  const int rc = analyse_safe(n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, w, slots);
  return rc == GNS_EUNSUPPORTED && *slots > GNS_PF_MAX_SLOTS ? GNS_OK : rc;
}

extern "C" int gns_pf_prepare_topology(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                       const int32_t* gen_bus, int32_t slack, void* topo_host_out, size_t topo_bytes) {
  if (!topo_host_out) return GNS_EINVAL;
  std::vector<int32_t> w;
  const int rc = analyse_safe(n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, w);
  if (rc != GNS_OK) return rc;
  if (w.size() * sizeof(int32_t) > topo_bytes) return GNS_ESIZE;
  std::memcpy(topo_host_out, w.data(), w.size() * sizeof(int32_t));
  return GNS_OK;
}

extern "C" int gns_pf_topology_info(const void* topo_host, gns_pf_info* info) {
  if (!topo_host || !info) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[PH_MAGIC] != GNS_PF_MAGIC) return GNS_EINVAL;
  info->n_bus = h[PH_N]; info->n_line = h[PH_E]; info->n_gen = h[PH_GN]; info->slack = h[PH_SLACK];
  info->n_pv = h[PH_NPV]; info->n_pq = h[PH_NPQ]; info->dim = h[PH_DIM]; info->nnz_jac = h[PH_NNZJ]; info->nnz_lu = h[PH_NNZLU];
  info->nnz_ybus = h[PH_NNZY]; info->n_ops = h[PH_NOPS]; info->n_steps = h[PH_NSTEPS];
  info->lds_bytes = pf_lds_bytes(h);
  info->n_adj_ops = h[PH_T_NOPS]; info->n_adj_steps = h[PH_T_NSTEPS];
  info->n_factor_steps = h[h[PH_T_STEP_PTR] + h[PH_T_NSTEPS] + 1];
  return GNS_OK;
}
