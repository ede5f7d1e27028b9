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

// One topology as the entry points take it.  out_gen: a generator row out of service (gns_pf_prepare_topology_out_gen), -1 for none.
struct TopologyArgs {
  int32_t n_bus, n_line, n_gen;
  const int32_t *f_bus, *t_bus, *gen_bus;
  int32_t slack;
  int32_t out_gen = -1;
};

struct PfBlob {
  std::vector<int32_t> w;
  PfBlob() : w(PF_HDR_WORDS, 0) {}
  void put(int slot, const std::vector<int32_t>& a) { w[slot] = (int32_t)w.size(); w.insert(w.end(), a.begin(), a.end()); }
};

// Minimum degree on the bus graph without the buses marked in skip (ties: lowest bus id); the elimination graph is kept as
// explicit sets.  The Newton-Raphson analysis and B' skip the slack, B'' every bus that is not PQ (its PQ-induced subgraph).
std::vector<int> min_degree_order(int N, const std::vector<char>& skip, const std::vector<std::set<int>>& adj0) {
  std::vector<std::set<int>> adj(adj0);
  std::vector<char> done(skip);
  int left = 0;
  for (int i = 0; i < N; ++i) {
    if (done[i]) adj[i].clear();
    else { ++left; for (auto it = adj[i].begin(); it != adj[i].end();) it = done[*it] ? adj[i].erase(it) : std::next(it); }
  }
  std::vector<int> order;
  for (int it = 0; it < left; ++it) {
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

// What both analyses share: the checked ids, the bus graph, roles, generators by bus and the Y-bus pattern with its stamps
struct PfGrid {
  std::vector<std::set<int>> adj;
  std::vector<int32_t> role, gen_ptr, gen_idx, y_ptr, y_col, y_diag, st_ptr, st;
  int npv = 0, npq = 0, nnzY = 0;
};

// out_gen >= 0: that generator row is out of service.  It gives its bus no role and is left off the by-bus lists, which keep the
// original row numbers of the others (Gn - 1 entries; the header's Gn and the indexing of generators [Bt,Gn,7] stay as they are).
int pf_grid(int N, int E, int Gn, const int32_t* f, const int32_t* t, const int32_t* gb, int slack, int out_gen, PfGrid& G) {
  if (N <= 0 || E < 0 || Gn < 0 || (E > 0 && (!f || !t)) || (Gn > 0 && !gb) || out_gen < -1 || out_gen >= Gn) return GNS_EINVAL;
  if (slack < 0 || slack >= N) return GNS_ETOPOLOGY;
  for (int e = 0; e < E; ++e) if (f[e] < 0 || f[e] >= N || t[e] < 0 || t[e] >= N) return GNS_ETOPOLOGY;
  for (int g = 0; g < Gn; ++g) if (gb[g] < 0 || gb[g] >= N) return GNS_ETOPOLOGY;

  std::vector<std::set<int>>& adj = G.adj;
  adj.assign(N, {});
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

  std::vector<int32_t>& role = G.role;
  std::vector<int32_t>& gen_ptr = G.gen_ptr;
  role.assign(N, 0); gen_ptr.assign(N + 1, 0); G.gen_idx.assign(std::max(Gn, 1), 0);
  for (int g = 0; g < Gn; ++g) if (g != out_gen) { role[gb[g]] = 1; ++gen_ptr[gb[g] + 1]; }
  role[slack] = 2;
  for (int i = 0; i < N; ++i) gen_ptr[i + 1] += gen_ptr[i];
  {
    std::vector<int32_t> c(gen_ptr.begin(), gen_ptr.end() - 1);
    for (int g = 0; g < Gn; ++g) if (g != out_gen) G.gen_idx[c[gb[g]]++] = g;
  }
  for (int i = 0; i < N; ++i) { G.npv += role[i] == 1; G.npq += role[i] == 0; }

  // Y-bus pattern (CSR, columns ascending, every diagonal present) and the stamps of every entry
  G.y_ptr.assign(N + 1, 0); G.y_diag.assign(N, 0); G.y_col.clear();
  std::vector<std::map<int, int>> ypos(N);
  for (int i = 0; i < N; ++i) {
    std::set<int> cols(adj[i]);
    cols.insert(i);
    for (int k : cols) { ypos[i][k] = (int)G.y_col.size(); G.y_col.push_back(k); }
    G.y_diag[i] = ypos[i][i];
    G.y_ptr[i + 1] = (int32_t)G.y_col.size();
  }
  const int nnzY = G.nnzY = (int)G.y_col.size();
  std::vector<std::vector<int32_t>> stl(nnzY);
  for (int e = 0; e < E; ++e) {
    stl[ypos[f[e]][f[e]]].push_back(4 * e + 0);
    stl[ypos[t[e]][t[e]]].push_back(4 * e + 1);
    stl[ypos[f[e]][t[e]]].push_back(4 * e + 2);
    stl[ypos[t[e]][f[e]]].push_back(4 * e + 3);
  }
  G.st_ptr.assign(nnzY + 1, 0); G.st.clear();
  for (int p = 0; p < nnzY; ++p) { G.st.insert(G.st.end(), stl[p].begin(), stl[p].end()); G.st_ptr[p + 1] = (int32_t)G.st.size(); }
  return GNS_OK;
}

// The symbolic LU of a structurally symmetric pattern P (dim x dim, diagonal set; no pivoting): P gains the fill, lower[k] /
// upper[k] list the rows i > k of column k and the columns j > k of row k, and slot numbers the entries of L + U row-major (nnz of
// them); the right-hand side / solution follows at slots nnz .. nnz + dim.
struct SymLU {
  int dim = 0, nnz = 0;
  std::vector<std::vector<char>> P;
  std::vector<std::vector<int>> lower, upper;
  std::vector<std::vector<int32_t>> slot;
  explicit SymLU(int d) : dim(d), P(d, std::vector<char>(d, 0)), lower(d), upper(d), slot(d, std::vector<int32_t>(d, -1)) {}
  void factorise_pattern() {
    for (int k = 0; k < dim; ++k) {
      for (int j = k + 1; j < dim; ++j) {
        if (P[j][k]) lower[k].push_back(j);
        if (P[k][j]) upper[k].push_back(j);
      }
      for (int i : lower[k]) for (int j : upper[k]) P[i][j] = 1;
    }
    nnz = 0;
    for (int i = 0; i < dim; ++i) for (int j = 0; j < dim; ++j) if (P[i][j]) slot[i][j] = nnz++;
  }
  // right-looking LU in place
  void factor_ops(std::vector<Op>& prog) const {
    for (int k = 0; k < dim; ++k) {
      for (int i : lower[k]) prog.push_back({slot[i][k], slot[k][k], -1});
      for (int i : lower[k]) for (int j : upper[k]) prog.push_back({slot[i][j], slot[i][k], slot[k][j]});
    }
  }
  // forward solve with unit L, backward solve with U, on the right-hand side at slots nnz ..
  void solve_ops(std::vector<Op>& prog) const {
    for (int k = 0; k < dim; ++k) for (int i : lower[k]) prog.push_back({nnz + i, slot[i][k], nnz + k});
    for (int k = dim - 1; k >= 0; --k) {
      prog.push_back({nnz + k, slot[k][k], -1});
      for (int i = 0; i < k; ++i) if (P[i][k]) prog.push_back({nnz + i, slot[i][k], nnz + k});
    }
  }
};

// With slots_out, the factor's slot count nnz(L+U) + dim is written there as soon as it is known, also when it is refused.
int analyse(const TopologyArgs& a, std::vector<int32_t>& out, int64_t* slots_out = nullptr) {
  const int N = a.n_bus, E = a.n_line, Gn = a.n_gen, slack = a.slack;
  PfGrid G;
  const int rc = pf_grid(N, E, Gn, a.f_bus, a.t_bus, a.gen_bus, slack, a.out_gen, G);
  if (rc != GNS_OK) return rc;
  const std::vector<int32_t>& role = G.role;
  const std::vector<int32_t>& y_ptr = G.y_ptr;
  const std::vector<int32_t>& y_col = G.y_col;
  const int nnzY = G.nnzY;

  // unknowns in elimination order: each bus's theta, then its |V| if it is a PQ bus
  std::vector<char> skip(N, 0);
  skip[slack] = 1;
  const std::vector<int> order = min_degree_order(N, skip, G.adj);
  std::vector<int32_t> th_idx(N, -1), vm_idx(N, -1), var_bus;
  for (int i : order) {
    th_idx[i] = (int32_t)var_bus.size(); var_bus.push_back(i);
    if (role[i] == 0) { vm_idx[i] = (int32_t)var_bus.size(); var_bus.push_back(i); }
  }
  const int dim = (int)var_bus.size();

  // Jacobian pattern in the ordered unknowns, then the symbolic LU (structurally symmetric, no pivoting)
  SymLU lu(dim);
  int nnzJ = 0;
  for (int i = 0; i < N; ++i) {
    if (i == slack) continue;
    const int rows[2] = {th_idx[i], vm_idx[i]};
    for (int p = y_ptr[i]; p < y_ptr[i + 1]; ++p) {
      const int k = y_col[p];
      if (k == slack) continue;
      const int cols[2] = {th_idx[k], vm_idx[k]};
      for (int r : rows) for (int c : cols) if (r >= 0 && c >= 0 && !lu.P[r][c]) { lu.P[r][c] = 1; ++nnzJ; }
    }
  }
  lu.factorise_pattern();
  const std::vector<std::vector<char>>& P = lu.P;
  const std::vector<std::vector<int>>& upper = lu.upper;
  const std::vector<std::vector<int32_t>>& slot = lu.slot;
  const int nnzLU = lu.nnz;
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
  lu.factor_ops(prog);
  lu.solve_ops(prog);
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
  b.w[PH_NPV] = G.npv; b.w[PH_NPQ] = G.npq; b.w[PH_DIM] = dim; b.w[PH_NNZJ] = nnzJ; b.w[PH_NNZLU] = nnzLU; b.w[PH_NNZY] = nnzY;
  b.w[PH_NOPS] = (int32_t)prog.size(); b.w[PH_NSTEPS] = nsteps;
  b.put(PH_ROLE, role); b.put(PH_TH_IDX, th_idx); b.put(PH_VM_IDX, vm_idx); b.put(PH_GEN_PTR, G.gen_ptr); b.put(PH_GEN_IDX, G.gen_idx);
  b.put(PH_Y_PTR, y_ptr); b.put(PH_Y_COL, y_col); b.put(PH_Y_DIAG, G.y_diag); b.put(PH_ST_PTR, G.st_ptr); b.put(PH_ST, G.st);
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

// The fast-decoupled analysis: B' on the PV+PQ buses and B'' on the PQ buses share the Y-bus pattern; each gets a minimum-degree
// ordering of its bus subgraph, a symbolic LU, and a factorisation and a solve program (layout: gns_pf_common.h, FH_*).  With
// slots_out, the larger of the two factors' slot counts is written there as soon as both are known.
int analyse_fd(const TopologyArgs& a, std::vector<int32_t>& out, int64_t* slots_out = nullptr) {
  const int N = a.n_bus, E = a.n_line, Gn = a.n_gen, slack = a.slack;
  PfGrid G;
  const int rc = pf_grid(N, E, Gn, a.f_bus, a.t_bus, a.gen_bus, slack, a.out_gen, G);
  if (rc != GNS_OK) return rc;
  const int nnzY = G.nnzY;
  std::vector<int32_t> idx[2] = {std::vector<int32_t>(N, -1), std::vector<int32_t>(N, -1)};
  std::vector<SymLU> lu;
  for (int m = 0; m < 2; ++m) {                 // m = 0: B' (every bus but the slack), 1: B'' (the PQ buses)
    std::vector<char> skip(N, 0);
    for (int i = 0; i < N; ++i) skip[i] = m == 0 ? i == slack : G.role[i] != 0;
    const std::vector<int> order = min_degree_order(N, skip, G.adj);
    for (size_t q = 0; q < order.size(); ++q) idx[m][order[q]] = (int32_t)q;
    lu.emplace_back((int)order.size());
    for (int i = 0; i < N; ++i) {
      if (idx[m][i] < 0) continue;
      for (int p = G.y_ptr[i]; p < G.y_ptr[i + 1]; ++p)
        if (idx[m][G.y_col[p]] >= 0) lu[m].P[idx[m][i]][idx[m][G.y_col[p]]] = 1;
    }
    lu[m].factorise_pattern();
  }
  const int64_t slots = std::max(lu[0].nnz + lu[0].dim, lu[1].nnz + lu[1].dim);
  if (slots_out) *slots_out = slots;
  if (slots > GNS_PF_MAX_SLOTS) return GNS_EUNSUPPORTED;

  std::vector<int32_t> bslot(2 * (size_t)nnzY, -1), pivot[2];
  for (int i = 0; i < N; ++i)
    for (int p = G.y_ptr[i]; p < G.y_ptr[i + 1]; ++p) {
      const int k = G.y_col[p];
      for (int m = 0; m < 2; ++m)
        if (idx[m][i] >= 0 && idx[m][k] >= 0) bslot[2 * p + m] = lu[m].slot[idx[m][i]][idx[m][k]];
    }
  std::vector<int32_t> step_ptr[4], ops[4];
  int nops[4], nsteps[4];
  for (int m = 0; m < 2; ++m) {
    for (int k = 0; k < lu[m].dim; ++k) pivot[m].push_back(lu[m].slot[k][k]);
    std::vector<Op> fprog, sprog;
    lu[m].factor_ops(fprog);
    lu[m].solve_ops(sprog);
    nops[2 * m] = (int)fprog.size();
    nops[2 * m + 1] = (int)sprog.size();
    nsteps[2 * m] = schedule(fprog, lu[m].nnz + lu[m].dim, step_ptr[2 * m], ops[2 * m]);
    nsteps[2 * m + 1] = schedule(sprog, lu[m].nnz + lu[m].dim, step_ptr[2 * m + 1], ops[2 * m + 1]);
  }

  PfBlob b;
  b.w.assign(FD_HDR_WORDS, 0);
  b.w[FH_MAGIC] = GNS_FD_MAGIC; b.w[FH_N] = N; b.w[FH_E] = E; b.w[FH_GN] = Gn; b.w[FH_SLACK] = slack;
  b.w[FH_NPV] = G.npv; b.w[FH_NPQ] = G.npq; b.w[FH_NNZY] = nnzY;
  b.w[FH_DIM1] = lu[0].dim; b.w[FH_NNZLU1] = lu[0].nnz; b.w[FH_DIM2] = lu[1].dim; b.w[FH_NNZLU2] = lu[1].nnz;
  for (int q = 0; q < 4; ++q) { b.w[FH_NOPS_F1 + 2 * q] = nops[q]; b.w[FH_NSTEPS_F1 + 2 * q] = nsteps[q]; }
  b.put(FH_ROLE, G.role); b.put(FH_P_IDX, idx[0]); b.put(FH_Q_IDX, idx[1]); b.put(FH_GEN_PTR, G.gen_ptr);
  b.put(FH_GEN_IDX, G.gen_idx); b.put(FH_Y_PTR, G.y_ptr); b.put(FH_Y_COL, G.y_col); b.put(FH_Y_DIAG, G.y_diag);
  b.put(FH_ST_PTR, G.st_ptr); b.put(FH_ST, G.st); b.put(FH_BSLOT, bslot); b.put(FH_PIVOT1, pivot[0]); b.put(FH_PIVOT2, pivot[1]);
  for (int q = 0; q < 4; ++q) {
    b.put(FH_STEP_F1 + 2 * q, step_ptr[q]);
    if (b.w.size() % 2) b.w.push_back(0);
    b.put(FH_OPS_F1 + 2 * q, ops[q]);
  }
  b.w[FH_TOTAL] = (int32_t)b.w.size();
  out.swap(b.w);
  return GNS_OK;
}

// The three entry points of an analysis (analyse or analyse_fd), written once.  An exception of the analysis (out of memory on an
// absurd shape) is GNS_EINVAL.
using Analysis = int (*)(const TopologyArgs&, std::vector<int32_t>&, int64_t*);

int analyse_safe(Analysis fn, const TopologyArgs& a, std::vector<int32_t>& w, int64_t* slots_out = nullptr) {
  try { return fn(a, w, slots_out); } catch (...) { return GNS_EINVAL; }
}

int topology_bytes(Analysis fn, const TopologyArgs& a, size_t* bytes) {
  if (!bytes) return GNS_EINVAL;
  std::vector<int32_t> w;
  const int rc = analyse_safe(fn, a, w);
  if (rc != GNS_OK) return rc;
  *bytes = w.size() * sizeof(int32_t);
  return GNS_OK;
}

int topology_slots(Analysis fn, const TopologyArgs& a, int64_t* slots) {
  if (!slots) return GNS_EINVAL;
  std::vector<int32_t> w;
  *slots = -1;
  const int rc = analyse_safe(fn, a, w, slots);
  return rc == GNS_EUNSUPPORTED && *slots > GNS_PF_MAX_SLOTS ? GNS_OK : rc;
}

int prepare_topology(Analysis fn, const TopologyArgs& a, void* topo_host_out, size_t topo_bytes) {
  if (!topo_host_out) return GNS_EINVAL;
  std::vector<int32_t> w;
  const int rc = analyse_safe(fn, a, w);
  if (rc != GNS_OK) return rc;
  if (w.size() * sizeof(int32_t) > topo_bytes) return GNS_ESIZE;
  std::memcpy(topo_host_out, w.data(), w.size() * sizeof(int32_t));
  return GNS_OK;
}

}  // namespace

extern "C" int gns_pf_topology_bytes(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, size_t* bytes) {
  return topology_bytes(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, bytes);
}

extern "C" int gns_pf_topology_slots(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, int64_t* slots) {
  return topology_slots(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, slots);
}

extern "C" int gns_pf_prepare_topology(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                       const int32_t* gen_bus, int32_t slack, void* topo_host_out, size_t topo_bytes) {
  return prepare_topology(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, topo_host_out, topo_bytes);
}

// The analysis with generator row out_gen out of service (-1: none, gns_pf_prepare_topology's blob byte for byte): what the AC
// generator contingency screen runs a row on.  The Y-bus pattern and its stamps come from the lines alone: the same words whatever
// out_gen is.
extern "C" int gns_pf_topology_bytes_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                             const int32_t* gen_bus, int32_t slack, int32_t out_gen, size_t* bytes) {
  return topology_bytes(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, out_gen}, bytes);
}

extern "C" int gns_pf_topology_slots_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                             const int32_t* gen_bus, int32_t slack, int32_t out_gen, int64_t* slots) {
  return topology_slots(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, out_gen}, slots);
}

extern "C" int gns_pf_prepare_topology_out_gen(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                               const int32_t* gen_bus, int32_t slack, int32_t out_gen, void* topo_host_out,
                                               size_t topo_bytes) {
  return prepare_topology(analyse, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack, out_gen}, topo_host_out, topo_bytes);
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

extern "C" int gns_fd_topology_bytes(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, size_t* bytes) {
  return topology_bytes(analyse_fd, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, bytes);
}

extern "C" int gns_fd_topology_slots(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                     const int32_t* gen_bus, int32_t slack, int64_t* slots) {
  return topology_slots(analyse_fd, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, slots);
}

extern "C" int gns_fd_prepare_topology(int32_t n_bus, int32_t n_line, int32_t n_gen, const int32_t* f_bus, const int32_t* t_bus,
                                       const int32_t* gen_bus, int32_t slack, void* topo_host_out, size_t topo_bytes) {
  return prepare_topology(analyse_fd, {n_bus, n_line, n_gen, f_bus, t_bus, gen_bus, slack}, topo_host_out, topo_bytes);
}

extern "C" int gns_fd_topology_info(const void* topo_host, gns_fd_info* info) {
  if (!topo_host || !info) return GNS_EINVAL;
  const int32_t* h = static_cast<const int32_t*>(topo_host);
  if (h[FH_MAGIC] != GNS_FD_MAGIC) return GNS_EINVAL;
  info->n_bus = h[FH_N]; info->n_line = h[FH_E]; info->n_gen = h[FH_GN]; info->slack = h[FH_SLACK];
  info->n_pv = h[FH_NPV]; info->n_pq = h[FH_NPQ]; info->nnz_ybus = h[FH_NNZY];
  info->dim_p = h[FH_DIM1]; info->nnz_lu_p = h[FH_NNZLU1]; info->dim_pp = h[FH_DIM2]; info->nnz_lu_pp = h[FH_NNZLU2];
  info->factor_p_ops = h[FH_NOPS_F1]; info->factor_p_steps = h[FH_NSTEPS_F1];
  info->solve_p_ops = h[FH_NOPS_S1]; info->solve_p_steps = h[FH_NSTEPS_S1];
  info->factor_pp_ops = h[FH_NOPS_F2]; info->factor_pp_steps = h[FH_NSTEPS_F2];
  info->solve_pp_ops = h[FH_NOPS_S2]; info->solve_pp_steps = h[FH_NSTEPS_S2];
  info->lds_bytes = fd_lds_bytes(h);
  return GNS_OK;
}
