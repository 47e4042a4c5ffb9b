// edges.cpp — eg3d_host_edge_chains, eg3d_host_write_ply_edges (include/eg3d/host_edges.h): the sequential statement of
// the 3-D edge model (csrc/eg3d_edges_core.h). The trace walks the successors of the half-edges polyline after polyline;
// the simplification evaluates every linearizable_polyline test point after point.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d/host_edges.h"
#include "eg3d_edges_core.h"

using namespace eg3d;
using namespace eg3d::edges;

namespace {

struct HostClaim {
  std::vector<uint8_t>& seen;
  bool operator()(uint64_t slot) {
    const bool was = seen[slot] != 0;
    seen[slot] = 1;
    return was;
  }
};

// the checks of the header, in the order the device makes them; deg: the degree of every node; n_loops
int check_graph(const eg3d_graph3d* g, std::vector<uint32_t>& deg, uint64_t* n_loops) {
  const uint64_t NN = g->n_nodes, NP = g->n_polylines;
  if (NN >= kMaxCount || NP >= kMaxCount) return -3;
  if ((NN && !g->node_X) || (NP && (!g->pl_start || !g->pl_end)) || !g->conn_off) return -1;
  uint64_t loops = 0;
  for (uint64_t p = 0; p < NP; p++) {
    if (g->pl_start[p] >= NN || g->pl_end[p] >= NN) return -1;
    loops += g->pl_start[p] == g->pl_end[p] ? 1 : 0;
  }
  const uint64_t expect = 2 * NP - loops;
  if (g->conn_off[0] != 0 || g->conn_off[NN] != expect) return -1;
  for (uint64_t v = 0; v < NN; v++)
    if (g->conn_off[v] > g->conn_off[v + 1] || g->conn_off[v + 1] > expect) return -1;
  if (expect && !g->conn_pl) return -1;
  std::vector<uint8_t> seen(2 * NP, 0);
  HostClaim claim{seen};
  deg.assign(NN, 0);
  bool ok = true;
  for (uint64_t v = 0; v < NN; v++) ok &= check_row((uint32_t)v, NP, g->pl_start, g->pl_end, g->conn_off, g->conn_pl, claim, &deg[v]);
  *n_loops = loops;
  return ok ? 0 : -1;
}

struct HostPts {
  const float* X;
  const uint32_t* node;
  void get(uint32_t i, float* p) const {
    const float* s = X + 3 * (uint64_t)node[i];
    p[0] = s[0], p[1] = s[1], p[2] = s[2];
  }
};
struct HostLin {  // linearizable_polyline, point after point
  HostPts P;
  float maxsq;
  bool operator()(uint32_t start, uint32_t end) {
    for (uint32_t i = start + 1; i < end; i++)
      if (point_off_line(P, start, end, i, maxsq)) return false;
    return true;
  }
};
struct HostOut {
  uint32_t* region;
  const uint32_t* node;
  uint32_t span;
  void front(uint32_t k, uint32_t i) { region[k] = node[i]; }
  void back(uint32_t k, uint32_t i) { region[span - 1 - k] = node[i]; }
};

template <typename T>
T* give(const std::vector<T>& v) {  // a malloc'ed copy (at least one element), or null when out of memory
  T* p = (T*)malloc(sizeof(T) * (v.size() ? v.size() : 1));
  if (p && !v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}

float ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" void eg3d_host_free_edge_chains(eg3d_edge_chain_set* c) {
  if (!c) return;
  void* all[] = {c->chain_off, c->chain_node, c->chain_flags, c->s_off, c->s_node, c->length};
  for (void* p : all) free(p);
  memset(c, 0, sizeof(*c));
}

extern "C" int eg3d_host_edge_chains(const eg3d_graph3d* g, float max_dist, int simplify, eg3d_edge_chain_set* out, eg3d_edges_stats* stats) {
  if (!g || !out) return -1;
  if (stats && stats->struct_size < sizeof(eg3d_edges_stats)) return -1;
  if (!std::isfinite(max_dist) || !(max_dist >= 0.0f)) return -1;
  std::vector<uint32_t> deg;
  uint64_t n_loops = 0;
  if (const int rc = check_graph(g, deg, &n_loops)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t NP = g->n_polylines;
  const uint32_t *ps = g->pl_start, *pe = g->pl_end;

  // ---- trace: polylines ascending; an unvisited one is the smallest of its chain
  std::vector<uint64_t> chain_off{0};
  std::vector<uint32_t> chain_node, chain_flags;
  std::vector<uint8_t> visited(NP, 0);
  std::vector<uint32_t> fwd, bwd;  // half-edges
  uint64_t n_rings = 0, longest = 0;
  for (uint64_t p = 0; p < NP; p++) {
    if (visited[p] || ps[p] == pe[p]) continue;
    fwd.clear();
    bwd.clear();
    bool ring = false;
    for (uint32_t h = 2u * (uint32_t)p; h != kNone; h = successor(h, deg[he_far(h, ps, pe)], ps, pe, g->conn_off, g->conn_pl)) {
      if (!fwd.empty() && h == fwd[0]) {
        ring = true;
        break;
      }
      fwd.push_back(h);
      visited[h >> 1] = 1;
    }
    if (!ring)  // the other way from p's start, p itself left out
      for (uint32_t h = successor(2u * (uint32_t)p + 1u, deg[ps[p]], ps, pe, g->conn_off, g->conn_pl); h != kNone;
           h = successor(h, deg[he_far(h, ps, pe)], ps, pe, g->conn_off, g->conn_pl)) {
        bwd.push_back(h);
        visited[h >> 1] = 1;
      }
    // the chain as half-edges in ONE direction: the reversed bwd list turned round, then fwd
    std::vector<uint32_t> list;
    for (size_t k = bwd.size(); k-- > 0;) list.push_back(bwd[k] ^ 1u);
    list.insert(list.end(), fwd.begin(), fwd.end());
    const size_t L = list.size();
    if (ring) {
      size_t at = 0;  // the half-edge that leaves the smallest node
      for (size_t k = 1; k < L; k++)
        if (he_from(list[k], ps, pe) < he_from(list[at], ps, pe)) at = k;
      const size_t before = (at + L - 1) % L;  // ... and the one that arrives there
      std::vector<uint32_t> r;
      if ((list[at] >> 1) < (list[before] >> 1))
        for (size_t k = 0; k < L; k++) r.push_back(list[(at + k) % L]);
      else
        for (size_t k = 0; k < L; k++) r.push_back(list[(before + L - k) % L] ^ 1u);
      list.swap(r);
      n_rings++;
    } else if (!head_is_chosen(list[0], list[L - 1])) {
      std::vector<uint32_t> r;
      for (size_t k = L; k-- > 0;) r.push_back(list[k] ^ 1u);
      list.swap(r);
    }
    for (size_t k = 0; k < L; k++) chain_node.push_back(he_from(list[k], ps, pe));
    chain_node.push_back(he_far(list[L - 1], ps, pe));
    chain_off.push_back(chain_node.size());
    chain_flags.push_back(ring ? EG3D_EDGES_FLAG_RING : 0u);
    longest = std::max<uint64_t>(longest, L + 1);
  }
  const uint64_t n_chains = chain_flags.size();
  const float ms_trace = ms_since(t0);

  // ---- simplify
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<uint64_t> s_off;
  std::vector<uint32_t> s_node;
  if (simplify) {
    const float maxsq = max_dist * max_dist;
    std::vector<uint32_t> region;
    s_off.push_back(0);
    for (uint64_t c = 0; c < n_chains; c++) {
      const uint32_t* node = chain_node.data() + chain_off[c];
      const uint32_t n = (uint32_t)(chain_off[c + 1] - chain_off[c]);
      const uint32_t span = simplified_span(n, node[0], node[n - 1]);
      region.assign(n, 0);
      HostLin lin{HostPts{g->node_X, node}, maxsq};
      HostOut o{region.data(), node, span};
      uint32_t nf = 0, nb = 0;
      simplify_indices(lin, span, o, &nf, &nb);
      if (span != n) region[n - 1] = node[n - 1], nb++;
      s_node.insert(s_node.end(), region.begin(), region.begin() + nf);
      s_node.insert(s_node.end(), region.end() - nb, region.end());
      s_off.push_back(s_node.size());
    }
  } else {
    s_off = chain_off;
    s_node = chain_node;
  }
  std::vector<float> length(n_chains);
  for (uint64_t c = 0; c < n_chains; c++) length[c] = polyline_length(g->node_X, s_node.data() + s_off[c], s_off[c + 1] - s_off[c]);
  const float ms_simplify = ms_since(t1);

  eg3d_edge_chain_set r;
  memset(&r, 0, sizeof(r));
  r.n_chains = n_chains;
  r.n_vertices = chain_node.size();
  r.n_kept = s_node.size();
  r.chain_off = give(chain_off);
  r.chain_node = give(chain_node);
  r.chain_flags = give(chain_flags);
  r.s_off = give(s_off);
  r.s_node = give(s_node);
  r.length = give(length);
  if (!r.chain_off || !r.chain_node || !r.chain_flags || !r.s_off || !r.s_node || !r.length) {
    eg3d_host_free_edge_chains(&r);
    return -2;
  }
  *out = r;
  if (stats) {
    eg3d_edges_stats s;
    memset(&s, 0, sizeof(s));
    s.struct_size = (uint32_t)sizeof(s);
    s.n_chains = n_chains;
    s.n_rings = n_rings;
    s.n_loops_dropped = n_loops;
    s.n_vertices_in = r.n_vertices;
    s.n_vertices_kept = r.n_kept;
    s.longest_chain = longest;
    s.ms_trace = ms_trace;
    s.ms_simplify = ms_simplify;
    *stats = s;
  }
  return 0;
}

extern "C" int eg3d_host_write_ply_edges(const char* path, const eg3d_edge_chain_set* c, const float* node_X) {
  if (!path || !c || (c->n_chains && (!c->s_off || !c->s_node)) || (c->n_kept && !node_X)) return -1;
  // the distinct kept nodes, ascending, and their new numbers
  uint32_t top = 0;
  for (uint64_t i = 0; i < c->n_kept; i++) top = std::max(top, c->s_node[i]);
  std::vector<uint32_t> number(c->n_kept ? (size_t)top + 1 : 0, kNone);
  for (uint64_t i = 0; i < c->n_kept; i++) number[c->s_node[i]] = 0;
  uint64_t n_vertices = 0, n_edges = 0;
  for (uint32_t& n : number)
    if (n != kNone) n = (uint32_t)n_vertices++;
  for (uint64_t k = 0; k < c->n_chains; k++) n_edges += c->s_off[k + 1] - c->s_off[k] - (c->s_off[k + 1] > c->s_off[k] ? 1 : 0);
  FILE* f = fopen(path, "wb");
  if (!f) return -2;
  std::string text = "ply\nformat ascii 1.0\nelement vertex " + std::to_string(n_vertices) +
                     "\nproperty float x\nproperty float y\nproperty float z\nelement edge " + std::to_string(n_edges) +
                     "\nproperty int vertex1\nproperty int vertex2\nend_header\n";
  bool ok = true;
  char line[160];
  auto flush = [&](bool all) {
    if (ok && (all ? !text.empty() : text.size() >= (1u << 20))) {
      ok = fwrite(text.data(), 1, text.size(), f) == text.size();
      text.clear();
    }
  };
  for (size_t v = 0; v < number.size() && ok; v++) {
    if (number[v] == kNone) continue;
    const int n = snprintf(line, sizeof(line), "%g %g %g\n", (double)node_X[3 * v], (double)node_X[3 * v + 1], (double)node_X[3 * v + 2]);
    text.append(line, (size_t)n);
    flush(false);
  }
  for (uint64_t k = 0; k < c->n_chains && ok; k++)
    for (uint64_t i = c->s_off[k] + 1; i < c->s_off[k + 1]; i++) {
      const int n = snprintf(line, sizeof(line), "%u %u\n", number[c->s_node[i - 1]], number[c->s_node[i]]);
      text.append(line, (size_t)n);
      flush(false);
    }
  flush(true);
  if (fclose(f) != 0) ok = false;
  return ok ? 0 : -2;
}
