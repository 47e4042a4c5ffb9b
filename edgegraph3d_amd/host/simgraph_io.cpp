// The file seam of pipeline 1 (eg3d_host.h): the reference hands its compatibility graph to the community detection as a
// text file and reads one community id per node back (community_detection_interface.cpp:42-73). Both sides of that seam
// and the step that follows it, on the arrays of eg3d_similarity_graph.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "eg3d_host.h"

// GraphAdjacencySetUndirectedNoTypeWeighted::write_to_file (graph_adjacency_set_undirected_no_type_weighted.cpp:54-74): the
// header with the DIRECTED edge count, then every adjacency entry with 1-based ids; the weight goes through an ofstream's
// operator<<(float), as there, so the text is the reference's whatever the C locale of the process is.
extern "C" int eg3d_host_write_compat_graph(const char* path, const eg3d_simgraph* g) {
  if (!path || !g || !g->adj_off) return EG3D_ERR_ARG;
  std::ofstream file(path);
  if (!file.is_open()) return EG3D_ERR_ARG;
  const unsigned long n_nodes = g->n_nodes, n_edges = g->adj_off[g->n_nodes];
  file << "p sp " << n_nodes << " " << n_edges << "\n";
  for (unsigned long node1 = 0; node1 < n_nodes; node1++)
    for (uint32_t k = g->adj_off[node1]; k < g->adj_off[node1 + 1]; k++)
      file << "a " << node1 + 1 << " " << (unsigned long)g->adj_node[k] + 1 << " " << g->adj_w[k] << "\n";
  file.close();
  return file.fail() ? EG3D_ERR_ARG : EG3D_OK;
}

// read_cluster_info (community_detection_interface.cpp:42-55): stoul of every line, stored as long — "-1" comes back as -1.
// A line stoul would throw on (the reference would terminate) is refused.
extern "C" int eg3d_host_read_communities(const char* path, int64_t** ids, uint64_t* n) {
  if (!path || !ids || !n) return EG3D_ERR_ARG;
  std::ifstream in(path);
  if (!in.is_open()) return EG3D_ERR_ARG;
  std::vector<int64_t> res;
  std::string line;
  while (std::getline(in, line)) {
    try {
      res.push_back((int64_t)(long)std::stoul(line, nullptr, 10));
    } catch (const std::exception&) {
      return EG3D_ERR_ARG;
    }
  }
  int64_t* out = (int64_t*)malloc(sizeof(int64_t) * (res.size() ? res.size() : 1));
  if (!out) return EG3D_ERR_ARG;
  if (!res.empty()) memcpy(out, res.data(), sizeof(int64_t) * res.size());
  *ids = out;
  *n = res.size();
  return EG3D_OK;
}

// The other direction of the same file: one id per line, printed with %ld as Grappolo prints the file the reference reads
// (a node without a neighbour is -1 there too).
extern "C" int eg3d_host_write_communities(const char* path, const int64_t* ids, uint64_t n) {
  if (!path || (n && !ids)) return EG3D_ERR_ARG;
  FILE* f = fopen(path, "w");
  if (!f) return EG3D_ERR_ARG;
  bool ok = true;
  for (uint64_t i = 0; i < n && ok; i++) ok = fprintf(f, "%ld\n", (long)ids[i]) > 0;
  return (fclose(f) == 0 && ok) ? EG3D_OK : EG3D_ERR_ARG;
}

extern "C" void eg3d_host_free_polyline_sets(eg3d_polyline_sets* s) {
  if (!s) return;
  free((void*)s->row_off);
  free((void*)s->pl_ids);
  memset(s, 0, sizeof(*s));
}

// compute_polyline_matches_from_nodes_component_ids (polyline_matcher.cpp:202-214): max id + 1 sets, a node with a negative
// id in none, a community no node names an empty set.
extern "C" int eg3d_host_sets_from_communities(const eg3d_simgraph* g, const int64_t* ids, uint64_t n, int32_t n_views,
                                               eg3d_polyline_sets* out) {
  if (!g || !out || n_views < 1 || n != g->n_nodes || (n && !ids)) return EG3D_ERR_ARG;
  int64_t max_id = -1;
  for (uint64_t i = 0; i < n; i++) max_id = ids[i] > max_id ? ids[i] : max_id;
  const uint64_t n_sets = (uint64_t)(max_id + 1);
  if (n_sets * (uint64_t)n_views >= 0xffffffffull) return EG3D_ERR_CAPACITY;
  for (uint64_t i = 0; i < n; i++)
    if (ids[i] >= 0 && g->node_view[i] >= (uint32_t)n_views) return EG3D_ERR_ARG;
  std::vector<std::set<uint32_t>> rows((size_t)n_sets * n_views);
  for (uint64_t i = 0; i < n; i++)
    if (ids[i] >= 0) rows[(size_t)ids[i] * n_views + g->node_view[i]].insert(g->node_pl[i]);
  size_t total = 0;
  for (const auto& r : rows) total += r.size();
  uint32_t* row_off = (uint32_t*)malloc(sizeof(uint32_t) * (rows.size() + 1));
  uint32_t* pl_ids = (uint32_t*)malloc(sizeof(uint32_t) * (total ? total : 1));
  if (!row_off || !pl_ids) {
    free(row_off);
    free(pl_ids);
    return EG3D_ERR_ARG;
  }
  size_t k = 0;
  row_off[0] = 0;
  for (size_t r = 0; r < rows.size(); r++) {
    for (uint32_t pl : rows[r]) pl_ids[k++] = pl;
    row_off[r + 1] = (uint32_t)k;
  }
  out->n_sets = (uint32_t)n_sets;
  out->row_off = row_off;
  out->pl_ids = pl_ids;
  return EG3D_OK;
}
