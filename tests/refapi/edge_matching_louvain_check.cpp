// GPU check of edge_matching() (include/eg3d_edge_matcher.hpp) with pipeline 1's community detection:
//   edge_matching_louvain_check <edge images folder> <input.json> <out folder/> <graph file> <communities file>
// First call: run_pipeline1 without a communities file and without pipeline1_detect_communities, as before this option
// existed: the stage stays skipped. Second call: pipeline1_detect_communities, the graph and the communities written to the
// two files. Then the compatibility graph of the same inputs once more, built the way edge_matching builds it, and printed
// for tests/test_gpu_louvain.py: "<rc> <skipped_pipelines>" of both calls, then n_nodes, adj_off, adj_node and the bits of
// adj_w, one line each.
#include <cstdio>
#include <cstring>

#include "eg3d_edge_matcher.hpp"

using namespace eg3d_ref;

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  try {
    edge_matcher_input_params emip;
    std::memset(&emip, 0, sizeof(emip));
    emip.input_edges_folder = argv[1];
    emip.sfm_data_file = argv[2];
    emip.em_out_folder = argv[3];
    const std::string out_json = std::string(argv[3]) + "out.json";
    emip.output_json = const_cast<char*>(out_json.c_str());
    EdgeMatchingOptions& o = edge_matching_options();
    o.require_images = false;
    o.quiet = true;
    o.run_pipeline1 = true;
    {
      SfMData sfm = read_sfm_data(argv[2]);
      const int rc = edge_matching(emip, sfm);
      std::printf("%d %d\n", rc, o.skipped_pipelines);
    }
    o.pipeline1_detect_communities = true;
    o.pipeline1_graph_file = argv[4];
    o.pipeline1_communities_out_file = argv[5];
    {
      SfMData sfm = read_sfm_data(argv[2]);
      const int rc = edge_matching(emip, sfm);
      std::printf("%d %d\n", rc, o.skipped_pipelines);
    }
    SfMData sfm = read_sfm_data(argv[2]);
    std::vector<PolyLineGraph2D> plgs;
    int w = 0, h = 0;
    if (!convert_edge_images_to_optimized_polyline_graphs(argv[1], sfm, plgs, w, h)) return 3;
    FundamentalMatrices F;
    if (!generate_all_fundamental_matrices(argv[2], sfm, F)) return 4;
    PLGEdgeManager em(sfm, F, plgs, 10.0f, 3.0f, 0);
    if (em.last_status() != EG3D_OK) return 5;
    const auto graph = polyline_matching_similarity_graph_before_communities(sfm, &em);
    const eg3d_simgraph& g = graph.raw;
    std::printf("%u\n", g.n_nodes);
    for (uint32_t i = 0; i <= g.n_nodes; i++) std::printf("%u ", g.adj_off[i]);
    std::printf("\n");
    for (uint32_t k = 0; k < g.adj_off[g.n_nodes]; k++) std::printf("%u ", g.adj_node[k]);
    std::printf("\n");
    for (uint32_t k = 0; k < g.adj_off[g.n_nodes]; k++) {
      uint32_t bits;
      std::memcpy(&bits, &g.adj_w[k], 4);
      std::printf("%u ", bits);
    }
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "failed: %s\n", e.what());
    return 1;
  }
  return 0;
}
