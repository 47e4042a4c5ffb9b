// examples/edge_matching_main.cpp — the reference's top-level call, edge_matching(emip) (edge_matcher.cpp:60-146), through
// the shim of include/eg3d_edge_matcher.hpp: edge images + OpenMVG JSON in, OpenMVG JSON with the edge-points out.
//   edge_matching_main <images folder> <edge images folder> <input.json> <out folder/> <output.json> [--estimate-F [--estimate-F-device]]
// (--estimate-F: the fundamental matrices are estimated from the tracks, on host threads; with --estimate-F-device on the GPU)
// (the longer examples/edge_matcher_refpoints.cpp drives the same steps one by one over the C ABI, with the polyline
// graphs in a container file and the polyline matches of pipelines 1-2 from files)
#include <cstdio>
#include <cstring>

#include "eg3d_edge_matcher.hpp"

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s <images folder> <edge images folder> <input.json> <out folder/> <output.json> [--estimate-F [--estimate-F-device]]\n", argv[0]);
    return 2;
  }
  eg3d_ref::edge_matcher_input_params emip;
  std::memset(&emip, 0, sizeof(emip));
  emip.images_folder = argv[1];
  emip.input_edges_folder = argv[2];
  emip.sfm_data_file = argv[3];
  emip.em_out_folder = argv[4];
  emip.output_json = argv[5];
  for (int a = 6; a < argc; a++) {
    if (std::strcmp(argv[a], "--estimate-F") == 0) eg3d_ref::edge_matching_options().estimate_F = true;
    if (std::strcmp(argv[a], "--estimate-F-device") == 0) eg3d_ref::edge_matching_options().estimate_F_device = true;
  }
  const eg3d_ref::EdgeMatchingOptions& o = eg3d_ref::edge_matching_options();
  std::printf("fundamental matrices: %s\n", o.estimate_F && o.estimate_F_device ? "least-median-of-squares estimate from the tracks, on the device"
                                            : o.estimate_F                      ? "least-median-of-squares estimate from the tracks, on the host"
                                                                                : "analytic from the cameras");
  try {
    const int rc = eg3d_ref::edge_matching(emip);
    std::printf("edge_matching returned %d\n", rc);
    return rc == 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "edge_matching failed: %s\n", e.what());
    return 1;
  }
}
