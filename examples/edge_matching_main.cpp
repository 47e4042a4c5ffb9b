// examples/edge_matching_main.cpp — the reference's top-level call, edge_matching(emip) (edge_matcher.cpp:60-146), through
// the shim of include/eg3d_edge_matcher.hpp: edge images + OpenMVG JSON in, OpenMVG JSON with the edge-points out.
//   edge_matching_main <images folder> <edge images folder> <input.json> <out folder/> <output.json> [--estimate-F [--estimate-F-device]]
//                      [--detect-edges LOW HIGH [--edge-smooth N]]
// (--estimate-F: the fundamental matrices are estimated from the tracks, on host threads; with --estimate-F-device on the GPU)
// (--detect-edges LOW HIGH: the edge maps are detected on the GPU from the PNG photographs of <images folder> — gradient
//  magnitude above LOW, connected to one above HIGH, after N smoothing passes (default 1) — and written to <out folder/>;
//  <edge images folder> is not opened)
// (the longer examples/edge_matcher_refpoints.cpp drives the same steps one by one over the C ABI, with the polyline
// graphs in a container file and the polyline matches of pipelines 1-2 from files)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eg3d_edge_matcher.hpp"

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr,
                 "usage: %s <images folder> <edge images folder> <input.json> <out folder/> <output.json> [--estimate-F [--estimate-F-device]] "
                 "[--detect-edges LOW HIGH [--edge-smooth N]]\n",
                 argv[0]);
    return 2;
  }
  eg3d_ref::edge_matcher_input_params emip;
  std::memset(&emip, 0, sizeof(emip));
  emip.images_folder = argv[1];
  emip.input_edges_folder = argv[2];
  emip.sfm_data_file = argv[3];
  emip.em_out_folder = argv[4];
  emip.output_json = argv[5];
  eg3d_ref::EdgeMatchingOptions& opt = eg3d_ref::edge_matching_options();
  for (int a = 6; a < argc; a++) {
    if (std::strcmp(argv[a], "--estimate-F") == 0) opt.estimate_F = true;
    if (std::strcmp(argv[a], "--estimate-F-device") == 0) opt.estimate_F_device = true;
    if (std::strcmp(argv[a], "--detect-edges") == 0) {
      if (a + 2 >= argc) {
        std::fprintf(stderr, "--detect-edges needs LOW and HIGH\n");
        return 2;
      }
      opt.detect_edges = true;
      opt.edge_low = std::atoi(argv[a + 1]);
      opt.edge_high = std::atoi(argv[a + 2]);
      a += 2;
    } else if (std::strcmp(argv[a], "--edge-smooth") == 0) {
      if (a + 1 >= argc) {
        std::fprintf(stderr, "--edge-smooth needs N\n");
        return 2;
      }
      opt.edge_smooth_passes = std::atoi(argv[++a]);
    }
  }
  const eg3d_ref::EdgeMatchingOptions& o = opt;
  std::printf("fundamental matrices: %s\n", o.estimate_F && o.estimate_F_device ? "least-median-of-squares estimate from the tracks, on the device"
                                            : o.estimate_F                      ? "least-median-of-squares estimate from the tracks, on the host"
                                                                                : "analytic from the cameras");
  if (o.detect_edges)
    std::printf("edge maps: detected on the device from the photographs (low %d, high %d, %d smoothing passes)\n", o.edge_low, o.edge_high,
                o.edge_smooth_passes);
  try {
    const int rc = eg3d_ref::edge_matching(emip);
    std::printf("edge_matching returned %d\n", rc);
    return rc == 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "edge_matching failed: %s\n", e.what());
    return 1;
  }
}
