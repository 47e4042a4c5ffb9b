// examples/edge_matcher_refpoints.cpp — the reference's `edge_matcher` run, all three stages of
// edge_reconstruction_pipeline (pipelines.cpp:201-246), end to end in C++ over the C ABI
// (what src/edgegraph3d/edge_matcher.cpp:57-182 + pipelines.cpp do):
//
//   OpenMVG JSON (cameras + SfM points)  +  polyline graphs of every view
//     -> fundamental matrices            (edge_matcher.cpp:96 -> geometric_utilities.cpp:754-820): pairs of views
//                                        with >= 10 common SfM points get a matrix, the others none (exact rule);
//                                        the matrix is analytic from the cameras by default, or the build's own
//                                        least-median-of-squares estimate from the tracks with --estimate-F
//                                        (on host threads; with --estimate-F-device too, on the GPU:
//                                        eg3d_estimate_fundamental) (the reference's cv::findFundamentalMat(FM_LMEDS) is randomised OpenCV
//                                        code: not reproducible)
//     -> [pipeline 1] polyline matches of the similarity-graph matcher  (pipelines.cpp:219 -> :68-111)
//     -> [pipeline 2] polyline matches by closeness to reference points (pipelines.cpp:223 -> :113-158)
//                                        each match = one set of potentially compatible polylines, given in a
//                                        file (--sets1 / --sets2; the matchers themselves — Louvain clustering,
//                                        third party — are out of scope): find_new_3d_points_from_compatible_
//                                        polylines_expandallviews_parallel per match   GPU: eg3d_match_polyline_sets
//     -> [pipeline 3] plg_matching_from_refpoints (pipelines.cpp:227 -> :164)    GPU: eg3d_match_refpoints
//                                        the three results are concatenated in that order (pipelines.cpp:219-227;
//                                        the matches manager stays empty until pipeline 3 in the parallel build, so
//                                        the stages do not see each other's matches)
//     -> filter_3d_points_close_2d_array (pipelines.cpp:236)            host, over the concatenation
//     -> add_3dpoints_to_sfmd            (edge_matcher.cpp:158)         host
//     -> [./filter -e] gaussNewtonFiltering + observation filter + removeOutliers   GPU + host
//     -> output_sfm_data                 (edge_matcher.cpp:169)         OpenMVG JSON out
//
// Usage:
//   edge_matcher_refpoints --make-synthetic <config 0..4> <dir>      writes <dir>/input.json, <dir>/plgs.bin
//   edge_matcher_refpoints --make-plgs <plgs.bin> <edge image 0.png> <edge image 1.png> ...
//        builds the polyline graph of every binary edge image (view i = i-th image; SURVEY N2,
//        edge_matcher.cpp:84-94 convert_edge_images_to_optimized_polyline_graphs) and writes the container
//   edge_matcher_refpoints <dir>/input.json <dir>/plgs.bin <out.json> [--filter] [--estimate-F [--estimate-F-device]] [--all-pairs]
//                          [--sets1 <polyline matches of pipeline 1>] [--sets2 <... of pipeline 2> | --match2]
//                          [--refpoints-first]   (pipeline 3 first; pipelines 1-2 skip what it already matched)
//                          [--resident-sets]     (--match2 / --louvain / --communities: the matches stay on the device —
//                                                 eg3d_polyline_matches_device, eg3d_sets_from_communities_device — and the
//                                                 extractor takes them there, eg3d_match_polyline_items; same output)
//                          [--triangulate-refpoints]   (before matching: the input's own reference-point tracks through
//                                                 eg3d_triangulate, EG3D_TRI_FROM_SCRATCH — how many of them triangulate under
//                                                 these cameras, how many are too short or start from a degenerate pair)
//                          [--align camera_poses.txt]   (after the JSON, before --ply: the reference's coordinate_system_transform
//                                                 on the final cloud — a similarity fitted to the target camera centres, one
//                                                 "x y z" per camera; the cameras on the host, the points through
//                                                 eg3d_transform_points. The PLY file is then in the target frame)
//                          [--edges FILE [--edges-tol T]]   (the 3-D edge model of pipeline 3's cloud as an ASCII PLY line file that
//                                                 MeshLab or CloudCompare opens: the reference points matched once more, device
//                                                 only, on the run's context; the cloud replayed into the 3-D polyline graph
//                                                 there (eg3d_replay_device); the graph traced into chains, simplified with
//                                                 tolerance T in scene units (default 0.01, the reference's 3-D constant) and
//                                                 measured there (eg3d_edge_chains_device, K17); eg3d_host_write_ply_edges. With
//                                                 --align the vertices are those of the aligned cloud)
//                          [--compare FILE --compare-max-dist D]   (the final cloud — after --align when both are given — against the
//                                                 reference cloud in FILE, a PLY file or an OpenMVG JSON: accuracy (cloud ->
//                                                 FILE) and completeness (FILE -> cloud) as mean and median nearest distance
//                                                 within D, on the run's context: eg3d_cloud_index_build,
//                                                 eg3d_cloud_nearest_points, K18)
//                          [--ply FILE [--ply-images DIR/]]   (after the JSON: the final cloud as the reference's json_to_ply
//                                                 writes it, eg3d_host_write_ply — white, or with --ply-images coloured on the
//                                                 device from DIR/ + the base name of every view's path, PNG only. The final
//                                                 cloud of this tool is the SfM data on the host, so the colours come through
//                                                 eg3d_colour_points; a cloud that stays resident takes eg3d_colour_device)
//        a match file is text: "eg3d-polyline-sets 1", then "<n_sets> <n_views>", then one line per (set, view):
//        "<count> <polyline id> ..." with view-local ids (the reference's vector<set<ulong>> per match)
//        (--make-synthetic also writes <dir>/sets1.txt and <dir>/sets2.txt: the polylines of 3-D curves 0-2 / 3-5)
//
// The polyline graphs travel in a container file so that the expensive one-off construction from the
// edge images (--make-plgs) is separate from the matching run. Build (see tests/test_gpu_edge_cases.py):
//   g++ -std=c++17 -I include examples/edge_matcher_refpoints.cpp -Ledgegraph3d_amd -leg3d -leg3d_host ...
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "eg3d.h"
#include "eg3d_host.h"
#include "eg3d_sets_device.h"
#include "eg3d_triangulate.h"
#include "eg3d_colour.h"
#include "eg3d_host_colour.h"
#include "eg3d_host_transform.h"
#include "eg3d_transform.h"
#include "eg3d/edges.h"
#include "eg3d/nearest.hpp"

static int fail(const char* what) {
  std::fprintf(stderr, "edge_matcher_refpoints: %s (%s)\n", what, eg3d_last_error());
  return 1;
}

// ---- polyline match files (input of pipelines 1-2)
struct MatchSets {
  uint32_t n_sets = 0;
  std::vector<uint32_t> row_off{0}, ids;
};
static bool read_match_sets(const char* path, int n_views, MatchSets& m) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char tag[64];
  int ver = 0;
  unsigned ns = 0, nv = 0;
  bool ok = std::fscanf(f, "%63s %d %u %u", tag, &ver, &ns, &nv) == 4 && std::strcmp(tag, "eg3d-polyline-sets") == 0 && ver == 1 &&
            (int)nv == n_views && ns < (1u << 24);
  for (uint64_t r = 0; ok && r < (uint64_t)ns * nv; r++) {
    unsigned k = 0;
    ok = std::fscanf(f, "%u", &k) == 1 && k < (1u << 24);
    unsigned long prev = 0;
    for (unsigned i = 0; ok && i < k; i++) {
      unsigned long id = 0;
      ok = std::fscanf(f, "%lu", &id) == 1 && id <= 0xfffffffful && (i == 0 || id > prev);  // a set: ascending, no repeats
      prev = id;
      m.ids.push_back((uint32_t)id);
    }
    m.row_off.push_back((uint32_t)m.ids.size());
  }
  std::fclose(f);
  m.n_sets = ns;
  if (m.ids.empty()) m.ids.push_back(0);
  return ok;
}
static bool write_match_sets(const std::string& path, const eg3d_scene* sc, const uint32_t* curve, uint32_t c0, uint32_t c1) {
  FILE* f = std::fopen(path.c_str(), "w");
  if (!f) return false;
  std::fprintf(f, "eg3d-polyline-sets 1\n%u %d\n", c1 - c0, sc->n_views);
  for (uint32_t c = c0; c < c1; c++)
    for (int v = 0; v < sc->n_views; v++) {
      std::vector<uint32_t> ids;
      for (uint32_t p = sc->view_pl_off[v]; p < sc->view_pl_off[v + 1]; p++)
        if (curve[p] == c && sc->pl_valid[p] && sc->pl_vtx_off[p + 1] - sc->pl_vtx_off[p] >= 2) ids.push_back(p - sc->view_pl_off[v]);
      std::fprintf(f, "%zu", ids.size());
      for (uint32_t id : ids) std::fprintf(f, " %u", id);
      std::fprintf(f, "\n");
    }
  return std::fclose(f) == 0;
}

// ---- the clouds of the three stages, concatenated in stage order (host arrays in the eg3d_edgepoints layout)
struct Cloud {
  std::vector<float> X, xy;
  std::vector<uint64_t> off{0};
  std::vector<int32_t> view;
  std::vector<uint32_t> pl, seg, key;
  void append(const eg3d_edgepoints& e) {
    const uint64_t base = (uint64_t)view.size();
    X.insert(X.end(), e.X, e.X + 3 * e.n_points);
    key.insert(key.end(), e.key, e.key + 4 * e.n_points);
    for (uint64_t i = 0; i < e.n_points; i++) off.push_back(base + e.obs_off[i + 1]);
    view.insert(view.end(), e.obs_view, e.obs_view + e.n_obs);
    pl.insert(pl.end(), e.obs_pl, e.obs_pl + e.n_obs);
    seg.insert(seg.end(), e.obs_seg, e.obs_seg + e.n_obs);
    xy.insert(xy.end(), e.obs_xy, e.obs_xy + 2 * e.n_obs);
  }
  eg3d_edgepoints view_as_edgepoints() {
    eg3d_edgepoints e;
    std::memset(&e, 0, sizeof(e));
    e.n_points = off.size() - 1;
    e.n_obs = view.size();
    if (X.empty()) X.assign(3, 0.f);  // never hand out null arrays
    if (key.empty()) key.assign(4, 0);
    if (view.empty()) {
      view.assign(1, 0);
      pl.assign(1, 0);
      seg.assign(1, 0);
      xy.assign(2, 0.f);
    }
    e.X = X.data();
    e.obs_off = off.data();
    e.obs_view = view.data();
    e.obs_pl = pl.data();
    e.obs_seg = seg.data();
    e.obs_xy = xy.data();
    e.key = key.data();
    return e;
  }
};

static int make_synthetic(int cfg_index, const std::string& dir) {
  eg3d_synth_config cfg;
  eg3d_synth_default_config(&cfg, cfg_index);
  eg3d_synth* syn = eg3d_synth_create(&cfg);
  if (!syn) return fail("synthetic scene");
  const eg3d_scene* sc = eg3d_synth_scene(syn);
  const eg3d_seeds* sd = eg3d_synth_seeds(syn);
  const float* truth = eg3d_synth_seed_truth(syn);
  eg3d_sfm* sfm = eg3d_sfm_create(sc->n_views, sc->width, sc->height);
  for (int v = 0; v < sc->n_views; v++) {
    float f, px, py, R[9], C[3];
    eg3d_synth_camera(syn, v, &f, &px, &py, R, C);
    char name[64];
    std::snprintf(name, sizeof(name), "%04d.png", v);
    eg3d_sfm_set_camera(sfm, v, f, px, py, R, C, name);
  }
  for (uint32_t i = 0; i < sd->n_seeds; i++) {
    const uint32_t a = sd->trk_off[i], b = sd->trk_off[i + 1];
    eg3d_sfm_add_point(sfm, truth + 3 * i, (int)(b - a), sd->trk_view + a, sd->trk_xy + 2 * a);
  }
  int rc = eg3d_sfm_write_json(sfm, nullptr, (dir + "/input.json").c_str());
  if (rc == 0) rc = eg3d_plg_write((dir + "/plgs.bin").c_str(), sc);
  // stand-ins for the polyline matchers' output: the polylines generated from 3-D curves 0-2 (pipeline 1) and 3-5 (pipeline 2)
  const uint32_t nc = eg3d_synth_n_curves(syn);
  const uint32_t c1 = nc < 3 ? nc : 3, c2 = nc < 6 ? nc : 6;
  if (rc == 0 && !(write_match_sets(dir + "/sets1.txt", sc, eg3d_synth_polyline_curve(syn), 0, c1) &&
                   write_match_sets(dir + "/sets2.txt", sc, eg3d_synth_polyline_curve(syn), c1, c2)))
    rc = -1;
  std::printf("wrote %s/input.json (%d views, %u points) and %s/plgs.bin (%u polylines)\n", dir.c_str(), sc->n_views,
              sd->n_seeds, dir.c_str(), sc->view_pl_off[sc->n_views]);
  eg3d_sfm_destroy(sfm);
  eg3d_synth_destroy(syn);
  return rc == 0 ? 0 : fail("writing the synthetic inputs");
}

static int make_plgs(const char* out_path, int n, char** images) {
  std::vector<eg3d_plg_view> views((size_t)n);
  int W = 0, H = 0;
  // all views at once, on the host's cores (the views are independent)
  const int bad = eg3d_plg_build_views_from_png(images, n, &W, &H, views.data());
  if (bad != 0) {
    std::fprintf(stderr, "edge_matcher_refpoints: cannot build the polyline graph of %s (unreadable, or not the size of the first image)\n",
                 bad < 0 && -bad - 1 < n ? images[-bad - 1] : "?");
    return 1;
  }
  eg3d_plg* g = eg3d_plg_from_views(n, W, H, views.data());
  uint64_t n_pl = 0;
  for (auto& v : views) {
    n_pl += v.n_polylines;
    eg3d_plg_view_free(&v);
  }
  if (!g || eg3d_plg_write(out_path, eg3d_plg_scene(g)) != 0) return fail("writing the polyline graphs");
  std::printf("wrote %s: %d views of %dx%d, %llu polylines\n", out_path, n, W, H, (unsigned long long)n_pl);
  eg3d_plg_destroy(g);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && std::strcmp(argv[1], "--make-synthetic") == 0) return make_synthetic(std::atoi(argv[2]), argv[3]);
  if (argc >= 4 && std::strcmp(argv[1], "--make-plgs") == 0) return make_plgs(argv[2], argc - 3, argv + 3);
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s <input.json> <plgs.bin> <out.json> [--filter] [--estimate-F [--estimate-F-device]] [--all-pairs] [--resident-dedup] [--refpoints-first] [--resident-sets] [--triangulate-refpoints]\n", argv[0]);
    return 2;
  }
  bool do_filter = false, estimate_F = false, all_pairs = false, estimate_F_device = false;
  // --resident-dedup: every stage is matched device_only and deduplicated on the device against the claims of the stages
  // before it (eg3d_dedup_resident); only the survivors cross to the host. The output is the default path's, byte for byte.
  bool resident_dedup = false;
  const char* sets_path[2] = {nullptr, nullptr};
  for (int a = 4; a < argc; a++) {
    do_filter |= std::strcmp(argv[a], "--filter") == 0;
    estimate_F |= std::strcmp(argv[a], "--estimate-F") == 0;
    all_pairs |= std::strcmp(argv[a], "--all-pairs") == 0;  // analytic F for every pair, ignoring the 10-point rule
    estimate_F_device |= std::strcmp(argv[a], "--estimate-F-device") == 0;  // with --estimate-F: estimated on the device
    resident_dedup |= std::strcmp(argv[a], "--resident-dedup") == 0;
    if (std::strcmp(argv[a], "--sets1") == 0 && a + 1 < argc) sets_path[0] = argv[++a];
    else if (std::strcmp(argv[a], "--sets2") == 0 && a + 1 < argc) sets_path[1] = argv[++a];
  }
  // --refpoints-first: pipeline 3 runs FIRST and the extractor of pipelines 1-2 consults the matched intervals its cloud
  // leaves in the PLGMatchesManager (eg3d_match_polyline_sets_matched): 20 px samples and epipolar hits inside one start
  // nothing. The intervals come from the replay of pipeline 3's cloud — on the device and read there in place with
  // --resident-dedup (eg3d_replay_device), on the host otherwise (eg3d_host_replay_matches). Pipeline 3's cloud is then
  // the first of the run's. Without the switch: the reference's order 1, 2, 3 and the output of earlier builds.
  bool refpoints_first = false;
  for (int a = 4; a < argc; a++) refpoints_first |= std::strcmp(argv[a], "--refpoints-first") == 0;
  // --match2: pipeline 2's polyline matches are computed on the device (eg3d_match_polylines_closeness) where --sets2 reads them
  bool match2 = false;
  for (int a = 4; a < argc; a++) match2 |= std::strcmp(argv[a], "--match2") == 0;
  if (match2 && sets_path[1]) {
    std::fprintf(stderr, "--match2 and --sets2 exclude each other\n");
    return 2;
  }
  // --match1-graph <file>: the compatibility graph of pipeline 1's polyline matcher is built on the device
  // (eg3d_similarity_graph) and written as the reference writes it for its community detection (Grappolo: third-party, not
  // part of this example). --communities <file>: one community id per node of that graph, from whatever clustered the file;
  // the sets they make go through pipeline 1's extractor where --sets1 reads them. --louvain [communities-out]: the
  // library's own community detection runs on the graph instead (eg3d_detect_communities, on the device; no --communities
  // needed) and its ids are written to communities-out if one is named.
  const char* graph_path = nullptr;
  const char* communities_path = nullptr;
  const char* louvain_out = nullptr;
  bool louvain = false;
  for (int a = 4; a < argc; a++) {
    if (std::strcmp(argv[a], "--match1-graph") == 0 && a + 1 < argc) graph_path = argv[++a];
    else if (std::strcmp(argv[a], "--communities") == 0 && a + 1 < argc) communities_path = argv[++a];
    else if (std::strcmp(argv[a], "--louvain") == 0) {
      louvain = true;
      if (a + 1 < argc && std::strncmp(argv[a + 1], "--", 2) != 0) louvain_out = argv[++a];
    }
  }
  // --resident-sets: the polyline matches of --match2 and of --louvain / --communities are not rebuilt as host rows and
  // uploaded again: the extractor reads them where K9 / K13 leave them (include/eg3d_sets_device.h)
  bool resident_sets = false;
  for (int a = 4; a < argc; a++) resident_sets |= std::strcmp(argv[a], "--resident-sets") == 0;
  if ((communities_path || louvain) && sets_path[0]) {
    std::fprintf(stderr, "--communities / --louvain and --sets1 exclude each other\n");
    return 2;
  }
  if (communities_path && louvain) {
    std::fprintf(stderr, "--communities and --louvain exclude each other\n");
    return 2;
  }

  // wall time of every stage of the run, host stages included (--times prints them; stderr)
  bool print_times = false;
  for (int a = 4; a < argc; a++) print_times |= std::strcmp(argv[a], "--times") == 0;
  auto t_last = std::chrono::steady_clock::now();
  const auto t_begin = t_last;
  auto lap = [&](const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (print_times)
      std::fprintf(stderr, "[time] %-44s %9.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  // ---- inputs (edge_matcher.cpp:64-95)
  eg3d_sfm* sfm = eg3d_sfm_read_json(argv[1]);
  lap("read the OpenMVG JSON");
  if (!sfm) return fail("reading the OpenMVG file");
  eg3d_plg* plg = eg3d_plg_read(argv[2]);
  if (!plg) return fail("reading the polyline graphs");
  lap("read the polyline graphs");
  const int V = eg3d_sfm_n_views(sfm);
  eg3d_scene sc = *eg3d_plg_scene(plg);
  if (sc.n_views != V) return fail("views of the SfM file and of the polyline graphs differ");
  std::vector<double> F((size_t)V * V * 9);
  std::vector<uint8_t> Fv((size_t)V * V);
  if (estimate_F && estimate_F_device) {  // the same estimator family on the device (eg3d_estimate_fundamental, K12)
    eg3d_seeds tracks;
    eg3d_sfm_seeds(sfm, &tracks);
    eg3d_fund_params fp;
    std::memset(&fp, 0, sizeof fp);
    fp.struct_size = sizeof fp;
    fp.rng_seed = 0xE63D2018ull;
    eg3d_fund_stats fs;
    std::memset(&fs, 0, sizeof fs);
    fs.struct_size = sizeof fs;
    if (eg3d_estimate_fundamental(0, V, &tracks, &fp, F.data(), Fv.data(), nullptr, &fs) != EG3D_OK) return fail("fundamental matrices");
    if (fs.n_pairs_failed) std::printf("%u view pairs: estimate failed, left without a matrix\n", fs.n_pairs_failed);
  } else if (estimate_F) {
    const int bad = eg3d_sfm_estimate_F(sfm, 1, 0xE63D2018ull, F.data(), Fv.data(), nullptr);
    if (bad < 0) return fail("fundamental matrices");
    if (bad > 0) std::printf("%d view pairs: estimate failed, left without a matrix\n", bad);
  } else {
    if (eg3d_sfm_analytic_F(sfm, F.data(), Fv.data()) != 0) return fail("fundamental matrices");
    if (!all_pairs) {  // the reference's rule for which pairs have a matrix at all
      std::vector<uint8_t> rule((size_t)V * V);
      if (eg3d_sfm_estimate_F(sfm, 0, 0, nullptr, rule.data(), nullptr) < 0) return fail("fundamental matrices");
      for (size_t k = 0; k < rule.size(); k++) Fv[k] &= rule[k];
    }
  }
  size_t n_pairs = 0;
  for (uint8_t v : Fv) n_pairs += v;
  std::printf("fundamental matrices for %zu of %d ordered view pairs (%s)\n", n_pairs, V * (V - 1),
              estimate_F && estimate_F_device ? "least-median-of-squares estimate from the tracks, on the device"
              : estimate_F                    ? "least-median-of-squares estimate from the tracks, on the host"
                                              : "analytic from the cameras");
  sc.cam_P = eg3d_sfm_cam_P(sfm);
  sc.F = F.data();
  sc.F_valid = Fv.data();
  const uint64_t first_edgepoint = eg3d_sfm_n_points(sfm);

  lap("fundamental matrices");
  eg3d_ctx* ctx = nullptr;
  if (eg3d_create(&sc, 0, &ctx) != EG3D_OK) return fail("eg3d_create");
  lap("eg3d_create (incl. HIP runtime start-up)");
  Cloud all_stages;
  eg3d_stage_times tm;
  // --resident-dedup: the cloud the last match left in HBM -> dedup against the earlier stages' claims (the first stage
  // resets them; index_base = points matched so far) -> compaction -> copy of the survivors -> append
  uint64_t n_matched = 0;
  bool first_stage = true;
  auto append_resident = [&](const eg3d_edgepoints& matched) -> bool {
    eg3d_edgepoints surv;
    eg3d_dedup_stats st;
    st.struct_size = (uint32_t)sizeof(st);
    if (eg3d_dedup_resident(ctx, n_matched, first_stage ? 1 : 0, 0, 0.f, 0, -1, nullptr, 1, &surv, nullptr, &st) != EG3D_OK)
      return false;
    std::printf("  dedup on the device: %llu of %llu points kept (kernels %.3f ms, compaction %.3f ms, copy %.3f ms)\n",
                (unsigned long long)st.n_kept, (unsigned long long)st.n_points_in, st.ms_dedup, st.ms_compact, st.ms_copy);
    all_stages.append(surv);
    eg3d_free_edgepoints(&surv);
    n_matched += matched.n_points;
    first_stage = false;
    return true;
  };
  // ---- pipeline 3 on the GPU (pipelines.cpp:160-176, :227); with --refpoints-first it also leaves the matched intervals
  eg3d_seeds seeds;
  eg3d_sfm_seeds(sfm, &seeds);
  // --triangulate-refpoints (off by default): the reference points' own tracks through compute_3d_point_coords on the
  // device. Cameras and tracks that disagree show here, before any edge is matched.
  bool triangulate_refpoints = false;
  for (int a = 4; a < argc; a++) triangulate_refpoints |= std::strcmp(argv[a], "--triangulate-refpoints") == 0;
  if (triangulate_refpoints && seeds.n_seeds) {
    std::vector<float> Xt(3 * (size_t)seeds.n_seeds);
    std::vector<uint8_t> ok(seeds.n_seeds);
    eg3d_tri_stats ts;
    ts.struct_size = (uint32_t)sizeof(ts);
    if (eg3d_triangulate(ctx, EG3D_TRI_FROM_SCRATCH, seeds.n_seeds, seeds.trk_off, seeds.trk_view, seeds.trk_xy, nullptr, Xt.data(),
                         ok.data(), nullptr, &ts) != EG3D_OK)
      return fail("eg3d_triangulate");
    std::printf("reference-point tracks: %llu of %llu triangulate from their own observations (%llu short, %llu with a degenerate "
                "DLT pair; kernels %.3f ms)\n", (unsigned long long)ts.n_valid, (unsigned long long)ts.n_tracks,
                (unsigned long long)ts.n_short, (unsigned long long)ts.n_degenerate, ts.ms_kernel);
    lap("triangulation of the reference-point tracks");
  }
  eg3d_graph3d held_host;
  std::memset(&held_host, 0, sizeof(held_host));
  eg3d_matched_intervals held;
  std::memset(&held, 0, sizeof(held));
  auto run_pipeline3 = [&]() -> int {
    eg3d_edgepoints e;
    if (eg3d_match_refpoints(ctx, &seeds, 0, seeds.n_seeds, resident_dedup ? 1 : 0, &e, &tm) != EG3D_OK)
      return fail("eg3d_match_refpoints");
    std::printf("matched %u reference points -> %llu edge-points (%llu observations) in %.2f ms on the GPU\n", seeds.n_seeds,
                (unsigned long long)e.n_points, (unsigned long long)e.n_obs, tm.ms_total);
    lap(resident_dedup ? "eg3d_match_refpoints (first call, device only)" : "eg3d_match_refpoints (first call, with the copy)");
    if (refpoints_first) {
      held.struct_size = (uint32_t)sizeof(held);
      if (resident_dedup) {  // the whole cloud is still in HBM: replay it there, before the dedup compacts it
        eg3d_device_graph3d dg;
        eg3d_replay_stats rs;
        std::memset(&rs, 0, sizeof(rs));
        rs.struct_size = (uint32_t)sizeof(rs);
        if (eg3d_replay_device(ctx, nullptr, &dg, nullptr, &rs) != EG3D_OK) return fail("eg3d_replay_device");
        held.on_device = 1;
        held.n_scene_polylines = dg.n_scene_polylines;
        held.iv_off = dg.iv_off;
        held.iv_start_seg = dg.iv_start_seg;
        held.iv_start_xy = dg.iv_start_xy;
        held.iv_end_seg = dg.iv_end_seg;
        held.iv_end_xy = dg.iv_end_xy;
        std::printf("  matches manager: %llu matched intervals (replayed on the device)\n", (unsigned long long)rs.n_intervals);
      } else {
        if (eg3d_host_replay_matches(&sc, &e, &held_host) != 0) return fail("eg3d_host_replay_matches");
        held.n_scene_polylines = held_host.n_scene_polylines;
        held.iv_off = held_host.iv_off;
        held.iv_start_seg = held_host.iv_start_seg;
        held.iv_start_xy = held_host.iv_start_xy;
        held.iv_end_seg = held_host.iv_end_seg;
        held.iv_end_xy = held_host.iv_end_xy;
        std::printf("  matches manager: %llu matched intervals (replayed on the host)\n",
                    (unsigned long long)held_host.iv_off[held_host.n_scene_polylines]);
      }
      lap("replay of pipeline 3's cloud (matched intervals)");
    }
    if (resident_dedup) {
      if (!append_resident(e)) return fail("eg3d_dedup_resident");
    } else {
      all_stages.append(e);
    }
    eg3d_free_edgepoints(&e);
    lap("append to the run's cloud");
    return 0;
  };
  if (refpoints_first && run_pipeline3() != 0) return 1;
  // ---- pipelines 1 and 2 (pipelines.cpp:219-223): the extractor over the polyline matches of each stage, in
  // match order (one call takes all matches of a stage: eg3d_match_polyline_sets emits them set by set)
  for (int stage = 0; stage < 2; stage++) {
    const bool match1 = stage == 0 && (graph_path || communities_path || louvain);
    if (!sets_path[stage] && !(stage == 1 && match2) && !match1) continue;
    MatchSets ms;
    eg3d_device_polyline_sets dsets;
    bool on_device = false;
    if (match1) {  // pipelines.cpp:219 -> polyline_matcher.cpp:222-336; the community detection: --louvain, or the caller's
      eg3d_seeds rp;
      eg3d_sfm_seeds(sfm, &rp);
      eg3d_simgraph sg;
      eg3d_simgraph_stats st;
      st.struct_size = (uint32_t)sizeof(st);
      if (eg3d_similarity_graph(ctx, &rp, 0, rp.n_seeds, &sg, &st) != EG3D_OK) return fail("eg3d_similarity_graph");
      std::printf("pipeline 1: compatibility graph of %llu polylines, %llu edges\n", (unsigned long long)st.n_nodes,
                  (unsigned long long)st.n_edges);
      if (graph_path && eg3d_host_write_compat_graph(graph_path, &sg) != EG3D_OK) return fail("writing the compatibility graph");
      if (!communities_path && !louvain) {
        std::fprintf(stderr, "pipeline 1: wrote %s; --louvain clusters it on the device, or cluster it yourself (--communities <file> continues)\n", graph_path);
        eg3d_free_simgraph(&sg);
        continue;
      }
      int64_t* ids = nullptr;
      uint64_t n_ids = 0;
      eg3d_communities cm;
      std::memset(&cm, 0, sizeof(cm));
      if (louvain) {  // community_detection_interface.cpp:57-73, on the device
        eg3d_louvain_stats ls;
        ls.struct_size = (uint32_t)sizeof(ls);
        if (eg3d_detect_communities(ctx, &sg, nullptr, &cm, &ls) != EG3D_OK) return fail("eg3d_detect_communities");
        std::printf("pipeline 1: %u communities in %u phases and %u sweeps, modularity %.6f\n", ls.n_communities, ls.n_phases,
                    ls.n_sweeps, ls.modularity);
        if (louvain_out && eg3d_host_write_communities(louvain_out, cm.ids, cm.n_nodes) != EG3D_OK) return fail("writing the communities");
        ids = cm.ids;
        n_ids = cm.n_nodes;
      } else if (eg3d_host_read_communities(communities_path, &ids, &n_ids) != EG3D_OK) {
        return fail("reading the communities");
      }
      eg3d_polyline_sets cs;
      std::memset(&cs, 0, sizeof(cs));
      // (--resident-sets: K13 on the graph's nodes where the graph call left them; --louvain's ids are on the device too)
      const int rc = resident_sets ? eg3d_sets_from_communities_device(ctx, louvain ? nullptr : ids, n_ids, &dsets, nullptr)
                                   : eg3d_host_sets_from_communities(&sg, ids, n_ids, V, &cs);
      if (louvain) eg3d_free_communities(&cm);
      else eg3d_host_free(ids);
      eg3d_free_simgraph(&sg);
      if (rc != EG3D_OK) return fail("the communities do not fit the graph (one id per node)");
      if (resident_sets) {
        on_device = true;
        ms.n_sets = dsets.n_sets;
      } else {
        ms.n_sets = cs.n_sets;
        ms.row_off.assign(cs.row_off, cs.row_off + (size_t)cs.n_sets * V + 1);
        ms.ids.assign(cs.pl_ids, cs.pl_ids + ms.row_off.back());
        if (ms.ids.empty()) ms.ids.push_back(0);
        eg3d_host_free_polyline_sets(&cs);
      }
    } else if (stage == 1 && match2) {  // pipelines.cpp:118
      eg3d_seeds rp;
      eg3d_sfm_seeds(sfm, &rp);
      eg3d_polyline_matches pm;
      if (eg3d_match_polylines_closeness(ctx, &rp, 0, rp.n_seeds, &pm, nullptr) != EG3D_OK)
        return fail("eg3d_match_polylines_closeness");
      ms.n_sets = pm.n_sets;
      ms.row_off.assign(pm.row_off, pm.row_off + (size_t)pm.n_sets * V + 1);
      ms.ids.assign(pm.pl_ids, pm.pl_ids + ms.row_off.back());
      if (ms.ids.empty()) ms.ids.push_back(0);
      std::printf("pipeline 2: %u reference points accepted by the polyline matcher\n", pm.n_refpoints);
      eg3d_free_polyline_matches(&pm);
      if (resident_sets) {
        if (eg3d_polyline_matches_device(ctx, &dsets) != EG3D_OK) return fail("eg3d_polyline_matches_device");
        on_device = true;
      }
    } else if (!read_match_sets(sets_path[stage], V, ms)) return fail("reading a polyline match file");
    eg3d_polyline_sets ps;
    ps.n_sets = ms.n_sets;
    ps.row_off = ms.row_off.data();
    ps.pl_ids = ms.ids.data();
    eg3d_edgepoints e;
    if (on_device) {  // every item of the resident sets, as one range
      const eg3d_items_call all = {(uint32_t)sizeof(eg3d_items_call), 0u, (uint32_t)dsets.n_ids, 0u};
      if (eg3d_match_polyline_items(ctx, &dsets, &all, refpoints_first ? &held : nullptr, resident_dedup ? 1 : 0, &e, &tm) != EG3D_OK)
        return fail("eg3d_match_polyline_items");
    } else if (eg3d_match_polyline_sets_matched(ctx, &ps, 0, ms.n_sets, refpoints_first ? &held : nullptr, resident_dedup ? 1 : 0,
                                                &e, &tm) != EG3D_OK)
      return fail("eg3d_match_polyline_sets");
    std::printf("pipeline %d: %u polyline matches -> %llu edge-points (%llu observations) in %.2f ms on the GPU\n", stage + 1,
                ms.n_sets, (unsigned long long)e.n_points, (unsigned long long)e.n_obs, tm.ms_total);
    if (resident_dedup) {
      if (!append_resident(e)) return fail("eg3d_dedup_resident");
    } else {
      all_stages.append(e);
    }
    eg3d_free_edgepoints(&e);
  }
  if (!refpoints_first && run_pipeline3() != 0) return 1;
  eg3d_host_free_graph3d(&held_host);

  // ---- --edges: replay -> K17 on the run's context, while the reference points are still the SfM data's only points. The
  // model and the positions of the graph's nodes are kept; the file is written after --align, in the frame that gives.
  const char* edges_path = nullptr;
  float edges_tol = 0.01f;
  for (int a = 4; a + 1 < argc; a++) {
    if (std::strcmp(argv[a], "--edges") == 0) edges_path = argv[a + 1];
    if (std::strcmp(argv[a], "--edges-tol") == 0) edges_tol = (float)std::atof(argv[a + 1]);
  }
  eg3d_edge_chain_set edge_model;
  std::memset(&edge_model, 0, sizeof(edge_model));
  std::vector<float> edge_node_X;
  if (edges_path) {
    eg3d_edgepoints none;
    if (eg3d_match_refpoints(ctx, &seeds, 0, seeds.n_seeds, 1, &none, &tm) != EG3D_OK) return fail("eg3d_match_refpoints (--edges)");
    eg3d_free_edgepoints(&none);
    eg3d_graph3d g3;
    if (eg3d_replay_device(ctx, nullptr, nullptr, &g3, nullptr) != EG3D_OK) return fail("eg3d_replay_device (--edges)");
    edge_node_X.assign(g3.node_X, g3.node_X + 3 * g3.n_nodes);
    const unsigned long long n_nodes = g3.n_nodes, n_pl = g3.n_polylines;
    eg3d_free_graph3d(&g3);
    eg3d_edges_stats es;
    std::memset(&es, 0, sizeof(es));
    es.struct_size = (uint32_t)sizeof(es);
    if (eg3d_edge_chains_device(ctx, nullptr, edges_tol, 1, nullptr, &edge_model, &es) != EG3D_OK) {
      std::fprintf(stderr, "edge_matcher_refpoints: %s\n", eg3d_last_error());
      return fail("eg3d_edge_chains_device (--edges)");
    }
    std::printf("edge model: %llu nodes, %llu polylines -> %llu chains (%llu rings, %llu loops dropped), longest %llu vertices; %llu "
                "vertices -> %llu kept at tolerance %g (trace %.3f ms, simplify %.3f ms, copy %.3f ms)\n", n_nodes, n_pl,
                (unsigned long long)es.n_chains, (unsigned long long)es.n_rings, (unsigned long long)es.n_loops_dropped,
                (unsigned long long)es.longest_chain, (unsigned long long)es.n_vertices_in, (unsigned long long)es.n_vertices_kept,
                edges_tol, es.ms_trace, es.ms_simplify, es.ms_copy);
    lap("3-D edge model (match, replay and K17 on the GPU)");
  }
  eg3d_edgepoints pts = all_stages.view_as_edgepoints();

  // ---- filter_3d_points_close_2d_array + add_3dpoints_to_sfmd (pipelines.cpp:236-239; edge_matcher.cpp:150-158)
  std::vector<uint8_t> keep(pts.n_points ? pts.n_points : 1);
  if (resident_dedup)
    std::fill(keep.begin(), keep.end(), (uint8_t)1);  // the cloud holds survivors only
  else if (eg3d_host_filter_close_2d(V, sc.width, sc.height, &pts, keep.data()) != 0)
    return fail("dedup");
  lap("3 px de-duplication (filter_3d_points_close_2d_array)");
  uint64_t kept = 0;
  for (uint64_t i = 0; i < pts.n_points; i++) kept += keep[i];
  if (eg3d_sfm_add_edgepoints(sfm, &pts, keep.data()) != 0) return fail("adding the edge-points");
  lap("add_3dpoints_to_sfmd");
  std::printf("kept %llu edge-points after the 3 px de-duplication; SfM data now holds %llu points\n",
              (unsigned long long)kept, (unsigned long long)eg3d_sfm_n_points(sfm));

  // ---- ./filter -e (src/utils/filter.cpp:48-115): Gauss-Newton refinement + observation-count filter
  if (do_filter) {
    eg3d_seeds all;
    eg3d_sfm_seeds(sfm, &all);
    const uint64_t n = all.n_seeds;
    std::vector<float> Xo(3 * n);
    std::vector<uint8_t> inl(n ? n : 1);
    if (eg3d_gn_filter(ctx, eg3d_sfm_points(sfm), all.trk_off, all.trk_view, all.trk_xy, n, 2.25f, 0, Xo.data(),
                       inl.data(), nullptr) != EG3D_OK)
      return fail("eg3d_gn_filter");
    eg3d_sfm_set_point_coords(sfm, Xo.data());   // inliers moved, outliers returned unchanged
    const int thr = eg3d_host_observation_filter(V, all.trk_off, n, first_edgepoint, -1, inl.data());
    uint64_t n_in = 0;
    for (uint64_t i = 0; i < n; i++) n_in += inl[i];
    eg3d_sfm_remove_outliers(sfm, inl.data());
    std::printf("filter: %llu of %llu points kept (Gauss-Newton mse < 2.25, more than %d observations)\n",
                (unsigned long long)n_in, (unsigned long long)n, thr);
    lap("filter (Gauss-Newton on the GPU + observation count)");
  }

  // ---- output_sfm_data (edge_matcher.cpp:169)
  if (eg3d_sfm_write_json(sfm, argv[1], argv[3]) != 0) return fail("writing the output");
  lap("write the OpenMVG JSON");
  std::printf("wrote %s (%llu points)\n", argv[3], (unsigned long long)eg3d_sfm_n_points(sfm));

  // ---- coordinate_system_transform (src/coordinate_system_transform/) on the final cloud: the fit on the host, the
  // cameras on the host, the points through K16 on the run's context (eg3d_transform_points: the final cloud of this tool
  // is the SfM data on the host; a cloud that stays resident takes eg3d_transform_device). The JSON above is written in
  // the reconstruction's own frame; what follows — the PLY file — is in the target frame.
  const char* align_path = nullptr;
  std::vector<double> align_T;  // (kept for --edges)
  for (int a = 4; a + 1 < argc; a++)
    if (std::strcmp(argv[a], "--align") == 0) align_path = argv[a + 1];
  if (align_path) {
    std::vector<double> target((size_t)V * 3), centres((size_t)V * 3), T(16);
    std::vector<uint8_t> null_mask((size_t)V);
    if (eg3d_host_read_camera_poses(align_path, V, target.data()) != 0) return fail("reading the target camera centres (--align)");
    eg3d_sfm_camera_centres(sfm, centres.data(), null_mask.data());
    eg3d_similarity_stats fit;
    fit.struct_size = sizeof(fit);
    if (eg3d_host_similarity_fit(V, centres.data(), target.data(), null_mask.data(), T.data(), &fit) != 0)
      return fail("fitting the similarity to the target camera centres (--align)");
    auto error = [&]() {
      std::vector<double> c64((size_t)V * 3);
      eg3d_sfm_camera_centres(sfm, c64.data(), nullptr);
      std::vector<float> c32(c64.begin(), c64.end());
      float e = 0;
      eg3d_host_camera_errors(V, c32.data(), null_mask.data(), target.data(), &e);
      return e;
    };
    align_T = T;
    const float before = error();
    const uint64_t n = eg3d_sfm_n_points(sfm);
    std::vector<float> Xa(3 * (size_t)n);
    eg3d_transform_stats ts;
    ts.struct_size = sizeof(ts);
    if (eg3d_transform_points(ctx, T.data(), eg3d_sfm_points(sfm), n, Xa.data(), &ts) != EG3D_OK) return fail("eg3d_transform_points");
    if (eg3d_sfm_apply_transform(sfm, T.data(), EG3D_SFM_TRANSFORM_CAMERAS) != 0) return fail("transforming the cameras (--align)");
    if (n) eg3d_sfm_set_point_coords(sfm, Xa.data());
    std::printf("align: %u cameras, scale %g%s; camera position errors before: %g, after: %g; %llu points, %llu not finite\n", fit.n_used,
                fit.scale, fit.reflection ? " (mirrored target)" : "", before, error(), (unsigned long long)ts.n_transformed,
                (unsigned long long)ts.n_nonfinite);
    lap("align to the target camera centres (fit on the host, points on the GPU)");
  }

  // ---- --edges: the line model, its vertices in the aligned frame when there is one (a node's position is its point's)
  if (edges_path) {
    if (!align_T.empty() && !edge_node_X.empty() &&
        eg3d_transform_points(ctx, align_T.data(), edge_node_X.data(), edge_node_X.size() / 3, edge_node_X.data(), nullptr) != EG3D_OK)
      return fail("eg3d_transform_points (--edges)");
    if (eg3d_host_write_ply_edges(edges_path, &edge_model, edge_node_X.data()) != 0) return fail("writing the PLY edge file");
    std::printf("wrote %s (%llu chains, %llu vertices kept%s)\n", edges_path, (unsigned long long)edge_model.n_chains,
                (unsigned long long)edge_model.n_kept, align_T.empty() ? "" : ", aligned");
    eg3d_free_edge_chains(&edge_model);
    lap("write the PLY edge file");
  }

  // ---- --compare: the final cloud against a reference cloud, both directions, on the run's context (K18)
  const char* compare_path = nullptr;
  float compare_md = 0.f;
  for (int a = 4; a + 1 < argc; a++) {
    if (std::strcmp(argv[a], "--compare") == 0) compare_path = argv[a + 1];
    if (std::strcmp(argv[a], "--compare-max-dist") == 0) compare_md = (float)std::atof(argv[a + 1]);
  }
  if (compare_path) {
    if (!(compare_md > 0.f)) return fail("--compare needs --compare-max-dist D with D > 0");
    std::vector<float> ref;
    const size_t len = std::strlen(compare_path);
    if (len > 5 && std::strcmp(compare_path + len - 5, ".json") == 0) {
      eg3d_sfm* other = eg3d_sfm_read_json(compare_path);
      if (!other) return fail("reading the reference cloud (--compare)");
      if (eg3d_sfm_n_points(other)) ref.assign(eg3d_sfm_points(other), eg3d_sfm_points(other) + 3 * eg3d_sfm_n_points(other));
      eg3d_sfm_destroy(other);
    } else {
      float* p = nullptr;
      uint64_t np = 0;
      if (eg3d_host_read_ply_points(compare_path, &p, &np) != 0) {
        std::fprintf(stderr, "%s\n", eg3d_host_nearest_last_error());
        return fail("reading the reference cloud (--compare)");
      }
      ref.assign(p, p + 3 * np);
      eg3d_host_free_points(p);
    }
    const uint64_t n = eg3d_sfm_n_points(sfm), m = ref.size() / 3;
    eg3d_nearest_stats side[2];
    eg3d_cloud_index* index[2] = {nullptr, nullptr};
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {  // 0: accuracy (cloud -> reference), 1: completeness (reference -> cloud)
      std::memset(&side[k], 0, sizeof(side[k]));
      side[k].struct_size = sizeof(side[k]);
      const float* R = k == 0 ? ref.data() : eg3d_sfm_points(sfm);
      const float* Q = k == 0 ? eg3d_sfm_points(sfm) : ref.data();
      ok = eg3d_cloud_index_build(ctx, R, k == 0 ? m : n, nullptr, compare_md, &index[k], nullptr) == EG3D_OK &&
           eg3d_cloud_nearest_points(ctx, Q, k == 0 ? n : m, nullptr, index[k], compare_md, nullptr, nullptr, &side[k]) == EG3D_OK;
    }
    eg3d_cloud_index_free(index[0]);
    eg3d_cloud_index_free(index[1]);
    if (!ok) return fail("eg3d_cloud_nearest_points (--compare)");
    for (int k = 0; k < 2; k++) {
      const double w = (double)side[k].n_within;
      std::printf("compare: %s: %llu points, %llu within %g, mean %.9g, median %.9g\n", k == 0 ? "accuracy" : "completeness",
                  (unsigned long long)side[k].n_queries, (unsigned long long)side[k].n_within, (double)compare_md,
                  w ? (double)side[k].sum_q32 * (double)compare_md / 4294967296.0 / w : 0.0, w ? std::sqrt((double)side[k].median_d2) : 0.0);
    }
    lap("compare with the reference cloud (K18, both directions)");
  }

  // ---- json_to_ply (src/utils/json_to_ply.cpp) on the final cloud
  const char* ply_path = nullptr;
  const char* ply_images = nullptr;
  for (int a = 4; a + 1 < argc; a++) {
    if (std::strcmp(argv[a], "--ply") == 0) ply_path = argv[a + 1];
    if (std::strcmp(argv[a], "--ply-images") == 0) ply_images = argv[a + 1];
  }
  if (ply_path) {
    eg3d_seeds all;
    eg3d_sfm_seeds(sfm, &all);
    const uint64_t n = all.n_seeds;
    std::vector<uint8_t> rgb;
    if (ply_images) {
      std::vector<int32_t> iw((size_t)V), ih((size_t)V);
      std::vector<uint8_t*> img((size_t)V, nullptr);
      bool ok = true;
      for (int v = 0; v < V && ok; v++) {
        const std::string name = eg3d_sfm_image_path(sfm, v);
        const std::string path = std::string(ply_images) + name.substr(name.find_last_of("/\\") + 1);
        int w = 0, h = 0;
        ok = eg3d_host_png_read_rgb(path.c_str(), &w, &h, &img[(size_t)v]) == 0;
        if (!ok) std::fprintf(stderr, "edge_matcher_refpoints: cannot read %s as a PNG image\n", path.c_str());
        iw[(size_t)v] = w;
        ih[(size_t)v] = h;
      }
      rgb.resize(3 * n + 1);
      eg3d_colour_stats cs;
      cs.struct_size = (uint32_t)sizeof(cs);
      ok = ok && eg3d_upload_images(ctx, V, iw.data(), ih.data(), img.data()) == EG3D_OK &&
           eg3d_colour_points(ctx, n, all.trk_off, all.trk_view, all.trk_xy, nullptr, rgb.data(), nullptr, &cs) == EG3D_OK;
      for (uint8_t* p : img) eg3d_host_free(p);
      if (!ok) return fail("colouring the final cloud");
      std::printf("coloured %llu points from %llu observations on the GPU (%llu without observations)\n",
                  (unsigned long long)cs.n_coloured, (unsigned long long)cs.n_obs_sampled, (unsigned long long)cs.n_empty);
      lap("colours of the final cloud (eg3d_colour_points)");
    }
    if (eg3d_host_write_ply(ply_path, n, eg3d_sfm_points(sfm), ply_images ? rgb.data() : nullptr, nullptr) != 0)
      return fail("writing the PLY file");
    std::printf("wrote %s (%llu points%s)\n", ply_path, (unsigned long long)n, ply_images ? ", coloured" : "");
  }
  if (print_times)
    std::fprintf(stderr, "[time] %-44s %9.2f ms\n", "whole run", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  eg3d_destroy(ctx);
  eg3d_plg_destroy(plg);
  eg3d_sfm_destroy(sfm);
  return 0;
}
