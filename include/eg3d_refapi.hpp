// eg3d_refapi.hpp — header-only C++ shim that offers the reference's call surface for the hot
// path on top of the C ABI (include/eg3d.h), so reference-side host code can switch with a
// type alias and without touching its callers. It mirrors, name for name:
//
//   plg_matching_from_refpoints_parallel(sfmd, em, cm, plgmm)
//        include/edgegraph3d/matching/plg_matching/plg_matching_from_refpoints.hpp:53,55
//   PLGEdgeManager(imgs, sfmd, F, plgs, 10, 3)  +  detect_nearby_intersections_and_correspondences_plgp(int)
//        include/edgegraph3d/edge_managers/plg_edge_manager.hpp:74,80
//   find_new_3d_points_from_compatible_polylines_expandallviews_parallel(sfmd, ..., potentially_compatible_polylines, ...)
//        include/edgegraph3d/matching/plg_matching/polyline_matching.hpp:55-56
//   gaussNewtonFiltering(SfMData&, std::vector<bool>&, float)
//        include/edgegraph3d/filtering/gauss_newton.hpp:20
//   filter(SfMData&, int[, float][, int])   (4 overloads)
//        include/edgegraph3d/filtering/outliers_filtering.hpp:18-21
//   EdgeManager (abstract), PLGPConsensusManager (abstract), PLGPCM3ViewsPLGFollowing
//        include/edgegraph3d/edge_managers/edge_manager.hpp:54-73,
//        include/edgegraph3d/matching/consensus_manager/plgp_consensus_manager.hpp:56-72, plgpcm_3views_plg_following.hpp:52-60
// so that the reference's call sites compile unchanged against these types:
//   pipelines.cpp:164        plg_matching_from_refpoints_parallel(sfmd, em, cm, plgmm)
//   outliers_filtering.cpp:39 gaussNewtonFiltering(sfm_data_, inliers, gn_max_mse)
//   edge_matcher.cpp:132      filter(sfmd, first_edgepoint)
// (include/eg3d_refapi_glm.hpp converts the reference's glm-typed structures to and from the ones below.)
//
// Types: the structs below have the fields of the reference types the path reads
// (SfMData.h:16-30, types_reconstructor.hpp:68-82, polyline_graph_2d.hpp:85-119,222-294) with
// plain float arrays in place of glm/cv::Mat. Error behaviour: the reference's functions have no error channel
// (an empty result means "no edges found"), so a FAILURE of the GPU path must not look like one — the functions with
// the reference's exact signatures throw eg3d_ref::Eg3dError (status + eg3d_last_error() text); the manager's own
// methods (match_all, match_polyline_set, detect_...) return an empty result and keep the status in last_status().
#pragma once
#include <array>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "eg3d.h"
#include "eg3d_host.h" /* eg3d_host_replay_matches (libeg3d_host.so) */
#include "eg3d_host_accumulate.h" /* eg3d_host_replay_state_* (libeg3d_host.so): PLGMatchesManager::set_accumulate */
#include "eg3d_triangulate.h" /* eg3d_triangulate (K14): compute_3d_point_coords */

namespace eg3d_ref {

struct vec2 {
  float x, y;
};
struct vec3 {
  float x, y, z;
};
struct CameraType {
  float cameraMatrix[4][4];  // cameraMatrix[r][c], last row zero (OpenMvgParser.cpp:107-125)
};
struct SfMData {  // SfMData.h:16-30
  int numPoints_ = 0, numCameras_ = 0;
  std::vector<vec3> points_;
  std::vector<CameraType> camerasList_;
  std::vector<std::string> camerasPaths_;
  std::vector<std::vector<int>> camViewingPointN_;
  std::vector<std::vector<int>> pointsVisibleFromCamN_;
  std::vector<std::vector<vec2>> point2DoncamViewingPoint_;
  int imageWidth_ = 0, imageHeight_ = 0;
};
// A failure of the GPU path behind a function that has the reference's signature (and therefore no status to return)
struct Eg3dError : std::runtime_error {
  int status;
  Eg3dError(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};
// thrown by the legacy (segment-based) virtuals of EdgeManager, as the reference's PLGEdgeManager does
// (plg_edge_manager.cpp:361-378: `throw new NotImplementedException()`)
struct NotImplementedException : std::logic_error {
  NotImplementedException() : std::logic_error("Function not yet implemented") {}
};
struct PolyLineGraph2D {
  struct polyline {
    unsigned long start = 0, end = 0;
    std::vector<vec2> polyline_coords;
  };
  struct pl_point {
    unsigned long segment_index;
    vec2 coords;
  };
  struct plg_point {
    unsigned long polyline_id;
    pl_point plp;
  };
  struct pl_interval {  // polyline::pl_interval (polyline_graph_2d.hpp): a matched stretch of one polyline
    pl_point start, end;
  };
  std::vector<polyline> polylines;
  std::vector<vec2> nodes_coords;
  // PolyLineGraph2D::is_valid_polyline (polyline_graph_2d.cpp:1141-1147)
  bool is_valid_polyline(size_t id) const {
    const polyline& p = polylines[id];
    auto valid_node = [&](unsigned long n) {
      return n < nodes_coords.size() && nodes_coords[n].x != -1 && nodes_coords[n].y != -1;
    };
    if (!valid_node(p.start) || !valid_node(p.end) || p.polyline_coords.size() <= 1) return false;
    const vec2 &a = nodes_coords[p.start], &b = nodes_coords[p.end];
    const vec2 &f = p.polyline_coords.front(), &l = p.polyline_coords.back();
    return a.x == f.x && a.y == f.y && b.x == l.x && b.y == l.y;
  }
};
using FundamentalMatrices = std::vector<std::vector<std::array<double, 9>>>;  // F[i][j]; all-zero => invalid (1x1 Mat)

using new_3dpoint_plgp_matches = std::tuple<vec3, std::vector<PolyLineGraph2D::plg_point>, std::vector<int>>;

// PLGMatchesManager of the path (plg_matches_manager.hpp:99-141): what add_matched_3dpolyline leaves
// behind — the 3-D polyline graph (get_plg3d()) and the matched 2-D intervals — rebuilt by
// eg3d_host_replay_matches (include/eg3d_host.h, row a17) from the ordered output of a run.
class PLGMatchesManager {
 public:
  PLGMatchesManager() { std::memset(&g_, 0, sizeof(g_)); }
  ~PLGMatchesManager() {
    eg3d_host_free_graph3d(&g_);
    eg3d_host_replay_state_destroy(state_);
  }
  PLGMatchesManager(const PLGMatchesManager&) = delete;
  PLGMatchesManager& operator=(const PLGMatchesManager&) = delete;
  const eg3d_graph3d& get_plg3d() const { return g_; }
  // matched_polyline_intervals[plg_id][polyline_id] as [begin, end) into the iv_* arrays of get_plg3d()
  std::pair<uint64_t, uint64_t> matched_intervals(const eg3d_scene& sc, int plg_id, unsigned long polyline_id) const {
    const uint64_t gpl = sc.view_pl_off[plg_id] + polyline_id;
    return {g_.iv_off[gpl], g_.iv_off[gpl + 1]};
  }
  // The intervals as the table eg3d_match_polyline_sets_matched / eg3d_host_is_matched take (host arrays of get_plg3d();
  // valid until the next replay). struct_size == 0: nothing has been replayed yet — no manager.
  eg3d_matched_intervals matched_table() const {
    eg3d_matched_intervals m;
    std::memset(&m, 0, sizeof(m));
    if (!g_.iv_off) return m;
    m.struct_size = (uint32_t)sizeof(m);
    m.n_scene_polylines = g_.n_scene_polylines;
    m.iv_off = g_.iv_off;
    m.iv_start_seg = g_.iv_start_seg;
    m.iv_start_xy = g_.iv_start_xy;
    m.iv_end_seg = g_.iv_end_seg;
    m.iv_end_xy = g_.iv_end_xy;
    return m;
  }
  // PLGMatchesManager::is_matched (plg_matches_manager.hpp:131, plg_matches_manager.cpp:54-85) against what the last
  // replay left: true + the containing interval. The rule is the library's (eg3d_host_is_matched: the one the kernels
  // of eg3d_match_polyline_sets_matched apply, quirks included). Throws Eg3dError for a point that is not on a segment
  // of its polyline.
  bool is_matched(const int plg_id, const unsigned long polyline_id, const PolyLineGraph2D::pl_point& plp,
                  PolyLineGraph2D::pl_interval& pli_containing_point) const {
    const eg3d_matched_intervals m = matched_table();
    if (!m.struct_size) return false;
    const int32_t view = plg_id;
    const uint32_t pl = (uint32_t)polyline_id, seg = (uint32_t)plp.segment_index;
    const float xy[2] = {plp.coords.x, plp.coords.y};
    int64_t k = -1;
    const int rc = polyline_id > 0xfffffffful || plp.segment_index > 0xfffffffful
                       ? -1
                       : eg3d_host_is_matched(&sc_, &m, 1, &view, &pl, &seg, xy, &k);
    if (rc == -1) throw Eg3dError(EG3D_ERR_ARG, "PLGMatchesManager::is_matched: the point is not on its polyline");
    if (k == -1) return false;
    if (k < -1) k = -2 - k;  // (matched by an interval the extractor's walk would not get past: still the manager's answer)
    const uint64_t at = g_.iv_off[sc_.view_pl_off[plg_id] + pl] + (uint64_t)k;
    pli_containing_point.start = {g_.iv_start_seg[at], {g_.iv_start_xy[2 * at], g_.iv_start_xy[2 * at + 1]}};
    pli_containing_point.end = {g_.iv_end_seg[at], {g_.iv_end_xy[2 * at], g_.iv_end_xy[2 * at + 1]}};
    return true;
  }
  bool is_matched(const int plg_id, const PolyLineGraph2D::plg_point& plgp, PolyLineGraph2D::pl_interval& pli_containing_point) const {
    return is_matched(plg_id, plgp.polyline_id, plgp.plp, pli_containing_point);
  }
  // concatenates the batches of a run (seed order) and replays them
  int replay(const eg3d_scene& sc, const std::vector<eg3d_edgepoints>& parts) {
    std::vector<float> X, xy;
    std::vector<uint32_t> pl, seg, key;
    std::vector<uint64_t> off(1, 0);
    std::vector<int32_t> view;
    for (const eg3d_edgepoints& e : parts) {
      const uint64_t base = (uint64_t)view.size();
      X.insert(X.end(), e.X, e.X + 3 * e.n_points);
      key.insert(key.end(), e.key, e.key + 4 * e.n_points);
      for (uint64_t i = 0; i < e.n_points; i++) off.push_back(base + e.obs_off[i + 1]);
      view.insert(view.end(), e.obs_view, e.obs_view + e.n_obs);
      pl.insert(pl.end(), e.obs_pl, e.obs_pl + e.n_obs);
      seg.insert(seg.end(), e.obs_seg, e.obs_seg + e.n_obs);
      xy.insert(xy.end(), e.obs_xy, e.obs_xy + 2 * e.n_obs);
    }
    eg3d_edgepoints all;
    std::memset(&all, 0, sizeof(all));
    all.n_points = off.size() - 1;
    all.n_obs = view.size();
    all.X = X.data();
    all.obs_off = off.data();
    all.obs_view = view.data();
    all.obs_pl = pl.data();
    all.obs_seg = seg.data();
    all.obs_xy = xy.data();
    all.key = key.data();
    return finish(sc, all);
  }

  // the same from chains held as the reference holds them (vector of point tuples per chain; key = seed, index of the
  // chain within the seed): every chain in the order given = the order add_matched_3dpolyline would have seen
  int replay_chains(const eg3d_scene& sc, const std::vector<std::vector<new_3dpoint_plgp_matches>>& chains,
                    const std::vector<std::array<uint32_t, 3>>& chain_key) {
    std::vector<float> X, xy;
    std::vector<uint32_t> pl, seg, key;
    std::vector<uint64_t> off(1, 0);
    std::vector<int32_t> view;
    for (size_t c = 0; c < chains.size(); c++)
      for (size_t i = 0; i < chains[c].size(); i++) {
        const vec3& p = std::get<0>(chains[c][i]);
        X.insert(X.end(), {p.x, p.y, p.z});
        const uint32_t k[4] = {chain_key[c][0], chain_key[c][1], chain_key[c][2], (uint32_t)i};
        key.insert(key.end(), k, k + 4);
        const auto& obs = std::get<1>(chains[c][i]);
        const auto& vs = std::get<2>(chains[c][i]);
        for (size_t j = 0; j < obs.size(); j++) {
          view.push_back(vs[j]);
          pl.push_back((uint32_t)obs[j].polyline_id);
          seg.push_back((uint32_t)obs[j].plp.segment_index);
          xy.push_back(obs[j].plp.coords.x);
          xy.push_back(obs[j].plp.coords.y);
        }
        off.push_back((uint64_t)view.size());
      }
    if (view.empty()) {  // nothing matched: an empty graph, not an error
      view.push_back(0);
      pl.push_back(0);
      seg.push_back(0);
      xy.assign(2, 0.f);
    }
    if (X.empty()) {
      X.assign(3, 0.f);
      key.assign(4, 0);
    }
    eg3d_edgepoints all;
    std::memset(&all, 0, sizeof(all));
    all.n_points = off.size() - 1;
    all.n_obs = all.n_points ? off.back() : 0;
    all.X = X.data();
    all.obs_off = off.data();
    all.obs_view = view.data();
    all.obs_pl = pl.data();
    all.obs_seg = seg.data();
    all.obs_xy = xy.data();
    all.key = key.data();
    return finish(sc, all);
  }

  // The reference's manager is ONE object that grows over every call it is passed to. set_accumulate(true) gives this
  // one those semantics: replay / replay_chains ADD their cloud to a host state (include/eg3d_host_accumulate.h), and
  // get_plg3d(), matched_table() and is_matched() answer from the graph of everything added so far. Off (the default) is
  // what this class always did: a replay replaces. Switching drops the state; the graph last built stays until the next replay.
  void set_accumulate(bool on) {
    if (on == accumulate_) return;
    accumulate_ = on;
    eg3d_host_replay_state_destroy(state_);
    state_ = nullptr;
  }
  bool accumulates() const { return accumulate_; }

 private:
  // what replay and replay_chains end with: the cloud replaces the graph, or is added to the state
  int finish(const eg3d_scene& sc, const eg3d_edgepoints& all) {
    if (!accumulate_) {
      eg3d_host_free_graph3d(&g_);
      sc_ = sc;
      return eg3d_host_replay_matches(&sc, &all, &g_);
    }
    if (!state_) {
      sc_ = sc;
      state_ = eg3d_host_replay_state_create(&sc_);  // (the state borrows sc_: this object's copy, whose arrays are the edge manager's)
      if (!state_) return -1;
    }
    const int rc = eg3d_host_replay_state_add(state_, &all);
    if (rc != 0) return rc;  // refused: the state and the graph are as they were
    eg3d_host_free_graph3d(&g_);
    return eg3d_host_replay_state_graph(state_, &g_);
  }
  eg3d_graph3d g_;
  eg3d_scene sc_{};  // the scene of the last replay (the edge manager's: its arrays outlive the run)
  bool accumulate_ = false;
  eg3d_replay_state* state_ = nullptr;
};

// EdgeManager (edge_manager.hpp:54-73): the abstract base the path's entry points take (`const EdgeManager* em`, which
// plg_matching_from_refpoints.cpp:67 downcasts to PLGEdgeManager*). The cv::Mat image accessors of the reference's
// base are not part of this path and are left out; the two pure virtuals keep their signatures.
class EdgeManager {
 public:
  virtual std::vector<vec2> detect_nearby_edge_intersections(const int imgId, const int startingPoint_id,
                                                             const float starting_detection_dist) = 0;
  virtual std::vector<std::vector<vec2>> detect_epipolar_intersections(const int starting_image_id, const int starting_point_id,
                                                                       const vec2& intersection_point_on_starting_image,
                                                                       const float max_correspondence_detection_radius) = 0;
  virtual ~EdgeManager() {}

 protected:
  explicit EdgeManager(const SfMData& input_sfmd) : sfmd(input_sfmd) {}
  const SfMData& sfmd;
};

// Owns the flattened scene and the GPU context: what `new PLGEdgeManager(imgs, sfmd, F, plgs, 10, 3)` and the 4 px
// PolyLine2DMapSearch maps hold in the reference (edge_matcher.cpp:101-107), resident in HBM.
class PLGEdgeManager : public EdgeManager {
 public:
  // the reference's constructor shape minus the images (plg_edge_manager.hpp:80): the two detection constants are
  // compile-time constants of the kernels (global_defines.hpp:35-36), other values are refused
  PLGEdgeManager(const SfMData& sfmd, const FundamentalMatrices& F, const std::vector<PolyLineGraph2D>& plgs,
                 const float starting_detection_dist, const float correspondence_detection_range_multiplication_factor,
                 int device = 0)
      : PLGEdgeManager(sfmd, F, plgs, device) {
    if (starting_detection_dist != 10.0f || correspondence_detection_range_multiplication_factor != 3.0f)
      throw std::invalid_argument("eg3d_ref::PLGEdgeManager: DETECTION_STARTING_RADIUS 10 / MULTIPLICATION_FACTOR 3 are built in");
  }
  // legacy segment-based interface: not implemented by the reference's PLGEdgeManager either
  std::vector<vec2> detect_nearby_edge_intersections(const int, const int, const float) override { throw NotImplementedException(); }
  std::vector<std::vector<vec2>> detect_epipolar_intersections(const int, const int, const vec2&, const float) override {
    throw NotImplementedException();
  }
  // the manager the 3-argument gaussNewtonFiltering / filter() take their GPU context from: the most recently
  // constructed one that is still alive (single caller thread, as in the reference)
  static PLGEdgeManager*& default_manager() {
    static PLGEdgeManager* d = nullptr;
    return d;
  }
  PLGEdgeManager(const SfMData& sfmd, const FundamentalMatrices& F, const std::vector<PolyLineGraph2D>& plgs,
                 int device = 0)
      : EdgeManager(sfmd), sfmd_(sfmd) {
    const int V = sfmd.numCameras_;
    for (int v = 0; v < V; v++)
      for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) P_.push_back(sfmd.camerasList_[v].cameraMatrix[r][c]);
    F_.assign((size_t)V * V * 9, 0.0);
    Fv_.assign((size_t)V * V, 0);
    for (int i = 0; i < V; i++)
      for (int j = 0; j < V; j++) {
        bool any = false;
        for (int k = 0; k < 9; k++) {
          F_[((size_t)i * V + j) * 9 + k] = F[i][j][k];
          any = any || F[i][j][k] != 0.0;
        }
        Fv_[(size_t)i * V + j] = (i != j && any) ? 1 : 0;
      }
    vpo_.push_back(0);
    pvo_.push_back(0);
    for (int v = 0; v < V; v++) {
      for (size_t p = 0; p < plgs[v].polylines.size(); p++) {
        const auto& pl = plgs[v].polylines[p];
        const bool ok = plgs[v].is_valid_polyline(p);
        pls_.push_back((uint32_t)pl.start);
        ple_.push_back((uint32_t)pl.end);
        plv_.push_back(ok ? 1 : 0);
        if (ok)
          for (const auto& c : pl.polyline_coords) {
            vtx_.push_back(c.x);
            vtx_.push_back(c.y);
          }
        pvo_.push_back((uint32_t)(vtx_.size() / 2));
      }
      vpo_.push_back((uint32_t)pls_.size());
    }
    eg3d_scene& sc = scene_;
    sc.n_views = V;
    sc.width = sfmd.imageWidth_;
    sc.height = sfmd.imageHeight_;
    sc.cam_P = P_.data();
    sc.F = F_.data();
    sc.F_valid = Fv_.data();
    sc.view_pl_off = vpo_.data();
    sc.pl_vtx_off = pvo_.data();
    sc.vtx_xy = vtx_.data();
    sc.pl_start = pls_.data();
    sc.pl_end = ple_.data();
    sc.pl_valid = plv_.data();
    status_ = eg3d_create(&sc, device, &ctx_);
    if (status_ == EG3D_OK) upload_seeds();
    if (status_ == EG3D_OK) default_manager() = this;
  }
  ~PLGEdgeManager() override {
    if (default_manager() == this) default_manager() = nullptr;
    if (ctx_) eg3d_destroy(ctx_);
  }
  PLGEdgeManager(const PLGEdgeManager&) = delete;
  PLGEdgeManager& operator=(const PLGEdgeManager&) = delete;

  int last_status() const { return status_; }
  eg3d_ctx* ctx() const { return ctx_; }
  const eg3d_scene& scene() const { return scene_; }

  // pair(starting intersections, [per starting intersection][per track entry] correspondences), per track entry
  using per_view_result = std::pair<std::vector<PolyLineGraph2D::plg_point>,
                                    std::vector<std::vector<std::vector<PolyLineGraph2D::plg_point>>>>;
  std::vector<per_view_result> detect_nearby_intersections_and_correspondences_plgp(const int starting_point_id) {
    std::vector<per_view_result> res;
    if (!ctx_) return res;
    eg3d_seeds s = seeds_struct();
    eg3d_candidates c;
    status_ = eg3d_candidates_run(ctx_, &s, (uint32_t)starting_point_id, (uint32_t)starting_point_id + 1, &c);
    if (status_ != EG3D_OK) return res;
    const uint32_t k = c.n_sv;
    res.resize(k);
    for (uint32_t a = 0; a < k; a++)
      for (uint32_t h = c.start_off[a]; h < c.start_off[a + 1]; h++)
        res[a].first.push_back({c.start_pl[h], {c.start_seg[h], {c.start_xy[2 * h], c.start_xy[2 * h + 1]}}});
    for (uint32_t t = 0; t < c.n_tasks; t++) {
      std::vector<std::vector<PolyLineGraph2D::plg_point>> lists;
      for (uint32_t l = c.task_list_off[t]; l < c.task_list_off[t + 1]; l++) {
        std::vector<PolyLineGraph2D::plg_point> v;
        for (uint32_t h = c.list_off[l]; h < c.list_off[l + 1]; h++)
          v.push_back({c.hit_pl[h], {c.hit_seg[h], {c.hit_xy[2 * h], c.hit_xy[2 * h + 1]}}});
        lists.push_back(std::move(v));
      }
      res[c.task_sv[t]].second.push_back(std::move(lists));
    }
    eg3d_free_candidates(&c);
    return res;
  }

  // plg_matching_from_refpoints_parallel over all reference points: ONE call of the C ABI. Seeds are independent
  // (plg_matching_from_refpoints.cpp:83-104 runs them on its OpenMP team); since round 6 the library itself cuts a call
  // into sub-batches that it keeps in flight on internal contexts and concatenates in seed order, which is the
  // reference's order (eg3d_set_pipelining; until round 5 this shim did the same above the ABI with eg3d_clone).
  // set_batching(seeds per sub-batch, sub-batches in flight): 0 / 0 = the library's defaults.
  void set_batching(uint32_t seeds_per_batch, int contexts) {
    batch_ = seeds_per_batch;
    n_ctx_ = contexts < 0 ? 0 : contexts;
  }
  std::vector<new_3dpoint_plgp_matches> match_all(PLGMatchesManager* plgmm = nullptr) {
    std::vector<new_3dpoint_plgp_matches> res;
    if (!ctx_) return res;
    const uint32_t n = (uint32_t)sfmd_.numPoints_;
    const uint32_t nb = 1;
    std::vector<eg3d_edgepoints> parts(nb);
    std::vector<int> rc(nb, EG3D_OK);
    eg3d_set_pipelining(ctx_, n_ctx_, batch_ ? (int)((n + batch_ - 1) / batch_) : 0);
    rc[0] = eg3d_match_resident(ctx_, 0, n, 0, &parts[0], nullptr);
    status_ = EG3D_OK;
    for (uint32_t i = 0; i < nb; i++)
      if (rc[i] != EG3D_OK) status_ = rc[i];
    if (status_ == EG3D_OK) {
      uint64_t total = 0;
      for (uint32_t i = 0; i < nb; i++) total += parts[i].n_points;
      res.reserve(total);
      for (uint32_t p = 0; p < nb; p++) {
        const eg3d_edgepoints& e = parts[p];
        for (uint64_t i = 0; i < e.n_points; i++) {
          std::vector<PolyLineGraph2D::plg_point> obs;
          std::vector<int> views;
          for (uint64_t j = e.obs_off[i]; j < e.obs_off[i + 1]; j++) {
            obs.push_back({e.obs_pl[j], {e.obs_seg[j], {e.obs_xy[2 * j], e.obs_xy[2 * j + 1]}}});
            views.push_back(e.obs_view[j]);
          }
          res.emplace_back(vec3{e.X[3 * i], e.X[3 * i + 1], e.X[3 * i + 2]}, std::move(obs), std::move(views));
        }
      }
      // plgmm.add_matched_3dpolyline(chain) for every emitted chain, in emission order
      // (plg_matching_from_refpoints.cpp:74-77): replayed on the host from the ordered cloud
      if (plgmm) status_ = plgmm->replay(scene_, parts);
    }
    for (uint32_t i = 0; i < nb; i++)
      if (rc[i] == EG3D_OK) eg3d_free_edgepoints(&parts[i]);
    return res;
  }

  // find_new_3d_points_from_compatible_polylines_expandallviews_parallel for ONE set of potentially
  // compatible polylines (per view: the reference's set<ulong> of polyline ids), as
  // pipelines.cpp:98,144 call it once per polyline match.
  // plgmm (may be null: no manager): the matches manager the extractor consults — samples and epipolar hits inside an
  // interval it holds are left out (eg3d_match_polyline_sets_matched).
  std::vector<new_3dpoint_plgp_matches> match_polyline_set(const std::vector<std::set<unsigned long>>& compat,
                                                           const PLGMatchesManager* plgmm = nullptr) {
    std::vector<new_3dpoint_plgp_matches> res;
    if (!ctx_) return res;
    std::vector<uint32_t> row_off(1, 0), ids;
    for (const auto& per_view : compat) {
      for (unsigned long id : per_view) {
        if (id > 0xfffffffful) {  // (narrowed, it would alias a smaller id and break the row's order)
          status_ = EG3D_ERR_ARG;
          return res;
        }
        ids.push_back((uint32_t)id);
      }
      row_off.push_back((uint32_t)ids.size());
    }
    if (ids.empty()) ids.push_back(0);
    eg3d_polyline_sets ps;
    ps.n_sets = 1;
    ps.row_off = row_off.data();
    ps.pl_ids = ids.data();
    eg3d_edgepoints e;
    eg3d_matched_intervals m;
    std::memset(&m, 0, sizeof(m));
    if (plgmm) m = plgmm->matched_table();
    status_ = m.struct_size ? eg3d_match_polyline_sets_matched(ctx_, &ps, 0, 1, &m, 0, &e, nullptr)
                            : eg3d_match_polyline_sets(ctx_, &ps, 0, 1, 0, &e, nullptr);
    if (status_ == EG3D_OK) {
      res.reserve(e.n_points);
      for (uint64_t i = 0; i < e.n_points; i++) {
        std::vector<PolyLineGraph2D::plg_point> obs;
        std::vector<int> views;
        for (uint64_t j = e.obs_off[i]; j < e.obs_off[i + 1]; j++) {
          obs.push_back({e.obs_pl[j], {e.obs_seg[j], {e.obs_xy[2 * j], e.obs_xy[2 * j + 1]}}});
          views.push_back(e.obs_view[j]);
        }
        res.emplace_back(vec3{e.X[3 * i], e.X[3 * i + 1], e.X[3 * i + 2]}, std::move(obs), std::move(views));
      }
      eg3d_free_edgepoints(&e);
    }
    return res;
  }

  // polyline_matching_closeness_to_refpoints (polyline_matcher.cpp:75-168) over all reference points: ONE call of the C ABI
  // (eg3d_match_polylines_closeness). first: the accepted reference points; second: per polyline match, per view, the set
  // of polyline ids. Empty result + last_status() on failure.
  std::pair<std::vector<unsigned long>, std::vector<std::vector<std::set<unsigned long>>>> match_polylines_closeness() {
    std::pair<std::vector<unsigned long>, std::vector<std::vector<std::set<unsigned long>>>> res;
    if (!ctx_) return res;
    eg3d_seeds s = seeds_struct();
    eg3d_polyline_matches m;
    status_ = eg3d_match_polylines_closeness(ctx_, &s, 0, (uint32_t)sfmd_.numPoints_, &m, nullptr);
    if (status_ != EG3D_OK) return res;
    res.first.assign(m.refpoints, m.refpoints + m.n_refpoints);
    const size_t V = (size_t)sfmd_.numCameras_;
    res.second.resize(m.n_sets, std::vector<std::set<unsigned long>>(V));
    for (size_t r = 0; r < (size_t)m.n_sets * V; r++)
      res.second[r / V][r % V].insert(m.pl_ids + m.row_off[r], m.pl_ids + m.row_off[r + 1]);
    eg3d_free_polyline_matches(&m);
    return res;
  }

  // The graph half of polyline_matching_similarity_graph (polyline_matcher.cpp:222-327) over all reference points: ONE call
  // of the C ABI (eg3d_similarity_graph). close_polylines[point][view], close_refpoints[view][polyline], the nodes
  // (polyline_matches_vector) and the weighted adjacency (adjacency_lists and weights of the reference's
  // GraphAdjacencySetUndirectedNoTypeWeighted); `raw` keeps the arrays for eg3d_host_write_compat_graph. Empty + last_status()
  // on failure.
  struct SimilarityGraph {
    std::vector<std::vector<std::set<unsigned long>>> close_polylines;
    std::vector<std::vector<std::vector<unsigned long>>> close_refpoints;
    std::vector<std::pair<int, unsigned long>> polyline_matches_vector;
    std::vector<std::set<unsigned long>> adjacency_lists;
    std::vector<std::vector<float>> weights;  // weights[n][k]: the edge to the k-th (ascending) neighbour of n
    eg3d_simgraph raw{};
    eg3d_ctx* ctx = nullptr;  // the manager's context (not owned): communities() runs on it
    SimilarityGraph() = default;
    SimilarityGraph(const SimilarityGraph&) = delete;
    SimilarityGraph& operator=(const SimilarityGraph&) = delete;
    SimilarityGraph(SimilarityGraph&& o) noexcept { *this = std::move(o); }
    SimilarityGraph& operator=(SimilarityGraph&& o) noexcept {
      if (this != &o) {
        eg3d_free_simgraph(&raw);
        close_polylines = std::move(o.close_polylines);
        close_refpoints = std::move(o.close_refpoints);
        polyline_matches_vector = std::move(o.polyline_matches_vector);
        adjacency_lists = std::move(o.adjacency_lists);
        weights = std::move(o.weights);
        raw = o.raw;
        ctx = o.ctx;
        std::memset(&o.raw, 0, sizeof(o.raw));
      }
      return *this;
    }
    ~SimilarityGraph() { eg3d_free_simgraph(&raw); }
    // write_to_file of the reference's weighted graph: the input of its community detection
    int write_to_file(const char* path) const { return eg3d_host_write_compat_graph(path, &raw); }
    // The community detection the reference runs on the graph, on the device (eg3d_detect_communities): one id per node,
    // numbered by ascending smallest member, -1 for a node without a neighbour. params == nullptr: the defaults. Throws on
    // failure; the manager must still be alive.
    std::vector<long> communities(const eg3d_louvain_params* params = nullptr, eg3d_louvain_stats* stats = nullptr) const {
      eg3d_communities m{};
      const int rc = eg3d_detect_communities(ctx, &raw, params, &m, stats);
      if (rc != EG3D_OK) throw Eg3dError(rc, std::string("SimilarityGraph::communities: ") + eg3d_last_error());
      std::vector<long> ids(m.ids, m.ids + m.n_nodes);
      eg3d_free_communities(&m);
      return ids;
    }
  };
  SimilarityGraph similarity_graph() {
    SimilarityGraph res;
    if (!ctx_) return res;
    eg3d_seeds s = seeds_struct();
    status_ = eg3d_similarity_graph(ctx_, &s, 0, (uint32_t)sfmd_.numPoints_, &res.raw, nullptr);
    if (status_ != EG3D_OK) return res;
    res.ctx = ctx_;
    const eg3d_simgraph& g = res.raw;
    const size_t V = (size_t)sfmd_.numCameras_;
    res.close_polylines.assign(g.n_points, std::vector<std::set<unsigned long>>(V));
    for (uint32_t i = 0; i < g.n_points; i++)
      for (uint32_t k = g.cp_off[i]; k < g.cp_off[i + 1]; k++) res.close_polylines[i][g.cp_view[k]].insert(g.cp_pl[k]);
    res.close_refpoints.resize(V);
    for (size_t v = 0; v < V; v++) {
      const uint32_t g0 = scene_.view_pl_off[v], g1 = scene_.view_pl_off[v + 1];
      res.close_refpoints[v].resize(g1 - g0);
      for (uint32_t gp = g0; gp < g1; gp++)
        res.close_refpoints[v][gp - g0].assign(g.cr_point + g.cr_off[gp], g.cr_point + g.cr_off[gp + 1]);
    }
    res.adjacency_lists.resize(g.n_nodes);
    res.weights.resize(g.n_nodes);
    for (uint32_t n = 0; n < g.n_nodes; n++) {
      res.polyline_matches_vector.emplace_back((int)g.node_view[n], (unsigned long)g.node_pl[n]);
      res.adjacency_lists[n].insert(g.adj_node + g.adj_off[n], g.adj_node + g.adj_off[n + 1]);
      res.weights[n].assign(g.adj_w + g.adj_off[n], g.adj_w + g.adj_off[n + 1]);
    }
    return res;
  }

  // All chains of ONE reference point, grouped the way the reference's loop produces them
  // (plg_matching_from_refpoints.cpp:69-78): [track entry][starting intersection] -> chain (possibly empty).
  // n_start[entry] = starting intersections of that entry (a chain-less intersection still has its — empty — slot).
  using chain = std::vector<new_3dpoint_plgp_matches>;
  std::vector<std::vector<chain>> match_refpoint_chains(const unsigned long refpoint_id) {
    std::vector<std::vector<chain>> res;
    if (!ctx_ || refpoint_id >= (unsigned long)sfmd_.numPoints_) return res;
    eg3d_seeds s = seeds_struct();
    eg3d_candidates c;
    status_ = eg3d_candidates_run(ctx_, &s, (uint32_t)refpoint_id, (uint32_t)refpoint_id + 1, &c);
    if (status_ != EG3D_OK) return res;
    res.resize(c.n_sv);
    for (uint32_t a = 0; a < c.n_sv; a++) res[a].resize(c.start_off[a + 1] - c.start_off[a]);
    eg3d_free_candidates(&c);
    eg3d_edgepoints e;
    status_ = eg3d_match_resident(ctx_, (uint32_t)refpoint_id, (uint32_t)refpoint_id + 1, 0, &e, nullptr);
    if (status_ != EG3D_OK) {
      res.clear();
      return res;
    }
    for (uint64_t i = 0; i < e.n_points; i++) {
      const uint32_t entry = e.key[4 * i + 1], hit = e.key[4 * i + 2];
      if (entry >= res.size() || hit >= res[entry].size()) continue;
      std::vector<PolyLineGraph2D::plg_point> obs;
      std::vector<int> views;
      for (uint64_t j = e.obs_off[i]; j < e.obs_off[i + 1]; j++) {
        obs.push_back({e.obs_pl[j], {e.obs_seg[j], {e.obs_xy[2 * j], e.obs_xy[2 * j + 1]}}});
        views.push_back(e.obs_view[j]);
      }
      res[entry][hit].emplace_back(vec3{e.X[3 * i], e.X[3 * i + 1], e.X[3 * i + 2]}, std::move(obs), std::move(views));
    }
    eg3d_free_edgepoints(&e);
    return res;
  }
  const SfMData& sfm_data() const { return sfmd_; }

 private:
  eg3d_seeds seeds_struct() {
    eg3d_seeds s;
    s.n_seeds = (uint32_t)sfmd_.numPoints_;
    s.trk_off = toff_.data();
    s.trk_view = tview_.data();
    s.trk_xy = txy_.data();
    return s;
  }
  void upload_seeds() {
    toff_.assign(1, 0);
    for (int i = 0; i < sfmd_.numPoints_; i++) {
      for (size_t j = 0; j < sfmd_.camViewingPointN_[i].size(); j++) {
        tview_.push_back(sfmd_.camViewingPointN_[i][j]);
        txy_.push_back(sfmd_.point2DoncamViewingPoint_[i][j].x);
        txy_.push_back(sfmd_.point2DoncamViewingPoint_[i][j].y);
      }
      toff_.push_back((uint32_t)tview_.size());
    }
    eg3d_seeds s = seeds_struct();
    status_ = eg3d_upload_seeds(ctx_, &s);
  }
  const SfMData& sfmd_;
  std::vector<float> P_, vtx_, txy_;
  std::vector<double> F_;
  std::vector<uint8_t> Fv_, plv_;
  std::vector<uint32_t> vpo_, pvo_, pls_, ple_, toff_;
  std::vector<int32_t> tview_;
  eg3d_scene scene_;
  eg3d_ctx* ctx_ = nullptr;
  int status_ = EG3D_OK;
  uint32_t batch_ = 0;
  int n_ctx_ = 0;
};

// PLGPConsensusManager (plgp_consensus_manager.hpp:56-72): the strategy interface of the path, same two pure virtuals.
class PLGPConsensusManager {
 public:
  using points = std::vector<new_3dpoint_plgp_matches>;
  using intersections_and_correspondences =
      std::pair<std::vector<PolyLineGraph2D::plg_point>, std::vector<std::vector<std::vector<PolyLineGraph2D::plg_point>>>>;
  virtual points consensus_strategy_single_point(const int starting_img_id, const int refpoint,
                                                 const intersections_and_correspondences& intersections_and_correspondences_pair) = 0;
  virtual std::vector<points> consensus_strategy_single_point_vector(
      const int starting_img_id, const int refpoint, const intersections_and_correspondences& intersections_and_correspondences_pair) = 0;
  virtual ~PLGPConsensusManager() {}
};

// PLGPCM3ViewsPLGFollowing (plgpcm_3views_plg_following.hpp:52-60; .cpp:40-69): 3-view consensus with polyline
// following and expand-to-all-views — kernels task_setup, K3a, K3s, K3b of the edge manager's context. The
// intersections handed in are the ones the SAME edge manager produced for that reference point (the only way the
// reference calls it, plg_matching_from_refpoints.cpp:67-72); the GPU path recomputes them, so their content is only
// used to tell apart two track entries of the same view (Q2).
class PLGPCM3ViewsPLGFollowing : public PLGPConsensusManager {
 public:
  explicit PLGPCM3ViewsPLGFollowing(PLGEdgeManager& em) : em_(em) {}
  PLGEdgeManager& edge_manager() const { return em_; }
  std::vector<points> consensus_strategy_single_point_vector(
      const int starting_img_id, const int refpoint, const intersections_and_correspondences& pair) override {
    if (cached_point_ != refpoint) {
      cache_ = em_.match_refpoint_chains((unsigned long)refpoint);
      if (em_.last_status() != EG3D_OK) throw Eg3dError(em_.last_status(), std::string("eg3d: ") + eg3d_last_error());
      cached_point_ = refpoint;
      served_.assign(cache_.size(), 0);
    }
    // The track entry this call is about. The reference's loop (plg_matching_from_refpoints.cpp:68-73) calls once per
    // track entry, in track order, so a view id that appears on several entries of the track is served entry by entry:
    // the first entry of that view not handed out yet (all handed out: the round starts again — a caller that walks
    // the track a second time). An entry whose starting intersections differ in number from the ones handed in is not
    // the caller's entry and is skipped while another candidate remains.
    const std::vector<int>& track = em_.sfm_data().camViewingPointN_[refpoint];
    int entry = -1, fallback = -1;
    for (int round = 0; round < 2 && entry < 0; round++) {
      for (size_t i = 0; i < track.size() && i < cache_.size(); i++) {
        if (track[i] != starting_img_id || served_[i]) continue;
        if (fallback < 0) fallback = (int)i;
        if (cache_[i].size() == pair.first.size()) {
          entry = (int)i;
          break;
        }
      }
      if (entry < 0 && fallback >= 0) entry = fallback;
      if (entry < 0)  // every entry of this view was served: forget and look again
        for (size_t i = 0; i < track.size() && i < served_.size(); i++)
          if (track[i] == starting_img_id) served_[i] = 0;
    }
    if (entry >= 0) served_[(size_t)entry] = 1;
    std::vector<points> res(pair.first.size());
    if (entry >= 0)
      for (size_t h = 0; h < res.size() && h < cache_[entry].size(); h++) res[h] = cache_[entry][h];
    return res;
  }
  points consensus_strategy_single_point(const int starting_img_id, const int refpoint,
                                         const intersections_and_correspondences& pair) override {
    points res;
    for (auto& ch : consensus_strategy_single_point_vector(starting_img_id, refpoint, pair))
      for (auto& p : ch) res.push_back(std::move(p));
    return res;
  }

 private:
  PLGEdgeManager& em_;
  int cached_point_ = -1;
  std::vector<std::vector<PLGEdgeManager::chain>> cache_;
  std::vector<uint8_t> served_;  // per track entry of the cached point: its chains were handed out
};

namespace detail {
inline void throw_if_failed(const PLGEdgeManager* em, const char* what) {
  if (em->last_status() != EG3D_OK)
    throw Eg3dError(em->last_status(), std::string(what) + ": " + eg3d_last_error());
}
}  // namespace detail

// plg_matching_from_refpoints[_parallel](sfm_data, em, cm, plgmm) — plg_matching_from_refpoints.hpp:53,55, the call of
// pipelines.cpp:164. `em` is downcast to PLGEdgeManager* exactly as plg_matching_from_refpoints.cpp:67 does. With the
// consensus manager of the path (PLGPCM3ViewsPLGFollowing of the same edge manager, what edge_matcher.cpp:115 builds)
// all reference points run as batches in flight on the GPU; any other PLGPConsensusManager is honoured through the
// reference's own per-point loop (candidates from the GPU, consensus from the caller's strategy). plgmm receives what
// add_matched_3dpolyline(chain) would have recorded for every chain, in emission order. Throws Eg3dError when the GPU
// path fails (the reference's signature has no status).
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoint(const SfMData& sfm_data, const EdgeManager* em,
                                                                        const PLGPConsensusManager* cm,
                                                                        const unsigned long refpoint_id,
                                                                        std::vector<PLGEdgeManager::chain>* chains_out = nullptr) {
  std::vector<new_3dpoint_plgp_matches> res;
  PLGEdgeManager* g = (PLGEdgeManager*)em;
  PLGPConsensusManager* c = const_cast<PLGPConsensusManager*>(cm);  // the reference calls the non-const virtual through its const pointer (-fpermissive)
  auto all_imgs = g->detect_nearby_intersections_and_correspondences_plgp((int)refpoint_id);
  detail::throw_if_failed(g, "detect_nearby_intersections_and_correspondences_plgp");
  for (size_t i = 0; i < sfm_data.camViewingPointN_[refpoint_id].size() && i < all_imgs.size(); i++) {
    const int starting_img_id = sfm_data.camViewingPointN_[refpoint_id][i];
    auto cur_res_vec = c->consensus_strategy_single_point_vector(starting_img_id, (int)refpoint_id, all_imgs[i]);
    for (auto& cur_res : cur_res_vec) {
      res.insert(res.end(), cur_res.begin(), cur_res.end());
      if (chains_out) chains_out->push_back(std::move(cur_res));
    }
  }
  return res;
}
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoints_parallel(const SfMData& sfm_data, const EdgeManager* em,
                                                                                  const PLGPConsensusManager* cm,
                                                                                  PLGMatchesManager& plgmm) {
  PLGEdgeManager* g = (PLGEdgeManager*)em;
  const PLGPCM3ViewsPLGFollowing* own = dynamic_cast<const PLGPCM3ViewsPLGFollowing*>(cm);
  if (own && &own->edge_manager() == g) {
    auto res = g->match_all(&plgmm);
    detail::throw_if_failed(g, "plg_matching_from_refpoints_parallel");
    return res;
  }
  // a caller-supplied consensus strategy: the reference's loop, point by point
  std::vector<new_3dpoint_plgp_matches> res;
  std::vector<PLGEdgeManager::chain> chains;
  std::vector<std::array<uint32_t, 3>> chain_key;
  for (unsigned long r = 0; r < (unsigned long)sfm_data.numPoints_; r++) {
    const size_t before = chains.size();
    auto cur = plg_matching_from_refpoint(sfm_data, em, cm, r, &chains);
    res.insert(res.end(), cur.begin(), cur.end());
    for (size_t k = before; k < chains.size(); k++) chain_key.push_back({(uint32_t)r, (uint32_t)(k - before), 0u});
  }
  const int rc = plgmm.replay_chains(g->scene(), chains, chain_key);
  if (rc != 0) throw Eg3dError(rc, "eg3d_host_replay_matches failed");
  return res;
}
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoints(const SfMData& sfm_data, const EdgeManager* em,
                                                                         const PLGPConsensusManager* cm, PLGMatchesManager& plgmm) {
  return plg_matching_from_refpoints_parallel(sfm_data, em, cm, plgmm);  // the reference's "parallel" loop is serial too
}

// Shorter forms kept from earlier rounds (the consensus manager of the path implied): empty result + last_status() on failure.
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoints_parallel(const SfMData&, PLGEdgeManager* em) {
  return em->match_all();
}
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoints_parallel(const SfMData&, PLGEdgeManager* em,
                                                                                  PLGMatchesManager& plgmm) {
  return em->match_all(&plgmm);
}
inline std::vector<new_3dpoint_plgp_matches> plg_matching_from_refpoints(const SfMData& s, PLGEdgeManager* em) {
  return plg_matching_from_refpoints_parallel(s, em);
}

// find_new_3d_points_from_compatible_polylines_expandallviews[_parallel]
// (include/edgegraph3d/matching/plg_matching/polyline_matching.hpp:55-56): plgs, F, the matches
// manager and the grid maps of the reference signature live in the edge manager.
inline std::vector<new_3dpoint_plgp_matches> find_new_3d_points_from_compatible_polylines_expandallviews_parallel(
    const SfMData&, PLGEdgeManager* em, const std::vector<std::set<unsigned long>>& potentially_compatible_polylines) {
  return em->match_polyline_set(potentially_compatible_polylines);
}
// ... with the reference's matches manager argument (polyline_matching.cpp:153): what plgmm holds — after
// plg_matching_from_refpoints_parallel(sfmd, em, cm, plgmm), say — is consulted as the reference consults it: a 20 px sample
// inside a held interval starts nothing and the walk goes on past the interval's end, an epipolar hit inside one is dropped.
// As in the reference's parallel build, plgmm is not updated by this call. A manager that has replayed nothing behaves as
// the overload above. Throws Eg3dError on failure.
inline std::vector<new_3dpoint_plgp_matches> find_new_3d_points_from_compatible_polylines_expandallviews_parallel(
    const SfMData&, PLGEdgeManager* em, const std::vector<std::set<unsigned long>>& potentially_compatible_polylines,
    PLGMatchesManager& plgmm) {
  auto res = em->match_polyline_set(potentially_compatible_polylines, &plgmm);
  if (em->last_status() != EG3D_OK)
    throw Eg3dError(em->last_status(), std::string("find_new_3d_points_from_compatible_polylines_expandallviews_parallel: ") + eg3d_last_error());
  return res;
}

// polyline_matching_closeness_to_refpoints (include/edgegraph3d/matching/polyline_matching/polyline_matcher.hpp): plgs and
// the image size of the reference signature live in the edge manager. Throws Eg3dError on failure.
inline std::pair<std::vector<unsigned long>, std::vector<std::vector<std::set<unsigned long>>>>
polyline_matching_closeness_to_refpoints(const SfMData&, PLGEdgeManager* em) {
  auto res = em->match_polylines_closeness();
  detail::throw_if_failed(em, "polyline_matching_closeness_to_refpoints");
  return res;
}

// The graph half of polyline_matching_similarity_graph (polyline_matcher.hpp; polyline_matcher.cpp:222-327): everything up to
// the community detection, which the reference hands to Grappolo through a file: compute_communities below runs the
// library's own on the device, or the caller clusters the file (SimilarityGraph::write_to_file writes it; read the ids back
// with eg3d_host_read_communities). Throws on failure.
inline PLGEdgeManager::SimilarityGraph polyline_matching_similarity_graph_before_communities(const SfMData&, PLGEdgeManager* em) {
  auto res = em->similarity_graph();
  detail::throw_if_failed(em, "polyline_matching_similarity_graph");
  return res;
}

// compute_communities (community_detection_interface.cpp:57-73), the reference's shape: writes the compatibility graph file,
// detects the communities (on the device, SimilarityGraph::communities, where the reference runs Grappolo), writes one id
// per line to out_polyline_communities and returns the ids. Either path may be null or empty: that file is not written.
inline std::vector<long> compute_communities(const PLGEdgeManager::SimilarityGraph& pmgw, const char* out_compatibility_graph_file,
                                             const char* out_polyline_communities) {
  if (out_compatibility_graph_file && *out_compatibility_graph_file && pmgw.write_to_file(out_compatibility_graph_file) != EG3D_OK)
    throw Eg3dError(EG3D_ERR_ARG, "compute_communities: cannot write the compatibility graph file");
  const std::vector<long> ids = pmgw.communities();
  if (out_polyline_communities && *out_polyline_communities) {
    const std::vector<int64_t> ids64(ids.begin(), ids.end());
    if (eg3d_host_write_communities(out_polyline_communities, ids64.data(), ids64.size()) != EG3D_OK)
      throw Eg3dError(EG3D_ERR_ARG, "compute_communities: cannot write the communities file");
  }
  return ids;
}

// compute_polyline_matches_from_nodes_component_ids (polyline_matcher.cpp:202-214), the reference's signature: one set per
// community id up to the largest, a node with a negative id in none.
inline std::vector<std::vector<std::set<unsigned long>>> compute_polyline_matches_from_nodes_component_ids(
    const std::vector<std::pair<int, unsigned long>>& polyline_matches_vector, int amount_of_plgs,
    const std::vector<long>& nodes_component_ids) {
  long max_id = -1;
  for (long id : nodes_component_ids) max_id = id > max_id ? id : max_id;
  std::vector<std::vector<std::set<unsigned long>>> res((size_t)(max_id + 1), std::vector<std::set<unsigned long>>((size_t)amount_of_plgs));
  for (size_t i = 0; i < polyline_matches_vector.size() && i < nodes_component_ids.size(); i++)
    if (nodes_component_ids[i] >= 0)
      res[(size_t)nodes_component_ids[i]][(size_t)polyline_matches_vector[i].first].insert(polyline_matches_vector[i].second);
  return res;
}

namespace detail {
// A GPU context for the filter: the registered edge manager's when it serves the same rig, else a private one built
// from the cameras alone (a scene without polylines — ./filter runs without any polyline graph, filter.cpp:48-115).
struct FilterContext {
  eg3d_ctx* ctx = nullptr;
  bool own = false;
  explicit FilterContext(const SfMData& s) {
    const int V = s.numCameras_;
    if (V <= 0 || s.camerasList_.size() < (size_t)V)
      throw Eg3dError(EG3D_ERR_ARG, "filter: the SfM data holds no cameras (numCameras_ / camerasList_)");
    // the registered manager's context serves this rig only when EVERY camera matrix is the same (a different rig that
    // shares camera 0 must not be filtered with the manager's cameras)
    PLGEdgeManager* d = PLGEdgeManager::default_manager();
    if (d && d->ctx() && d->scene().n_views == V) {
      bool same = true;
      for (int v = 0; v < V && same; v++)
        same = std::memcmp(d->scene().cam_P + (size_t)v * 16, &s.camerasList_[(size_t)v].cameraMatrix[0][0], sizeof(float) * 16) == 0;
      if (same) {
        ctx = d->ctx();
        return;
      }
    }
    std::vector<float> P;
    for (int v = 0; v < V; v++)
      for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) P.push_back(s.camerasList_[v].cameraMatrix[r][c]);
    std::vector<double> F((size_t)V * V * 9, 0.0);
    std::vector<uint8_t> Fv((size_t)V * V, 0);
    std::vector<uint32_t> vpo((size_t)V + 1, 0), pvo(1, 0), none(1, 0);
    std::vector<float> vtx(2, 0.f);
    std::vector<uint8_t> plv(1, 0);
    eg3d_scene sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.n_views = V;
    sc.width = s.imageWidth_ > 0 ? s.imageWidth_ : 1;
    sc.height = s.imageHeight_ > 0 ? s.imageHeight_ : 1;
    sc.cam_P = P.data();
    sc.F = F.data();
    sc.F_valid = Fv.data();
    sc.view_pl_off = vpo.data();
    sc.pl_vtx_off = pvo.data();
    sc.vtx_xy = vtx.data();
    sc.pl_start = none.data();
    sc.pl_end = none.data();
    sc.pl_valid = plv.data();
    const int rc = eg3d_create(&sc, 0, &ctx);
    if (rc != EG3D_OK) throw Eg3dError(rc, std::string("eg3d_create (filter context): ") + eg3d_last_error());
    own = true;
  }
  ~FilterContext() {
    if (own && ctx) eg3d_destroy(ctx);
  }
  FilterContext(const FilterContext&) = delete;
  FilterContext& operator=(const FilterContext&) = delete;
};
}  // namespace detail

// gaussNewtonFiltering(SfMData&, std::vector<bool>&, const float) — gauss_newton.hpp:20 (gauss_newton.cpp:136-178):
// FP32 Gauss-Newton from the stored X over all observations of every point; inliers get their point replaced. The GPU
// context is the registered edge manager's (PLGEdgeManager::default_manager()) or a private one. Throws Eg3dError on
// a failure of the GPU path.
inline void gaussNewtonFiltering(SfMData& sfm_data_, std::vector<bool>& inliers, const float gn_max_mse) {
  const size_t n = sfm_data_.points_.size();
  inliers.assign(n, false);
  if (!n) return;
  std::vector<float> X(3 * n), Xo(3 * n), xy;
  std::vector<uint32_t> off(1, 0);
  std::vector<int32_t> view;
  for (size_t i = 0; i < n; i++) {
    X[3 * i] = sfm_data_.points_[i].x;
    X[3 * i + 1] = sfm_data_.points_[i].y;
    X[3 * i + 2] = sfm_data_.points_[i].z;
    for (size_t j = 0; j < sfm_data_.camViewingPointN_[i].size(); j++) {
      view.push_back(sfm_data_.camViewingPointN_[i][j]);
      xy.push_back(sfm_data_.point2DoncamViewingPoint_[i][j].x);
      xy.push_back(sfm_data_.point2DoncamViewingPoint_[i][j].y);
    }
    if (view.size() > 0xffffffffull) throw Eg3dError(EG3D_ERR_ARG, "gaussNewtonFiltering: more than 2^32 - 1 observations");
    off.push_back((uint32_t)view.size());
  }
  if (view.empty()) {
    view.push_back(0);
    xy.assign(2, 0.f);
  }
  std::vector<uint8_t> inl(n);
  detail::FilterContext fc(sfm_data_);
  const int rc = eg3d_gn_filter(fc.ctx, X.data(), off.data(), view.data(), xy.data(), n, gn_max_mse, 0, Xo.data(), inl.data(), nullptr);
  if (rc != EG3D_OK) throw Eg3dError(rc, std::string("eg3d_gn_filter: ") + eg3d_last_error());
  for (size_t i = 0; i < n; i++)
    if (inl[i]) {
      sfm_data_.points_[i] = {Xo[3 * i], Xo[3 * i + 1], Xo[3 * i + 2]};
      inliers[i] = true;
    }
}
// earlier rounds' form with an explicit manager (kept): the manager's context, same behaviour
inline void gaussNewtonFiltering(SfMData& sfm_data_, std::vector<bool>& inliers, const float gn_max_mse, PLGEdgeManager* em) {
  PLGEdgeManager*& d = PLGEdgeManager::default_manager();
  PLGEdgeManager* saved = d;
  d = em;
  try {
    gaussNewtonFiltering(sfm_data_, inliers, gn_max_mse);
  } catch (...) {
    d = saved;
    throw;
  }
  d = saved;
}

// compute_3d_point_coords(const SfMData&, const vector<glm::vec2>&, const vector<int>&, glm::vec3&, bool&) —
// triangulation.hpp:48 (triangulation.cpp:468-481): fewer than two observations are not valid; otherwise the 2-view DLT on
// (the first entry with the minimal view id, the last entry) and FP64 Gauss-Newton over all of them, on the GPU
// (eg3d_triangulate, EG3D_TRI_FROM_SCRATCH). new_point_data is assigned only when valid. The GPU context is the registered
// edge manager's or a private one, as for gaussNewtonFiltering; one call per point pays a launch and two copies — many
// points go through the batched overload below. Throws Eg3dError on a failure of the GPU path (a view id outside the rig).
//
// Batched: track i is (coords[i], ids[i]); points / valid get one entry per track (a point that is not valid is (0, 0, 0));
// flags, optional, the EG3D_TRI_FLAG_* of every track.
inline void compute_3d_point_coords(const SfMData& sfmd, const std::vector<std::vector<vec2>>& coords,
                                    const std::vector<std::vector<int>>& ids, std::vector<vec3>& points, std::vector<bool>& valid,
                                    std::vector<uint8_t>* flags = nullptr) {
  const size_t n = coords.size();
  if (ids.size() != n) throw Eg3dError(EG3D_ERR_ARG, "compute_3d_point_coords: coords and ids differ in length");
  points.assign(n, vec3{0.f, 0.f, 0.f});
  valid.assign(n, false);
  if (flags) flags->assign(n, 0);
  if (!n) return;
  std::vector<uint32_t> off(1, 0);
  std::vector<int32_t> view;
  std::vector<float> xy;
  for (size_t i = 0; i < n; i++) {
    if (coords[i].size() != ids[i].size()) throw Eg3dError(EG3D_ERR_ARG, "compute_3d_point_coords: a track's coords and ids differ in length");
    for (size_t j = 0; j < ids[i].size(); j++) {
      view.push_back(ids[i][j]);
      xy.push_back(coords[i][j].x);
      xy.push_back(coords[i][j].y);
    }
    if (view.size() > 0xffffffffull) throw Eg3dError(EG3D_ERR_ARG, "compute_3d_point_coords: more than 2^32 - 1 observations");
    off.push_back((uint32_t)view.size());
  }
  if (view.empty()) {
    view.push_back(0);
    xy.assign(2, 0.f);
  }
  std::vector<float> X(3 * n);
  std::vector<uint8_t> ok(n), fl(n);
  detail::FilterContext fc(sfmd);
  const int rc = eg3d_triangulate(fc.ctx, EG3D_TRI_FROM_SCRATCH, n, off.data(), view.data(), xy.data(), nullptr, X.data(), ok.data(),
                                  fl.data(), nullptr);
  if (rc != EG3D_OK) throw Eg3dError(rc, std::string("eg3d_triangulate: ") + eg3d_last_error());
  for (size_t i = 0; i < n; i++) {
    points[i] = vec3{X[3 * i], X[3 * i + 1], X[3 * i + 2]};
    valid[i] = ok[i] != 0;
    if (flags) (*flags)[i] = fl[i];
  }
}
inline void compute_3d_point_coords(const SfMData& sfmd, const std::vector<vec2>& selected_2d_reprojections_coords,
                                    const std::vector<int>& selected_2d_reprojections_ids, vec3& new_point_data, bool& valid) {
  std::vector<vec3> p;
  std::vector<bool> v;
  compute_3d_point_coords(sfmd, std::vector<std::vector<vec2>>(1, selected_2d_reprojections_coords),
                          std::vector<std::vector<int>>(1, selected_2d_reprojections_ids), p, v);
  valid = v[0];
  if (valid) new_point_data = p[0];
}

#define EG3D_REF_GN_MAX_MSE 2.25f           /* GN_MAX_MSE, gauss_newton.hpp:18 */
#define EG3D_REF_INVALID_FORCED_MIN_FILTER -1 /* outliers_filtering.cpp:12 */

// compute_inliers (outliers_filtering.cpp:37-64): Gauss-Newton inliers, then points >= first_edgepoint need MORE than
// max(3, median track length / 2 - 1) observations (or the forced amount)
inline std::vector<bool> compute_inliers(SfMData& sfm_data_, const int first_edgepoint, const float gn_max_mse,
                                         const int forced_min_filter) {
  std::vector<bool> inliers;
  gaussNewtonFiltering(sfm_data_, inliers, gn_max_mse);
  const size_t n = sfm_data_.points_.size();
  std::vector<uint32_t> off(1, 0);
  for (size_t i = 0; i < n; i++) off.push_back(off.back() + (uint32_t)sfm_data_.camViewingPointN_[i].size());
  std::vector<uint8_t> inl(n ? n : 1);
  for (size_t i = 0; i < n; i++) inl[i] = inliers[i] ? 1 : 0;
  eg3d_host_observation_filter(sfm_data_.numCameras_, off.data(), n, (uint64_t)(first_edgepoint < 0 ? 0 : first_edgepoint),
                               forced_min_filter, inl.data());
  for (size_t i = 0; i < n; i++) inliers[i] = inl[i] != 0;
  return inliers;
}
// removeOutliers (outliers_filtering.cpp:66-92)
inline void removeOutliers(SfMData& sfmd, const std::vector<bool>& inliers) {
  SfMData res;
  res.camerasList_ = sfmd.camerasList_;
  res.camerasPaths_ = sfmd.camerasPaths_;
  res.numCameras_ = sfmd.numCameras_;
  res.imageWidth_ = sfmd.imageWidth_;
  res.imageHeight_ = sfmd.imageHeight_;
  res.pointsVisibleFromCamN_.resize(res.numCameras_);
  int curpt = 0;
  for (size_t i = 0; i < inliers.size(); i++)
    if (inliers[i]) {
      res.points_.push_back(sfmd.points_[i]);
      res.camViewingPointN_.push_back(sfmd.camViewingPointN_[i]);
      res.point2DoncamViewingPoint_.push_back(sfmd.point2DoncamViewingPoint_[i]);
      for (const int cam_id : sfmd.camViewingPointN_[i]) res.pointsVisibleFromCamN_[cam_id].push_back(curpt);
      curpt++;
    }
  res.numPoints_ = (int)res.points_.size();
  sfmd = res;
}
// filter(): the four overloads of outliers_filtering.hpp:18-21 (outliers_filtering.cpp:94-114), without the prints
inline void filter(SfMData& sfmd, const int first_edgepoint, const float gn_max_mse, const int forced_min_filter) {
  const std::vector<bool> inliers = compute_inliers(sfmd, first_edgepoint, gn_max_mse, forced_min_filter);
  removeOutliers(sfmd, inliers);
}
inline void filter(SfMData& sfmd, const int first_edgepoint) {
  filter(sfmd, first_edgepoint, EG3D_REF_GN_MAX_MSE, EG3D_REF_INVALID_FORCED_MIN_FILTER);
}
inline void filter(SfMData& sfmd, const int first_edgepoint, const float gn_max_mse) {
  filter(sfmd, first_edgepoint, gn_max_mse, EG3D_REF_INVALID_FORCED_MIN_FILTER);
}
inline void filter(SfMData& sfmd, const int first_edgepoint, const int forced_min_filter) {
  filter(sfmd, first_edgepoint, EG3D_REF_GN_MAX_MSE, forced_min_filter);
}

}  // namespace eg3d_ref
