// Row N4, the host statement of the device estimator (eg3d_estimate_fundamental, K12): the arithmetic of
// csrc/eg3d_fund_core.h used in the plain way — one pair after the other on each thread, the common points collected into
// lists, the median by std::nth_element, the inliers appended — exactly as fmatrix.cpp does it. This file is what the
// device is compared with bit for bit, and what a caller without a GPU uses to get the same matrices. fmatrix.cpp
// (eg3d_host_estimate_F) stays as it is; the one arithmetic difference between the two is named in eg3d_fund_core.h.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <vector>

#include "eg3d_fund_core.h"
#include "eg3d_host.h"

namespace {
using namespace eg3d::fund;

struct PairCounts {
  uint64_t fits = 0, degenerate = 0;
};

bool lmeds(const std::vector<Corr>& pts, uint32_t iterations, uint64_t seed, double (&F)[9], PairCounts& pc) {
  const int n = (int)pts.size();
  std::vector<double> err((size_t)n);
  const auto median_of = [&](const double (&Fc)[9]) {
    for (int k = 0; k < n; k++) err[(size_t)k] = residual(Fc, pts[(size_t)k]);
    std::nth_element(err.begin(), err.begin() + n / 2, err.end());
    return err[(size_t)(n / 2)];
  };
  Rng rng{seed};
  double best_med = kHuge, bestF[9];
  bool have = false;
  for (uint32_t it = 0; it < iterations; it++) {
    uint32_t idx[kSample];
    draw_sample(rng, (uint32_t)n, idx);
    double Fc[9];
    pc.fits++;
    if (!eight_point([&](int k) { return pts[idx[k]]; }, kSample, Fc)) {
      pc.degenerate++;
      continue;
    }
    const double med = median_of(Fc);
    if (med < best_med) {
      best_med = med;
      memcpy(bestF, Fc, sizeof bestF);
      have = true;
    }
  }
  if (!have) return false;
  const double thr = inlier_threshold(best_med, n);
  std::vector<int> in;
  for (int k = 0; k < n; k++)
    if (residual(bestF, pts[(size_t)k]) <= thr) in.push_back(k);
  if ((int)in.size() >= kSample) {
    double Fr[9];
    // keep the refit only if it does not make the median worse
    if (eight_point([&](int k) { return pts[(size_t)in[(size_t)k]]; }, (int)in.size(), Fr) && median_of(Fr) <= best_med)
      memcpy(bestF, Fr, sizeof bestF);
  }
  memcpy(F, bestF, sizeof bestF);
  return true;
}

// per view: ascending ids of the points seen from it; a repeated view id counts once, an id outside the rig not at all
std::vector<std::vector<uint32_t>> points_on_views(int V, uint64_t N, const uint32_t* off, const int32_t* view) {
  std::vector<std::vector<uint32_t>> pv((size_t)V);
  for (uint64_t p = 0; p < N; p++)
    for (uint32_t k = off[p]; k < off[p + 1]; k++) {
      const int32_t v = view[k];
      if (v < 0 || v >= V) continue;
      auto& l = pv[(size_t)v];
      if (l.empty() || l.back() != (uint32_t)p) l.push_back((uint32_t)p);
    }
  return pv;
}

// the last listed observation with that view id
void obs_of(const uint32_t* off, const int32_t* view, const float* xy, uint32_t p, int v, double& x, double& y) {
  x = y = 0;
  for (uint32_t k = off[p]; k < off[p + 1]; k++)
    if (view[k] == v) {
      x = (double)xy[2 * (size_t)k];
      y = (double)xy[2 * (size_t)k + 1];
    }
}

}  // namespace

extern "C" int eg3d_host_estimate_fundamental(int32_t n_views, const eg3d_seeds* seeds, const eg3d_fund_params* params, double* F,
                                              uint8_t* F_valid, uint32_t* n_common, eg3d_fund_stats* stats) {
  if (stats && stats->struct_size < sizeof(eg3d_fund_stats)) return EG3D_ERR_ARG;
  if (params && params->struct_size < sizeof(eg3d_fund_params)) return EG3D_ERR_ARG;
  if (n_views <= 0 || !seeds || !F || !F_valid) return EG3D_ERR_ARG;
  const uint64_t N = seeds->n_seeds;
  if (N && (!seeds->trk_off || !seeds->trk_view || !seeds->trk_xy)) return EG3D_ERR_ARG;
  if (N && seeds->trk_off[0] != 0) return EG3D_ERR_ARG;
  for (uint64_t p = 0; p < N; p++)
    if (seeds->trk_off[p + 1] < seeds->trk_off[p]) return EG3D_ERR_ARG;
  const int V = n_views;
  const uint32_t iterations = params && params->iterations ? params->iterations : kDefaultIterations;
  const uint64_t rng_seed = params ? params->rng_seed : 0;
  const uint32_t* off = seeds->trk_off;
  const int32_t* view = seeds->trk_view;
  const float* xy = seeds->trk_xy;
  const auto pv = points_on_views(V, N, off, view);
  std::vector<uint32_t> both;
  std::vector<Corr> pts;
  uint64_t n_valid = 0, n_failed = 0, n_common_total = 0, n_fits = 0, n_degenerate = 0;
#pragma omp parallel for schedule(dynamic) firstprivate(both, pts) reduction(+ : n_valid, n_failed, n_common_total, n_fits, n_degenerate)
  for (int i = 0; i < V; i++)
    for (int j = 0; j < V; j++) {
      const size_t ij = (size_t)i * V + j;
      F_valid[ij] = 0;
      if (n_common) n_common[ij] = 0;
      memset(F + ij * 9, 0, sizeof(double) * 9);
      if (i == j) continue;
      both.clear();
      std::set_intersection(pv[(size_t)i].begin(), pv[(size_t)i].end(), pv[(size_t)j].begin(), pv[(size_t)j].end(),
                            std::back_inserter(both));
      if (n_common) n_common[ij] = (uint32_t)both.size();
      if ((int)both.size() < kMinCommon) continue;
      pts.clear();
      for (uint32_t p : both) {
        Corr c;
        obs_of(off, view, xy, p, i, c.x1, c.y1);
        obs_of(off, view, xy, p, j, c.x2, c.y2);
        pts.push_back(c);
      }
      n_common_total += both.size();
      PairCounts pc;
      double Fij[9];
      if (lmeds(pts, iterations, stream_seed(rng_seed, (uint64_t)ij), Fij, pc)) {
        memcpy(F + ij * 9, Fij, sizeof Fij);
        F_valid[ij] = 1;
        n_valid++;
      } else {
        n_failed++;
      }
      n_fits += pc.fits;
      n_degenerate += pc.degenerate;
    }
  if (stats) {
    const uint32_t sz = stats->struct_size;
    memset(stats, 0, sizeof(eg3d_fund_stats));
    stats->struct_size = sz;
    stats->n_pairs_valid = (uint32_t)n_valid;
    stats->n_pairs_failed = (uint32_t)n_failed;
    stats->n_common_total = n_common_total;
    stats->n_fits = n_fits;
    stats->n_fits_degenerate = n_degenerate;
  }
  return EG3D_OK;
}
