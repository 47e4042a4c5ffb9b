// eg3d_api_filter.hip — the Gauss-Newton filter, the compaction and the 3 px de-duplication on a device-resident cloud
#include <cmath>

#include "eg3d_api_internal.h"

// hist_all: [V + 2] (bin k for k <= V, bin V + 1 for longer lists)
static int gn_filter_device_impl(eg3d_ctx* c, const eg3d_device_edgepoints* d, const uint8_t* keep_dev, float gn_max_mse,
                                 int legacy_abs, float* X_out_dev, uint8_t* inlier_dev, std::vector<uint64_t>& hist_all,
                                 float* ms_kernel) {
  const size_t bins = (size_t)c->V + 2;
  hist_all.assign(bins, 0);
  hipStream_t st = c->stream;
  BUF_TRY(c->r_hist.ensure(8 * bins + 8));
  HIP_TRY(hipMemsetAsync(c->r_hist.p, 0, 8 * bins + 8, st));
  K5Dev ext{keep_dev, d->n_obs, c->r_hist.as<unsigned long long>(), (uint32_t*)(c->r_hist.as<unsigned long long>() + bins)};
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k5_device(st, c->ds.cam_P, c->V, d->X, d->obs_off, d->obs_view, d->obs_xy, d->n_points, gn_max_mse, legacy_abs, X_out_dev,
                   inlier_dev, ext);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  std::vector<uint64_t> back(bins + 1);
  HIP_TRY(hipMemcpyAsync(back.data(), c->r_hist.p, 8 * bins + 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (ms_kernel) HIP_TRY(hipEventElapsedTime(ms_kernel, c->ea[0], c->eb[0]));
  const uint32_t flags = (uint32_t)back[bins];
  if (flags) return device_flags_error("eg3d_gn_filter_device", flags);
  std::copy(back.begin(), back.begin() + bins, hist_all.begin());
  return EG3D_OK;
}

extern "C" int eg3d_gn_filter_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, float gn_max_mse,
                                     int legacy_abs, float* X_out_dev, uint8_t* inlier_dev, uint64_t* obs_hist_host,
                                     uint64_t* n_inliers_host, float* ms_kernel) {
  if (!c || !cloud || (cloud->n_points && (!X_out_dev || !inlier_dev))) {
    g_err = "eg3d_gn_filter_device: bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_cloud(cloud, "eg3d_gn_filter_device", false));
  HIP_TRY(hipSetDevice(c->device));
  std::vector<uint64_t> hist;
  if (ms_kernel) *ms_kernel = 0;
  BUF_TRY(gn_filter_device_impl(c, cloud, keep_dev, gn_max_mse, legacy_abs, X_out_dev, inlier_dev, hist, ms_kernel));
  if (obs_hist_host) std::copy(hist.begin(), hist.begin() + c->V + 1, obs_hist_host);
  if (n_inliers_host) {
    *n_inliers_host = 0;
    for (uint64_t h : hist) *n_inliers_host += h;  // (the last bin: lists longer than the rig has views)
  }
  return EG3D_OK;
}

static int compact_device_impl(eg3d_ctx* c, const eg3d_device_edgepoints* d, const uint8_t* keep_dev, const float* X_new_dev,
                               int32_t min_obs, eg3d_device_edgepoints* out, float* ms) {
  const void* mine[] = {c->c_X.p, c->c_off.p, c->c_view.p, c->c_pl.p, c->c_seg.p, c->c_xy.p, c->c_key.p};
  const void* theirs[] = {d->X, d->obs_off, d->obs_view, d->obs_pl, d->obs_seg, d->obs_xy, d->key, X_new_dev};
  for (const void* a : mine)
    for (const void* b : theirs)
      if (a && a == b) {
        g_err = "eg3d_compact_device: the input views this context's compaction buffers, which the call overwrites";
        return EG3D_ERR_ARG;
      }
  hipStream_t st = c->stream;
  const CloudView in = cloud_view(d);
  const uint64_t nb = (d->n_points + K6_BLOCK - 1) / K6_BLOCK;
  BUF_TRY(c->r_blk.ensure(16 * (nb + 1) + 8));
  unsigned long long* blk = c->r_blk.as<unsigned long long>();
  uint32_t* flags = (uint32_t*)(blk + 2 * (nb + 1));
  HIP_TRY(hipMemsetAsync(flags, 0, 8, st));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_compact_count(st, in, keep_dev, min_obs, blk, flags);
  launch_compact_scan(st, nb, blk);
  HIP_TRY(hipGetLastError());
  uint64_t back[3];  // surviving points, surviving observations, flags
  HIP_TRY(hipMemcpyAsync(back, blk + 2 * nb, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if ((uint32_t)back[2]) return device_flags_error("eg3d_compact_device", (uint32_t)back[2]);
  const uint64_t np = back[0], no = back[1];
  BUF_TRY(c->c_X.ensure(12 * np));
  BUF_TRY(c->c_off.ensure(8 * np));
  BUF_TRY(c->c_key.ensure(16 * np));
  BUF_TRY(c->c_view.ensure(4 * no));
  BUF_TRY(c->c_pl.ensure(4 * no));
  BUF_TRY(c->c_seg.ensure(4 * no));
  BUF_TRY(c->c_xy.ensure(8 * no));
  CloudOut o{c->c_X.as<float>(), c->c_off.as<eg3d_off_t>(), c->c_view.as<int32_t>(), c->c_pl.as<uint32_t>(),
             c->c_seg.as<uint32_t>(), c->c_xy.as<float>(), c->c_key.as<uint32_t>()};
  launch_compact_scatter(st, in, keep_dev, X_new_dev, min_obs, blk, o, c->tune.compact_nt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));
  if (ms) HIP_TRY(hipEventElapsedTime(ms, c->ea[0], c->eb[0]));
  out->n_points = np;
  out->n_obs = no;
  out->X = o.X;
  out->obs_off = o.obs_off;
  out->obs_view = o.obs_view;
  out->obs_pl = o.obs_pl;
  out->obs_seg = o.obs_seg;
  out->obs_xy = o.obs_xy;
  out->key = o.key;
  out->complete = 1;
  return EG3D_OK;
}

extern "C" int eg3d_compact_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev,
                                   const float* X_new_dev, int32_t min_obs, eg3d_device_edgepoints* out) {
  if (!c || !cloud || !out) {
    g_err = "eg3d_compact_device: bad arguments";
    return EG3D_ERR_ARG;
  }
  if ((const void*)out == (const void*)cloud) {
    g_err = "eg3d_compact_device: out must not alias cloud";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_cloud(cloud, "eg3d_compact_device", true));
  HIP_TRY(hipSetDevice(c->device));
  return compact_device_impl(c, cloud, keep_dev, X_new_dev, min_obs, out, nullptr);
}

// The rule of eg3d_host_observation_filter (host/post_steps.cpp) on a histogram by list length: hist[k], k = 0 .. V, and
// `count` points in all (lists longer than V are counted but sit in no bin, as there).
static int observation_threshold(const uint64_t* hist, int V, uint64_t count, int forced_min_filter) {
  uint64_t acc = 0;
  int median = 0;
  for (median = 0; median < V; median++) {
    acc += hist[median + 1];
    if (acc >= count / 2) break;
  }
  int threshold = median / 2 - 1;
  if (threshold < 3) threshold = 3;
  if (forced_min_filter > -1) threshold = forced_min_filter;
  return threshold;
}

// The copy of a compacted cloud into a library-owned host cloud (obs_off with its sentinel); *ms_copy: wall time.
static int copy_survivors_to_host(eg3d_ctx* c, const eg3d_device_edgepoints& o, eg3d_edgepoints* out_host, const char* who,
                                  float* ms_copy) {
  const auto t0 = std::chrono::steady_clock::now();
  memset(out_host, 0, sizeof(*out_host));
  const uint64_t np = o.n_points, no = o.n_obs;
  out_host->X = (float*)malloc(12 * std::max<uint64_t>(np, 1));
  out_host->obs_off = (uint64_t*)malloc(8 * (np + 1));
  out_host->key = (uint32_t*)malloc(16 * std::max<uint64_t>(np, 1));
  out_host->obs_view = (int32_t*)malloc(4 * std::max<uint64_t>(no, 1));
  out_host->obs_pl = (uint32_t*)malloc(4 * std::max<uint64_t>(no, 1));
  out_host->obs_seg = (uint32_t*)malloc(4 * std::max<uint64_t>(no, 1));
  out_host->obs_xy = (float*)malloc(8 * std::max<uint64_t>(no, 1));
  if (!out_host->X || !out_host->obs_off || !out_host->key || !out_host->obs_view || !out_host->obs_pl ||
      !out_host->obs_seg || !out_host->obs_xy) {
    eg3d_free_edgepoints(out_host);
    g_err = std::string(who) + ": out of host memory";
    return EG3D_ERR_HIP;
  }
  struct { void* dst; const void* src; size_t bytes; } cp[] = {
      {out_host->X, o.X, 12 * np},          {out_host->obs_off, o.obs_off, 8 * np}, {out_host->key, o.key, 16 * np},
      {out_host->obs_view, o.obs_view, 4 * no}, {out_host->obs_pl, o.obs_pl, 4 * no},   {out_host->obs_seg, o.obs_seg, 4 * no},
      {out_host->obs_xy, o.obs_xy, 8 * no}};
  for (auto& q : cp)
    if (q.bytes) {
      const hipError_t e = hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, c->stream);
      if (e != hipSuccess) {
        eg3d_free_edgepoints(out_host);
        g_err = std::string(who) + ": copy to the host: " + hipGetErrorString(e);
        return EG3D_ERR_HIP;
      }
    }
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    eg3d_free_edgepoints(out_host);
    g_err = std::string(who) + ": copy to the host failed";
    return EG3D_ERR_HIP;
  }
  out_host->obs_off[np] = no;
  out_host->n_points = np;
  out_host->n_obs = no;
  *ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return EG3D_OK;
}

extern "C" int eg3d_filter_resident(eg3d_ctx* c, float gn_max_mse, int legacy_abs, int forced_min_filter,
                                    const uint64_t* base_hist, int to_host, eg3d_edgepoints* out_host,
                                    eg3d_device_edgepoints* out_dev, eg3d_filter_stats* stats) {
  if (!c || (to_host && !out_host)) {
    g_err = "eg3d_filter_resident: bad arguments";
    return EG3D_ERR_ARG;
  }
  if (stats) BUF_TRY(check_struct_size("eg3d_filter_resident", "eg3d_filter_stats", stats->struct_size, sizeof(eg3d_filter_stats)));
  eg3d_device_edgepoints d;
  BUF_TRY(eg3d_last_device_output(c, &d));
  BUF_TRY(check_cloud(&d, "eg3d_filter_resident", true));
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t n = d.n_points;
  BUF_TRY(c->r_Xo.ensure(12 * n));
  BUF_TRY(c->r_inl.ensure(n));
  std::vector<uint64_t> hist;
  float ms_filter = 0, ms_compact = 0;
  BUF_TRY(gn_filter_device_impl(c, &d, nullptr, gn_max_mse, legacy_abs, c->r_Xo.as<float>(), c->r_inl.as<uint8_t>(), hist,
                                &ms_filter));
  uint64_t inliers = 0, count = 0;
  for (uint64_t h : hist) inliers += h;
  count = inliers;
  if (base_hist)
    for (int k = 0; k <= c->V; k++) {
      hist[k] += base_hist[k];
      count += base_hist[k];
    }
  const int threshold = observation_threshold(hist.data(), c->V, count, forced_min_filter);
  eg3d_device_edgepoints o;
  BUF_TRY(compact_device_impl(c, &d, c->r_inl.as<uint8_t>(), c->r_Xo.as<float>(), threshold, &o, &ms_compact));
  float ms_copy = 0;
  if (to_host) BUF_TRY(copy_survivors_to_host(c, o, out_host, "eg3d_filter_resident", &ms_copy));
  if (out_dev) *out_dev = o;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_filter_stats);
    stats->threshold = threshold;
    stats->n_points_in = n;
    stats->n_masked_in = n;
    stats->n_gn_inliers = inliers;
    stats->n_kept = o.n_points;
    stats->n_obs_kept = o.n_obs;
    stats->ms_filter = ms_filter;
    stats->ms_compact = ms_compact;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}

// ---- the 3 px de-duplication on a device-resident cloud ------------------------------------------------------------------
// The combined call, in the steps the phased calls are made of (eg3d_api_dedup_phases.hip): the map filled when `reset` or
// not valid, claim, keep, one read-back of the kept count and the flags.
static int dedup_device_impl(eg3d_ctx* c, const eg3d_device_edgepoints* d, uint64_t index_base, int reset, uint8_t* keep_dev,
                             uint64_t* n_kept, float* ms) {
  hipStream_t st = c->stream;
  K7Map m;
  BUF_TRY(dedup_map_open(c, reset != 0, &m));  // (dedup_valid is false from here until the call is known to have completed)
  unsigned long long* cnt = nullptr;
  BUF_TRY(dedup_counters_zero(c, &cnt));
  const CloudView in = cloud_view(d);
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_dedup_claim(st, in, m, (uint32_t)index_base);
  launch_dedup_keep(st, in, m, (uint32_t)index_base, keep_dev, cnt, (uint32_t*)(cnt + 1));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  uint64_t kept = 0;
  // (claims made through bad offsets are discarded: dedup_valid stays false, the next call starts from an empty map)
  BUF_TRY(dedup_counters_read(c, "eg3d_dedup_device", &kept));
  if (ms) HIP_TRY(hipEventElapsedTime(ms, c->ea[0], c->eb[0]));
  c->dedup_valid = true;
  if (n_kept) *n_kept = kept;
  return EG3D_OK;
}

extern "C" int eg3d_dedup_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, uint64_t index_base, int reset,
                                 uint8_t* keep_dev, uint64_t* n_kept_host) {
  if (cloud) BUF_TRY(dedup_index_check("eg3d_dedup_device", index_base, cloud->n_points));
  if (!c || !cloud || (cloud->n_points && !keep_dev)) {
    g_err = "eg3d_dedup_device: bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_cloud(cloud, "eg3d_dedup_device", false));
  HIP_TRY(hipSetDevice(c->device));
  return dedup_device_impl(c, cloud, index_base, reset, keep_dev, n_kept_host, nullptr);
}

extern "C" int eg3d_dedup_resident(eg3d_ctx* c, uint64_t index_base, int reset, int with_filter, float gn_max_mse,
                                   int legacy_abs, int forced_min_filter, const uint64_t* base_hist, int to_host,
                                   eg3d_edgepoints* out_host, eg3d_device_edgepoints* out_dev, eg3d_dedup_stats* stats) {
  if (stats) BUF_TRY(check_struct_size("eg3d_dedup_resident", "eg3d_dedup_stats", stats->struct_size, sizeof(eg3d_dedup_stats)));
  if (!c || (to_host && !out_host)) {
    g_err = "eg3d_dedup_resident: bad arguments";
    return EG3D_ERR_ARG;
  }
  eg3d_device_edgepoints d;
  BUF_TRY(eg3d_last_device_output(c, &d));
  BUF_TRY(dedup_index_check("eg3d_dedup_resident", index_base, d.n_points));
  BUF_TRY(check_cloud(&d, "eg3d_dedup_resident", true));
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t n = d.n_points;
  BUF_TRY(c->d_keep.ensure(n));
  uint64_t dedup_kept = 0, inliers = 0;
  float ms_dedup = 0, ms_filter = 0, ms_compact = 0, ms_copy = 0;
  BUF_TRY(dedup_device_impl(c, &d, index_base, reset, c->d_keep.as<uint8_t>(), &dedup_kept, &ms_dedup));
  // a step that fails from here on leaves no cloud for the claims just made: they are discarded with the earlier ones
  struct ClaimGuard {
    eg3d_ctx* c;
    bool ok = false;
    ~ClaimGuard() { if (!ok) c->dedup_valid = false; }
  } guard{c};
  int threshold = -1;
  eg3d_device_edgepoints o;
  if (with_filter) {
    // a masked-out point gets inlier 0, so r_inl is dedup AND inlier, and the histogram counts the deduplicated inliers
    BUF_TRY(c->r_Xo.ensure(12 * n));
    BUF_TRY(c->r_inl.ensure(n));
    std::vector<uint64_t> hist;
    BUF_TRY(gn_filter_device_impl(c, &d, c->d_keep.as<uint8_t>(), gn_max_mse, legacy_abs, c->r_Xo.as<float>(),
                                  c->r_inl.as<uint8_t>(), hist, &ms_filter));
    for (uint64_t hh : hist) inliers += hh;
    uint64_t count = inliers;
    if (base_hist)
      for (int k = 0; k <= c->V; k++) {
        hist[k] += base_hist[k];
        count += base_hist[k];
      }
    threshold = observation_threshold(hist.data(), c->V, count, forced_min_filter);
    BUF_TRY(compact_device_impl(c, &d, c->r_inl.as<uint8_t>(), c->r_Xo.as<float>(), threshold, &o, &ms_compact));
  } else {
    BUF_TRY(compact_device_impl(c, &d, c->d_keep.as<uint8_t>(), nullptr, -1, &o, &ms_compact));
  }
  if (to_host) BUF_TRY(copy_survivors_to_host(c, o, out_host, "eg3d_dedup_resident", &ms_copy));
  guard.ok = true;
  if (out_dev) *out_dev = o;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_dedup_stats);
    stats->threshold = threshold;
    stats->n_points_in = n;
    stats->n_dedup_kept = dedup_kept;
    stats->n_gn_inliers = inliers;
    stats->n_kept = o.n_points;
    stats->n_obs_kept = o.n_obs;
    stats->ms_dedup = ms_dedup;
    stats->ms_filter = ms_filter;
    stats->ms_compact = ms_compact;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}
