// eg3d_api_nearest.hip — cloud-to-cloud nearest distances on the device (include/eg3d/nearest.hpp): the host side of K18.
// An index is an object of its own: it holds the grid, the work buffers of its build and of the queries made against it
// (DevBuf, sized with ensure, so a second query of the same size allocates nothing) and the context it works for.
#include <cmath>

#include "eg3d_api_internal.h"
#include "eg3d_k18_nearest.h"
#include "../../include/eg3d/nearest.hpp"

using namespace eg3d::nearest;

struct eg3d_cloud_index {
  eg3d_ctx* ctx = nullptr;
  int device = 0;
  int group = 1;  // lanes that share a query
  uint64_t n_indexed = 0;
  Grid g{};  // (device addresses)
  eg3d_cloud_index_stats stats{};
  DevBuf pts, cell_key, cell_start;                    // the index
  DevBuf b_ctr, b_key[2], b_val[2], b_head, b_rank;    // the build (released when it is done)
  DevBuf tmp;                                          // rocPRIM scratch
  DevBuf u_X, u_keep;                                  // a host array uploaded (build: released; query: kept)
  DevBuf q_ctr, q_d2, q_nn, q_sorted;                  // a query: the counters, d2 / nn where the caller gives none, the sorted bits
};

static int refuse(int code, const char* who, const char* text) {
  g_err = std::string(who) + ": " + text;
  return code;
}

// what both builds check before anything else
static int check_build(const char* who, const eg3d_ctx* c, float cell, eg3d_cloud_index** index, const eg3d_cloud_index_stats* stats) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_cloud_index_stats", stats->struct_size, sizeof(eg3d_cloud_index_stats)));
  if (!c || !index) return refuse(EG3D_ERR_ARG, who, "bad arguments");
  if (check_cell(cell)) return refuse(EG3D_NEAREST_ERR_CELL, who, "cell must be finite and > 0");
  return EG3D_OK;
}

// A cloud as K18 reads it: only X, which must be there when there are points, of a whole cloud.
static int open_cloud(const char* who, eg3d_ctx* c, const eg3d_device_edgepoints* cloud, eg3d_device_edgepoints* d) {
  if (cloud)
    *d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, d));
  if (d->n_points && !d->X) return refuse(EG3D_ERR_ARG, who, "the device view has no X");
  if (!d->complete) return refuse(EG3D_ERR_ARG, who, "the device view does not hold a whole cloud (complete == 0)");
  if (d->n_points >= (1ull << 32)) return refuse(EG3D_ERR_CAPACITY, who, "2^32 points or more");
  return EG3D_OK;
}

// The build proper, on arrays that are on the device. On failure the caller deletes the index.
static int build_index(const char* who, eg3d_ctx* c, eg3d_cloud_index* ix, const float* X, uint64_t n, const uint8_t* keep, float cell) {
  hipStream_t st = c->stream;
  eg3d_cloud_index_stats& s = ix->stats;
  s.struct_size = (uint32_t)sizeof(s);
  s.n_points = n;
  s.cell = ix->g.cell = cell;
  if (const char* e = getenv("EG3D_K18_GROUP")) ix->group = atoi(e) == 64 ? 64 : atoi(e) == 8 ? 8 : atoi(e) == 1 ? 1 : 0;
  else ix->group = 0;
  BUF_TRY(ix->cell_start.ensure(sizeof(uint32_t)));
  ix->g.cell_start = ix->cell_start.as<uint32_t>();
  if (!n) {
    if (!ix->group) ix->group = 1;
    return EG3D_OK;  // (n_cells == 0: the search reads nothing)
  }
  u64 back[K18B_COUNT];
  BUF_TRY(ix->b_ctr.ensure(sizeof(back)));
  u64* ctr = ix->b_ctr.as<u64>();
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k18_init(st, ctr, false);
  launch_k18_minmax(st, X, n, keep, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s.n_dropped = back[K18B_DROPPED];
  s.n_nonfinite = back[K18B_NONFINITE];
  s.n_indexed = ix->n_indexed = n - s.n_dropped - s.n_nonfinite;
  if (s.n_indexed) {
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) {
      mn[a] = s.origin[a] = ix->g.origin[a] = ordered_decode((uint32_t)back[K18B_MIN + a]);
      mx[a] = ordered_decode((uint32_t)back[K18B_MAX + a]);
    }
    if (!grid_dims(mn, mx, cell, ix->g.dims)) return refuse(EG3D_NEAREST_ERR_EXTENT, who, "2^21 cells or more on an axis");
    for (int a = 0; a < 3; a++) s.dims[a] = ix->g.dims[a];
    const uint64_t m = s.n_indexed;
    for (int i = 0; i < 2; i++) {
      BUF_TRY(ix->b_key[i].ensure(sizeof(u64) * n));
      BUF_TRY(ix->b_val[i].ensure(sizeof(uint32_t) * n));
    }
    BUF_TRY(ix->b_head.ensure(sizeof(uint32_t) * (m + 1)));
    BUF_TRY(ix->b_rank.ensure(sizeof(uint32_t) * (m + 1)));
    BUF_TRY(ix->pts.ensure(sizeof(Pt) * m));
    BUF_TRY(ix->cell_key.ensure(sizeof(u64) * m));
    BUF_TRY(ix->cell_start.ensure(sizeof(uint32_t) * (m + 1)));
    launch_k18_keys(st, ix->g, X, n, keep, ix->b_key[0].as<u64>(), ix->b_val[0].as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // (the points that are not indexed carry the largest key: they sort behind the n_indexed others)
    BUF_TRY(prim_call(st, ix->tmp, "k8_sort_pairs", k8_sort_pairs, (const u64*)ix->b_key[0].as<u64>(), ix->b_key[1].as<u64>(),
                      (const uint32_t*)ix->b_val[0].as<uint32_t>(), ix->b_val[1].as<uint32_t>(), (size_t)n));
    launch_k18_gather(st, X, ix->b_key[1].as<u64>(), ix->b_val[1].as<uint32_t>(), m, ix->pts.as<Pt>(), ix->b_head.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(prim_call(st, ix->tmp, "k8_scan_u32", k8_scan_u32, (const uint32_t*)ix->b_head.as<uint32_t>(), ix->b_rank.as<uint32_t>(),
                      (size_t)m + 1));
    launch_k18_cells(st, ix->b_key[1].as<u64>(), ix->b_head.as<uint32_t>(), ix->b_rank.as<uint32_t>(), m, ix->cell_key.as<u64>(),
                     ix->cell_start.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    uint32_t n_cells = 0;
    HIP_TRY(hipMemcpyAsync(&n_cells, ix->b_rank.as<uint32_t>() + m, sizeof(n_cells), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_cells == 0 || n_cells > m) return refuse(EG3D_ERR_HIP, who, "the cell count read back from the device is impossible");
    launch_k18_max_cell(st, ix->cell_start.as<uint32_t>(), n_cells, ctr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[0], st));
    HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&s.ms_build, c->ea[0], c->eb[0]));
    s.n_cells = ix->g.n_cells = n_cells;
    s.max_cell_points = back[K18B_MAXCELL];
    ix->g.cell_key = ix->cell_key.as<uint64_t>();
    ix->g.cell_start = ix->cell_start.as<uint32_t>();
    ix->g.pts = ix->pts.as<Pt>();
  }
  // Lanes per query: a lane of its own, eight lanes when the cells are crowded. Measured ("K18"): at 19 and 21
  // points per occupied cell one lane is 1.7x and 2.3x faster than eight, at 37 eight lanes are 6 % faster than one.
  if (!ix->group) ix->group = (s.n_cells && s.n_indexed / s.n_cells >= 32) ? 8 : 1;
  for (DevBuf* b : {&ix->b_ctr, &ix->b_key[0], &ix->b_key[1], &ix->b_val[0], &ix->b_val[1], &ix->b_head, &ix->b_rank, &ix->tmp, &ix->u_X, &ix->u_keep})
    b->release();
  return EG3D_OK;
}

static int finish_build(int rc, eg3d_cloud_index* ix, eg3d_cloud_index** index, eg3d_cloud_index_stats* stats) {
  if (rc != EG3D_OK) {
    delete ix;
    return rc;
  }
  if (stats) *stats = ix->stats;
  *index = ix;
  return EG3D_OK;
}

extern "C" int eg3d_cloud_index_build_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, float cell,
                                             eg3d_cloud_index** index, eg3d_cloud_index_stats* stats) {
  const char* who = "eg3d_cloud_index_build_device";
  BUF_TRY(check_build(who, c, cell, index, stats));
  eg3d_device_edgepoints d;
  BUF_TRY(open_cloud(who, c, cloud, &d));
  HIP_TRY(hipSetDevice(c->device));
  eg3d_cloud_index* ix = new eg3d_cloud_index;
  ix->ctx = c;
  ix->device = c->device;
  return finish_build(build_index(who, c, ix, d.X, d.n_points, keep_dev, cell), ix, index, stats);
}

extern "C" int eg3d_cloud_index_build(eg3d_ctx* c, const float* X_host, uint64_t n, const uint8_t* keep_host, float cell,
                                      eg3d_cloud_index** index, eg3d_cloud_index_stats* stats) {
  const char* who = "eg3d_cloud_index_build";
  BUF_TRY(check_build(who, c, cell, index, stats));
  if (n && !X_host) return refuse(EG3D_ERR_ARG, who, "X_host is NULL");
  if (n >= (1ull << 32)) return refuse(EG3D_ERR_CAPACITY, who, "2^32 points or more");
  HIP_TRY(hipSetDevice(c->device));
  eg3d_cloud_index* ix = new eg3d_cloud_index;
  ix->ctx = c;
  ix->device = c->device;
  const auto w0 = std::chrono::steady_clock::now();
  int rc = upload(ix->u_X, X_host, 3 * n, c->stream);
  if (rc == EG3D_OK && keep_host) rc = upload(ix->u_keep, keep_host, n, c->stream);
  if (rc == EG3D_OK) rc = build_index(who, c, ix, ix->u_X.as<float>(), n, keep_host ? ix->u_keep.as<uint8_t>() : nullptr, cell);
  if (rc == EG3D_OK) {
    const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    ix->stats.ms_copy = std::max(0.f, wall - ix->stats.ms_build);
  } else {
    (void)hipStreamSynchronize(c->stream);  // (no copy still reads the caller's arrays, none writes into what is freed)
  }
  return finish_build(rc, ix, index, stats);
}

extern "C" void eg3d_cloud_index_free(eg3d_cloud_index* index) {
  if (!index) return;
  (void)hipSetDevice(index->device);
  delete index;
}

// what both queries check before anything else; t: the squared thresholds
static int check_query(const char* who, const eg3d_ctx* c, const eg3d_cloud_index* ix, float max_dist, const eg3d_nearest_stats* stats,
                       K18Thresholds* t) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_nearest_stats", stats->struct_size, sizeof(eg3d_nearest_stats)));
  if (!c || !ix) return refuse(EG3D_ERR_ARG, who, "bad arguments");
  if (ix->ctx != c) return refuse(EG3D_NEAREST_ERR_FOREIGN, who, "the index was built by another context");
  if (check_reach(max_dist, ix->g.cell)) return refuse(EG3D_NEAREST_ERR_MAXDIST, who, "max_dist must be finite, > 0 and <= the index's cell");
  if (check_thresholds(stats ? stats->n_thresholds : 0, stats ? stats->thresholds : nullptr, max_dist, t->t2))
    return refuse(EG3D_NEAREST_ERR_THRESHOLD, who, "at most 8 thresholds, each finite and in (0, max_dist]");
  return EG3D_OK;
}

// The query proper, on arrays that are on the device: the counters at their neutral values, the kernel, the sort of the d2
// bits and the median, one read-back. d2 / nn: where the results go on the device (d2: the index's own buffer when null).
static int run_query(eg3d_ctx* c, eg3d_cloud_index* ix, const float* X, uint64_t n, const uint8_t* keep, float max_dist,
                     const K18Thresholds& t, float* d2, uint32_t* nn, eg3d_nearest_stats* s) {
  hipStream_t st = c->stream;
  s->n_queries = n;
  s->min_d2 = s->max_d2 = s->median_d2 = bits_f32(kInfBits);
  if (!n) return EG3D_OK;
  if (!d2) {
    BUF_TRY(ix->q_d2.ensure(sizeof(float) * n));
    d2 = ix->q_d2.as<float>();
  }
  BUF_TRY(ix->q_ctr.ensure(sizeof(u64) * K18Q_COUNT));
  BUF_TRY(ix->q_sorted.ensure(sizeof(uint32_t) * n));
  u64* ctr = ix->q_ctr.as<u64>();
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k18_init(st, ctr, true);
  launch_k18_query(st, ix->group, ix->g, X, n, keep, max_dist, t, d2, nn, ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(prim_call(st, ix->tmp, "k18_sort_bits", k18_sort_bits, (const uint32_t*)d2, ix->q_sorted.as<uint32_t>(), (size_t)n));
  launch_k18_median(st, ix->q_sorted.as<uint32_t>(), ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  u64 back[K18Q_COUNT];
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->n_dropped = back[K18Q_DROPPED];
  s->n_nonfinite = back[K18Q_NONFINITE];
  s->n_within = back[K18Q_WITHIN];
  s->sum_q32 = back[K18Q_SUM];
  for (uint32_t k = 0; k < s->n_thresholds; k++) s->n_below[k] = back[K18Q_BELOW + k];
  if (s->n_within) {
    s->min_d2 = bits_f32((uint32_t)back[K18Q_MIN]);
    s->max_d2 = bits_f32((uint32_t)back[K18Q_MAX]);
    s->median_d2 = bits_f32((uint32_t)back[K18Q_MEDIAN]);
  }
  HIP_TRY(hipEventElapsedTime(&s->ms_kernel, c->ea[0], c->eb[0]));
  return EG3D_OK;
}

// the figures of a call start from the caller's thresholds and nothing else
static eg3d_nearest_stats fresh_stats(const eg3d_nearest_stats* in) {
  eg3d_nearest_stats s{};
  s.struct_size = (uint32_t)sizeof(s);
  if (in) {
    s.n_thresholds = in->n_thresholds;
    for (int k = 0; k < kMaxThresholds; k++) s.thresholds[k] = in->thresholds[k];
  }
  return s;
}

extern "C" int eg3d_cloud_nearest_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, eg3d_cloud_index* ix,
                                         float max_dist, float* d2_out_dev, uint32_t* nn_out_dev, eg3d_nearest_stats* stats) {
  const char* who = "eg3d_cloud_nearest_device";
  K18Thresholds t;
  BUF_TRY(check_query(who, c, ix, max_dist, stats, &t));
  eg3d_device_edgepoints d;
  BUF_TRY(open_cloud(who, c, cloud, &d));
  HIP_TRY(hipSetDevice(c->device));
  eg3d_nearest_stats s = fresh_stats(stats);
  BUF_TRY(run_query(c, ix, d.X, d.n_points, keep_dev, max_dist, t, d2_out_dev, nn_out_dev, &s));
  if (stats) *stats = s;
  return EG3D_OK;
}

extern "C" int eg3d_cloud_nearest_points(eg3d_ctx* c, const float* X_host, uint64_t n, const uint8_t* keep_host, eg3d_cloud_index* ix,
                                         float max_dist, float* d2_out_host, uint32_t* nn_out_host, eg3d_nearest_stats* stats) {
  const char* who = "eg3d_cloud_nearest_points";
  K18Thresholds t;
  BUF_TRY(check_query(who, c, ix, max_dist, stats, &t));
  if (n && !X_host) return refuse(EG3D_ERR_ARG, who, "X_host is NULL");
  if (n >= (1ull << 32)) return refuse(EG3D_ERR_CAPACITY, who, "2^32 points or more");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  eg3d_nearest_stats s = fresh_stats(stats);
  const auto w0 = std::chrono::steady_clock::now();
  if (n) {
    BUF_TRY(upload(ix->u_X, X_host, 3 * n, st));
    if (keep_host) BUF_TRY(upload(ix->u_keep, keep_host, n, st));
    if (nn_out_host) BUF_TRY(ix->q_nn.ensure(sizeof(uint32_t) * n));
    BUF_TRY(ix->q_d2.ensure(sizeof(float) * n));
  }
  const int rc = run_query(c, ix, ix->u_X.as<float>(), n, keep_host ? ix->u_keep.as<uint8_t>() : nullptr, max_dist, t, ix->q_d2.as<float>(),
                           nn_out_host ? ix->q_nn.as<uint32_t>() : nullptr, &s);
  if (rc != EG3D_OK) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (n) {
    if (d2_out_host) HIP_TRY(hipMemcpyAsync(d2_out_host, ix->q_d2.p, sizeof(float) * n, hipMemcpyDeviceToHost, st));
    if (nn_out_host) HIP_TRY(hipMemcpyAsync(nn_out_host, ix->q_nn.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  s.ms_copy = std::max(0.f, wall - s.ms_kernel);
  if (stats) *stats = s;
  return EG3D_OK;
}
