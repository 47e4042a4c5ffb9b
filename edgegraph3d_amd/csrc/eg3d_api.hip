// eg3d_api.hip — implementation of the C ABI declared in include/eg3d.h.
//
// Host orchestration of the phase pipeline: HBM-resident scene (cameras, F, polyline CSR, the
// two uniform grids), resident seeds, grow-only device work buffers, rocPRIM/hipCUB exclusive
// scans between phases, HIP events for per-stage timing. No CPU fallback exists: every entry
// point fails with EG3D_ERR_NODEVICE / EG3D_ERR_HIP when no gfx950 device is usable.
//
// This file: the context (create, clone, destroy), the grids, the seeds, eg3d_gn_filter, the probes, and the definitions of
// what eg3d_api_internal.h declares — the only place that includes hipCUB. The match pipeline is in eg3d_api_match.hip, the
// post stages' drivers in eg3d_api_filter / _replay / _polymatch / _simgraph / _louvain.hip.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/eg3d_host.h"
#include "eg3d_api_internal.h"
#include "eg3d_host_copy.h"

thread_local std::string eg3d::api::g_err;
extern "C" const char* eg3d_last_error(void) { return g_err.c_str(); }

// ---- the one place device memory is allocated and freed -------------------------------------------------------------------
static std::atomic<int64_t> g_live_device_bytes{0};
/* Tests only, not declared in include/eg3d.h (tests/test_gpu_buffer_ownership.py): bytes of device memory the library holds
 * in this process, over all contexts. */
extern "C" int64_t eg3d_test_live_device_bytes(void) { return g_live_device_bytes.load(); }
EG3D_API_BEGIN
int dev_alloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    g_err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
    return EG3D_ERR_HIP;
  }
  g_live_device_bytes += (int64_t)bytes;
  return EG3D_OK;
}
void dev_free(void* p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  g_live_device_bytes -= (int64_t)bytes;
}
int DevBuf::ensure_keep(size_t bytes, size_t keep, hipStream_t st) {
  if (bytes <= cap && p) return EG3D_OK;
  if (!p || !keep) return ensure(bytes);
  void* q = nullptr;
  const size_t q_cap = bytes + bytes / 2;
  BUF_TRY(dev_alloc(&q, q_cap));
  hipError_t e = hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    dev_free(q, q_cap);
    g_err = std::string("growing a device buffer: ") + hipGetErrorString(e);
    return EG3D_ERR_HIP;
  }
  release();
  p = q;
  cap = q_cap;
  return EG3D_OK;
}
EG3D_API_END


int eg3d::api::scan_exclusive_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one) {
  // in[n] must be 0 (or ignored): out[n] = total
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, out, (int)n_plus_one, c->stream));
  BUF_TRY(c->b_scan_tmp.ensure(tmp_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->b_scan_tmp.p, tmp_bytes, in, out, (int)n_plus_one, c->stream));
  return EG3D_OK;
}
EG3D_API_BEGIN
// ---- small read-backs through the mailbox ----------------------------------------------------------
// b_scanchk: [0..3] "scan wrapped" flag words (ORed by k_scan_check, cleared by k_publish), [4..5] a saved
// 64-bit counter.
int ensure_mailbox(eg3d_ctx* c) {
  if (!c->mbox) {
    void* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, sizeof(uint32_t) * EG3D_MBOX_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
    memset(h, 0, sizeof(uint32_t) * EG3D_MBOX_WORDS);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipHostFree(h);
      g_err = "eg3d: hipHostGetDevicePointer failed for the read-back mailbox";
      return EG3D_ERR_HIP;
    }
    c->mbox = (uint32_t*)h;
    c->mbox_dev = (uint32_t*)d;
  }
  if (!c->b_scanchk.p) {
    BUF_TRY(c->b_scanchk.ensure(8 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->b_scanchk.p, 0, 8 * sizeof(uint32_t), c->stream));
  }
  return EG3D_OK;
}
int Readback::run() {
  if (a.n > 6 || a.n_clear > 3 || used > EG3D_MBOX_WORDS) {
    g_err = "eg3d: internal: read-back too large";
    return EG3D_ERR_ARG;
  }
  const uint32_t seq = ++c->mbox_seq;
  launch_publish(c->stream, a, c->mbox_dev, seq);
  HIP_TRY(hipGetLastError());
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spin = 0;; spin++) {
    if (__atomic_load_n(c->mbox, __ATOMIC_ACQUIRE) == seq) return EG3D_OK;
    __builtin_ia32_pause();
    if ((spin & 255u) == 255u &&
        std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1500))
      break;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (__atomic_load_n(c->mbox, __ATOMIC_ACQUIRE) != seq) {
    g_err = "eg3d: the read-back mailbox was not written";
    return EG3D_ERR_HIP;
  }
  return EG3D_OK;
}
// Exclusive scan queued on the stream, its wrap check ORed into flag word `slot`; the total is out[n].
int scan_queue_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one, int slot) {
  BUF_TRY(ensure_mailbox(c));
  BUF_TRY(scan_exclusive_u32(c, in, out, n_plus_one));
  launch_scan_check(c->stream, out, n_plus_one, c->b_scanchk.as<uint32_t>() + slot);
  return EG3D_OK;
}
int wrapped_error(const char* what) {
  g_err = std::string("eg3d: the number of ") + what + " of this batch exceeds 2^32-1; use smaller seed / set ranges";
  return EG3D_ERR_CAPACITY;
}
// Exclusive scan + its total on the host, with overflow detection: phase totals (candidate slots,
// tasks, lists, hits, hypotheses) are 32-bit; a batch whose total does not fit is refused with
// EG3D_ERR_CAPACITY instead of sizing buffers from a wrapped number.
int scan_total_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one, uint32_t& total, const char* what) {
  BUF_TRY(scan_queue_u32(c, in, out, n_plus_one, 0));
  Readback rb(c);
  const int it = rb.add(out + (n_plus_one - 1), 1);
  const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 1);
  rb.clear_after(c->b_scanchk.as<uint32_t>());
  BUF_TRY(rb.run());
  if (*rb.item(iw)) return wrapped_error(what);
  total = *rb.item(it);
  return EG3D_OK;
}
EG3D_API_END

// K0: one uniform grid of the scene `sc` on the device (its polylines are already resident: sc.ds), queued on c's stream
// with c's scratch — in eg3d_create `sc` is the scene being made, which the context does not share yet: count the (cell,
// polyline) pairs of every polyline, exclusive scan, write them as 64-bit keys, radix sort, unique, CSR. The temporaries (24 B
// per pair) belong to the caller, which frees them once the stream has drained.
struct GridTemps {
  DevBuf cnt, off, keys, keys2, n;  // n: [0] unique keys, [1] samples outside the image (summed over the builds)
};
static int build_grid_device(eg3d_ctx* c, const SceneFacts& sc, float cell, GridTemps& t, DevBuf& g_off, DevBuf& g_ids,
                             uint32_t* out_w, uint32_t* out_h, uint32_t* dropped) {
  hipStream_t st = c->stream;
  const int V = sc.V;
  const uint32_t NP = sc.n_pl;
  if (!t.n.p) {
    BUF_TRY(t.n.ensure(2 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(t.n.p, 0, 2 * sizeof(uint32_t), st));
  }
  const int map_w = (int)std::ceil(sc.W / cell), map_h = (int)std::ceil(sc.H / cell);  // (as host/grid_build.cpp: float division)
  *out_w = (uint32_t)map_w;
  *out_h = (uint32_t)map_h;
  const unsigned long long total_cells = (unsigned long long)V * (unsigned long long)map_w * (unsigned long long)map_h;
  if (total_cells >= 0xffffffffull) {
    g_err = "eg3d: the scene's grids have more than 2^32-2 cells";
    return EG3D_ERR_CAPACITY;
  }
  BUF_TRY(t.cnt.ensure(sizeof(uint32_t) * ((size_t)NP + 1)));
  BUF_TRY(t.off.ensure(sizeof(uint32_t) * ((size_t)NP + 1)));
  HIP_TRY(hipMemsetAsync(t.cnt.as<uint32_t>() + NP, 0, sizeof(uint32_t), st));
  launch_k0_pairs(st, false, sc.ds, NP, cell, map_w, map_h, t.cnt.as<uint32_t>(), nullptr, nullptr, t.n.as<uint32_t>() + 1);
  uint32_t n_pairs = 0;
  BUF_TRY(scan_total_u32(c, t.cnt.as<uint32_t>(), t.off.as<uint32_t>(), (size_t)NP + 1, n_pairs, "(cell, polyline) entries of the grids"));
  BUF_TRY(g_off.ensure(sizeof(uint32_t) * ((size_t)total_cells + 1)));
  uint32_t n_unique = 0;
  {
    if (n_pairs) {
      BUF_TRY(t.keys.ensure(sizeof(unsigned long long) * (size_t)n_pairs));
      BUF_TRY(t.keys2.ensure(sizeof(unsigned long long) * (size_t)n_pairs));
      launch_k0_pairs(st, true, sc.ds, NP, cell, map_w, map_h, nullptr, t.off.as<uint32_t>(), t.keys.as<unsigned long long>(), nullptr);
      int end_bit = EG3D_K0_PL_BITS_HOST;
      while (end_bit < 64 && (total_cells >> (end_bit - EG3D_K0_PL_BITS_HOST)) != 0) end_bit++;
      size_t tmp = 0;
      HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, t.keys.as<unsigned long long>(), t.keys2.as<unsigned long long>(),
                                                (int)n_pairs, 0, end_bit, st));
      BUF_TRY(c->b_scan_tmp.ensure(tmp));
      HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->b_scan_tmp.p, tmp, t.keys.as<unsigned long long>(), t.keys2.as<unsigned long long>(),
                                                (int)n_pairs, 0, end_bit, st));
      tmp = 0;
      HIP_TRY(hipcub::DeviceSelect::Unique(nullptr, tmp, t.keys2.as<unsigned long long>(), t.keys.as<unsigned long long>(),
                                           t.n.as<uint32_t>(), (int)n_pairs, st));
      BUF_TRY(c->b_scan_tmp.ensure(tmp));
      HIP_TRY(hipcub::DeviceSelect::Unique(c->b_scan_tmp.p, tmp, t.keys2.as<unsigned long long>(), t.keys.as<unsigned long long>(),
                                           t.n.as<uint32_t>(), (int)n_pairs, st));
      Readback rb(c);
      const int in = rb.add(t.n.p, 2);
      BUF_TRY(rb.run());
      n_unique = rb.item(in)[0];
      *dropped = rb.item(in)[1];  // (every cell size built with `t` so far has been counted by now)
    }
    BUF_TRY(g_ids.ensure(sizeof(uint32_t) * std::max<size_t>(n_unique, 1)));
    if (n_unique)
      launch_k0_csr(st, t.keys.as<unsigned long long>(), n_unique, (uint32_t)total_cells, (uint32_t*)g_off.p, (uint32_t*)g_ids.p);
    else
      HIP_TRY(hipMemsetAsync(g_off.p, 0, sizeof(uint32_t) * ((size_t)total_cells + 1), st));
  }
  return EG3D_OK;
}
// eg3d_create: the 30 px and 4 px grids on the device.
static int build_grids_device(eg3d_ctx* c, Scene& s) {
  GridTemps t;
  for (int which = 0; which < 2; which++)
    BUF_TRY(build_grid_device(c, s, which == 0 ? 30.0f : 4.0f, t, s.g_off[which], s.g_ids[which], &s.gw[which], &s.gh[which],
                              &s.grid_dropped));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the temporaries go away
  return EG3D_OK;
}
int eg3d::api::ensure_grid10(eg3d_ctx* c, K9Grid* out, float* ms) {
  Scene& s = *c->scene;
  std::lock_guard<std::mutex> lk(s.mu);
  if (!s.built10) {
    const auto t0 = std::chrono::steady_clock::now();
    // (the build runs on the calling context's stream and scratch; `mu` only keeps a second context of the family from
    // building the same map at the same time)
    GridTemps t;
    uint32_t dropped = 0;
    int rc = build_grid_device(c, s, 10.0f, t, s.g_off[2], s.g_ids[2], &s.w10, &s.h10, &dropped);
    if (rc == EG3D_OK && hipStreamSynchronize(c->stream) != hipSuccess) {
      g_err = "eg3d_match_polylines_closeness: building the 10 px map failed";
      rc = EG3D_ERR_HIP;
    }
    if (rc != EG3D_OK) {
      (void)hipStreamSynchronize(c->stream);
      s.g_off[2].release();
      s.g_ids[2].release();
      return rc;
    }
    s.built10 = true;
    if (ms) *ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  out->w = (int32_t)s.w10;
  out->h = (int32_t)s.h10;
  out->off = s.d_off(2);
  out->ids = s.d_ids(2);
  return EG3D_OK;
}

// (defined behind the grid builders: the library's hipCUB kernels keep the order they were instantiated in)
int eg3d::api::sort_pairs_desc_u32(eg3d_ctx* c, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                                   uint32_t* vals_out, uint32_t n) {
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 32, c->stream));
  BUF_TRY(c->b_scan_tmp.ensure(tmp_bytes));
  HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(c->b_scan_tmp.p, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 32, c->stream));
  return EG3D_OK;
}

extern "C" int eg3d_dlt_rows(void) { return EG3D_DLT_ROWS; }

extern "C" int eg3d_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Everything about a scene that can be checked on the host, before a device is touched: the library indexes
// device arrays with these offsets and ids, so an inconsistent scene is refused here instead of faulting there.
static int validate_scene(const eg3d_scene* sc) {
  if (sc->n_views < 1 || sc->width < 1 || sc->height < 1 || !sc->cam_P || !sc->F || !sc->F_valid || !sc->view_pl_off ||
      !sc->pl_vtx_off || !sc->pl_start || !sc->pl_end || !sc->pl_valid) {
    g_err = "eg3d_create: bad arguments (null array, no views or empty image)";
    return EG3D_ERR_ARG;
  }
  if (sc->n_views > EG3D_MAX_VIEWS) {
    g_err = "eg3d_create: more than " + std::to_string(EG3D_MAX_VIEWS) + " views";
    return EG3D_ERR_CAPACITY;
  }
  if (sc->view_pl_off[0] != 0) {
    g_err = "eg3d_create: view_pl_off[0] must be 0";
    return EG3D_ERR_ARG;
  }
  for (int v = 0; v < sc->n_views; v++) {
    if (sc->view_pl_off[v + 1] < sc->view_pl_off[v]) {
      g_err = "eg3d_create: view_pl_off is not ascending";
      return EG3D_ERR_ARG;
    }
    if (sc->view_pl_off[v + 1] - sc->view_pl_off[v] > (uint32_t)EG3D_MAX_POLYLINES_PER_VIEW) {
      g_err = "eg3d_create: a view has more than " + std::to_string(EG3D_MAX_POLYLINES_PER_VIEW) + " polylines";
      return EG3D_ERR_CAPACITY;
    }
  }
  const uint32_t np_all = sc->view_pl_off[sc->n_views];
  if (sc->pl_vtx_off[0] != 0) {
    g_err = "eg3d_create: pl_vtx_off[0] must be 0";
    return EG3D_ERR_ARG;
  }
  for (uint32_t p = 0; p < np_all; p++)
    if (sc->pl_vtx_off[p + 1] < sc->pl_vtx_off[p]) {
      g_err = "eg3d_create: pl_vtx_off is not ascending";
      return EG3D_ERR_ARG;
    }
  if (sc->pl_vtx_off[np_all] && !sc->vtx_xy) {
    g_err = "eg3d_create: vtx_xy is null";
    return EG3D_ERR_ARG;
  }
  // Vertex coordinates of valid polylines must be finite and within +-1e7 px. The grid construction samples
  // every segment each ~2.6 px (polyline_graph_2d.cpp:819-835) whether or not it lies inside the image: a stray
  // 1e20 coordinate would keep the reference (and this library's host grid builder) sampling for years, and a
  // NaN makes its cell conversions undefined. Such a scene is refused instead.
  for (uint32_t p = 0; p < np_all; p++) {
    if (!sc->pl_valid[p]) continue;
    for (size_t k = 2 * (size_t)sc->pl_vtx_off[p]; k < 2 * (size_t)sc->pl_vtx_off[p + 1]; k++)
      if (!(std::fabs(sc->vtx_xy[k]) <= 1e7f)) {
        g_err = "eg3d_create: polyline " + std::to_string(p) + " has a vertex coordinate that is not finite or beyond +-1e7 px";
        return EG3D_ERR_ARG;
      }
  }
  return EG3D_OK;
}

// ---- eg3d_create, step by step (the list is at the end) ---------------------------------------------------------------------
int eg3d::api::make_own_resources(eg3d_ctx* c, StreamPrio prio) {
  if (prio == StreamPrio::plain) {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  } else {
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int priority = prio == StreamPrio::greatest ? greatest : prio == StreamPrio::middle ? (least + greatest) / 2 : least;
    HIP_TRY(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, priority));
  }
  for (int i = 0; i < 8; i++) {
    HIP_TRY(hipEventCreate(&c->ea[i]));
    HIP_TRY(hipEventCreate(&c->eb[i]));
  }
  for (int i = 0; i < 7; i++) HIP_TRY(hipEventCreateWithFlags(&c->ecopy[i], hipEventDisableTiming));
  return EG3D_OK;
}

// An invalid polyline (pl_valid == 0) is one the reference has invalidated: it keeps its id but its
// coordinates are cleared (polyline_graph_2d.cpp:1047-1058, Q8). The ABI tolerates a caller that
// leaves vertices on such a polyline; the device must not see them (the polyline-sets path takes
// raw polyline ids), so they are dropped here: compacted vertex array, zero-length slices.
namespace {
struct SceneVertices {
  std::vector<uint32_t> pvo_c;
  std::vector<float> vtx_c;
  const uint32_t* pvo = nullptr;  // the caller's arrays, or the compacted ones above
  const float* vtx = nullptr;
};
}  // namespace
static void drop_invalid_vertices(const eg3d_scene* sc, uint32_t NP, SceneVertices& a) {
  a.pvo = sc->pl_vtx_off;
  a.vtx = sc->vtx_xy;
  bool stray = false;
  for (uint32_t p = 0; p < NP && !stray; p++) stray = !sc->pl_valid[p] && sc->pl_vtx_off[p + 1] > sc->pl_vtx_off[p];
  if (!stray) return;
  a.pvo_c.assign(1, 0);
  for (uint32_t p = 0; p < NP; p++) {
    if (sc->pl_valid[p])
      a.vtx_c.insert(a.vtx_c.end(), sc->vtx_xy + 2 * (size_t)sc->pl_vtx_off[p], sc->vtx_xy + 2 * (size_t)sc->pl_vtx_off[p + 1]);
    a.pvo_c.push_back((uint32_t)(a.vtx_c.size() / 2));
  }
  if (a.vtx_c.empty()) a.vtx_c.assign(2, 0.f);
  a.pvo = a.pvo_c.data();
  a.vtx = a.vtx_c.data();
}

static int upload_scene_arrays(eg3d_ctx* c, Scene& s, const eg3d_scene* sc, const SceneVertices& a) {
  const size_t V = (size_t)s.V;
  // (A plain shorthand now: it destroys nothing, the caller's guard does. It keeps its name and first line because
  // build.device_source_fingerprint() hashes the preprocessor lines of this file, and the committed PMC profile
  // (profiles/pmc_traffic.json) is valid for exactly that hash; whoever regenerates the profile can write the calls out.)
#define UP(buf, ptr, n)                                        \
  BUF_TRY(upload(s.buf, ptr, (size_t)(n), c->stream))
  UP(camP, sc->cam_P, V * 16);
  UP(F, sc->F, V * V * 9);
  UP(Fv, sc->F_valid, V * V);
  UP(vpo, sc->view_pl_off, V + 1);
  UP(pvo, a.pvo, (size_t)s.n_pl + 1);
  UP(vtx, a.vtx, (size_t)s.n_vtx * 2);
  UP(pls, sc->pl_start, s.n_pl);
  UP(ple, sc->pl_end, s.n_pl);
#undef UP
  DevScene& d = s.ds;
  d.n_views = s.V;
  d.width = s.W;
  d.height = s.H;
  d.cam_P = s.camP.as<float>();
  d.F = s.F.as<double>();
  d.F_valid = s.Fv.as<uint8_t>();
  d.view_pl_off = s.vpo.as<uint32_t>();
  d.pl_vtx_off = s.pvo.as<uint32_t>();
  d.vtx = s.vtx.as<f2>();
  d.pl_start = s.pls.as<uint32_t>();
  d.pl_end = s.ple.as<uint32_t>();
  return EG3D_OK;
}

// bounding boxes of blocks of EG3D_BB_SEGS segments (the pre-test of the expand stage's closest-point scans)
static int upload_block_boxes(eg3d_ctx* c, Scene& s, const SceneVertices& a) {
  const uint32_t NP = s.n_pl;
  std::vector<uint32_t> bbo(NP + 1, 0);
  std::vector<float> bb;
  for (uint32_t p = 0; p < NP; p++) {
    const uint32_t v0 = a.pvo[p], v1 = a.pvo[p + 1];
    const uint32_t nseg = v1 > v0 + 1 ? v1 - v0 - 1 : 0;
    for (uint32_t s0 = 0; s0 < nseg; s0 += EG3D_BB_SEGS) {
      const uint32_t s1 = std::min(nseg, s0 + (uint32_t)EG3D_BB_SEGS);
      float x0 = a.vtx[2 * (size_t)(v0 + s0)], y0 = a.vtx[2 * (size_t)(v0 + s0) + 1], x1 = x0, y1 = y0;
      for (uint32_t i = s0 + 1; i <= s1; i++) {
        const float x = a.vtx[2 * (size_t)(v0 + i)], y = a.vtx[2 * (size_t)(v0 + i) + 1];
        x0 = std::min(x0, x);
        y0 = std::min(y0, y);
        x1 = std::max(x1, x);
        y1 = std::max(y1, y);
      }
      bb.insert(bb.end(), {x0, y0, x1, y1});
    }
    bbo[p + 1] = (uint32_t)(bb.size() / 4);
  }
  if (bb.empty()) bb.assign(4, 0.f);
  BUF_TRY(upload(s.bbo, bbo.data(), bbo.size(), c->stream));
  BUF_TRY(upload(s.bb, bb.data(), bb.size(), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // `bbo` / `bb` go out of scope
  s.ds.pl_bb_off = s.bbo.as<uint32_t>();
  s.ds.pl_bb = s.bb.as<float>();
  return EG3D_OK;
}

// Runs `work` on up to `n` threads, the caller included (at most EG3D_COPY_THREADS and what the machine has; when no more
// threads can be started, those that did start and the calling thread do what is left).
template <typename Work>
static void run_on_threads(unsigned n, Work work) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int nthr = (int)std::min<unsigned>(std::min<unsigned>(hw, EG3D_COPY_THREADS), n);
  std::vector<std::thread> th;
  try {
    for (int t = 1; t < nthr; t++) th.emplace_back(work);
  } catch (...) {
  }
  work();
  for (auto& t : th) t.join();
}

// EG3D_GRID_ON_HOST=1 (diagnostic): the host builder instead of K0 — the 2 x V builds are independent
// (polyLine_2d_map.cpp:40-58 constructs one map per view), so they run on a few host threads; serially, as until round 5,
// this was 2x the whole hot path of a dtu006-sized job (90 ms for C3', 0.87 s for C4). The per-view arrays are kept for
// eg3d_get_grid; the device CSR over (view, cell) is assembled on the same threads.
static int build_grids_host(eg3d_ctx* c, Scene& s, const eg3d_scene* sc) {
  const int V = s.V;
  struct GridJob {
    uint32_t w = 0, h = 0, dropped = 0, *o = nullptr, *i = nullptr;
    int rc = 0;
  };
  std::vector<GridJob> jobs((size_t)2 * V);
  struct FreeJobs {
    std::vector<GridJob>& j;
    ~FreeJobs() {
      for (auto& g : j) {
        free(g.o);
        free(g.i);
      }
    }
  } free_jobs{jobs};
  std::atomic<int> next{0};
  run_on_threads((unsigned)(2 * V), [&]() {
    for (int j; (j = next.fetch_add(1)) < 2 * V;) {
      GridJob& g = jobs[(size_t)j];
      // (the 4 px grids first: they are the long jobs)
      g.rc = eg3d_host_build_grid(sc, j % V, j < V ? 4.0f : 30.0f, &g.w, &g.h, &g.o, &g.i, &g.dropped);
    }
  });
  for (auto& g : jobs)
    if (g.rc != 0) {
      g_err = "eg3d_create: grid construction failed";
      return EG3D_ERR_ARG;
    }
  for (int which = 0; which < 2; which++) {
    const auto job_of = [&](int v) -> const GridJob& { return jobs[(size_t)(which == 0 ? V + v : v)]; };
    s.h_off[which].resize((size_t)V);
    s.h_ids[which].resize((size_t)V);
    std::vector<size_t> id_base((size_t)V + 1, 0), off_base((size_t)V + 1, 0);
    for (int v = 0; v < V; v++) {
      const GridJob& g = job_of(v);
      s.h_off[which][(size_t)v].assign(g.o, g.o + (size_t)g.w * g.h + 1);
      s.h_ids[which][(size_t)v].assign(g.i, g.i + g.o[(size_t)g.w * g.h]);
      s.gw[which] = g.w;
      s.gh[which] = g.h;
      s.grid_dropped += g.dropped;
      id_base[(size_t)v + 1] = id_base[(size_t)v] + g.o[(size_t)g.w * g.h];
      off_base[(size_t)v + 1] = off_base[(size_t)v] + (size_t)g.w * g.h;
    }
    s.have[which] = true;
    if (id_base[(size_t)V] > 0xffffffffull) {
      g_err = "eg3d_create: the grids of this scene hold more than 2^32-1 (cell, polyline) entries";
      return EG3D_ERR_CAPACITY;
    }
    std::vector<uint32_t> off(off_base[(size_t)V] + 1), ids(std::max<size_t>(id_base[(size_t)V], 1));
    off[0] = 0;
    std::atomic<int> nextv{0};
    run_on_threads((unsigned)V, [&]() {
      for (int v; (v = nextv.fetch_add(1)) < V;) {
        const GridJob& g = job_of(v);
        const size_t nc = (size_t)g.w * g.h;
        const uint32_t base = (uint32_t)id_base[(size_t)v];
        uint32_t* dst = off.data() + off_base[(size_t)v] + 1;
        for (size_t cc = 0; cc < nc; cc++) dst[cc] = base + g.o[cc + 1];
        if (g.o[nc]) memcpy(ids.data() + id_base[(size_t)v], g.i, sizeof(uint32_t) * g.o[nc]);
      }
    });
    BUF_TRY(upload(s.g_off[which], off.data(), off.size(), c->stream));
    BUF_TRY(upload(s.g_ids[which], ids.data(), ids.size(), c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) {  // `off`/`ids` go out of scope
      g_err = "eg3d_create: uploading the grids failed";
      return EG3D_ERR_HIP;
    }
  }
  return EG3D_OK;
}

// grids (row a3), one CSR over (view, cell) per cell size: built on the DEVICE (K0) from the polylines just uploaded
static int build_grids(eg3d_ctx* c, Scene& s, const eg3d_scene* sc) {
  BUF_TRY(c->tune.grid_on_host ? build_grids_host(c, s, sc) : build_grids_device(c, s));
  DevScene& d = s.ds;
  d.g30_w = (int)s.gw[0];
  d.g30_h = (int)s.gh[0];
  d.g4_w = (int)s.gw[1];
  d.g4_h = (int)s.gh[1];
  d.g30_off = s.d_off(0);
  d.g30_ids = s.d_ids(0);
  d.g4_off = s.d_off(1);
  d.g4_ids = s.d_ids(1);
  return EG3D_OK;
}

// every camera entry that is not zero lies in 2^-100 .. 2^100 (NaN fails)
static void flag_cams_mid_range(Scene& s, const eg3d_scene* sc) {
  bool mid = true;
  for (size_t v = 0; v < (size_t)s.V && mid; v++)
    for (int k = 0; k < 12 && mid; k++) {
      const float p = sc->cam_P[v * 16 + k];
      if (p != 0.0f) {
        const float a = p < 0 ? -p : p;
        mid = a >= 7.888609052210118e-31f && a <= 1.2676506002282294e+30f;
      }
    }
  s.ds.cams_mid_range = mid ? 1 : 0;
}

// What the expand stage starts from: the scene's longest polyline, the context's first capacities, and the slot pools
// sized from the occupancy query.
static int size_pools_and_slots(eg3d_ctx* c, Scene& s, const eg3d_scene* sc) {
  // the longest valid polyline of the scene (a scene whose polylines all fit the side walks' LDS staging area, and
  // that has few views, runs the smaller build of the expand kernel: launch_k3b)
  for (uint32_t p = 0; p < s.n_pl; p++)
    if (sc->pl_valid[p]) s.max_pl_vtx = std::max(s.max_pl_vtx, sc->pl_vtx_off[p + 1] - sc->pl_vtx_off[p]);
  // observation slots per chain (blocks double when they fill, so budget ~3x the live count);
  // grown automatically when a chain overflows
  // (many-view scenes: points carry ~V/3 observations and blocks are relocated as they double — C4 settles at 196 608; starting
  // at 24 576 as until round 6 cost the first call three extra rounds of the expand stage)
  Learned& L = c->learned;
  L.pool_cap = std::min<uint32_t>(131072, 768u * (uint32_t)std::min(s.V, 128));
  if (L.pool_cap < 6144) L.pool_cap = 6144;
  if (c->tune.pool_cap0) L.pool_cap = c->tune.pool_cap0;
  if (c->tune.chain_cap0) L.chain_cap = c->tune.chain_cap0;
  const int device = s.device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  s.n_simd = (uint32_t)prop.multiProcessorCount * 4;
  if (hipDeviceGetAttribute(&s.wall_clock_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) s.wall_clock_khz = 0;
  // working-slice slots per XCD: what can be resident (occupancy query x CUs of an XCD) plus a margin —
  // the occupancy API may be one block per CU off, and a pool must never be smaller than the residency
  const int per_cu = k3b_blocks_per_cu();
  if (per_cu < 1) {
    g_err = "eg3d_create: occupancy query of the expand kernel failed";
    return EG3D_ERR_HIP;
  }
  // XCDs of THIS device: 8 on the whole MI355X (32 CUs each), fewer when the GPU is partitioned (CPX: one XCD of 32
  // CUs appears as a device, DPX / QPX: four / two) — all its blocks then draw from the pools of those XCDs only, so a
  // pool is sized for CUs / XCDs compute units, not for an eighth of whatever the device reports
  const uint32_t cus = (uint32_t)prop.multiProcessorCount;
  const uint32_t n_xcd = std::min(8u, std::max(1u, cus / 32u));
  // (at least 40: an XCD of 38 CUs on a part with fewer than 8 XCDs would be undersized by the estimate cus / 32 — the
  // pools cost a few tens of MB more on gfx950, where an XCD has 32)
  const uint32_t cus_per_xcd = std::max<uint32_t>((cus + n_xcd - 1u) / n_xcd, 40u);
  s.slots_per_xcd = ((uint32_t)per_cu + 1u) * cus_per_xcd + 16u;
  if (c->tune.slots_per_xcd) s.slots_per_xcd = c->tune.slots_per_xcd;  // tests / experiments
  // (the lane-per-chain engine is an opt-in second form: only a context that asks for it depends on its kernel)
  if (c->tune.k3b_engine != 0) {
#ifdef EG3D_WITH_K3C_ENGINE
    s.k3c_per_cu = k3c_blocks_per_cu();
    if (s.k3c_per_cu < 1) {
      g_err = "eg3d_create: occupancy query of the expand engine failed";
      return EG3D_ERR_HIP;
    }
#else
    g_err = "eg3d_create: EG3D_K3B_ENGINE=1, but this library was built without the lane-per-chain engine "
            "(-DEG3D_WITH_K3C_ENGINE: edgegraph3d_amd/variants/libeg3d_engine.so)";
    return EG3D_ERR_ARG;
#endif
  }
  return EG3D_OK;
}

extern "C" int eg3d_create(const eg3d_scene* sc, int device, eg3d_ctx** out) {
  if (!sc || !out) {
    g_err = "eg3d_create: bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(validate_scene(sc));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_err = "eg3d_create: no HIP device available (this library has no CPU fallback)";
    return EG3D_ERR_NODEVICE;
  }
  if (device < 0 || device >= ndev) {
    g_err = "eg3d_create: device index out of range";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(device));
  // (declared in this order: a failing exit first drains and destroys the context, then lets the scene's arrays go)
  auto scene = std::make_shared<Scene>();
  CtxGuard guard(new eg3d_ctx(), eg3d_destroy);
  eg3d_ctx* c = guard.get();
  Scene& s = *scene;
  s.device = c->device = device;  // (the context's own copy: eg3d_destroy works on a context that shares no scene yet)
  s.V = sc->n_views;
  s.W = sc->width;
  s.H = sc->height;
  c->seeds = std::make_shared<Seeds>(device);
  c->tune = Tunables::from_env();
  if (c->tune.hyp_cap) c->learned.hyp_cap = c->tune.hyp_cap;
  BUF_TRY(make_own_resources(c, c->tune.lane_priorities ? StreamPrio::greatest : StreamPrio::plain));
  SceneVertices vertices;
  s.n_pl = sc->view_pl_off[s.V];
  drop_invalid_vertices(sc, s.n_pl, vertices);
  s.n_vtx = vertices.pvo[s.n_pl];
  BUF_TRY(upload_scene_arrays(c, s, sc, vertices));
  BUF_TRY(upload_block_boxes(c, s, vertices));
  BUF_TRY(build_grids(c, s, sc));
  flag_cams_mid_range(s, sc);
  BUF_TRY(size_pools_and_slots(c, s, sc));
  HIP_TRY(hipStreamSynchronize(c->stream));
  share_scene(c, std::move(scene));
  *out = guard.release();
  return EG3D_OK;
}

/* A second context on the same device that SHARES the parent's immutable scene (cameras, F,
 * polylines, grids) and its currently resident seeds, with its own stream, events and work
 * buffers: the way to keep several independent batches in flight (one host thread per context). */
int eg3d::api::clone_ctx(eg3d_ctx* parent, StreamPrio prio, eg3d_ctx** out) {
  HIP_TRY(hipSetDevice(parent->device));
  CtxGuard c(new eg3d_ctx(), eg3d_destroy);
  share_scene(c.get(), parent->scene);
  c->seeds = parent->seeds;
  c->tune = parent->tune;
  c->learned = parent->learned;
  BUF_TRY(make_own_resources(c.get(), prio));
  *out = c.release();
  return EG3D_OK;
}
extern "C" int eg3d_clone(eg3d_ctx* parent, eg3d_ctx** out) {
  if (!parent || !out) {
    g_err = "eg3d_clone: bad arguments";
    return EG3D_ERR_ARG;
  }
  return clone_ctx(parent, StreamPrio::plain, out);
}

extern "C" void eg3d_destroy(eg3d_ctx* c) {
  if (!c) return;
  for (size_t l = 1; l < c->lanes.size(); l++) eg3d_destroy(c->lanes[l]);  // (lane 0 is the context itself)
  c->lanes.clear();
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->mbox) (void)hipHostFree(c->mbox);
  for (int i = 0; i < 8; i++) {
    if (c->ea[i]) (void)hipEventDestroy(c->ea[i]);
    if (c->eb[i]) (void)hipEventDestroy(c->eb[i]);
  }
  for (int i = 0; i < 7; i++)
    if (c->ecopy[i]) (void)hipEventDestroy(c->ecopy[i]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  // (nothing is queued on the stream any more: the work buffers release themselves, and the scene and the seeds go with
  // the last context that shares them)
  delete c;
}

extern "C" int eg3d_get_grid(eg3d_ctx* c, int view, int which, uint32_t* ncols, uint32_t* nrows,
                             const uint32_t** cell_off, const uint32_t** ids) {
  if (!c || view < 0 || view >= c->V || which < 0 || which > 2) {
    g_err = "eg3d_get_grid: bad arguments";
    return EG3D_ERR_ARG;
  }
  Scene& s = *c->scene;
  {
    std::lock_guard<std::mutex> lk(s.mu);
    if (which == 2 && !s.built10) {
      g_err = "eg3d_get_grid: the 10 px map does not exist before the first eg3d_match_polylines_closeness call";
      return EG3D_ERR_ARG;
    }
    if (!s.have[which]) {  // first request for this cell size: fetch the device CSR and cut it into per-view CSRs
      HIP_TRY(hipSetDevice(s.device));
      const size_t cpv = s.cells_per_view(which), V = (size_t)s.V;
      std::vector<uint32_t> off(V * cpv + 1);
      HIP_TRY(hipMemcpy(off.data(), s.d_off(which), sizeof(uint32_t) * off.size(), hipMemcpyDeviceToHost));
      std::vector<uint32_t> all(std::max<size_t>(off.back(), 1));
      if (off.back()) HIP_TRY(hipMemcpy(all.data(), s.d_ids(which), sizeof(uint32_t) * off.back(), hipMemcpyDeviceToHost));
      s.h_off[which].resize(V);
      s.h_ids[which].resize(V);
      for (size_t v = 0; v < V; v++) {
        const uint32_t base = off[v * cpv];
        s.h_off[which][v].resize(cpv + 1);
        for (size_t cc = 0; cc <= cpv; cc++) s.h_off[which][v][cc] = off[v * cpv + cc] - base;
        s.h_ids[which][v].assign(all.begin() + base, all.begin() + off[(v + 1) * cpv]);
      }
      s.have[which] = true;
    }
  }
  *ncols = which == 2 ? s.w10 : c->gw[which];
  *nrows = which == 2 ? s.h10 : c->gh[which];
  *cell_off = s.h_off[which][(size_t)view].data();
  *ids = s.h_ids[which][(size_t)view].data();
  return EG3D_OK;
}

extern "C" int eg3d_upload_seeds(eg3d_ctx* c, const eg3d_seeds* s) {
  if (!c || !s) {
    g_err = "eg3d_upload_seeds: bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (!s->trk_off || (s->n_seeds && s->trk_off[s->n_seeds] && (!s->trk_view || !s->trk_xy))) {
    g_err = "eg3d_upload_seeds: null array";
    return EG3D_ERR_ARG;
  }
  const uint32_t n = s->n_seeds;
  if (s->trk_off[0] != 0) {
    g_err = "eg3d_upload_seeds: trk_off[0] must be 0";
    return EG3D_ERR_ARG;
  }
  for (uint32_t i = 0; i < n; i++)
    if (s->trk_off[i + 1] < s->trk_off[i]) {
      g_err = "eg3d_upload_seeds: trk_off is not ascending";
      return EG3D_ERR_ARG;
    }
  const uint32_t m = s->trk_off[n];
  for (uint32_t i = 0; i < m; i++)
    if (s->trk_view[i] < 0 || s->trk_view[i] >= c->V) {
      g_err = "eg3d_upload_seeds: view id out of range";
      return EG3D_ERR_ARG;
    }
  // A fresh object: the previous one may still be in use by clones of this context. The context lets go of it first (its
  // arrays are freed before the new ones are allocated when nobody else holds them) and has no seeds if the upload fails.
  c->seeds = std::make_shared<Seeds>(c->device);
  auto fresh = std::make_shared<Seeds>(c->device);
  BUF_TRY(upload(fresh->toff, s->trk_off, n + 1, c->stream));
  BUF_TRY(upload(fresh->tview, s->trk_view, m, c->stream));
  BUF_TRY(upload(fresh->txy, s->trk_xy, (size_t)m * 2, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  fresh->trk_off.assign(s->trk_off, s->trk_off + n + 1);
  fresh->n_seeds = n;
  c->seeds = std::move(fresh);
  return EG3D_OK;
}

extern "C" int eg3d_gn_filter(eg3d_ctx* c, const float* X, const uint32_t* obs_off, const int32_t* obs_view,
                              const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
                              uint8_t* inlier, float* ms_kernel) {
  if (!c || !X || !obs_off || !X_out || !inlier) {
    g_err = "eg3d_gn_filter: bad arguments";
    return EG3D_ERR_ARG;
  }
  if (n >= 0xffffffffull) {
    g_err = "eg3d_gn_filter: more than 2^32-2 points in one call";
    return EG3D_ERR_CAPACITY;
  }
  if (n && obs_off[0] != 0) {
    g_err = "eg3d_gn_filter: obs_off[0] must be 0";
    return EG3D_ERR_ARG;
  }
  for (uint64_t i = 0; i < n; i++)
    if (obs_off[i + 1] < obs_off[i]) {
      g_err = "eg3d_gn_filter: obs_off is not ascending";
      return EG3D_ERR_ARG;
    }
  const uint64_t m = n ? obs_off[n] : 0;
  if (m && (!obs_view || !obs_xy)) {
    g_err = "eg3d_gn_filter: null observation arrays";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  for (uint64_t i = 0; i < m; i++)
    if (obs_view[i] < 0 || obs_view[i] >= c->V) {
      g_err = "eg3d_gn_filter: view id out of range";
      return EG3D_ERR_ARG;
    }
  hipStream_t st = c->stream;
  BUF_TRY(upload(c->f_X, X, n * 3, st));
  BUF_TRY(upload(c->f_off, obs_off, n + 1, st));
  BUF_TRY(upload(c->f_view, obs_view, m, st));
  BUF_TRY(upload(c->f_xy, obs_xy, m * 2, st));
  BUF_TRY(c->f_Xo.ensure(sizeof(float) * 3 * (n + 1)));
  BUF_TRY(c->f_inl.ensure(n + 1));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k5(st, c->ds.cam_P, c->V, c->f_X.as<float>(), c->f_off.as<uint32_t>(), c->f_view.as<int32_t>(), c->f_xy.as<float>(),
            n, gn_max_mse, legacy_abs, c->f_Xo.as<float>(), c->f_inl.as<uint8_t>());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  if (n) {
    HIP_TRY(hipMemcpyAsync(X_out, c->f_Xo.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(inlier, c->f_inl.p, n, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (ms_kernel) HIP_TRY(hipEventElapsedTime(ms_kernel, c->ea[0], c->eb[0]));
  return EG3D_OK;
}

// ---- the filter and the compaction on a device-resident cloud ----------------------------------------------------------
extern "C" int eg3d_context_info(eg3d_ctx* c, int32_t* n_views, int32_t* device) {
  if (!c) {
    g_err = "eg3d_context_info: bad arguments";
    return EG3D_ERR_ARG;
  }
  if (n_views) *n_views = c->V;
  if (device) *device = c->device;
  return EG3D_OK;
}
CloudView eg3d::api::cloud_view(const eg3d_device_edgepoints* d) {
  return CloudView{d->n_points, d->n_obs, d->X, d->obs_off, d->obs_view, d->obs_pl, d->obs_seg, d->obs_xy, d->key};
}
int eg3d::api::check_cloud(const eg3d_device_edgepoints* d, const char* who, bool all_arrays) {
  const bool pts = !d->n_points || (d->X && d->obs_off && (!all_arrays || d->key));
  const bool obs = !d->n_obs || (d->obs_view && d->obs_xy && (!all_arrays || (d->obs_pl && d->obs_seg)));
  if (!pts || !obs || (d->n_obs && !d->n_points)) {
    g_err = std::string(who) + ": the device view has null arrays";
    return EG3D_ERR_ARG;
  }
  if (!d->complete) {
    g_err = std::string(who) + ": the device view does not hold a whole cloud (complete == 0)";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}
int eg3d::api::device_flags_error(const char* who, uint32_t flags) {
  if (flags & K5_FLAG_BAD_VIEW)
    g_err = std::string(who) + ": view id out of range";
  else
    g_err = std::string(who) + ": obs_off is not ascending within [0, n_obs], or a list holds more than 2^24 observations";
  return EG3D_ERR_ARG;
}

// ---- eg3d_api_internal.h: one copy of each idiom of the post stages -------------------------------------------------------
EG3D_API_BEGIN
int check_struct_size(const char* who, const char* type_name, size_t got, size_t want, const char* arg) {
  if (got >= want) return EG3D_OK;
  g_err = std::string(who) + ": " + arg + "->struct_size is smaller than this library's " + type_name + " (" + std::to_string(want) +
          " bytes): set it to sizeof(" + type_name + ")";
  return EG3D_ERR_ARG;
}

int open_seed_range(eg3d_ctx* c, const char* who, const eg3d_seeds* seeds, uint32_t b, uint32_t e, const void* out,
                    DevBuf eg3d_ctx::*ctr_of, DevBuf eg3d_ctx::*svseed_of, SeedRange* r) {
  if (!c || !out) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if (seeds) BUF_TRY(eg3d_upload_seeds(c, seeds));
  if (b > e || e > c->seeds->n_seeds) {
    g_err = std::string(who) + ": bad seed range (seeds uploaded?)";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  r->n_seeds = e - b;
  r->sv_base = r->n_seeds ? c->seeds->trk_off[b] : 0;
  r->n_sv = r->n_seeds ? c->seeds->trk_off[e] - r->sv_base : 0;
  r->active = r->n_sv && c->n_pl;
  if (!r->active) return EG3D_OK;
  BUF_TRY(ensure_grid10(c, &r->g10, &r->ms_grid));
  DevBuf &ctr = c->*ctr_of, &svseed = c->*svseed_of;
  r->sd = c->seeds->dev();
  // ---- the view ids, before anything indexes with them
  BUF_TRY(ctr.ensure(4 * sizeof(uint32_t)));
  BUF_TRY(svseed.ensure(sizeof(uint32_t) * r->n_sv));
  HIP_TRY(hipMemsetAsync(ctr.p, 0, 4 * sizeof(uint32_t), c->stream));
  launch_k9_prep(c->stream, r->sd, c->V, b, r->n_seeds, r->sv_base, svseed.as<uint32_t>(), ctr.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  BUF_TRY(ensure_mailbox(c));
  Readback rb(c);
  const int it = rb.add(ctr.p, 1);
  BUF_TRY(rb.run());
  if (*rb.item(it) & K9_FLAG_BAD_VIEW) {
    g_err = std::string(who) + ": view id out of range";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}

int copy_out(hipStream_t st, const char* who, std::initializer_list<HostCopy> items) {
  hipError_t e = hipSuccess;
  bool oom = false;
  for (const HostCopy& q : items) *q.dst = nullptr;
  for (const HostCopy& q : items) {
    const bool copy = q.src && q.bytes;
    *q.dst = copy ? malloc(q.bytes) : calloc(std::max<size_t>(q.bytes, 1), 1);
    if (!*q.dst) {
      oom = true;
      break;
    }
    if (copy && (e = hipMemcpyAsync(*q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
  }
  const hipError_t es = hipStreamSynchronize(st);  // (also after a failure: no copy may still be writing what is freed)
  if (e == hipSuccess) e = es;
  if (!oom && e == hipSuccess) return EG3D_OK;
  for (const HostCopy& q : items) {
    free(*q.dst);
    *q.dst = nullptr;
  }
  g_err = oom ? std::string(who) + ": out of host memory" : std::string(who) + ": copy to the host: " + hipGetErrorString(e);
  return EG3D_ERR_HIP;
}
EG3D_API_END


#ifdef EG3D_SECTION_TIMING
// Tuning diagnostics, present only in builds made with -DEG3D_SECTION_TIMING (tools/section_timing*.py):
// per-section shader-clock ticks of the most recent k3b_expand launch, summed over the chains
// (sum[16]) and of the slowest chain (slowest[16]).
extern "C" int eg3d_probe_sections(eg3d_ctx* c, double* sum, double* slowest, uint32_t* n_chains) {
  if (!c || !sum || !slowest) return EG3D_ERR_ARG;
  std::vector<ChainOut> co(c->last_nc ? c->last_nc : 1);
  if (c->last_nc) HIP_TRY(hipMemcpy(co.data(), c->b_couts.p, sizeof(ChainOut) * c->last_nc, hipMemcpyDeviceToHost));
  // sum / slowest hold 16 doubles: 0..11 the section ticks, 12..14 the follow diagnostics packed in
  // tsec[11] (sequential N-view steps, look-ahead steps accepted, look-ahead rounds redone)
  for (int k = 0; k < 16; k++) sum[k] = slowest[k] = 0;
  uint64_t worst = 0;
  for (uint32_t j = 0; j < c->last_nc; j++) {
    for (int k = 0; k < 12; k++) sum[k] += (double)co[j].tsec[k];
    sum[12] += (double)(co[j].tsec[11] & 0xffffu);
    sum[13] += (double)((co[j].tsec[11] >> 16) & 0xffffu);
    sum[14] += (double)(co[j].tsec[11] >> 32);
    if (co[j].tsec[7] >= worst) {
      worst = co[j].tsec[7];
      for (int k = 0; k < 12; k++) slowest[k] = (double)co[j].tsec[k];
      slowest[12] = (double)(co[j].tsec[11] & 0xffffu);
      slowest[13] = (double)((co[j].tsec[11] >> 16) & 0xffffu);
      slowest[14] = (double)(co[j].tsec[11] >> 32);
      slowest[15] = (double)co[j].n_points;
    }
  }
  if (n_chains) *n_chains = c->last_nc;
  return EG3D_OK;
}

// the raw per-section sums (16 doubles: Chain::tsec) of the most recent k3b_expand launch — what the LIGHT timing builds
// (-DEG3D_ONE_SECTION=k: section k and the whole chain only) are read through; tools/section_light.py
extern "C" int eg3d_probe_sections_raw(eg3d_ctx* c, double* sum16, uint32_t* n_chains) {
  if (!c || !sum16) return EG3D_ERR_ARG;
  std::vector<ChainOut> co(c->last_nc ? c->last_nc : 1);
  if (c->last_nc) HIP_TRY(hipMemcpy(co.data(), c->b_couts.p, sizeof(ChainOut) * c->last_nc, hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; k++) sum16[k] = 0;
  for (uint32_t j = 0; j < c->last_nc; j++)
    for (int k = 0; k < 16; k++) sum16[k] += (double)co[j].tsec[k];
  if (n_chains) *n_chains = c->last_nc;
  return EG3D_OK;
}

#ifndef EG3D_ONE_SECTION
// Gauss-Newton diagnostics of the expand kernel since the last reset (eg3d_dev_coopgn.h g_gn_dbg)
namespace eg3d { int gn_dbg_read(unsigned long long* out, int reset); }
extern "C" int eg3d_probe_gn(unsigned long long* out128, int reset) { return eg3d::gn_dbg_read(out128, reset); }
#endif

extern "C" int eg3d_probe_hyp_sections(eg3d_ctx* c, double* sum, double* slowest, uint32_t* counts) {
  if (!c || !sum || !slowest || !counts) return EG3D_ERR_ARG;
  const uint32_t n = c->last_nhyp;
  std::vector<HypResult> r(n ? n : 1);
  if (n) HIP_TRY(hipMemcpy(r.data(), c->b_res.p, sizeof(HypResult) * n, hipMemcpyDeviceToHost));
  for (int k = 0; k < 6; k++) sum[k] = slowest[k] = 0;
  for (int k = 0; k < 5; k++) counts[k] = 0;
  counts[0] = n;
  for (uint32_t h = 0; h < n; h++) {
    if (r[h].status & HYP_TRI) counts[1]++;
    if (r[h].status & HYP_D1) counts[2]++;
    if (r[h].status & HYP_D2) counts[3]++;
    if (hyp_compatible(r[h].status, r[h].n1, r[h].n2)) counts[4]++;
    // list lengths (the per-section tick fields were retired): sum[0..1] = total n1, n2;
    // slowest[0..1] = longest n1, n2; sum[2] = hypotheses whose lists total >= 32 points
    sum[0] += r[h].n1;
    sum[1] += r[h].n2;
    if (r[h].n1 > slowest[0]) slowest[0] = r[h].n1;
    if (r[h].n2 > slowest[1]) slowest[1] = r[h].n2;
    if (r[h].n1 + r[h].n2 >= 32) sum[2] += 1;
  }
  return EG3D_OK;
}

#endif
#if defined(EG3D_WITH_K3C_ENGINE) || defined(EG3D_SECTION_TIMING)
// The K3a walk service's counters (eg3d_k3a_engine.h) of the match calls of this context since the last probe, summed over
// the lanes the calls ran on: out2[0] = walks a wave finished for one of its lanes, out2[1] = the 64-segment passes they
// took. Test-only builds (the engine variant, the timing builds): the product library carries no probe.
extern "C" int eg3d_probe_k3a_walks(eg3d_ctx* c, unsigned long long* out2) {
  if (!c || !out2) return EG3D_ERR_ARG;
  out2[0] = out2[1] = 0;
  std::vector<eg3d_ctx*> all = c->lanes;
  if (all.empty()) all.push_back(c);
  for (eg3d_ctx* l : all) {
    out2[0] += l->k3a_walks_served;
    out2[1] += l->k3a_walk_passes;
    l->k3a_walks_served = l->k3a_walk_passes = 0;
  }
  return EG3D_OK;
}
#endif
#if defined(EG3D_WITH_K3C_ENGINE) && (defined(EG3D_SECTION_TIMING) || defined(EG3D_K3C_TIMING))
// ... and of the lane-per-chain engine (eg3d_k3c_engine.h g_k3c_dbg)
namespace eg3d { int k3c_dbg_read(unsigned long long* out, int reset); }
extern "C" int eg3d_probe_k3c(unsigned long long* out128, int reset) { return eg3d::k3c_dbg_read(out128, reset); }
#endif
  // EG3D_SECTION_TIMING
