// eg3d_api_edgemap.hip — the edge maps of the source images on the device (include/eg3d/edgemap.hh): the host side of K19.
// Context-free like eg3d_estimate_fundamental: the call makes its own stream, events and DevBufs and releases them when it
// returns, whichever way. The images of all views lie one after the other in one array, and so does every stage's output;
// a table says where each view starts (K19View).
#include "eg3d_api_internal.h"
#include "eg3d_k19_edgemap.h"
#include "../../include/eg3d/edgemap.hh"

using namespace eg3d::edgemap;

namespace {
struct EdgemapCall {
  hipStream_t st = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf rgb, grey[2], cls, table, dirty[2], ctr, changed;
  ~EdgemapCall() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};
struct DeviceRestore {
  int prev = -1;
  ~DeviceRestore() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
// Launches of the propagation queued between two looks at their "changed" words: 8 at first, doubled while every round of a
// batch still changed something, up to 128. A round after the one that changed nothing finds no marked tile and costs a
// launch of workgroups that return at once, so a batch that overshoots is cheap and one that undershoots costs a
// synchronisation (tools/bench_edgemaps.py times both kinds of input).
constexpr int kFirstBatch = 8, kMaxBatch = 128;
}  // namespace

extern "C" int eg3d_edge_maps(int device, int32_t n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                              const eg3d_edgemap_params* params, uint8_t* const* masks, eg3d_edgemap_stats* stats) {
  static const char who[] = "eg3d_edge_maps";
  if (const char* why = refusal(n_views, width, height, rgb, params, masks, stats)) {
    g_err = std::string(who) + ": " + why;
    return EG3D_EDGEMAP_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_err = "eg3d_edge_maps: no HIP device available (eg3d_host_edge_maps computes the same masks on the host)";
    return EG3D_ERR_NODEVICE;
  }
  if (device < 0 || device >= ndev) {
    g_err = "eg3d_edge_maps: device index out of range";
    return EG3D_ERR_ARG;
  }
  const eg3d_edgemap_params p = *params;
  const bool l2 = p.l2 != 0;
  std::vector<K19View> table((size_t)n_views);
  K19Views vs{};
  vs.n_views = (uint32_t)n_views;
  u64 n_pixels = 0, n_tiles = 0;
  for (int32_t v = 0; v < n_views; v++) {
    const uint32_t tx = k19_tiles(width[v]), ty = k19_tiles(height[v]);
    table[(size_t)v] = K19View{n_pixels, n_tiles, width[v], height[v]};
    n_pixels += (u64)width[v] * (u64)height[v];
    n_tiles += (u64)tx * ty;
    vs.max_tx = std::max(vs.max_tx, tx);
    vs.max_ty = std::max(vs.max_ty, ty);
  }

  DeviceRestore restore;
  if (hipGetDevice(&restore.prev) != hipSuccess) restore.prev = -1;
  HIP_TRY(hipSetDevice(device));
  EdgemapCall c;
  HIP_TRY(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
  for (hipEvent_t& e : c.ev) HIP_TRY(hipEventCreate(&e));
  hipStream_t st = c.st;
  eg3d_edgemap_stats s;
  memset(&s, 0, sizeof s);
  s.struct_size = (uint32_t)sizeof s;
  s.n_views = (uint32_t)n_views;
  s.n_pixels = n_pixels;

  // ---- the images and the table go up
  BUF_TRY(c.rgb.ensure_exact(3 * (size_t)n_pixels));
  BUF_TRY(c.cls.ensure_exact((size_t)n_pixels + 4));
  for (int i = 0; i < std::min<int>(p.smooth_passes, 2); i++) BUF_TRY(c.grey[i].ensure_exact((size_t)n_pixels));
  BUF_TRY(c.dirty[0].ensure_exact((size_t)n_tiles));
  BUF_TRY(c.dirty[1].ensure_exact((size_t)n_tiles));
  BUF_TRY(c.ctr.ensure(sizeof(u64) * K19C_COUNT));
  BUF_TRY(c.changed.ensure(sizeof(unsigned int) * kMaxBatch));
  HIP_TRY(hipEventRecord(c.ev[0], st));
  BUF_TRY(upload(c.table, table.data(), table.size(), st));
  for (int32_t v = 0; v < n_views; v++)
    HIP_TRY(hipMemcpyAsync(c.rgb.as<uint8_t>() + 3 * (size_t)table[(size_t)v].off, rgb[v], 3 * (size_t)width[v] * (size_t)height[v],
                           hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c.ctr.p, 0, sizeof(u64) * K19C_COUNT, st));
  HIP_TRY(hipMemsetAsync(c.dirty[0].p, 1, (size_t)n_tiles, st));
  HIP_TRY(hipMemsetAsync(c.dirty[1].p, 0, (size_t)n_tiles, st));
  vs.views = c.table.as<K19View>();

  // ---- E1 - E5 and the classes: the first stage reads the images, a pass reads the pass before it
  HIP_TRY(hipEventRecord(c.ev[1], st));
  const uint8_t* src = c.rgb.as<uint8_t>();
  bool from_rgb = true;
  for (int pass = 0; pass < p.smooth_passes; pass++) {
    uint8_t* dst = c.grey[pass & 1].as<uint8_t>();
    launch_k19_smooth(st, vs, from_rgb, src, dst);
    HIP_TRY(hipGetLastError());
    src = dst;
    from_rgb = false;
  }
  u64* ctr = c.ctr.as<u64>();
  uint8_t* cls = c.cls.as<uint8_t>();
  launch_k19_classify(st, vs, from_rgb, src, l2, threshold(p.low, l2), threshold(p.high, l2), cls, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c.ev[2], st));
  u64 back[K19C_COUNT];
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof back, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s.n_candidates = back[K19C_CANDIDATES];
  s.n_strong = back[K19C_STRONG];
  if (s.n_strong > s.n_candidates || s.n_candidates > n_pixels) {
    g_err = "eg3d_edge_maps: the counts read back from the device are impossible";
    return EG3D_ERR_HIP;
  }

  // ---- E6: rounds of the propagation until one changes nothing. With no strong pixel, or no weak one, nothing can turn.
  HIP_TRY(hipEventRecord(c.ev[3], st));
  if (s.n_strong && s.n_strong < s.n_candidates) {
    // a round that changes something turns at least one weak candidate: n_weak changing rounds and the one that finds none
    const u64 bound = s.n_candidates - s.n_strong + 1;
    unsigned int* changed = c.changed.as<unsigned int>();
    u64 rounds = 0;
    int batch = kFirstBatch;
    for (bool done = false; !done; batch = std::min(2 * batch, kMaxBatch)) {
      if (rounds >= bound) {
        g_err = "eg3d_edge_maps: the hysteresis passed its bound of rounds";
        return EG3D_EDGEMAP_ERR_ROUNDS;
      }
      HIP_TRY(hipMemsetAsync(changed, 0, sizeof(unsigned int) * batch, st));
      for (int i = 0; i < batch; i++) {
        launch_k19_hysteresis(st, vs, cls, c.dirty[(rounds + i) & 1].as<uint8_t>(), c.dirty[(rounds + i + 1) & 1].as<uint8_t>(), changed + i);
        HIP_TRY(hipGetLastError());
      }
      unsigned int seen[kMaxBatch];
      HIP_TRY(hipMemcpyAsync(seen, changed, sizeof(unsigned int) * batch, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      // (after a round that changed nothing no tile is marked: the rest of the batch did nothing)
      int i = 0;
      while (i < batch && seen[i]) i++;
      done = i < batch;
      rounds += done ? i + 1 : batch;
    }
    s.hysteresis_rounds = (uint32_t)std::min<u64>(rounds, 0xffffffffull);
  }
  launch_k19_mask(st, cls, n_pixels, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c.ev[4], st));
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof back, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s.n_edges = back[K19C_EDGES];

  // ---- the masks come back (the first byte written to the caller's arrays: everything before this could still refuse)
  for (int32_t v = 0; v < n_views; v++)
    HIP_TRY(hipMemcpyAsync(masks[v], cls + (size_t)table[(size_t)v].off, (size_t)width[v] * (size_t)height[v], hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(c.ev[5], st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipEventElapsedTime(&s.ms_upload, c.ev[0], c.ev[1]));
  HIP_TRY(hipEventElapsedTime(&s.ms_kernel, c.ev[1], c.ev[2]));
  HIP_TRY(hipEventElapsedTime(&s.ms_hysteresis, c.ev[3], c.ev[4]));
  HIP_TRY(hipEventElapsedTime(&s.ms_copy, c.ev[4], c.ev[5]));
  if (stats) *stats = s;
  return EG3D_OK;
}
