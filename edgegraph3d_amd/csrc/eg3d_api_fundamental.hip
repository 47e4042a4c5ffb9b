// eg3d_api_fundamental.hip — the fundamental matrices from the tracks on the device (K12, eg3d_k12_fundamental.hip).
// Context-free: F is part of the scene eg3d_create takes, so the call makes its own stream, events and DevBufs and
// releases them when it returns, whichever way.
#include "eg3d_api_internal.h"
#include "eg3d_fund_core.h"
#include "eg3d_k12_fundamental.h"

namespace {
// the stream, the events and every device block of one call
struct FundCall {
  hipStream_t st = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  DevBuf toff, tview, txy, key[2], val[2], flag, pos, ckey, cxy, voff, ncom, has, has_rank, size, size_off, pts, pairs, idx, fits, refits,
      normals, sel, err, inl, F, valid, ctr, tmp;
  ~FundCall() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }
};
// the caller thread's current device is put back when the call returns (after the call's buffers are gone)
struct DeviceRestore {
  int prev = -1;
  ~DeviceRestore() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
}  // namespace

extern "C" int eg3d_estimate_fundamental(int device, int32_t n_views, const eg3d_seeds* seeds, const eg3d_fund_params* params, double* F,
                                         uint8_t* F_valid, uint32_t* n_common, eg3d_fund_stats* stats) {
  static const char who[] = "eg3d_estimate_fundamental";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_fund_stats", stats->struct_size, sizeof(eg3d_fund_stats)));
  if (params) BUF_TRY(check_struct_size(who, "eg3d_fund_params", params->struct_size, sizeof(eg3d_fund_params), "params"));
  if (n_views <= 0 || !seeds || !F || !F_valid) {
    g_err = "eg3d_estimate_fundamental: bad arguments (n_views <= 0, or seeds, F or F_valid is NULL)";
    return EG3D_ERR_ARG;
  }
  const uint32_t N = seeds->n_seeds;
  if (N && (!seeds->trk_off || !seeds->trk_view || !seeds->trk_xy)) {
    g_err = "eg3d_estimate_fundamental: a track array is NULL";
    return EG3D_ERR_ARG;
  }
  bool ascending = !N || seeds->trk_off[0] == 0;
  for (uint32_t p = 0; ascending && p < N; p++) ascending = seeds->trk_off[p + 1] >= seeds->trk_off[p];
  if (!ascending) {
    g_err = "eg3d_estimate_fundamental: trk_off does not start at 0 or does not ascend";
    return EG3D_ERR_ARG;
  }
  if (n_views > EG3D_MAX_VIEWS) {
    g_err = "eg3d_estimate_fundamental: more than " + std::to_string(EG3D_MAX_VIEWS) + " views";
    return EG3D_ERR_CAPACITY;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_err = "eg3d_estimate_fundamental: no HIP device available (eg3d_host_estimate_fundamental computes the same matrices on the host)";
    return EG3D_ERR_NODEVICE;
  }
  if (device < 0 || device >= ndev) {
    g_err = "eg3d_estimate_fundamental: device index out of range";
    return EG3D_ERR_ARG;
  }
  const uint32_t V = (uint32_t)n_views, M = N ? seeds->trk_off[N] : 0;
  const size_t VV = (size_t)V * V;
  const uint32_t iterations = params && params->iterations ? params->iterations : fund::kDefaultIterations;
  const uint64_t rng_seed = params ? params->rng_seed : 0;
  const uint64_t fit_budget = std::max<uint64_t>(params && params->fit_budget ? params->fit_budget : (1u << 20), iterations);
  const uint32_t stage_points = std::min<uint32_t>(params && params->stage_points ? params->stage_points : 1024u, 4096u);
  const uint32_t per_chunk = (uint32_t)(fit_budget / iterations);  // whole pairs; at least one

  DeviceRestore restore;
  if (hipGetDevice(&restore.prev) != hipSuccess) restore.prev = -1;
  HIP_TRY(hipSetDevice(device));
  FundCall c;
  HIP_TRY(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
  for (hipEvent_t& e : c.ev) HIP_TRY(hipEventCreate(&e));
  hipStream_t st = c.st;
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  eg3d_fund_stats s;
  memset(&s, 0, sizeof s);

  // ---- upload
  auto t0 = now();
  BUF_TRY(c.toff.ensure(4 * ((size_t)N + 1)));
  BUF_TRY(c.tview.ensure(4 * std::max<size_t>(M, 1)));
  BUF_TRY(c.txy.ensure(8 * std::max<size_t>(M, 1)));
  BUF_TRY(c.F.ensure(8 * 9 * VV));
  BUF_TRY(c.valid.ensure(VV));
  BUF_TRY(c.ncom.ensure(4 * VV));
  BUF_TRY(c.ctr.ensure(8 * K12_N_CTR));
  if (N) HIP_TRY(hipMemcpyAsync(c.toff.p, seeds->trk_off, 4 * ((size_t)N + 1), hipMemcpyHostToDevice, st));
  if (M) {
    HIP_TRY(hipMemcpyAsync(c.tview.p, seeds->trk_view, 4 * (size_t)M, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.txy.p, seeds->trk_xy, 8 * (size_t)M, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemsetAsync(c.F.p, 0, 8 * 9 * VV, st));
  HIP_TRY(hipMemsetAsync(c.valid.p, 0, VV, st));
  HIP_TRY(hipMemsetAsync(c.ncom.p, 0, 4 * VV, st));
  HIP_TRY(hipMemsetAsync(c.ctr.p, 0, 8 * K12_N_CTR, st));
  HIP_TRY(hipStreamSynchronize(st));
  s.ms_upload = ms_since(t0);

  // ---- lists: the observations sorted by (view, point), the counts, the correspondences of the pairs with >= 10
  t0 = now();
  for (int k = 0; k < 2; k++) {
    BUF_TRY(c.key[k].ensure(8 * std::max<size_t>(M, 1)));
    BUF_TRY(c.val[k].ensure(4 * std::max<size_t>(M, 1)));
  }
  BUF_TRY(c.flag.ensure(4 * ((size_t)M + 1)));
  BUF_TRY(c.pos.ensure(4 * ((size_t)M + 1)));
  BUF_TRY(c.voff.ensure(4 * ((size_t)V + 1)));
  BUF_TRY(c.has.ensure(4 * (VV + 1)));
  BUF_TRY(c.has_rank.ensure(4 * (VV + 1)));
  BUF_TRY(c.size.ensure(8 * (VV + 1)));
  BUF_TRY(c.size_off.ensure(8 * (VV + 1)));
  u64* const key0 = c.key[0].as<u64>();
  u64* const key1 = c.key[1].as<u64>();
  launch_k12_keys(st, N, M, n_views, c.toff.as<uint32_t>(), c.tview.as<int32_t>(), key0, c.val[0].as<uint32_t>());
  if (M) BUF_TRY(prim_call(st, c.tmp, "k8_sort_pairs", k8_sort_pairs, (const u64*)key0, key1, (const uint32_t*)c.val[0].as<uint32_t>(),
                           c.val[1].as<uint32_t>(), (size_t)M));  // (stable: equal keys keep the order of the track)
  launch_k12_heads(st, M, key1, c.flag.as<uint32_t>());
  BUF_TRY(prim_call(st, c.tmp, "k8_scan_u32", k8_scan_u32, (const uint32_t*)c.flag.as<uint32_t>(), c.pos.as<uint32_t>(), (size_t)M + 1));
  uint32_t n_obs = 0;
  HIP_TRY(hipMemcpyAsync(&n_obs, c.pos.as<uint32_t>() + M, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  BUF_TRY(c.ckey.ensure(8 * std::max<size_t>(n_obs, 1)));
  BUF_TRY(c.cxy.ensure(8 * std::max<size_t>(n_obs, 1)));
  launch_k12_compact(st, M, key1, c.val[1].as<uint32_t>(), c.flag.as<uint32_t>(), c.pos.as<uint32_t>(), c.txy.as<float>(), c.ckey.as<u64>(),
                     c.cxy.as<float2>());
  launch_k12_view_off(st, n_views, n_obs, c.ckey.as<u64>(), c.voff.as<uint32_t>());
  HIP_TRY(hipMemsetAsync(c.has.p, 0, 4 * (VV + 1), st));
  HIP_TRY(hipMemsetAsync(c.size.p, 0, 8 * (VV + 1), st));
  launch_k12_common(st, false, n_views, c.voff.as<uint32_t>(), c.ckey.as<u64>(), c.cxy.as<float2>(), c.ncom.as<uint32_t>(),
                    c.has.as<uint32_t>(), c.size.as<u64>(), nullptr, nullptr, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(prim_call(st, c.tmp, "k8_scan_u32", k8_scan_u32, (const uint32_t*)c.has.as<uint32_t>(), c.has_rank.as<uint32_t>(), VV + 1));
  BUF_TRY(prim_call(st, c.tmp, "k10_scan_u64", k10_scan_u64, (const u64*)c.size.as<u64>(), c.size_off.as<u64>(), VV + 1));
  uint32_t n_unordered = 0;
  u64 n_corr = 0;
  HIP_TRY(hipMemcpyAsync(&n_unordered, c.has_rank.as<uint32_t>() + VV, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&n_corr, c.size_off.as<u64>() + VV, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t n_pairs = 2 * n_unordered;  // (< V * V <= 2^26)
  if (n_pairs) {
    BUF_TRY(c.pts.ensure(16 * (size_t)n_corr));
    BUF_TRY(c.pairs.ensure(sizeof(K12Pair) * (size_t)n_pairs));
    launch_k12_common(st, true, n_views, c.voff.as<uint32_t>(), c.ckey.as<u64>(), c.cxy.as<float2>(), c.ncom.as<uint32_t>(),
                      c.has.as<uint32_t>(), c.size.as<u64>(), c.has_rank.as<uint32_t>(), c.size_off.as<u64>(), c.pts.as<float4>(),
                      c.pairs.as<K12Pair>());
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  s.ms_lists = ms_since(t0);

  // ---- the pairs, `per_chunk` of them at a time
  if (n_pairs) {
    const uint32_t chunk_cap = std::min(per_chunk, n_pairs);
    BUF_TRY(c.idx.ensure(4 * 8 * (size_t)chunk_cap * iterations));
    BUF_TRY(c.fits.ensure(sizeof(K12Fit) * (size_t)chunk_cap * iterations));
    BUF_TRY(c.refits.ensure(sizeof(K12Fit) * (size_t)chunk_cap));
    BUF_TRY(c.normals.ensure(sizeof(K12Normal) * (size_t)chunk_cap));
    BUF_TRY(c.sel.ensure(sizeof(K12Sel) * (size_t)chunk_cap));
    BUF_TRY(c.err.ensure(8 * 2 * (size_t)n_corr));
    BUF_TRY(c.inl.ensure(4 * 2 * (size_t)n_corr));
    for (uint32_t p0 = 0; p0 < n_pairs; p0 += chunk_cap) {
      const uint32_t np = std::min(chunk_cap, n_pairs - p0);
      const K12Pair* pairs = c.pairs.as<K12Pair>();
      const float4* pts = c.pts.as<float4>();
      HIP_TRY(hipEventRecord(c.ev[0], st));
      launch_k12_samples(st, p0, np, iterations, n_views, rng_seed, pairs, c.idx.as<uint32_t>());
      HIP_TRY(hipEventRecord(c.ev[1], st));
      launch_k12_fit(st, p0, np, iterations, pairs, pts, c.idx.as<uint32_t>(), nullptr, c.fits.as<K12Fit>());
      HIP_TRY(hipEventRecord(c.ev[2], st));
      launch_k12_select(st, p0, np, iterations, stage_points, n_views, pairs, pts, c.fits.as<K12Fit>(), c.err.as<u64>(),
                        c.inl.as<uint32_t>(), c.normals.as<K12Normal>(), c.sel.as<K12Sel>(), c.F.as<double>(), c.valid.as<uint8_t>(),
                        c.ctr.as<u64>());
      HIP_TRY(hipEventRecord(c.ev[3], st));
      launch_k12_fit(st, p0, np, iterations, pairs, pts, nullptr, c.normals.as<K12Normal>(), c.refits.as<K12Fit>());
      launch_k12_final(st, p0, np, n_views, pairs, pts, c.refits.as<K12Fit>(), c.sel.as<K12Sel>(), c.F.as<double>());
      HIP_TRY(hipEventRecord(c.ev[4], st));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(st));
      float* const into[4] = {&s.ms_samples, &s.ms_fits, &s.ms_select, &s.ms_refit};
      for (int k = 0; k < 4; k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c.ev[k], c.ev[k + 1]));
        *into[k] += ms;
      }
      s.n_chunks++;
    }
  }

  // ---- copy: into buffers of the call first, so that a failure leaves the caller's arrays as they were
  t0 = now();
  std::vector<double> hF(9 * VV);
  std::vector<uint8_t> hvalid(VV);
  std::vector<uint32_t> hncom(VV);
  u64 ctr[K12_N_CTR];
  HIP_TRY(hipMemcpyAsync(hF.data(), c.F.p, 8 * 9 * VV, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hvalid.data(), c.valid.p, VV, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(hncom.data(), c.ncom.p, 4 * VV, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ctr, c.ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(F, hF.data(), 8 * 9 * VV);
  memcpy(F_valid, hvalid.data(), VV);
  if (n_common) memcpy(n_common, hncom.data(), 4 * VV);
  s.ms_copy = ms_since(t0);
  if (stats) {
    s.struct_size = stats->struct_size;
    s.n_pairs_valid = (uint32_t)ctr[K12_C_VALID];
    s.n_pairs_failed = (uint32_t)ctr[K12_C_FAILED];
    s.n_common_total = 2 * n_corr;
    s.n_fits = (uint64_t)n_pairs * iterations;
    s.n_fits_degenerate = ctr[K12_C_DEGENERATE];
    s.n_exact_medians = ctr[K12_C_EXACT];
    memcpy(stats, &s, sizeof s);
  }
  return EG3D_OK;
}
