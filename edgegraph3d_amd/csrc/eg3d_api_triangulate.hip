// eg3d_api_triangulate.hip — FP64 triangulation of caller-supplied tracks (include/eg3d_triangulate.h): the host side of K14
#include "eg3d_api_internal.h"
#include "../../include/eg3d_triangulate.h"

static_assert(K14_OUT_SHORT == EG3D_TRI_FLAG_SHORT && K14_OUT_DEGENERATE == EG3D_TRI_FLAG_DEGENERATE, "the kernel writes the public flags");

// Staging budget in observations (16 bytes each): EG3D_TRI_STAGE_OBS, read at the call. The default, 2^24 records = 256 MiB,
// is a choice, not a measurement: large enough that config 4's 4.1 G observations are ~250 batches of > 200 000 tracks each.
#define EG3D_TRI_STAGE_OBS_DEFAULT (1ull << 24)
static uint64_t stage_budget() {
  if (const char* e = getenv("EG3D_TRI_STAGE_OBS")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v) return std::min<unsigned long long>(v, 1ull << 40);
  }
  return EG3D_TRI_STAGE_OBS_DEFAULT;
}

// The call proper, on arrays that are on the device: check and cut (one read-back), then per batch the conversion into
// records and the solve, queued without a wait in between, then the flag word and the counts (one read-back).
static int triangulate_tracks(eg3d_ctx* c, const char* who, int mode, const K14Tracks& t, float* X_out, uint8_t* valid, uint8_t* flags,
                              eg3d_tri_stats* s) {
  if (t.n_tracks >> 36) {
    g_err = std::string(who) + ": more than 2^36 tracks";
    return EG3D_ERR_CAPACITY;
  }
  hipStream_t st = c->stream;
  const uint64_t budget = stage_budget();
  // two consecutive batches hold more than `budget` observations between them (the first would have taken more tracks otherwise)
  const uint64_t cap = std::min<uint64_t>(t.n_tracks, 2 * (t.n_obs / budget) + 2);
  const size_t cut_words = 1 + 2 * (cap + 1);
  BUF_TRY(c->k14_ctr.ensure(4 * sizeof(unsigned long long)));
  BUF_TRY(c->k14_cuts.ensure(cut_words * sizeof(unsigned long long)));
  unsigned long long* ctr = c->k14_ctr.as<unsigned long long>();  // [0] flag word, [1..3] valid, short, degenerate
  HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k14_check(st, t, (uint32_t*)ctr);
  launch_k14_cut(st, t, budget, cap, c->k14_cuts.as<unsigned long long>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  unsigned long long back[4] = {0, 0, 0, 0};
  std::vector<unsigned long long> cuts(cut_words);
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cuts.data(), c->k14_cuts.p, cut_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  auto refuse = [&](uint32_t f) {
    g_err = std::string(who) + (f & K14_BAD_OFFSETS ? ": obs_off is not ascending within [0, n_obs]"
                                : f & K14_LONG_LIST ? ": a list holds more than 32 767 observations"
                                                    : ": view id out of range");
    return EG3D_ERR_ARG;
  };
  if ((uint32_t)back[0]) return refuse((uint32_t)back[0]);
  const uint64_t nb = cuts[0];
  if (nb > cap) {
    g_err = std::string(who) + ": internal error: the call's batches outgrew their bound";
    return EG3D_ERR_CAPACITY;
  }
  uint64_t max_obs = 1;
  for (uint64_t k = 0; k < nb; k++) max_obs = std::max<uint64_t>(max_obs, cuts[2 + 2 * (k + 1)] - cuts[2 + 2 * k]);
  BUF_TRY(c->k14_rec.ensure(K14_REC_BYTES * max_obs));
  HIP_TRY(hipEventRecord(c->ea[1], st));
  for (uint64_t k = 0; k < nb; k++) {
    const uint64_t t0 = cuts[1 + 2 * k], o0 = cuts[2 + 2 * k], t1 = cuts[1 + 2 * (k + 1)], o1 = cuts[2 + 2 * (k + 1)];
    launch_k14_stage(st, t, c->V, o0, o1, c->k14_rec.as<Obs>(), (uint32_t*)ctr);
    launch_k14_solve(st, c->ds.cam_P, c->ds.cams_mid_range, mode, t, t0, t1, o0, c->k14_rec.as<Obs>(), X_out, valid, flags, ctr + 1);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->eb[1], st));
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if ((uint32_t)back[0]) return refuse((uint32_t)back[0]);
  s->n_batches = (uint32_t)std::min<uint64_t>(nb, 0xffffffffull);
  s->n_tracks = t.n_tracks;
  s->n_valid = back[1];
  s->n_short = back[2];
  s->n_degenerate = back[3];
  HIP_TRY(hipEventElapsedTime(&s->ms_stage, c->ea[0], c->eb[0]));
  HIP_TRY(hipEventElapsedTime(&s->ms_kernel, c->ea[1], c->eb[1]));
  return EG3D_OK;
}

static int check_call(const char* who, const eg3d_ctx* c, int mode, const eg3d_tri_stats* stats) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_tri_stats", stats->struct_size, sizeof(eg3d_tri_stats)));
  if (!c) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if (mode != EG3D_TRI_FROM_SCRATCH && mode != EG3D_TRI_REFINE) {
    g_err = std::string(who) + ": unknown mode (EG3D_TRI_FROM_SCRATCH or EG3D_TRI_REFINE)";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}
static void give_stats(eg3d_tri_stats* stats, eg3d_tri_stats s) {
  if (!stats) return;
  s.struct_size = (uint32_t)sizeof(eg3d_tri_stats);
  *stats = s;
}

extern "C" int eg3d_triangulate(eg3d_ctx* c, int mode, uint64_t n, const uint32_t* obs_off, const int32_t* obs_view,
                                const float* obs_xy, const float* X0, float* X_out, uint8_t* valid, uint8_t* flags,
                                eg3d_tri_stats* stats) {
  const char* who = "eg3d_triangulate";
  BUF_TRY(check_call(who, c, mode, stats));
  eg3d_tri_stats s{};
  if (!n) {
    give_stats(stats, s);
    return EG3D_OK;
  }
  if (!obs_off || !X_out || !valid || (mode == EG3D_TRI_REFINE && !X0)) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  const uint64_t m = obs_off[n];
  if (m && (!obs_view || !obs_xy)) {
    g_err = std::string(who) + ": null observation arrays";
    return EG3D_ERR_ARG;
  }
  const auto w0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  std::vector<eg3d_off_t> off64(obs_off, obs_off + n);  // (widened, not interpreted: the device checks them)
  BUF_TRY(upload(c->k14_off, off64.data(), n, st));
  BUF_TRY(upload(c->k14_view, obs_view, m, st));
  BUF_TRY(upload(c->k14_xy, obs_xy, 2 * m, st));
  if (mode == EG3D_TRI_REFINE) BUF_TRY(upload(c->k14_X0, X0, 3 * n, st));
  BUF_TRY(c->k14_Xo.ensure(12 * n));
  BUF_TRY(c->k14_valid.ensure(n));
  if (flags) BUF_TRY(c->k14_flags.ensure(n));
  HIP_TRY(hipStreamSynchronize(st));  // (off64 is read by the copy queued above)
  const K14Tracks t{n, m, c->k14_off.as<eg3d_off_t>(), c->k14_view.as<int32_t>(), c->k14_xy.as<float>(),
                    mode == EG3D_TRI_REFINE ? c->k14_X0.as<float>() : nullptr};
  BUF_TRY(triangulate_tracks(c, who, mode, t, c->k14_Xo.as<float>(), c->k14_valid.as<uint8_t>(),
                             flags ? c->k14_flags.as<uint8_t>() : nullptr, &s));
  HIP_TRY(hipMemcpyAsync(X_out, c->k14_Xo.p, 12 * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(valid, c->k14_valid.p, n, hipMemcpyDeviceToHost, st));
  if (flags) HIP_TRY(hipMemcpyAsync(flags, c->k14_flags.p, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  s.ms_copy = std::max(0.f, wall - s.ms_stage - s.ms_kernel);
  give_stats(stats, s);
  return EG3D_OK;
}

extern "C" int eg3d_triangulate_device(eg3d_ctx* c, int mode, const eg3d_device_edgepoints* cloud, float* X_out_dev,
                                       uint8_t* valid_dev, uint8_t* flags_dev, eg3d_tri_stats* stats) {
  const char* who = "eg3d_triangulate_device";
  BUF_TRY(check_call(who, c, mode, stats));
  eg3d_device_edgepoints d;
  if (cloud)
    d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, &d));
  BUF_TRY(check_cloud(&d, who, false));
  eg3d_tri_stats s{};
  if (!d.n_points) {
    give_stats(stats, s);
    return EG3D_OK;
  }
  if (!X_out_dev || !valid_dev) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  const K14Tracks t{d.n_points, d.n_obs, d.obs_off, d.obs_view, d.obs_xy, mode == EG3D_TRI_REFINE ? d.X : nullptr};
  BUF_TRY(triangulate_tracks(c, who, mode, t, X_out_dev, valid_dev, flags_dev, &s));
  give_stats(stats, s);
  return EG3D_OK;
}
