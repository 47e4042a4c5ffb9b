// eg3d_api_colour.hip — the colours of a cloud from the source images (include/eg3d_colour.h): the host side of K15
#include "eg3d_api_internal.h"
#include "eg3d_dev_colour.h"
#include "../../include/eg3d_colour.h"

static_assert(K15_OUT_EMPTY == EG3D_COLOUR_FLAG_EMPTY, "the kernel writes the public flag");

extern "C" int eg3d_release_images(eg3d_ctx* c) {
  if (!c) {
    g_err = "eg3d_release_images: bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (no call of this context reads them any more)
  c->k15_have_images = false;
  c->k15_n_images = 0;
  c->k15_img.release();
  c->k15_tab.release();
  return EG3D_OK;
}

extern "C" int eg3d_upload_images(eg3d_ctx* c, int n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb) {
  const char* who = "eg3d_upload_images";
  if (!c || !width || !height || !rgb) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if (n_views != c->V) {
    g_err = std::string(who) + ": n_views differs from the context's " + std::to_string(c->V);
    return EG3D_ERR_ARG;
  }
  std::vector<size_t> at((size_t)n_views, 0);
  size_t total = 0;
  uint32_t n_images = 0;
  for (int v = 0; v < n_views; v++) {
    if (!rgb[v]) continue;
    if (width[v] < 1 || height[v] < 1 || width[v] > EG3D_COLOUR_MAX_IMAGE_SIDE || height[v] > EG3D_COLOUR_MAX_IMAGE_SIDE) {
      g_err = std::string(who) + ": view " + std::to_string(v) + ": width and height must be in 1 .. 32768";
      return EG3D_ERR_ARG;
    }
    at[(size_t)v] = total;
    total += ((size_t)width[v] * (size_t)height[v] * 3u + 15u) & ~(size_t)15u;
    n_images++;
  }
  BUF_TRY(eg3d_release_images(c));  // a failed upload leaves the context without images, never with a mixture
  hipStream_t st = c->stream;
  BUF_TRY(c->k15_img.ensure_exact(total));
  std::vector<K15Image> tab((size_t)n_views);
  for (int v = 0; v < n_views; v++) {
    K15Image& im = tab[(size_t)v];
    im.rgb = nullptr;
    im.w = im.h = 0;
    if (!rgb[v]) continue;
    im.rgb = c->k15_img.as<uint8_t>() + at[(size_t)v];
    im.w = width[v];
    im.h = height[v];
    HIP_TRY(hipMemcpyAsync(c->k15_img.as<uint8_t>() + at[(size_t)v], rgb[v], (size_t)width[v] * (size_t)height[v] * 3u,
                           hipMemcpyHostToDevice, st));
  }
  BUF_TRY(upload(c->k15_tab, tab.data(), tab.size(), st));
  HIP_TRY(hipStreamSynchronize(st));  // (tab and the caller's images are read by the copies queued above)
  c->k15_n_images = n_images;
  c->k15_have_images = true;
  return EG3D_OK;
}

// The call proper, on arrays that are on the device: the sampling pass, the mixing pass, then the flag word and the
// counts (one read-back).
static int colour_cloud(eg3d_ctx* c, const char* who, const K15Cloud& cl, uint8_t* rgb, uint8_t* flags, eg3d_colour_stats* s) {
  hipStream_t st = c->stream;
  BUF_TRY(c->k15_ctr.ensure(4 * sizeof(unsigned long long)));
  BUF_TRY(c->k15_words.ensure(sizeof(uint32_t) * std::max<uint64_t>(cl.n_obs, 1)));
  unsigned long long* ctr = c->k15_ctr.as<unsigned long long>();  // [0] flag word, [1..3] coloured, empty, observations
  HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_k15_sample(st, cl, c->k15_tab.as<K15Image>(), c->V, c->k15_words.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipEventRecord(c->ea[1], st));
  launch_k15_mix(st, cl, c->k15_words.as<uint32_t>(), rgb, flags, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[1], st));
  unsigned long long back[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(back, ctr, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (const uint32_t f = (uint32_t)back[0]) {
    g_err = std::string(who) + (f & K15_BAD_OFFSETS ? ": obs_off is not ascending within [0, n_obs]"
                                : f & K15_LONG_LIST ? ": a list holds more than 32 767 observations"
                                : f & K15_BAD_VIEW  ? ": view id out of range"
                                : f & K15_NO_IMAGE  ? ": an observation names a view without an image"
                                                    : ": a coordinate is not finite or not below 1e7 in magnitude");
    return EG3D_ERR_ARG;
  }
  s->n_images = c->k15_n_images;
  s->n_points = cl.n_points;
  s->n_coloured = back[1];
  s->n_empty = back[2];
  s->n_obs_sampled = back[3];
  HIP_TRY(hipEventElapsedTime(&s->ms_sample, c->ea[0], c->eb[0]));
  HIP_TRY(hipEventElapsedTime(&s->ms_mix, c->ea[1], c->eb[1]));
  return EG3D_OK;
}

static int check_call(const char* who, const eg3d_ctx* c, const eg3d_colour_stats* stats) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_colour_stats", stats->struct_size, sizeof(eg3d_colour_stats)));
  if (!c) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if (!c->k15_have_images) {
    g_err = std::string(who) + ": no images uploaded to this context (eg3d_upload_images; a clone does not inherit them)";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}
static void give_stats(const eg3d_ctx* c, eg3d_colour_stats* stats, eg3d_colour_stats s) {
  if (!stats) return;
  s.struct_size = (uint32_t)sizeof(eg3d_colour_stats);
  s.n_images = c->k15_n_images;
  *stats = s;
}

extern "C" int eg3d_colour_points(eg3d_ctx* c, uint64_t n, const uint32_t* obs_off, const int32_t* obs_view, const float* obs_xy,
                                  const uint8_t* keep, uint8_t* rgb_out, uint8_t* flags_out, eg3d_colour_stats* stats) {
  const char* who = "eg3d_colour_points";
  BUF_TRY(check_call(who, c, stats));
  eg3d_colour_stats s{};
  if (!n) {
    give_stats(c, stats, s);
    return EG3D_OK;
  }
  if (!obs_off || !rgb_out) {
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
  BUF_TRY(upload(c->k15_off, off64.data(), n, st));
  BUF_TRY(upload(c->k15_view, obs_view, m, st));
  BUF_TRY(upload(c->k15_xy, obs_xy, 2 * m, st));
  if (keep) BUF_TRY(upload(c->k15_keep, keep, n, st));
  BUF_TRY(c->k15_rgb.ensure(3 * n));
  if (flags_out) BUF_TRY(c->k15_flags.ensure(n));
  HIP_TRY(hipStreamSynchronize(st));  // (off64 is read by the copy queued above)
  const K15Cloud cl{n, m, c->k15_off.as<eg3d_off_t>(), c->k15_view.as<int32_t>(), c->k15_xy.as<float>(),
                    keep ? c->k15_keep.as<uint8_t>() : nullptr};
  BUF_TRY(colour_cloud(c, who, cl, c->k15_rgb.as<uint8_t>(), flags_out ? c->k15_flags.as<uint8_t>() : nullptr, &s));
  HIP_TRY(hipMemcpyAsync(rgb_out, c->k15_rgb.p, 3 * n, hipMemcpyDeviceToHost, st));
  if (flags_out) HIP_TRY(hipMemcpyAsync(flags_out, c->k15_flags.p, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  s.ms_copy = std::max(0.f, wall - s.ms_sample - s.ms_mix);
  give_stats(c, stats, s);
  return EG3D_OK;
}

extern "C" int eg3d_colour_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, const uint8_t* keep_dev, uint8_t* rgb_dev,
                                  uint8_t* flags_dev, eg3d_colour_stats* stats) {
  const char* who = "eg3d_colour_device";
  BUF_TRY(check_call(who, c, stats));
  eg3d_device_edgepoints d;
  if (cloud)
    d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, &d));
  BUF_TRY(check_cloud(&d, who, false));
  eg3d_colour_stats s{};
  if (!d.n_points) {
    give_stats(c, stats, s);
    return EG3D_OK;
  }
  if (!rgb_dev) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  const K15Cloud cl{d.n_points, d.n_obs, d.obs_off, d.obs_view, d.obs_xy, keep_dev};
  BUF_TRY(colour_cloud(c, who, cl, rgb_dev, flags_dev, &s));
  give_stats(c, stats, s);
  return EG3D_OK;
}
