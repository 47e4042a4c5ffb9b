// eg3d_api_dedup_phases.hip — the 3 px de-duplication in its phases (include/eg3d_dedup_phases.h): claim, keep, the claim
// map itself and the minimum that joins two maps; and the steps these and the combined calls of eg3d_api_filter.hip share.
#include <cmath>

#include "../../include/eg3d_dedup_phases.h"
#include "eg3d_api_internal.h"

// ---- the shared steps (declared in eg3d_api_internal.h) ----------------------------------------------------------------------
#define EG3D_DEDUP_MAX_INDEX 0xFFFFFFFFull /* K7_UNCLAIMED: index_base + n_points stays below it */
int eg3d::api::dedup_index_check(const char* who, uint64_t index_base, uint64_t n_points) {
  if (index_base >= EG3D_DEDUP_MAX_INDEX || n_points >= EG3D_DEDUP_MAX_INDEX - index_base) {
    g_err = std::string(who) + ": index_base + n_points must stay below 2^32 - 1 (the claim map holds 32-bit point indices)";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}
uint64_t eg3d::api::dedup_n_cells(const eg3d_ctx* c, int* w_out, int* h_out) {
  const int w = (int)std::ceil((float)c->W / 3), h = (int)std::ceil((float)c->H / 3);  // as host/post_steps.cpp
  if (w_out) *w_out = w;
  if (h_out) *h_out = h;
  return (uint64_t)c->V * (uint64_t)w * (uint64_t)h;
}
int eg3d::api::dedup_map_open(eg3d_ctx* c, bool reset, K7Map* m) {
  int w = 0, h = 0;
  const size_t map_bytes = 4 * (size_t)dedup_n_cells(c, &w, &h);
  if (!c->d_first.p) c->dedup_valid = false;
  BUF_TRY(c->d_first.ensure_exact(map_bytes));  // (it never grows, and a many-view rig's map is hundreds of MB)
  const bool fill = reset || !c->dedup_valid;
  c->dedup_valid = false;  // until the call is known to have completed: a failure leaves the map to be refilled
  if (fill) HIP_TRY(hipMemsetAsync(c->d_first.p, 0xFF, map_bytes, c->stream));
  *m = K7Map{c->d_first.as<uint32_t>(), c->V, w, h};
  return EG3D_OK;
}
int eg3d::api::dedup_counters_zero(eg3d_ctx* c, unsigned long long** cnt) {
  BUF_TRY(c->d_cnt.ensure(16));
  HIP_TRY(hipMemsetAsync(c->d_cnt.p, 0, 16, c->stream));
  *cnt = c->d_cnt.as<unsigned long long>();
  return EG3D_OK;
}
int eg3d::api::dedup_counters_read(eg3d_ctx* c, const char* who, uint64_t* count) {
  uint64_t back[2];  // a count, flags
  HIP_TRY(hipMemcpyAsync(back, c->d_cnt.p, sizeof(back), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((uint32_t)back[1]) return device_flags_error(who, (uint32_t)back[1]);
  if (count) *count = back[0];
  return EG3D_OK;
}

// A phased call that fails after its arguments were accepted discards all claims; `keep_claims` is set on the way out of a
// call that completed (or that was refused by a check that ran before the map was touched).
namespace {
struct ClaimsGuard {
  eg3d_ctx* c;
  bool keep_claims = false;
  ~ClaimsGuard() { if (!keep_claims) c->dedup_valid = false; }
};
}  // namespace

// ---- the phases ------------------------------------------------------------------------------------------------------------
extern "C" int eg3d_dedup_claim(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, uint64_t index_base, int reset) {
  if (cloud) BUF_TRY(dedup_index_check("eg3d_dedup_claim", index_base, cloud->n_points));
  if (!c || !cloud) {
    g_err = "eg3d_dedup_claim: bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_cloud(cloud, "eg3d_dedup_claim", false));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const CloudView in = cloud_view(cloud);
  // The combined call leaves the offsets to its keep kernel and discards the claims of a bad cloud; a claim pass on its own
  // must know before it writes: one lane per point, one read-back. Nothing of the map (a reset included) has happened yet,
  // so a cloud that fails leaves the claims exactly as they were.
  unsigned long long* cnt = nullptr;
  BUF_TRY(dedup_counters_zero(c, &cnt));
  HIP_TRY(hipEventRecord(c->ea[0], st));  // (the phase's device time covers the check and its read-back: they are its price)
  launch_offsets_check(st, in, (uint32_t*)(cnt + 1));
  HIP_TRY(hipGetLastError());
  BUF_TRY(dedup_counters_read(c, "eg3d_dedup_claim", nullptr));
  ClaimsGuard guard{c};
  K7Map m;
  BUF_TRY(dedup_map_open(c, reset != 0, &m));
  launch_dedup_claim(st, in, m, (uint32_t)index_base);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));  // the cloud may be overwritten, and a peer may read the map, as soon as the call returns
  c->dedup_valid = guard.keep_claims = true;
  return EG3D_OK;
}

extern "C" int eg3d_dedup_keep(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, uint64_t index_base, uint8_t* keep_dev,
                               uint64_t* n_kept_host) {
  if (cloud) BUF_TRY(dedup_index_check("eg3d_dedup_keep", index_base, cloud->n_points));
  if (!c || !cloud || (cloud->n_points && !keep_dev)) {
    g_err = "eg3d_dedup_keep: bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_cloud(cloud, "eg3d_dedup_keep", false));
  if (!c->d_first.p || !c->dedup_valid) {
    g_err = "eg3d_dedup_keep: the context holds no valid claim map (nothing was claimed or merged, or a dedup call failed)";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  int w = 0, h = 0;
  dedup_n_cells(c, &w, &h);
  const K7Map m{c->d_first.as<uint32_t>(), c->V, w, h};
  ClaimsGuard guard{c};
  unsigned long long* cnt = nullptr;
  BUF_TRY(dedup_counters_zero(c, &cnt));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_dedup_keep(st, cloud_view(cloud), m, (uint32_t)index_base, keep_dev, cnt, (uint32_t*)(cnt + 1));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  uint64_t kept = 0;
  const int rc = dedup_counters_read(c, "eg3d_dedup_keep", &kept);
  // offsets that do not ascend are a refusal of the cloud (the keep pass reads the map and writes none of it: the claims
  // stand); any other failure discards them
  guard.keep_claims = rc == EG3D_OK || rc == EG3D_ERR_ARG;
  BUF_TRY(rc);
  if (n_kept_host) *n_kept_host = kept;
  return EG3D_OK;
}

extern "C" int eg3d_dedup_claims(eg3d_ctx* c, uint32_t** first_dev, uint64_t* n_cells) {
  if (!c || !first_dev) {
    g_err = "eg3d_dedup_claims: bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  ClaimsGuard guard{c};
  guard.keep_claims = c->d_first.p && c->dedup_valid;  // (a failed allocation below leaves a valid map valid)
  if (!guard.keep_claims) {
    K7Map m;
    BUF_TRY(dedup_map_open(c, true, &m));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's own stream or a peer may touch the map next
    c->dedup_valid = guard.keep_claims = true;
  }
  *first_dev = c->d_first.as<uint32_t>();
  if (n_cells) *n_cells = dedup_n_cells(c);
  return EG3D_OK;
}

extern "C" int eg3d_dedup_merge_claims(eg3d_ctx* c, const uint32_t* other_dev, uint64_t n_cells, uint64_t* n_lowered_host) {
  if (!c || !other_dev || ((uintptr_t)other_dev & 3u)) {
    g_err = "eg3d_dedup_merge_claims: bad arguments (other_dev must be a 4-byte aligned device address)";
    return EG3D_ERR_ARG;
  }
  if (n_cells != dedup_n_cells(c)) {
    g_err = "eg3d_dedup_merge_claims: n_cells is not this context's (n_views x ceil(width / 3) x ceil(height / 3) = " +
            std::to_string(dedup_n_cells(c)) + ")";
    return EG3D_ERR_ARG;
  }
  if (n_lowered_host) *n_lowered_host = 0;
  if (c->d_first.p && c->dedup_valid && other_dev == c->d_first.as<uint32_t>()) return EG3D_OK;  // min(a, a)
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  ClaimsGuard guard{c};
  K7Map m;
  BUF_TRY(dedup_map_open(c, false, &m));  // a context without a valid map gets one: fill, then min
  unsigned long long* cnt = nullptr;
  BUF_TRY(dedup_counters_zero(c, &cnt));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  launch_claims_min(st, m.first, other_dev, n_cells, cnt, c->tune.merge_write_all);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  uint64_t lowered = 0;
  BUF_TRY(dedup_counters_read(c, "eg3d_dedup_merge_claims", &lowered));
  c->dedup_valid = guard.keep_claims = true;
  if (n_lowered_host) *n_lowered_host = lowered;
  return EG3D_OK;
}

extern "C" int eg3d_dedup_phase_ms(eg3d_ctx* c, float* ms) {
  if (!c || !ms) {
    g_err = "eg3d_dedup_phase_ms: bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventElapsedTime(ms, c->ea[0], c->eb[0]));
  return EG3D_OK;
}
