// Host-visible declarations of K14 (eg3d_k14_triangulate.hip): FP64 triangulation of caller-supplied tracks
// (include/eg3d_triangulate.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

struct Obs;  // eg3d_dev_tri.h: the 16-byte observation record the solver reads
#define K14_REC_BYTES 16

#define K14_BLOCK 256
#define K14_MAX_ROWS 32767u /* observations of one track: the 15-bit row count of the solver's request table (CoopLds::n16) */
// flag word of the checks
#define K14_BAD_VIEW 1u    /* a view id outside [0, n_views) */
#define K14_BAD_OFFSETS 2u /* a list that is not an ascending range inside [0, n_obs] */
#define K14_LONG_LIST 4u   /* a list of more than K14_MAX_ROWS observations */

// per-track output flags (= EG3D_TRI_FLAG_SHORT / EG3D_TRI_FLAG_DEGENERATE: eg3d_api_triangulate.hip asserts it)
#define K14_OUT_SHORT 1u
#define K14_OUT_DEGENERATE 2u

// The tracks as both entry points hand them over: 64-bit offsets WITHOUT a sentinel (track i ends where track i + 1
// begins, the last one at n_obs), SoA observations, start points (EG3D_TRI_REFINE; may alias the output).
struct K14Tracks {
  uint64_t n_tracks, n_obs;
  const eg3d_off_t* obs_off;
  const int32_t* obs_view;
  const float* obs_xy;
  const float* X0;
};

// (1) one lane per track: *flags |= K14_BAD_OFFSETS / K14_LONG_LIST. Nothing is indexed with an offset.
void launch_k14_check(hipStream_t st, K14Tracks t, uint32_t* flags);
// (2) one lane in all: the call's batches. cuts[0] = the number of batches B, then B + 1 pairs (track, observation):
//     cuts[1 + 2 k], cuts[2 + 2 k] = first track and first observation of batch k; pair B = (n_tracks, n_obs). A batch is
//     the longest run of whole tracks from its first one whose observations number at most `budget` — one track when
//     that track alone has more. At most `cap` batches are written; cuts[0] = cap + 1 says there would have been more
//     (possible only with offsets the check refuses). Bisection over the offsets: stays inside obs_off whatever it holds.
void launch_k14_cut(hipStream_t st, K14Tracks t, uint64_t budget, uint64_t cap, unsigned long long* cuts);
// (3) one lane per observation of [o0, o1): rec[q - o0] = (view, x, y) of observation q as a 16-byte record; a view id
//     outside the rig is recorded as view 0 and raises K14_BAD_VIEW, so nothing downstream indexes with it.
void launch_k14_stage(hipStream_t st, K14Tracks t, int n_views, uint64_t o0, uint64_t o1, Obs* rec, uint32_t* flags);
// (4) one single-wave workgroup per window of EG3D_COOP_REQ tracks of [t0, t1), whose records are rec[obs_off - o0]:
//     X_out / valid / flags_out (may be null) at the track's own index; counts[0..2] += valid, short, degenerate tracks.
void launch_k14_solve(hipStream_t st, const float* cam_P, int cams_mid_range, int mode, K14Tracks t, uint64_t t0, uint64_t t1,
                      uint64_t o0, const Obs* rec, float* X_out, uint8_t* valid, uint8_t* flags_out, unsigned long long* counts);

}  // namespace eg3d
