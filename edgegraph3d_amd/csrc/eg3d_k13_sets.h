// Host-visible declarations of K13 (eg3d_k13_sets.hip): polyline sets that stay on the device (include/eg3d_sets_device.h) —
// the sets of a community assignment, and the checks of a caller's uploaded sets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

#define K13_BLOCK 256
// flag word of eg3d_sets_from_communities_device (counters[1])
#define K13_BAD_VIEW 1u /* a named node's view is not one of the scene's */
#define K13_BAD_PL 2u   /* a named node's polyline id does not fit the key's EG3D_K0_PL_BITS */
// flag word of eg3d_upload_polyline_sets
#define K13_SETS_BAD_START 1u  /* row_off[0] != 0 */
#define K13_SETS_BAD_ORDER 2u  /* row_off descends somewhere */
#define K13_SETS_BAD_RANGE 4u  /* an id is not below its view's polyline count */
#define K13_SETS_BAD_STRICT 8u /* ids of a row do not ascend strictly */

// (1) one lane per node: named[i] = ids[i] >= 0; counters[0] = max over the named nodes of id + 1 (the number of sets),
//     counters[1] |= K13_BAD_* of the named nodes. Nothing is indexed with an id, a view or a polyline id.
void launch_k13_validate(hipStream_t st, const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl, uint32_t n,
                         uint32_t n_views, uint32_t* named, unsigned long long* counters);
// (2) one lane per node, after the scan of `named`: keys[pos[i]] = (id * V + view) << EG3D_K0_PL_BITS | pl for the named
//     nodes — the key launch_k0_csr takes, over n_sets * V "cells". The caller has read the counters: every key fits.
void launch_k13_keys(hipStream_t st, const int64_t* ids, const uint32_t* node_view, const uint32_t* node_pl, uint32_t n,
                     uint32_t n_views, const uint32_t* named, const uint32_t* pos, unsigned long long* keys);
// The checks of uploaded sets, one lane per row boundary and one per id: *bad |= K13_SETS_BAD_*. The id pass finds its row
// by bisection, which stays inside row_off whatever the offsets hold, so both may run before either verdict is read.
void launch_k13_check_sets(hipStream_t st, DevScene s, SetsDev sets, uint32_t n_rows, uint32_t n_ids, uint32_t* bad);

}  // namespace eg3d
