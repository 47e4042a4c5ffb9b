// Host-visible declarations of K9 (eg3d_k9_polymatch.hip): pipeline 2 of the reference, polyline matching by closeness to
// the reference points (eg3d_match_polylines_closeness).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_kernels.h"

namespace eg3d {

#define K9_BLOCK 256
#define K9_NONE (~0ull)            /* first / component key of a polyline no accepted point touched */
#define K9_FLAG_BAD_VIEW 1u        /* a track entry names a view outside the rig */

// The 10 px map of PolyLine2DMapSearch(plg, img_sz, FIND_WITHIN_DIST): one CSR over (view, cell), as DevScene's 30 px and
// 4 px grids (K0 builds all three).
struct K9Grid {
  int32_t w, h;
  const uint32_t* off;
  const uint32_t* ids;
};
// Per track entry of the call's range (index = entry - sv_base): the result of the reference's search at the point's
// observation in the entry's view.
struct K9Entries {
  uint32_t* cnt;   // polylines with d^2 <= 100
  uint32_t* pl;    // the first of them (view-local id); the rule reads it only where cnt == 1
  float* dist;     // sqrtf(d^2) of that polyline
};
// The match graph over the scene's global polyline indices g = view_pl_off[view] + pl (all arrays [n_pl]).
struct K9Graph {
  unsigned long long* first;  // smallest accepted point that lists g (K9_NONE: no node)
  uint32_t* parent;           // union-find: parent[g] <= g
  uint32_t* root_of;          // flattened
  unsigned long long* ckey;   // at a root: min over the component of first[g] << 32 | g
  uint32_t* rank_of;          // at a root: the component's position in the result
};

// (1) one lane per seed: sv_seed of its entries; K9_FLAG_BAD_VIEW into *flags (zeroed before) for a view id outside the rig
void launch_k9_prep(hipStream_t st, SeedsDev sd, int32_t n_views, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                    uint32_t* sv_seed, uint32_t* flags);
// (2) one wavefront per entry: find_polylines_within_search_dist_with_reprojections on the 10 px map
void launch_k9_close_polylines(hipStream_t st, DevScene s, K9Grid g10, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                               const uint32_t* sv_seed, K9Entries out);
// (3) parent[g] = g, first[g] = ckey[g] = K9_NONE
void launch_k9_init(hipStream_t st, uint32_t n_pl, K9Graph g);
// (4) one lane per seed: the acceptance rule; an accepted point claims its nodes (64-bit atomicMin of its id) and unites
//     them with its first node. accept is [n_seeds + 1], the last entry 0 (the scan's sentinel)
void launch_k9_refpoint_rule(hipStream_t st, DevScene s, SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                             K9Entries in, uint32_t* accept, K9Graph g);
// (5) one lane per polyline: root_of, the component keys; *n_nodes (zeroed before) += nodes
void launch_k9_flatten(hipStream_t st, uint32_t n_pl, K9Graph g, uint32_t* n_nodes);
// (6) over the sorted component keys: rank_of[root] = position; *n_sets (zeroed before) += components
void launch_k9_rank(hipStream_t st, const unsigned long long* ckey_sorted, uint32_t n_pl, K9Graph g, uint32_t* n_sets);
// (7) per polyline the key (rank * n_views + view) << EG3D_K0_PL_BITS | view-local id (K9_NONE: no node): sorted, it is
//     the input of launch_k0_csr with n_sets * n_views "cells"
void launch_k9_node_keys(hipStream_t st, DevScene s, uint32_t n_pl, K9Graph g, unsigned long long* keys);
// (8) accepted[off[i]] = seed_begin + i where accept[i]
void launch_k9_compact(hipStream_t st, const uint32_t* accept, const uint32_t* off, uint32_t seed_begin, uint32_t n_seeds,
                       uint32_t* accepted);

}  // namespace eg3d
