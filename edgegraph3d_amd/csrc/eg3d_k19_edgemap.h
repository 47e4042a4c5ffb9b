// Host-visible declarations of K19 (eg3d_k19_edgemap.hip): the edge maps of the source images (include/eg3d/edgemap.hh;
// the per-pixel rules: eg3d_edgemap_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_edgemap_core.h"

namespace eg3d {

#define K19_BLOCK 256
#define K19_TILE 32            /* a workgroup's tile is K19_TILE x K19_TILE pixels; an image need not be a multiple of it */
#define K19_VIEWS_PER_LAUNCH 32768 /* gridDim.z of one launch; a call with more views launches again */

// The views of a call lie one after the other in every per-pixel array; so do their tiles in the two per-tile arrays.
struct K19View {
  unsigned long long off;       // the view's first pixel
  unsigned long long tile_off;  // the view's first tile
  int32_t w, h;
};
// what every tiled launch needs: the table on the device, its length, the largest tile counts of any view
struct K19Views {
  const K19View* views;
  uint32_t n_views;
  uint32_t max_tx, max_ty;
};
EG3D_HD uint32_t k19_tiles(int32_t n) { return ((uint32_t)n + K19_TILE - 1) / K19_TILE; }

// the counters of a call (64-bit words)
enum { K19C_CANDIDATES, K19C_STRONG, K19C_EDGES, K19C_COUNT };

// One smoothing pass (E2). from_rgb: `src` holds the images (3 bytes a pixel) and E1 is applied on the way in; otherwise
// it holds grey values. dst: grey values.
void launch_k19_smooth(hipStream_t st, K19Views v, bool from_rgb, const uint8_t* src, uint8_t* dst);
// E3 - E5 and the class of every pixel (E6's first half) -> cls; candidates and strong pixels added to ctr
void launch_k19_classify(hipStream_t st, K19Views v, bool from_rgb, const uint8_t* src, bool l2, uint32_t low, uint32_t high, uint8_t* cls,
                         unsigned long long* ctr);
// One round of E6's propagation: every tile whose dirty_in byte is set turns the weak candidates that a strong pixel
// reaches inside the tile (its 1-pixel frame included) strong, clears its dirty_in byte and, if it changed anything, sets
// the dirty_out bytes of its eight neighbours and adds 1 to *changed.
void launch_k19_hysteresis(hipStream_t st, K19Views v, uint8_t* cls, uint8_t* dirty_in, uint8_t* dirty_out, unsigned int* changed);
// classes -> mask, in place (strong: 1, everything else: 0); the edges added to ctr[K19C_EDGES]
void launch_k19_mask(hipStream_t st, uint8_t* cls, unsigned long long n, unsigned long long* ctr);

}  // namespace eg3d
