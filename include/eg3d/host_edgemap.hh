/*
 * eg3d/host_edgemap.hh — the edge maps of the source images, their sequential statement; the PNG writer of a mask; the
 * polyline graphs of many masks at once (libeg3d_host.so), K19.
 *
 * (Why .hh: the older ABI tests pin the sets of .h and .hpp files under include/ and may not change. The text is the
 * C/C++ common subset like every other ABI header — it compiles as C99 — and is a row of the open registry:
 * _cabi.OPEN_HEADERS, _cdefs.MIRRORS_OPEN, tests/test_abi_open.py. The next header is a row there, of any suffix.)
 *
 * DEFINITION. An image is [H][W][3] bytes, R G B, row-major; W and H are 1 .. 16384 and the views of a call may differ in
 * size. Every value below is an integer; the rules are this project's own (E1 and E5 are written after OpenCV's cvtColor
 * and Canny from memory and are NOT pinned against them: no parity is claimed).
 *
 *   E1 grey       Y = (4899 R + 9617 G + 1868 B + 8192) >> 14
 *   E2 smoothing  smooth_passes passes (0 .. 4), each the 5 x 5 binomial (1 4 6 4 1) x (1 4 6 4 1):
 *                 out = (sum + 128) >> 8, the sum over both directions with no rounding in between. An index outside
 *                 the image folds as reflect-101: for n = 1 the index is 0; otherwise i = |i| mod 2(n - 1), and if
 *                 i >= n then i = 2(n - 1) - i. Defined for every n >= 1.
 *   E3 gradient   the 3 x 3 Sobel pair on the smoothed grey, borders replicated:
 *                 gx = (p[r-1][c+1] + 2 p[r][c+1] + p[r+1][c+1]) - (p[r-1][c-1] + 2 p[r][c-1] + p[r+1][c-1])
 *                 gy = (p[r+1][c-1] + 2 p[r+1][c] + p[r+1][c+1]) - (p[r-1][c-1] + 2 p[r-1][c] + p[r-1][c+1])
 *   E4 magnitude  m = |gx| + |gy|, compared with low and high; with l2 = 1: m = gx^2 + gy^2, compared with low^2 and
 *                 high^2. 0 <= low <= high <= 65535.
 *   E5 non-maximum suppression. Magnitudes outside the image are 0. x = |gx|, y = |gy| << 15, t22 = x * 13573,
 *                 t67 = t22 + (x << 16), in 64 bits.
 *                   y < t22:   kept iff m > m[r][c-1] and m >= m[r][c+1]
 *                   y > t67:   kept iff m > m[r-1][c] and m >= m[r+1][c]
 *                   otherwise: s = ((gx ^ gy) < 0) ? -1 : 1; kept iff m > m[r-1][c-s] and m > m[r+1][c+s]
 *   E6 hysteresis A pixel is a CANDIDATE iff it is kept and m > low; a candidate is STRONG iff m > high (the squared
 *                 bounds under l2). A pixel is an EDGE iff it is a candidate whose 8-connected component of candidates
 *                 holds a strong pixel. This is a set: no visiting order enters it.
 *   E7 refusals   decided on the host before anything is computed or launched, -1 (EG3D_EDGEMAP_ERR_ARG) with a message, the
 *                 masks and the stats untouched: a null pointer (width, height, rgb, masks, params, or one rgb[v] /
 *                 masks[v]), n_views <= 0, a side < 1 or > 16384, low / high / smooth_passes out of range, l2 other than
 *                 0 or 1, a params or stats struct whose struct_size is smaller than the library's.
 *
 * The mask of view v is [H][W] bytes, 1 = edge, 0 otherwise: what eg3d_plg_build_from_mask takes.
 */
#ifndef EG3D_HOST_EDGEMAP_HH_
#define EG3D_HOST_EDGEMAP_HH_
#include <stdint.h>

#include "../eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_EDGEMAP_ERR_ARG -1
#define EG3D_EDGEMAP_ERR_FILE -2    /* the PNG writer: the file cannot be written */
#define EG3D_EDGEMAP_ERR_MEMORY -6  /* out of host memory */
#define EG3D_EDGEMAP_ERR_ROUNDS -25 /* (device only) the hysteresis passed its bound of rounds: no mask is written */

#define EG3D_EDGEMAP_MAX_DIM 16384
#define EG3D_EDGEMAP_MAX_SMOOTH_PASSES 4
#define EG3D_EDGEMAP_MAX_THRESHOLD 65535

typedef struct eg3d_edgemap_params {
  uint32_t struct_size; /* sizeof(eg3d_edgemap_params), set by the caller; a smaller value is refused */
  int32_t low;
  int32_t high;
  int32_t smooth_passes; /* 0 .. 4; the Python layer's default is 1 */
  int32_t l2;            /* 0: |gx| + |gy|; 1: gx^2 + gy^2 against the squared bounds */
  uint32_t reserved;
} eg3d_edgemap_params;

typedef struct eg3d_edgemap_stats {
  uint32_t struct_size; /* sizeof(eg3d_edgemap_stats), set by the caller; a smaller value is refused */
  uint32_t n_views;
  uint64_t n_pixels;     /* over all views */
  uint64_t n_candidates; /* E6's candidates, the strong ones included */
  uint64_t n_strong;
  uint64_t n_edges;
  uint32_t hysteresis_rounds; /* device: launches of the propagation up to and including the first that changed nothing
                                 (it depends on how the workgroups of a launch interleave; the masks do not); host: 1 */
  uint32_t reserved;
  float ms_upload;     /* device: the images to the device; host: 0 */
  float ms_kernel;     /* E1 - E6's classes (device: the front-end kernels; host: wall time) */
  float ms_hysteresis; /* E6's components, the masks and their count */
  float ms_copy;       /* device: the masks to the host; host: 0 */
} eg3d_edgemap_stats;

const char* eg3d_host_edgemap_last_error(void); /* per thread: which rule refused the last call of this header */

/* The statement: the views one after the other on OpenMP threads, each view sequential. stats may be NULL. */
int eg3d_host_edge_maps(int32_t n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                        const eg3d_edgemap_params* params, uint8_t* const* masks, eg3d_edgemap_stats* stats);

/* A mask (non-zero = edge) as a 1-bit greyscale PNG, white = edge, non-interlaced: what eg3d_png_read_edge_mask and any
 * PNG reader decode. 0, EG3D_EDGEMAP_ERR_ARG (a null pointer, a side < 1 or > 16384), .._FILE or .._MEMORY. */
int eg3d_host_png_write_mask(const char* path, const uint8_t* mask, int32_t width, int32_t height);

/* The polyline graphs of n_views masks (mask v: [height[v]][width[v]], non-zero = edge), built concurrently on the
 * host's cores; out[v] is what eg3d_plg_build_from_mask gives for mask v (released with eg3d_plg_view_free). Returns 0,
 * EG3D_EDGEMAP_ERR_ARG, or -(v + 2) for the first view (in order) whose build failed; on failure nothing is left allocated. */
int eg3d_host_plg_build_views_from_masks(const uint8_t* const* masks, int32_t n_views, const int32_t* width, const int32_t* height,
                                         eg3d_plg_view* out);

#ifdef __cplusplus
}
#endif
#endif
