/*
 * eg3d/host_nearest.hpp — cloud-to-cloud nearest distances, their sequential statement, and the PLY point reader
 * (libeg3d_host.so), K18.
 *
 * (Why .hpp: tests/test_abi.py and tests/test_abi_edges.py pin the set of .h files under include/ and may not change. The
 * text is the C/C++ common subset like every other ABI header — it compiles as C99 — and has a registry of its own:
 * _cabi.HPP_HEADERS, _cdefs.MIRRORS_HPP, tests/test_abi_nearest.py.)
 *
 * DEFINITION. Reference points R[j] (FP32 xyz, j < n_ref < 2^32), query points Q[i], max_dist > 0 finite, FP32.
 * md2 = max_dist * max_dist in FP32. Every operation is FP32 without FMA:
 *     dx = q.x - r.x; dy = q.y - r.y; dz = q.z - r.z;   d2 = (dx * dx + dy * dy) + dz * dz
 *   r is within reach of q iff d2 < md2 (strict). The result for q is the smallest d2 over the indexed reference points
 *   within reach; nn is the smallest original index j among those that attain it. A query with nothing in reach gets
 *   d2 = +inf (bits 0x7f800000) and nn = 0xffffffff; so does a query its `keep` drops (keep[i] == 0) or that has a
 *   non-finite coordinate. A reference point its `keep` drops or that has a non-finite coordinate is not indexed; both
 *   kinds are counted. nn names the position in the reference array as given.
 *
 * INDEX. A uniform grid of edge `cell` (FP32, finite, > 0) whose origin is the component-wise minimum of the indexed
 *   points (no indexed point: 0); the cell coordinate of a value x on an axis is
 *   floor(((double)x - (double)origin) / (double)cell). An axis may span fewer than 2^21 cells (EG3D_NEAREST_ERR_EXTENT
 *   otherwise). Per axis a query scans the cells of fl32(q - max_dist) .. fl32(q + max_dist), clamped to the grid;
 *   max_dist > cell is refused (it would unbound the work). csrc/eg3d_nearest_core.h holds the arithmetic and the argument
 *   why no reference point within reach is missed (BOUNDS).
 *
 * FIGURES, all exact and independent of the order of evaluation. The WITHIN set: the queries with a result.
 *   n_queries, n_dropped (by keep), n_nonfinite (kept, a non-finite coordinate), n_within
 *   n_below[k] = #{d2 < t_k * t_k}, the product in FP32, for the caller's n_thresholds <= 8 thresholds
 *                (each finite, 0 < t_k <= max_dist)
 *   min_d2, max_d2 over the within set; median_d2 = the element of ascending rank (n_within - 1) / 2
 *   sum_q32 = the sum over the within set of (uint64_t)(sqrt((double)d2) * (4294967296.0 / (double)max_dist)):
 *             mean distance = sum_q32 * max_dist / 2^32 / n_within, accurate to max_dist * 2^-32
 *   n_within == 0: the three d2 figures are +inf, sum_q32 is 0.
 *
 * REFUSALS, decided before anything is written (d2, nn and stats stay untouched): a stats struct smaller than the
 * library's, a null array with a count above 0 (EG3D_NEAREST_ERR_ARG); cell not finite or <= 0 (.._CELL); max_dist not
 * finite, <= 0 or > cell (.._MAXDIST); more than 8 thresholds, or one outside the rule above (.._THRESHOLD); n_ref or n
 * >= 2^32 (.._CAPACITY); 2^21 cells or more on an axis (.._EXTENT). n_ref == 0 and n == 0 are no refusals.
 * eg3d_host_nearest_last_error() says which rule, per thread.
 */
#ifndef EG3D_HOST_NEAREST_HPP_
#define EG3D_HOST_NEAREST_HPP_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG3D_NEAREST_MAX_THRESHOLDS 8
#define EG3D_NEAREST_NONE 0xffffffffu

#define EG3D_NEAREST_ERR_ARG -1
#define EG3D_NEAREST_ERR_CAPACITY -3
#define EG3D_NEAREST_ERR_CELL -18
#define EG3D_NEAREST_ERR_MAXDIST -19
#define EG3D_NEAREST_ERR_THRESHOLD -20
#define EG3D_NEAREST_ERR_EXTENT -21
#define EG3D_NEAREST_ERR_FOREIGN -22 /* (device only) the index was built by another context */
#define EG3D_NEAREST_ERR_FILE -23    /* the PLY reader: the file cannot be opened or read */
#define EG3D_NEAREST_ERR_PLY -24     /* the PLY reader: the file is refused; the last-error text says why */

typedef struct eg3d_cloud_index_stats {
  uint32_t struct_size; /* sizeof(eg3d_cloud_index_stats), set by the caller; a smaller value is refused */
  uint32_t reserved;
  uint64_t n_points;    /* the reference array's length */
  uint64_t n_dropped;   /* ... of which keep drops */
  uint64_t n_nonfinite; /* ... of which kept, with a non-finite coordinate */
  uint64_t n_indexed;
  uint64_t n_cells;         /* occupied cells */
  uint64_t max_cell_points; /* the largest cell population */
  float origin[3];
  float cell;
  uint32_t dims[3]; /* cells per axis (0 without an indexed point) */
  uint32_t reserved2;
  float ms_build; /* device: the kernels and primitives of the build; host: wall time */
  float ms_copy;  /* device: the upload of a host array */
} eg3d_cloud_index_stats;

typedef struct eg3d_nearest_stats {
  uint32_t struct_size;  /* sizeof(eg3d_nearest_stats), set by the caller; a smaller value is refused */
  uint32_t n_thresholds; /* IN: <= EG3D_NEAREST_MAX_THRESHOLDS */
  float thresholds[8];   /* IN: distances, each finite and in (0, max_dist] */
  uint64_t n_queries;
  uint64_t n_dropped;
  uint64_t n_nonfinite;
  uint64_t n_within;
  uint64_t n_below[8];
  uint64_t sum_q32;
  float min_d2;
  float max_d2;
  float median_d2;
  float ms_kernel; /* device: the query kernel and the sort behind the median; host: wall time */
  float ms_copy;   /* device: uploads and downloads of host arrays */
  float reserved;
} eg3d_nearest_stats;

const char* eg3d_host_nearest_last_error(void);

/* The statement: its own grid over ref_X [n_ref][3] (ref_keep [n_ref] or NULL), the queries X [n][3] (keep [n] or NULL)
 * one after the other. d2 [n] and nn [n] may each be NULL. stats carries the thresholds in and the figures out. */
int eg3d_host_cloud_nearest(const float* ref_X, uint64_t n_ref, const uint8_t* ref_keep, const float* X, uint64_t n,
                            const uint8_t* keep, float cell, float max_dist, float* d2, uint32_t* nn, eg3d_nearest_stats* stats);

/* what the statement's grid over the reference looks like: the figures eg3d_cloud_index_build reports */
int eg3d_host_cloud_index_stats(const float* ref_X, uint64_t n_ref, const uint8_t* ref_keep, float cell, eg3d_cloud_index_stats* stats);

/* The `element vertex` of a PLY file as points: `format ascii 1.0` and `format binary_little_endian 1.0`, scalar
 * properties only; the float properties x, y, z are taken (an ASCII coordinate is (float)strtod(text)), every other scalar
 * property — colours, normals — is skipped by its size, elements after `vertex` are ignored. *X: [*n][3], malloc'd,
 * released with eg3d_host_free_points; both untouched on failure. EG3D_NEAREST_ERR_FILE: the file cannot be read.
 * EG3D_NEAREST_ERR_PLY, each with its own last-error text: no "ply" magic, a header that does not end, a big-endian or
 * unknown format, no `element vertex` or an element before it, a list property inside `vertex`, an unknown property
 * type, a missing or non-float x, y or z, a body shorter than the header promises. */
int eg3d_host_read_ply_points(const char* path, float** X, uint64_t* n);
void eg3d_host_free_points(float* X);

#ifdef __cplusplus
}
#endif
#endif
