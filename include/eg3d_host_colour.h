/*
 * eg3d_host_colour.h — the host statement of include/eg3d_colour.h, the PLY writer and the RGB PNG reader
 * (libeg3d_host.so). No GPU.
 *
 * eg3d_host_colour_points is the sequential definition of eg3d_colour_points / eg3d_colour_device (the sample and the mix
 * as include/eg3d_colour.h states them, the border rule as its loop), threaded over points: the same checks, the same
 * refusals (return -1, outputs unspecified), the same colours, flags and counts.
 *
 * eg3d_host_write_ply writes what the reference's output_point_cloud / output_colored_point_cloud write, with and without
 * `inliers` (io/output/output_point_cloud.cpp:127-257): ASCII PLY; ten header lines (ply, format ascii 1.0,
 * element vertex <count>, six property lines, end_header), each ended by '\n'; one line "x y z r g b" per written point,
 * floats as `ostream << float` prints them (%g of the widened value, precision 6), colours as ints; a '\n' after a line
 * UNLESS the point's index is n_points - 1 — so a file whose last point is kept does not end in a newline and one whose
 * last point is dropped does. <count> is the number of kept points.
 *
 * eg3d_host_png_read_rgb decodes what eg3d_png_read_edge_mask decodes (every colour type and bit depth, no interlacing)
 * into RGB8 interleaved: grey replicated, the palette expanded, alpha dropped, 16-bit samples by their high byte, sub-byte
 * grey scaled to 0 .. 255 (v * 255 / (2^depth - 1)). JPEG is not read.
 */
#ifndef EG3D_HOST_COLOUR_H_
#define EG3D_HOST_COLOUR_H_
#include "eg3d_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* images as eg3d_upload_images takes them; arrays as eg3d_colour_points takes them; counts [3], may be NULL: coloured
 * points, empty points, observations of the kept points. 0, or -1 when the arguments are refused. */
int eg3d_host_colour_points(int n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb, uint64_t n_points,
                            const uint32_t* obs_off, const int32_t* obs_view, const float* obs_xy, const uint8_t* keep,
                            int n_threads, uint8_t* rgb_out, uint8_t* flags_out, uint64_t* counts);

/* cv::borderInterpolate(p, len, BORDER_REFLECT_101), len >= 1: the loop the statement uses, and the closed form the
 * kernel uses (the host compilation of csrc/eg3d_dev_colour.h), so that a CPU test can hold one to the other */
int eg3d_host_reflect101_loop(int p, int len);
int eg3d_host_reflect101_closed(int p, int len);

/* X [n_points][3]; rgb [n_points][3], NULL = every point white (255 255 255); keep [n_points], NULL = all.
 * 0, -1 bad arguments, -2 the file cannot be written */
int eg3d_host_write_ply(const char* path, uint64_t n_points, const float* X, const uint8_t* rgb, const uint8_t* keep);

/* *rgb_out: width * height * 3 bytes, malloc'ed (eg3d_host_free). Return codes as eg3d_png_read_edge_mask. */
int eg3d_host_png_read_rgb(const char* path, int* width, int* height, uint8_t** rgb_out);

#ifdef __cplusplus
}
#endif
#endif
