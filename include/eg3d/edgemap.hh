/*
 * eg3d/edgemap.hh — the edge maps of the source images on the device (libeg3d.so, libeg3d_dlt4x4.so), K19.
 *
 * (Why .hh: see eg3d/host_edgemap.hh, which also holds the DEFINITION E1 - E7, the structs and the error codes.)
 *
 * Context-free like eg3d_estimate_fundamental: the edge maps come before any scene, so the call makes its own stream and
 * buffers on `device` and releases them when it returns. The images go up once; grey values, smoothed values and classes
 * stay on the device; one byte per pixel comes back. The masks and every count are bit for bit those of
 * eg3d_host_edge_maps.
 *
 * Hysteresis: a workgroup owns a tile of classes, propagates "strong" to its fixed point in LDS and writes what changed;
 * launches repeat until one changes nothing (workgroups meet only at kernel boundaries and through one agent-scope
 * counter). The loop is bounded by n_candidates + 1 rounds — a round that changes something turns at least one candidate —
 * and EG3D_EDGEMAP_ERR_ROUNDS past that bound writes no mask.
 *
 * Refusals (E7) are decided before the device is touched; EG3D_ERR_NODEVICE / EG3D_ERR_HIP (eg3d.h) after that.
 * eg3d_last_error() says which rule.
 */
#ifndef EG3D_EDGEMAP_HH_
#define EG3D_EDGEMAP_HH_
#include <stdint.h>

#include "host_edgemap.hh"

#ifdef __cplusplus
extern "C" {
#endif

/* rgb[v]: [height[v]][width[v]][3] on the host; masks[v]: [height[v]][width[v]] on the host, written only on success.
 * stats may be NULL. */
int eg3d_edge_maps(int device, int32_t n_views, const int32_t* width, const int32_t* height, const uint8_t* const* rgb,
                   const eg3d_edgemap_params* params, uint8_t* const* masks, eg3d_edgemap_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
