/*
 * eg3d_dedup_phases.h — the 3 px de-duplication of a device-resident cloud in its phases (libeg3d.so, libeg3d_dlt4x4.so;
 * K7 and K7b). eg3d_dedup_device (include/eg3d.h) runs the claim pass and the keep pass back to back against the claim map
 * of one context: right when the clouds of a run reach that context in cloud order. The rule itself does not care about
 * order — keep[i] holds exactly when some observation of point i lies in a cell whose SMALLEST claiming index is i, and a
 * minimum is the same whoever arrives first — so the phases are offered on their own, with the operation that joins maps:
 *
 *   claim   every cloud of the run, in any order, on any context, each with its run-wide index_base;
 *   merge   the maps of the contexts (eg3d_dedup_merge_claims) or of the ranks (eg3d_allreduce_claims, eg3d_rccl_claims.h)
 *           into each other: an element-wise minimum;
 *   keep    every cloud against a map that holds all claims of the clouds in front of it (it may hold later ones too:
 *           a larger index never wins a cell).
 *
 * The masks are byte for byte those of eg3d_host_filter_close_2d on the concatenation of the clouds in index order
 * (eg3d_host_dedup_claim / _keep / _merge of eg3d_host_dedup_phases.h are the sequential statement of the phases). The
 * combined calls of eg3d.h keep their results and are made of the same steps; they and the phased calls share the context's
 * map, so the two forms can be mixed within a run.
 *
 * Failure rule, as for eg3d_dedup_device: a call that is refused up front (EG3D_ERR_ARG from the argument checks below)
 * leaves the claims as they were; a call that fails after its arguments were accepted (a HIP or allocation failure)
 * discards ALL claims of the context — the next call that needs a map starts from an empty one, and eg3d_dedup_keep refuses
 * until something has been claimed or merged again. Every call returns after its work has completed on the context's
 * stream: the cloud may be overwritten, and another context or a peer may read the map, as soon as it returns.
 */
#ifndef EG3D_DEDUP_PHASES_H_
#define EG3D_DEDUP_PHASES_H_
#include "eg3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The claim pass alone: first[cell] = min(first[cell], index_base + i) for every observation of every point i of `cloud`
 * that has a cell. reset != 0 empties the map first. index_base + n_points must stay below 2^32 - 1 (checked before any
 * launch). Unlike the combined call, which leaves it to its keep kernel, this one checks on the device, before it claims,
 * that every list is an ascending range inside [0, n_obs]: a cloud that fails returns EG3D_ERR_ARG and leaves the map —
 * a reset asked for by the refused call included — as it was. */
int eg3d_dedup_claim(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, uint64_t index_base, int reset);

/* The keep pass alone, against the map as it stands: keep_dev[i] (n_points bytes of HBM) = 1 when an observation of point i
 * lies in a cell that holds index_base + i. n_kept_host may be NULL. A context with no valid map is refused
 * (EG3D_ERR_ARG): the caller has claimed nothing. Offsets that do not ascend are refused as by eg3d_dedup_device; the pass
 * writes nothing of the map, so the claims stand. */
int eg3d_dedup_keep(eg3d_ctx* ctx, const eg3d_device_edgepoints* cloud, uint64_t index_base, uint8_t* keep_dev,
                    uint64_t* n_kept_host);

/* The context's claim map in HBM: n_cells = n_views * ceil(width / 3) * ceil(height / 3) entries [view][cell row][cell
 * column], 0xFFFFFFFF = untouched. It is created and filled with 0xFFFFFFFF if it does not exist or is not valid. The
 * pointer is borrowed: valid until the context is destroyed or a dedup call on it fails. The caller may LOWER entries in
 * place, as a minimum all-reduce does (eg3d_allreduce_claims); the map then holds the caller's claims too, and every later
 * keep pass of this context answers against them. Raising an entry, or writing while a dedup call of the context runs, is
 * not supported. n_cells may be NULL. */
int eg3d_dedup_claims(eg3d_ctx* ctx, uint32_t** first_dev, uint64_t* n_cells);

/* first[c] = min(first[c], other_dev[c]) for every cell, on the context's stream. other_dev: any device-readable array of
 * n_cells uint32 — another context's map (after that context's calls have returned), or a buffer a peer copy filled; it
 * needs 4-byte alignment only, is never written, and must not overlap the context's map unless it IS the map (a no-op).
 * n_cells other than the context's is EG3D_ERR_ARG. Merging into a context without a valid map makes one: fill, then min.
 * n_lowered_host (may be NULL): the entries that got smaller. */
int eg3d_dedup_merge_claims(eg3d_ctx* ctx, const uint32_t* other_dev, uint64_t n_cells, uint64_t* n_lowered_host);

/* Device time, in milliseconds between HIP events on the context's stream, of the last eg3d_dedup_claim (offsets check,
 * its read-back and the claim kernel), eg3d_dedup_keep or eg3d_dedup_merge_claims (the kernel) that completed on `ctx`:
 * what tools/bench_dedup_phases.py reports. */
int eg3d_dedup_phase_ms(eg3d_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif
