/*
 * eg3d_rccl_claims.h — the dedup of a cloud that is sharded over ranks (libeg3d_rccl.so): the two exchanges the phased
 * dedup (include/eg3d_dedup_phases.h) needs before a rank can run its keep pass against every other rank's claims, for a
 * C/C++ host without torch. The sequence on every rank, clouds still in the HBM they were built in:
 *
 *   eg3d_exscan_points        -> base = points of the lower ranks (rank order = seed order = index order)
 *   eg3d_dedup_claim          (ctx, cloud, run_base + base, reset)
 *   eg3d_dedup_claims         -> the rank's map
 *   eg3d_allreduce_claims     min over the ranks, in place
 *   eg3d_dedup_keep           (ctx, cloud, run_base + base, keep_dev, ...)
 *   eg3d_gn_filter_device / eg3d_compact_device / eg3d_allgather_edgepoints of the survivors only.
 *
 * Every rank ends with what eg3d_dedup_resident gives on the concatenation of the shards, and the raw cloud never travels.
 * Both calls are collective (every rank must call them), return the codes of eg3d_rccl.h, the same on every rank for
 * everything decided before the payload moves, and return after the exchange has completed on `hip_stream`.
 */
#ifndef EG3D_RCCL_CLAIMS_H_
#define EG3D_RCCL_CLAIMS_H_
#include "eg3d_rccl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* first_dev[c] = min over the ranks of their first_dev[c], c < n_cells, in place (ncclAllReduce, ncclUint32, ncclMin) in
 * pieces of at most chunk_bytes (0 = 1 GiB; rounded down to whole entries, at least one). First an 8-byte agreement round,
 * like the gather's status words: local_ok = 0 ("this rank has no usable map": its claim failed) on ANY rank makes every
 * rank return EG3D_GATHER_ERR_INCOMPLETE, ranks that pass different n_cells make every rank return EG3D_GATHER_ERR_ARG,
 * both before any payload moves; first_dev may be NULL with local_ok = 0. A HIP / RCCL failure between the collectives
 * aborts the communicator (EG3D_GATHER_ERR_FATAL), as in eg3d_allgather_edgepoints. After an error the map of a rank is
 * as it was (agreement) or undefined (fatal). */
int eg3d_allreduce_claims(void* nccl_comm, int n_ranks, int rank, void* hip_stream, uint32_t* first_dev, uint64_t n_cells,
                          int local_ok, uint64_t chunk_bytes);

/* *base = the sum of local_points of the ranks below `rank`, *total = the sum over all ranks (either may be NULL): the
 * index base of a rank's shard within the step's cloud. EG3D_GATHER_ERR_ARG when the total would not stay below 2^32 - 1
 * (the claim map holds 32-bit indices), on every rank. */
int eg3d_exscan_points(void* nccl_comm, int n_ranks, int rank, void* hip_stream, uint64_t local_points, uint64_t* base,
                       uint64_t* total);

#ifdef __cplusplus
}
#endif
#endif
