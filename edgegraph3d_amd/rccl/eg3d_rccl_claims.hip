// eg3d_rccl_claims.hip — the exchanges of the phased dedup over ranks (include/eg3d_rccl_claims.h): the minimum
// all-reduce of the claim maps and the exclusive scan of the ranks' point counts. No kernel of its own: RCCL's reduction
// does the work on the map where it lies.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/eg3d_rccl_claims.h"

namespace {
// The few control words of a call, on the device for the collective (freed on every way out).
struct Words {
  uint64_t* p = nullptr;
  explicit Words(size_t n) {
    if (hipMalloc((void**)&p, sizeof(uint64_t) * n) != hipSuccess) p = nullptr;
  }
  ~Words() {
    if (p) (void)hipFree(p);
  }
};
}  // namespace

// (as in eg3d_rccl.hip) a rank-local runtime failure between two collectives cannot be reported to the peers any more:
// abort the communicator so that their pending collectives fail instead of blocking for ever.
#define FATAL_UNLESS(ok)                   \
  do {                                     \
    if (!(ok)) {                           \
      (void)ncclCommAbort(comm);           \
      return EG3D_GATHER_ERR_FATAL;        \
    }                                      \
  } while (0)

// All ranks' words [R] on the host: one ncclAllGather of 8 bytes per rank.
static int gather_words(ncclComm_t comm, hipStream_t st, int n_ranks, uint64_t mine, std::vector<uint64_t>* all) {
  const size_t R = (size_t)n_ranks;
  int device = -1;  // the communicator's device: the control words and the stream belong to it
  FATAL_UNLESS(ncclCommCuDevice(comm, &device) == ncclSuccess && hipSetDevice(device) == hipSuccess);
  Words w(R + 1);
  FATAL_UNLESS(w.p != nullptr);
  all->assign(R, 0);
  FATAL_UNLESS(hipMemcpyAsync(w.p + R, &mine, sizeof(mine), hipMemcpyHostToDevice, st) == hipSuccess);
  FATAL_UNLESS(ncclAllGather(w.p + R, w.p, 1, ncclUint64, comm, st) == ncclSuccess);
  FATAL_UNLESS(hipMemcpyAsync(all->data(), w.p, sizeof(uint64_t) * R, hipMemcpyDeviceToHost, st) == hipSuccess);
  FATAL_UNLESS(hipStreamSynchronize(st) == hipSuccess);
  return 0;
}

extern "C" int eg3d_allreduce_claims(void* nccl_comm, int n_ranks, int rank, void* hip_stream, uint32_t* first_dev,
                                     uint64_t n_cells, int local_ok, uint64_t chunk_bytes) {
  if (!nccl_comm || n_ranks < 1 || rank < 0 || rank >= n_ranks) return EG3D_GATHER_ERR_ARG;
  ncclComm_t comm = (ncclComm_t)nccl_comm;
  hipStream_t st = (hipStream_t)hip_stream;
  // the agreement word: n_cells, or all ones for "no usable map" (no map has 2^64 - 1 cells)
  const bool usable = local_ok && (first_dev || !n_cells);
  std::vector<uint64_t> all;
  const int rc = gather_words(comm, st, n_ranks, usable ? n_cells : ~0ull, &all);
  if (rc) return rc;
  for (uint64_t a : all)
    if (a == ~0ull) return EG3D_GATHER_ERR_INCOMPLETE;  // same verdict on every rank
  for (uint64_t a : all)
    if (a != all[0]) return EG3D_GATHER_ERR_ARG;  // the ranks do not describe the same rig
  const uint64_t piece = std::max<uint64_t>(1, (chunk_bytes ? chunk_bytes : (1ull << 30)) / sizeof(uint32_t));
  for (uint64_t o = 0; o < n_cells; o += piece)
    FATAL_UNLESS(ncclAllReduce(first_dev + o, first_dev + o, (size_t)std::min<uint64_t>(piece, n_cells - o), ncclUint32, ncclMin,
                               comm, st) == ncclSuccess);
  FATAL_UNLESS(hipStreamSynchronize(st) == hipSuccess);
  return 0;
}

extern "C" int eg3d_exscan_points(void* nccl_comm, int n_ranks, int rank, void* hip_stream, uint64_t local_points,
                                  uint64_t* base, uint64_t* total) {
  if (!nccl_comm || n_ranks < 1 || rank < 0 || rank >= n_ranks) return EG3D_GATHER_ERR_ARG;
  ncclComm_t comm = (ncclComm_t)nccl_comm;
  std::vector<uint64_t> all;
  const int rc = gather_words(comm, (hipStream_t)hip_stream, n_ranks, local_points, &all);
  if (rc) return rc;
  uint64_t below = 0, sum = 0;
  for (int r = 0; r < n_ranks; r++) {
    if (all[r] >= 0xFFFFFFFFull - sum) return EG3D_GATHER_ERR_ARG;  // same verdict on every rank
    if (r < rank) below += all[r];
    sum += all[r];
  }
  if (base) *base = below;
  if (total) *total = sum;
  return 0;
}
