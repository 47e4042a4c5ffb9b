// eg3d_k7b_claims.hip — K7b (gfx950): what the phased dedup adds to K7 (eg3d_k7_dedup.hip, whose two kernels are unchanged):
// the element-wise minimum that joins two claim maps (k7_claims_min) and the offsets check a claim pass on its own needs
// before it may touch the map (k7_offsets_check).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ K7b --------
// first[c] = min(first[c], other[c]) over n cells; *n_lowered += the cells that got smaller. Pure bandwidth: 21 MB (C3')
// to 171 MB (C4) per map, read twice, written at most once. `first` is a context's own allocation, 16-byte aligned: words
// of four cells are laid over it, a lane takes one word per grid-stride step — one 16-byte load of each operand, one
// 16-byte store. `other` needs 4-byte alignment only: its words are loaded through a 4-byte-aligned vector type (global
// memory takes a dword-aligned 16-byte load; a wave's loads then straddle one more 64-byte line than aligned ones would).
// The up to 3 cells behind the last word are single lanes of block 0. SKIP: a word is stored only when one of its cells
// was lowered — min() never raises an entry, so a word without a lowered cell already holds the result (the choice
// between the two forms is measured: DESIGN_LOG.md, "Dedup in phases"). Lowered cells: counted per lane, summed per wave
// by shuffles, per block through LDS, one atomic per block.
typedef uint32_t k7b_u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) K7bWordA4 {
  k7b_u32x4 v;
};

template <bool SKIP>
__global__ void __launch_bounds__(K7B_BLOCK) k7_claims_min(uint32_t* __restrict__ first, const uint32_t* __restrict__ other,
                                                           uint64_t n, unsigned long long* n_lowered) {
  __shared__ uint32_t s_n[K7B_BLOCK / 64];
  const uint32_t t = threadIdx.x;
  const uint64_t n_words = n >> 2;
  uint32_t cnt = 0;
  if (blockIdx.x == 0 && t < (uint32_t)(n & 3u)) {  // the tail
    const uint64_t e = 4 * n_words + t;
    const uint32_t a = first[e], b = other[e];
    if (b < a) {
      first[e] = b;
      cnt = 1;
    }
  }
  k7b_u32x4* fw = reinterpret_cast<k7b_u32x4*>(first);
  const K7bWordA4* ow = reinterpret_cast<const K7bWordA4*>(other);
  for (uint64_t w = (uint64_t)blockIdx.x * K7B_BLOCK + t; w < n_words; w += (uint64_t)gridDim.x * K7B_BLOCK) {
    const k7b_u32x4 a = fw[w], b = ow[w].v;
    k7b_u32x4 r;
    uint32_t low = 0;
    r.x = b.x < a.x ? (low++, b.x) : a.x;
    r.y = b.y < a.y ? (low++, b.y) : a.y;
    r.z = b.z < a.z ? (low++, b.z) : a.z;
    r.w = b.w < a.w ? (low++, b.w) : a.w;
    if (!SKIP || low) fw[w] = r;
    cnt += low;
  }
  for (int d = 32; d; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((t & 63u) == 0) s_n[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
    for (uint32_t q = 0; q < K7B_BLOCK / 64; q++) sum += s_n[q];
    if (sum) atomicAdd(n_lowered, (unsigned long long)sum);
  }
}

// One lane per point: the test k7_dedup_keep makes of a list (an ascending range inside [0, n_obs]), on its own, so that a
// claim pass can refuse a cloud before it has written a claim. K5_FLAG_BAD_OFFSETS into *flags.
__global__ void __launch_bounds__(K7B_BLOCK) k7_offsets_check(CloudView in, uint32_t* flags) {
  const uint64_t i = (uint64_t)blockIdx.x * K7B_BLOCK + threadIdx.x;
  if (i >= in.n_points) return;
  const uint64_t a = in.obs_off[i], b = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
  if (!(a <= b && b <= in.n_obs)) atomicOr(flags, K5_FLAG_BAD_OFFSETS);
}

void launch_claims_min(hipStream_t st, uint32_t* first, const uint32_t* other, uint64_t n, unsigned long long* n_lowered,
                       bool write_all) {
  if (!n) return;
  // a memory-bound sweep: at most 8 blocks per CU of the 256, the rest by grid stride
  const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(((n >> 2) + K7B_BLOCK - 1) / K7B_BLOCK, K7B_MAX_BLOCKS));
  if (write_all)
    hipLaunchKernelGGL(k7_claims_min<false>, dim3(blocks), dim3(K7B_BLOCK), 0, st, first, other, n, n_lowered);
  else
    hipLaunchKernelGGL(k7_claims_min<true>, dim3(blocks), dim3(K7B_BLOCK), 0, st, first, other, n, n_lowered);
}
void launch_offsets_check(hipStream_t st, CloudView in, uint32_t* flags) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k7_offsets_check, blocks_for(in.n_points, K7B_BLOCK), dim3(K7B_BLOCK), 0, st, in, flags);
}

}  // namespace eg3d
