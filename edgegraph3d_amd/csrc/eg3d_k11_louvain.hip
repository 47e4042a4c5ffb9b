// eg3d_k11_louvain.hip — K11: pipeline 1's community detection on the device (eg3d_detect_communities). The reference hands
// the compatibility graph to Grappolo; this is a Louvain of the project's own with Grappolo's rules (synchronous sweeps,
// ties to the smaller label, singleton swap protection, phases) and exact arithmetic. tests/louvain_ref.py is the definition.
//
// No floating-point sum exists here. A weight w in (0, 1] is the integer q = llrint((double)w * 2^32) (the product is exact);
// degrees, community totals and M, the sum of all directed q, are 64-bit integer sums (the API refuses 2^31 entries or more, so
// M < 2^63); a gain and the modularity numerator are signed 128-bit integers. Atomics and reductions in any lane order give
// the same bits, and the tie rule (the smaller label) is part of the key every reduction compares.
//   k11_validate      1 lane / offset and entry   the input rules; erow, q
//   k11_degrees       1 lane / vertex             k, M, C = identity
//   k11_totals        1 lane / vertex             a, size
//   k11_targets       1 WAVE / vertex             e[y] in a per-wave LDS hash table (64-bit atomicAdd), then the best (G, y)
//   k11_ovf_*         1 WAVE / overflow row       rows whose communities do not fit the table: keys, sort, reduce_by_key, best
//   k11_inside        1 lane / entry              the numerator's internal weight, one atomic per block
//   k11_squares       1 lane / community          the 32-bit limbs of a_c^2
//   k11_min_member .. k11_split_keys              renumbering by first appearance and the coarse graph's keys
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "eg3d_k11_louvain.h"

namespace eg3d {

typedef unsigned long long u64;
typedef __int128 i128;

__device__ __forceinline__ u64 k11_wave_sum(u64 v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Everything a wavefront did to its LDS table is done before anything after this reads it (one wavefront per table: no
// s_barrier, the waves of a block run different numbers of vertices).
__device__ __forceinline__ void k11_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(K11_BLOCK) k11_validate(uint32_t n, uint32_t nnz, const uint32_t* off, const uint32_t* nbr,
                                                          const float* w, uint32_t* erow, u64* q, u64* flags) {
  const u64 t = (u64)blockIdx.x * K11_BLOCK + threadIdx.x;
  uint32_t bad = 0;
  if (t <= n) {  // offsets: 0 first, monotone, nnz last
    const uint32_t o = off[t];
    if (t == 0 && o != 0) bad |= K11_BAD_OFFSETS;
    if (t == n ? o != nnz : o > off[t + 1]) bad |= K11_BAD_OFFSETS;
  } else if (t - (n + 1) < nnz) {
    const uint32_t e = (uint32_t)(t - (n + 1));
    // the row: the last r < n with off[r] <= e (any offsets leave it inside 0 .. n - 1)
    uint32_t lo = 0, hi = n;  // first r in [0, n) with off[r] > e
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (off[mid] <= e) lo = mid + 1; else hi = mid;
    }
    const uint32_t r = lo ? lo - 1 : 0;
    erow[e] = r;
    const uint32_t j = nbr[e];
    const float we = w[e];
    const bool w_ok = we > 0.0f && we <= 1.0f;  // (false for a NaN)
    q[e] = w_ok ? (u64)llrint((double)we * 4294967296.0) : 0ull;
    if (!w_ok) bad |= K11_BAD_WEIGHT;
    if (j >= n) {
      bad |= K11_BAD_NEIGHBOUR;
    } else {
      if (j == r) bad |= K11_SELF_LOOP;
      if (e > off[r] && nbr[e - 1] >= j) bad |= K11_BAD_ORDER;
      // the reverse entry, by binary search in row j (offsets clamped: a bad offset is reported above, never followed)
      uint32_t a = off[j] < nnz ? off[j] : nnz, b = off[j + 1] < nnz ? off[j + 1] : nnz;
      while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (nbr[mid] < r) a = mid + 1; else b = mid;
      }
      const uint32_t end = off[j + 1] < nnz ? off[j + 1] : nnz;
      if (a >= end || nbr[a] != r) bad |= K11_ASYMMETRIC;
      else if (__float_as_uint(w[a]) != __float_as_uint(we)) bad |= K11_WEIGHT_MISMATCH;
    }
  }
  if (bad) atomicOr(flags, (u64)bad);
}

__global__ void __launch_bounds__(K11_BLOCK) k11_members(uint32_t n, const uint32_t* off, uint32_t* member) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (i < n) member[i] = off[i + 1] > off[i] ? i : K11_NONE;
}

__global__ void __launch_bounds__(K11_BLOCK) k11_degrees(K11Csr g, u64* k, uint32_t* C, u64* total) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  u64 s = 0;
  if (i < g.n) {
    for (uint32_t p = g.off[i]; p < g.off[i + 1]; p++) s += g.q[p];
    k[i] = s;
    C[i] = i;
  }
  s = k11_wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

__global__ void __launch_bounds__(K11_BLOCK) k11_totals(uint32_t n, const uint32_t* C, const u64* k, u64* a, uint32_t* size) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (i >= n) return;
  atomicAdd(a + C[i], k[i]);
  atomicAdd(size + C[i], 1u);
}

// ---- the choice of a target --------------------------------------------------------------------------------------------------
// A candidate is (G, y); the better one has the larger G, or the same G and the smaller y. (0, K11_NONE) stands for "none";
// a candidate with G == 0 beats it here and is dropped by the final G > 0 test.
struct K11Best {
  i128 G;
  uint32_t y;
};
__device__ __forceinline__ bool k11_better(i128 G1, uint32_t y1, i128 G2, uint32_t y2) { return G1 > G2 || (G1 == G2 && y1 < y2); }
// G(y) = (e[y] - e[x]) * M - k[i] * (a[y] - (a[x] - k[i])): every factor fits 64 signed bits, the products 127
__device__ __forceinline__ void k11_offer(K11Best& b, const K11Part& p, u64 ki, u64 eix, u64 ax, uint32_t y, u64 ey) {
  const i128 G = (i128)(long long)(ey - eix) * (i128)p.M - (i128)ki * (i128)(long long)(p.a[y] - ax);
  if (k11_better(G, y, b.G, b.y)) {
    b.G = G;
    b.y = y;
  }
}
// The wave's best candidate, then the rules that need no table: G > 0, and swap protection (two singletons do not trade
// places: the one with the smaller label stays). Lane 0 writes T[i] and counts a changed vertex.
__device__ __forceinline__ void k11_decide(K11Best b, const K11Part& p, uint32_t i, uint32_t x, uint32_t* T, u64* ctr) {
  for (int o = 32; o; o >>= 1) {
    const u64 lo = __shfl_xor((u64)b.G, o, 64), hi = __shfl_xor((u64)(b.G >> 64), o, 64);
    const uint32_t y = __shfl_xor(b.y, o, 64);
    const i128 G = (i128)(((unsigned __int128)hi << 64) | lo);
    if (k11_better(G, y, b.G, b.y)) {
      b.G = G;
      b.y = y;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    uint32_t best = (b.y != K11_NONE && b.G > 0) ? b.y : x;
    if (best != x && p.size[x] == 1 && p.size[best] == 1 && best > x) best = x;
    T[i] = best;
    if (best != x) atomicAdd(ctr + K11_C_CHANGED, 1ull);
  }
}

__device__ __forceinline__ uint32_t k11_hash(uint32_t y, uint32_t log2_slots) { return (y * 0x9E3779B1u) >> (32u - log2_slots); }

extern __shared__ __attribute__((aligned(16))) char k11_smem[];

// One wavefront per vertex. The row is read coalesced; every entry adds its q to the slot of its neighbour's community (open
// addressing, linear probing; a slot is claimed with a compare-and-swap, the sum is a 64-bit LDS atomicAdd). A lane that has
// probed every slot without finding its key or a free one has met a full table: the row holds more distinct communities than
// slots and is an overflow row (exactly then: with no more keys than slots every probe sequence ends). The scan empties the
// table as it reads it.
__global__ void __launch_bounds__(K11_BLOCK) k11_targets(K11Csr g, K11Part p, uint32_t log2_slots, uint32_t* T, uint32_t* ovf,
                                                         u64* ctr) {
  const uint32_t slots = 1u << log2_slots, mask = slots - 1;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64* const val = reinterpret_cast<u64*>(k11_smem) + (size_t)wave * slots;
  uint32_t* const key = reinterpret_cast<uint32_t*>(k11_smem + (size_t)K11_WAVES * slots * sizeof(u64)) + (size_t)wave * slots;
  for (uint32_t s = lane; s < slots; s += 64) {
    key[s] = K11_NONE;
    val[s] = 0;
  }
  k11_wave_sync();
  for (uint32_t i = blockIdx.x * K11_WAVES + wave; i < g.n; i += gridDim.x * K11_WAVES) {
    const uint32_t x = p.C[i], b = g.off[i], e = g.off[i + 1];
    bool full = false;
    for (uint32_t q0 = b + lane; q0 < e; q0 += 64) {
      const uint32_t j = g.nbr[q0];
      if (j == i) continue;  // (a coarse vertex's self-loop: in k[i], not in e)
      const uint32_t y = p.C[j];
      uint32_t h = k11_hash(y, log2_slots), t = 0;
      for (; t < slots; t++) {
        const uint32_t old = atomicCAS(key + h, K11_NONE, y);
        if (old == K11_NONE || old == y) {
          atomicAdd(val + h, g.q[q0]);
          break;
        }
        h = (h + 1) & mask;
      }
      if (t == slots) full = true;
    }
    k11_wave_sync();
    const bool overflow = __ballot(full) != 0;
    // e[x]: the probe sequence of x (the same in every lane) ends at x or at a free slot unless the table is full
    u64 eix = 0;
    if (!overflow) {
      uint32_t h = k11_hash(x, log2_slots);
      for (uint32_t t = 0; t < slots; t++) {
        const uint32_t kk = key[h];
        if (kk == x) eix = val[h];
        if (kk == x || kk == K11_NONE) break;
        h = (h + 1) & mask;
      }
    }
    const u64 ki = p.k[i], ax = p.a[x] - ki;
    K11Best best{0, K11_NONE};
    for (uint32_t s = lane; s < slots; s += 64) {
      const uint32_t y = key[s];
      if (y == K11_NONE) continue;
      const u64 ey = val[s];
      key[s] = K11_NONE;
      val[s] = 0;
      if (!overflow && y != x) k11_offer(best, p, ki, eix, ax, y, ey);
    }
    k11_wave_sync();
    if (!overflow) {
      k11_decide(best, p, i, x, T, ctr);
    } else if (lane == 0) {
      ovf[atomicAdd(ctr + K11_C_OVF_ROWS, 1ull)] = i;
      atomicAdd(ctr + K11_C_OVF_ENTRIES, (u64)(e - b));
    }
  }
}

__global__ void __launch_bounds__(K11_BLOCK) k11_ovf_counts(K11Csr g, const uint32_t* ovf, uint32_t n_ovf, uint32_t* cnt) {
  const uint32_t r = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (r > n_ovf) return;
  cnt[r] = r < n_ovf ? g.off[ovf[r] + 1] - g.off[ovf[r]] : 0u;
}

__global__ void __launch_bounds__(K11_BLOCK) k11_ovf_expand(K11Csr g, const uint32_t* C, const uint32_t* ovf, uint32_t n_ovf,
                                                            const uint32_t* ooff, u64* key, u64* val) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * K11_WAVES + (threadIdx.x >> 6); r < n_ovf; r += gridDim.x * K11_WAVES) {
    const uint32_t i = ovf[r], b = g.off[i], len = g.off[i + 1] - b, o = ooff[r];
    for (uint32_t t = lane; t < len; t += 64) {
      const uint32_t j = g.nbr[b + t];
      key[o + t] = (u64)r << 32 | C[j];
      val[o + t] = j == i ? 0ull : g.q[b + t];
    }
  }
}

__device__ __forceinline__ uint32_t k11_lower_bound(const u64* keys, uint32_t n, u64 v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(K11_BLOCK) k11_ovf_targets(K11Part p, const uint32_t* ovf, uint32_t n_ovf, const u64* key, const u64* e,
                                                             const u64* n_pairs, uint32_t* T, u64* ctr) {
  const uint32_t lane = threadIdx.x & 63, n = (uint32_t)*n_pairs;
  for (uint32_t r = blockIdx.x * K11_WAVES + (threadIdx.x >> 6); r < n_ovf; r += gridDim.x * K11_WAVES) {
    const uint32_t i = ovf[r], x = p.C[i];
    const uint32_t b = k11_lower_bound(key, n, (u64)r << 32), end = k11_lower_bound(key, n, (u64)(r + 1) << 32);
    const uint32_t px = k11_lower_bound(key, n, (u64)r << 32 | x);
    const u64 eix = (px < end && key[px] == ((u64)r << 32 | x)) ? e[px] : 0ull;
    const u64 ki = p.k[i], ax = p.a[x] - ki;
    K11Best best{0, K11_NONE};
    for (uint32_t t = b + lane; t < end; t += 64) {
      const uint32_t y = (uint32_t)key[t];
      if (y != x) k11_offer(best, p, ki, eix, ax, y, e[t]);
    }
    k11_decide(best, p, i, x, T, ctr);
  }
}

// ---- the numerator -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K11_BLOCK) k11_inside(K11Csr g, const uint32_t* T, u64* ctr) {
  __shared__ u64 part[K11_WAVES];
  const uint32_t e = blockIdx.x * K11_BLOCK + threadIdx.x;
  u64 s = 0;
  if (e < g.nnz && T[g.erow[e]] == T[g.nbr[e]]) s = g.q[e];
  s = k11_wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < K11_WAVES; k++) t += part[k];
    if (t) atomicAdd(ctr + K11_C_INSIDE, t);
  }
}

// a_c^2 is a 128-bit number: its four 32-bit limbs are added into four 64-bit sums (fewer than 2^31 communities: no sum
// leaves 64 bits); the host adds limb l << 32 l with carries.
__global__ void __launch_bounds__(K11_BLOCK) k11_squares(uint32_t n, const u64* a, u64* ctr) {
  const uint32_t c = blockIdx.x * K11_BLOCK + threadIdx.x;
  const u64 v = c < n ? a[c] : 0ull;
  const unsigned __int128 sq = (unsigned __int128)v * v;
  for (int l = 0; l < 4; l++) {
    const u64 s = k11_wave_sum((u64)(uint32_t)(sq >> (32 * l)));
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(ctr + K11_C_LIMB0 + l, s);
  }
}

// ---- renumbering and coarsening ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(K11_BLOCK) k11_min_member(uint32_t n, const uint32_t* C, uint32_t* minm, u64* ctr) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (i >= n) return;
  atomicMin(minm + C[i], i);
  if (C[i] != i) atomicAdd(ctr + K11_C_NOT_IDENTITY, 1ull);
}
__global__ void __launch_bounds__(K11_BLOCK) k11_first_flags(uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* off,
                                                             uint32_t* flag) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (i > n) return;
  flag[i] = (i < n && minm[C[i]] == i && off[i + 1] > off[i]) ? 1u : 0u;
}
__global__ void __launch_bounds__(K11_BLOCK) k11_relabel(uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* rank,
                                                         uint32_t* Cn) {
  const uint32_t i = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (i < n) Cn[i] = rank[minm[C[i]]];
}
__global__ void __launch_bounds__(K11_BLOCK) k11_compose(uint32_t n_nodes, const uint32_t* Cn, uint32_t* member) {
  const uint32_t v = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (v < n_nodes && member[v] != K11_NONE) member[v] = Cn[member[v]];
}
__global__ void __launch_bounds__(K11_BLOCK) k11_coarse_keys(K11Csr g, const uint32_t* Cn, u64* key) {
  const uint32_t e = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (e < g.nnz) key[e] = (u64)Cn[g.erow[e]] << 32 | Cn[g.nbr[e]];
}
__global__ void __launch_bounds__(K11_BLOCK) k11_split_keys(const u64* key, uint32_t n, uint32_t* erow, uint32_t* nbr) {
  const uint32_t e = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (e < n) {
    erow[e] = (uint32_t)(key[e] >> 32);
    nbr[e] = (uint32_t)key[e];
  }
}
__global__ void __launch_bounds__(K11_BLOCK) k11_ids(uint32_t n_nodes, const uint32_t* member, int64_t* ids) {
  const uint32_t v = blockIdx.x * K11_BLOCK + threadIdx.x;
  if (v < n_nodes) ids[v] = member[v] == K11_NONE ? -1 : (int64_t)member[v];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static inline uint32_t k11_blocks(u64 n) { return (uint32_t)((n + K11_BLOCK - 1) / K11_BLOCK); }
static inline uint32_t k11_wave_blocks(uint32_t n) { return std::min<uint32_t>((n + K11_WAVES - 1) / K11_WAVES, 1u << 16); }

void launch_k11_validate(hipStream_t st, uint32_t n, uint32_t nnz, const uint32_t* off, const uint32_t* nbr, const float* w,
                         uint32_t* erow, unsigned long long* q, unsigned long long* flags) {
  hipLaunchKernelGGL(k11_validate, dim3(k11_blocks((u64)n + 1 + nnz)), dim3(K11_BLOCK), 0, st, n, nnz, off, nbr, w, erow, q, flags);
}
void launch_k11_members(hipStream_t st, uint32_t n, const uint32_t* off, uint32_t* member) {
  if (n) hipLaunchKernelGGL(k11_members, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, n, off, member);
}
void launch_k11_degrees(hipStream_t st, K11Csr g, unsigned long long* k, uint32_t* C, unsigned long long* total) {
  if (g.n) hipLaunchKernelGGL(k11_degrees, dim3(k11_blocks(g.n)), dim3(K11_BLOCK), 0, st, g, k, C, total);
}
void launch_k11_totals(hipStream_t st, uint32_t n, const uint32_t* C, const unsigned long long* k, unsigned long long* a,
                       uint32_t* size) {
  if (n) hipLaunchKernelGGL(k11_totals, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, n, C, k, a, size);
}
void launch_k11_targets(hipStream_t st, K11Csr g, K11Part p, uint32_t log2_slots, uint32_t* T, uint32_t* ovf,
                        unsigned long long* ctr) {
  const size_t lds = (size_t)K11_WAVES * ((size_t)1 << log2_slots) * (sizeof(u64) + sizeof(uint32_t));
  if (g.n) hipLaunchKernelGGL(k11_targets, dim3(k11_wave_blocks(g.n)), dim3(K11_BLOCK), lds, st, g, p, log2_slots, T, ovf, ctr);
}
void launch_k11_ovf_counts(hipStream_t st, K11Csr g, const uint32_t* ovf, uint32_t n_ovf, uint32_t* cnt) {
  hipLaunchKernelGGL(k11_ovf_counts, dim3(k11_blocks((u64)n_ovf + 1)), dim3(K11_BLOCK), 0, st, g, ovf, n_ovf, cnt);
}
void launch_k11_ovf_expand(hipStream_t st, K11Csr g, const uint32_t* C, const uint32_t* ovf, uint32_t n_ovf, const uint32_t* ooff,
                           unsigned long long* key, unsigned long long* val) {
  if (n_ovf) hipLaunchKernelGGL(k11_ovf_expand, dim3(k11_wave_blocks(n_ovf)), dim3(K11_BLOCK), 0, st, g, C, ovf, n_ovf, ooff, key, val);
}
void launch_k11_ovf_targets(hipStream_t st, K11Part p, const uint32_t* ovf, uint32_t n_ovf, const unsigned long long* key,
                            const unsigned long long* e, const unsigned long long* n_pairs, uint32_t* T, unsigned long long* ctr) {
  if (n_ovf) hipLaunchKernelGGL(k11_ovf_targets, dim3(k11_wave_blocks(n_ovf)), dim3(K11_BLOCK), 0, st, p, ovf, n_ovf, key, e, n_pairs, T, ctr);
}
void launch_k11_inside(hipStream_t st, K11Csr g, const uint32_t* T, unsigned long long* ctr) {
  if (g.nnz) hipLaunchKernelGGL(k11_inside, dim3(k11_blocks(g.nnz)), dim3(K11_BLOCK), 0, st, g, T, ctr);
}
void launch_k11_squares(hipStream_t st, uint32_t n, const unsigned long long* a, unsigned long long* ctr) {
  if (n) hipLaunchKernelGGL(k11_squares, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, n, a, ctr);
}
void launch_k11_min_member(hipStream_t st, uint32_t n, const uint32_t* C, uint32_t* minm, unsigned long long* ctr) {
  if (n) hipLaunchKernelGGL(k11_min_member, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, n, C, minm, ctr);
}
void launch_k11_first_flags(hipStream_t st, uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* off, uint32_t* flag) {
  hipLaunchKernelGGL(k11_first_flags, dim3(k11_blocks((u64)n + 1)), dim3(K11_BLOCK), 0, st, n, C, minm, off, flag);
}
void launch_k11_relabel(hipStream_t st, uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* rank, uint32_t* Cn) {
  if (n) hipLaunchKernelGGL(k11_relabel, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, n, C, minm, rank, Cn);
}
void launch_k11_compose(hipStream_t st, uint32_t n_nodes, const uint32_t* Cn, uint32_t* member) {
  if (n_nodes) hipLaunchKernelGGL(k11_compose, dim3(k11_blocks(n_nodes)), dim3(K11_BLOCK), 0, st, n_nodes, Cn, member);
}
void launch_k11_coarse_keys(hipStream_t st, K11Csr g, const uint32_t* Cn, unsigned long long* key) {
  if (g.nnz) hipLaunchKernelGGL(k11_coarse_keys, dim3(k11_blocks(g.nnz)), dim3(K11_BLOCK), 0, st, g, Cn, key);
}
void launch_k11_split_keys(hipStream_t st, const unsigned long long* key, uint32_t n, uint32_t* erow, uint32_t* nbr) {
  if (n) hipLaunchKernelGGL(k11_split_keys, dim3(k11_blocks(n)), dim3(K11_BLOCK), 0, st, key, n, erow, nbr);
}
void launch_k11_ids(hipStream_t st, uint32_t n_nodes, const uint32_t* member, int64_t* ids) {
  if (n_nodes) hipLaunchKernelGGL(k11_ids, dim3(k11_blocks(n_nodes)), dim3(K11_BLOCK), 0, st, n_nodes, member, ids);
}

hipError_t k11_sort_pairs(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                          const unsigned long long* val_in, unsigned long long* val_out, size_t n) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, val_out, n, 0, 64, st);
}
hipError_t k11_reduce_by_key(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in,
                             const unsigned long long* val_in, unsigned long long* key_out, unsigned long long* sum_out,
                             unsigned long long* n_out, size_t n) {
  return rocprim::reduce_by_key(tmp, tmp_bytes, key_in, val_in, n, key_out, sum_out, n_out, rocprim::plus<unsigned long long>(),
                                rocprim::equal_to<unsigned long long>(), st);
}

}  // namespace eg3d
