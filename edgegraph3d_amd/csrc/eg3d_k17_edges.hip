// eg3d_k17_edges.hip — K17: the 3-D edge model of a graph3d, traced, simplified and measured on the device
// (include/eg3d/edges.h). The rules and every piece of arithmetic are eg3d_edges_core.h; what is here is how the work is
// spread over lanes.
//
//   checks    one lane per polyline (node ids, loops counted), per offset, per node (its row: ids, ends, no polyline twice —
//             a flag per (polyline, end) is claimed atomically — and the node's degree). Each runs only after the host has
//             read the flag word of the one before it: nothing is indexed with an unchecked value.
//   trace     one lane per half-edge throughout. k17_successors builds the lists; k17_jump is ONE round of pointer jumping
//             from one buffer into the other (the host launches ceil(log2(2 n_polylines)) of them: no kernel waits for
//             another lane); k17_cut_rings resets what has reached no end — it lies on a ring — with the ring cut at its
//             smallest node, and the same rounds rank it again; k17_heads marks, per chain, its smallest polyline id and
//             the half-edge it starts with; a scan of the marks numbers the chains; k17_chain_sizes and a 64-bit scan give
//             the offsets; k17_fill writes every half-edge's from-node to its place (the position of a half-edge in its
//             list is the rank of its reverse in the opposite list, the head of its list the reverse of that list's end).
//   simplify  one wavefront per chain (a workgroup is one wavefront; it takes chain, chain + grid, ...). Every lane runs
//             simplify_indices with the same values; inside a linearizable_polyline test the lanes take 64 interior points
//             at a time and a ballot answers "any distance > maxsq". A chain of at most K17_LDS_VERTICES vertices is staged
//             in LDS, a longer one reads node_X through its node ids. Lane 0 writes the kept nodes to the chain's region
//             (front list from the left, end list from the right); k17_compact packs the regions behind a scan of the
//             counts (the two-pass pattern of K6 / K8).
//   length    one lane per chain, the sequential FP32 sum in vertex order.
// No scratch, no spills; LDS only in k17_simplify. Independent of EG3D_DLT_ROWS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eg3d_edges_core.h"
#include "eg3d_k17_edges.h"

namespace eg3d {

using namespace edges;
using u64 = unsigned long long;

// adds the number of lanes with `pred` to *ctr, one atomic per wavefront and none for a wavefront without; every lane of
// the wavefront must call it
__device__ __forceinline__ void k17_count(bool pred, u64* ctr) {
  const u64 m = __ballot(pred);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(ctr, (u64)__popcll(m));
}
__device__ __forceinline__ void k17_flag(bool pred, uint32_t flag, u64* ctr) {
  const u64 m = __ballot(pred);
  if ((threadIdx.x & 63u) == 0 && m) atomicOr(&ctr[K17C_FLAGS], (u64)flag);
}

__global__ void __launch_bounds__(K17_BLOCK) k17_check_polylines(K17Graph g, u64* ctr) {
  const uint32_t p = blockIdx.x * K17_BLOCK + threadIdx.x;
  const bool mine = p < g.n_polylines;
  const uint32_t s = mine ? g.pl_start[p] : 0u, t = mine ? g.pl_end[p] : 0u;
  k17_flag(mine && (s >= g.n_nodes || t >= g.n_nodes), K17_FLAG_BAD_NODE, ctr);
  k17_count(mine && s == t, &ctr[K17C_LOOPS]);
}

// entries 0 .. n_nodes of conn_off: from 0, ascending, to `expect`
__global__ void __launch_bounds__(K17_BLOCK) k17_check_offsets(K17Graph g, u64 expect, u64* ctr) {
  const uint32_t i = blockIdx.x * K17_BLOCK + threadIdx.x;
  bool bad = false;
  if (i <= g.n_nodes) {
    const u64 a = g.conn_off[i];
    if (i == 0 && a != 0) bad = true;
    if (i == g.n_nodes ? a != expect : (a > g.conn_off[i + 1] || g.conn_off[i + 1] > expect)) bad = true;
  }
  k17_flag(bad, K17_FLAG_BAD_OFFSETS, ctr);
}

struct K17Claim {
  uint32_t* seen;
  __device__ bool operator()(u64 slot) { return atomicExch(&seen[slot], 1u) != 0u; }
};
__global__ void __launch_bounds__(K17_BLOCK) k17_check_rows(K17Graph g, uint32_t* seen, uint32_t* deg, u64* ctr) {
  const uint32_t v = blockIdx.x * K17_BLOCK + threadIdx.x;
  bool ok = true;
  if (v < g.n_nodes) {
    K17Claim claim{seen};
    uint32_t d = 0;
    ok = check_row(v, g.n_polylines, g.pl_start, g.pl_end, (const uint64_t*)g.conn_off, g.conn_pl, claim, &d);
    deg[v] = d;
  }
  k17_flag(!ok, K17_FLAG_BAD_ROW, ctr);
}

__global__ void __launch_bounds__(K17_BLOCK) k17_successors(K17Graph g, const uint32_t* deg, uint32_t* succ, K17State s) {
  const uint32_t h = blockIdx.x * K17_BLOCK + threadIdx.x;
  if (h >= 2u * g.n_polylines) return;
  const uint32_t p = h >> 1;
  uint32_t next = kNone;
  if (g.pl_start[p] != g.pl_end[p])
    next = successor(h, deg[he_far(h, g.pl_start, g.pl_end)], g.pl_start, g.pl_end, (const uint64_t*)g.conn_off, g.conn_pl);
  succ[h] = next;
  s.ptr[h] = next;
  s.rank[h] = next != kNone ? 1u : 0u;
  s.minp[h] = p;
  s.minn[h] = he_from(h, g.pl_start, g.pl_end);
  s.last[h] = h;
}

__global__ void __launch_bounds__(K17_BLOCK) k17_jump(uint32_t n_halfedges, K17State in, K17State out) {
  const uint32_t h = blockIdx.x * K17_BLOCK + threadIdx.x;
  if (h >= n_halfedges) return;
  const uint32_t n = in.ptr[h];
  uint32_t ptr = n, rank = in.rank[h], minp = in.minp[h], minn = in.minn[h], last = in.last[h];
  if (n != kNone) {
    ptr = in.ptr[n];
    rank += in.rank[n];
    minp = min(minp, in.minp[n]);
    minn = min(minn, in.minn[n]);
    last = in.last[n];
  }
  out.ptr[h] = ptr;
  out.rank[h] = rank;
  out.minp[h] = minp;
  out.minn[h] = minn;
  out.last[h] = last;
}

// After the rounds a half-edge whose list has reached no end lies on a ring, and minn is the ring's smallest node id (the
// rounds covered 2^rounds >= 2 n_polylines half-edges: the whole cycle). Its state is reset with the ring cut there.
__global__ void __launch_bounds__(K17_BLOCK) k17_cut_rings(K17Graph g, const uint32_t* succ, K17State s, uint32_t* cut_node, u64* ctr) {
  const uint32_t h = blockIdx.x * K17_BLOCK + threadIdx.x;
  const bool ring = h < 2u * g.n_polylines && s.ptr[h] != kNone;
  if (h < 2u * g.n_polylines) {
    uint32_t cut = kNone;
    if (ring) {
      cut = s.minn[h];
      const uint32_t next = he_far(h, g.pl_start, g.pl_end) == cut ? kNone : succ[h];
      s.ptr[h] = next;
      s.rank[h] = next != kNone ? 1u : 0u;
      s.minp[h] = h >> 1;
      s.last[h] = h;
    }
    cut_node[h] = cut;
  }
  k17_count(ring, &ctr[K17C_RING_HALFEDGES]);
}

// The first half-edge of each chain: it leaves a terminal (a ring: the cut node), and of the chain's two directions it is
// the chosen one. minp of a list's first half-edge is the chain's smallest polyline id.
__global__ void __launch_bounds__(K17_BLOCK) k17_heads(K17Graph g, const uint32_t* deg, const uint32_t* cut_node, K17State s,
                                                       uint32_t* head_flag, uint32_t* head_of) {
  const uint32_t h = blockIdx.x * K17_BLOCK + threadIdx.x;
  if (h >= 2u * g.n_polylines || g.pl_start[h >> 1] == g.pl_end[h >> 1]) return;
  const uint32_t from = he_from(h, g.pl_start, g.pl_end), cut = cut_node[h];
  const bool first = cut != kNone ? from == cut : deg[from] != 2u;
  if (!first || !head_is_chosen(h, s.last[h])) return;
  const uint32_t mp = s.minp[h];
  head_flag[mp] = 1u;
  head_of[mp] = h;
}

__global__ void __launch_bounds__(K17_BLOCK) k17_chain_sizes(K17Graph g, const uint32_t* head_flag, const uint32_t* chain_id,
                                                             const uint32_t* head_of, const uint32_t* cut_node, K17State s, u64* n_vtx,
                                                             uint32_t* chain_flags, uint32_t* chain_of_head, u64* ctr) {
  const uint32_t p = blockIdx.x * K17_BLOCK + threadIdx.x;
  const bool mine = p < g.n_polylines && head_flag[p] != 0u;
  bool ring = false;
  u64 n = 0;
  if (mine) {
    const uint32_t c = chain_id[p], h = head_of[p];
    ring = cut_node[h] != kNone;
    n = (u64)s.rank[h] + 2u;
    n_vtx[c] = n;
    chain_flags[c] = ring ? 1u : 0u;
    chain_of_head[h] = c;
  }
  k17_count(ring, &ctr[K17C_RINGS]);
  // the longest chain: the wavefront's maximum, one atomic per wavefront that has a chain
  for (int d = 32; d > 0; d >>= 1) n = max(n, (u64)__shfl_xor((unsigned long long)n, d));
  if ((threadIdx.x & 63u) == 0 && n) atomicMax(&ctr[K17C_LONGEST], n);
}

__global__ void __launch_bounds__(K17_BLOCK) k17_fill(K17Graph g, K17State s, const uint32_t* chain_of_head, const u64* chain_off,
                                                      uint32_t* chain_node, u64* ctr) {
  const uint32_t h = blockIdx.x * K17_BLOCK + threadIdx.x;
  bool bad = false;
  if (h < 2u * g.n_polylines && g.pl_start[h >> 1] != g.pl_end[h >> 1]) {
    const uint32_t r = h ^ 1u, head = s.last[r] ^ 1u, c = chain_of_head[head];
    if (c != kNone) {  // (kNone: the direction that is not the chain's)
      const u64 at = chain_off[c] + s.rank[r], end = chain_off[c + 1];
      const bool is_last = s.ptr[h] == kNone && s.rank[h] == 0u;
      if (at + (is_last ? 1u : 0u) < end) {
        chain_node[at] = he_from(h, g.pl_start, g.pl_end);
        if (is_last) chain_node[at + 1] = he_far(h, g.pl_start, g.pl_end);
      } else {
        bad = true;
      }
    }
  }
  k17_flag(bad, K17_FLAG_INTERNAL, ctr);
}

// ---- simplify --------------------------------------------------------------------------------------------------------
struct K17Pts {
  const float* staged;   // the chain's vertices in LDS, or null
  const float* node_X;
  const uint32_t* node;  // the chain's node ids
  __device__ void get(uint32_t i, float* p) const {
    const float* s = staged ? staged + 3u * i : node_X + 3ull * node[i];
    p[0] = s[0], p[1] = s[1], p[2] = s[2];
  }
};
struct K17Lin {  // linearizable_polyline, 64 interior points at a time
  K17Pts P;
  float maxsq;
  uint32_t lane;
  __device__ bool operator()(uint32_t start, uint32_t end) {
    for (uint32_t base = start + 1; base < end; base += 64u) {
      const uint32_t i = base + lane;
      const bool off = i < end && point_off_line(P, start, end, i, maxsq);
      if (__ballot(off)) return false;
    }
    return true;
  }
};
struct K17Out {
  uint32_t* region;  // null in every lane but lane 0
  const uint32_t* node;
  uint32_t span;
  __device__ void front(uint32_t k, uint32_t i) {
    if (region) region[k] = node[i];
  }
  __device__ void back(uint32_t k, uint32_t i) {
    if (region) region[span - 1u - k] = node[i];
  }
};

__global__ void __launch_bounds__(64) k17_simplify(const float* node_X, uint64_t n_chains, const u64* chain_off, const uint32_t* chain_node,
                                                   float maxsq, uint32_t* region, uint32_t* n_front, uint32_t* n_back, u64* n_kept) {
  __shared__ float staged[3 * K17_LDS_VERTICES];
  const uint32_t lane = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_chains; c += gridDim.x) {
    const u64 off = chain_off[c];
    const uint32_t n = (uint32_t)(chain_off[c + 1] - off);
    const uint32_t* node = chain_node + off;
    const uint32_t span = simplified_span(n, node[0], node[n - 1]);
    const bool stage = span <= K17_LDS_VERTICES;
    __syncthreads();  // (the chain before this one is done with the staging area)
    if (stage)
      for (uint32_t i = lane; i < span; i += 64u) {
        const float* s = node_X + 3ull * node[i];
        staged[3u * i] = s[0], staged[3u * i + 1u] = s[1], staged[3u * i + 2u] = s[2];
      }
    __syncthreads();
    K17Lin lin{K17Pts{stage ? staged : nullptr, node_X, node}, maxsq, lane};
    K17Out out{lane == 0 ? region + off : nullptr, node, span};
    uint32_t nf = 0, nb = 0;
    simplify_indices(lin, span, out, &nf, &nb);
    if (lane == 0) {
      if (span != n) region[off + n - 1u] = node[n - 1u], nb++;  // E1: the closing vertex again
      n_front[c] = nf;
      n_back[c] = nb;
      n_kept[c] = (u64)nf + nb;
    }
  }
}

__global__ void __launch_bounds__(K17_BLOCK) k17_compact(uint64_t n_chains, const u64* chain_off, const uint32_t* region,
                                                         const uint32_t* n_front, const uint32_t* n_back, const u64* s_off, uint32_t* s_node) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_waves = (uint64_t)gridDim.x * (K17_BLOCK / 64);
  for (uint64_t c = (uint64_t)blockIdx.x * (K17_BLOCK / 64) + (threadIdx.x >> 6); c < n_chains; c += n_waves) {
    const uint32_t nf = n_front[c], nb = n_back[c];
    const uint32_t* src = region + chain_off[c];
    const uint32_t* src_back = region + chain_off[c + 1] - nb;
    uint32_t* dst = s_node + s_off[c];
    for (uint32_t k = lane; k < nf; k += 64u) dst[k] = src[k];
    for (uint32_t k = lane; k < nb; k += 64u) dst[nf + k] = src_back[k];
  }
}

__global__ void __launch_bounds__(K17_BLOCK) k17_length(const float* node_X, uint64_t n_chains, const u64* s_off, const uint32_t* s_node,
                                                        float* length) {
  const uint64_t c = (uint64_t)blockIdx.x * K17_BLOCK + threadIdx.x;
  if (c >= n_chains) return;
  length[c] = polyline_length(node_X, s_node + s_off[c], s_off[c + 1] - s_off[c]);
}

// ---- launches ----------------------------------------------------------------------------------------------------------
static unsigned k17_blocks(uint64_t n) { return (unsigned)((n + K17_BLOCK - 1) / K17_BLOCK); }

void launch_k17_check_polylines(hipStream_t st, K17Graph g, u64* ctr) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_check_polylines, dim3(k17_blocks(g.n_polylines)), dim3(K17_BLOCK), 0, st, g, ctr);
}
void launch_k17_check_offsets(hipStream_t st, K17Graph g, u64 expect, u64* ctr) {
  hipLaunchKernelGGL(k17_check_offsets, dim3(k17_blocks((uint64_t)g.n_nodes + 1)), dim3(K17_BLOCK), 0, st, g, expect, ctr);
}
void launch_k17_check_rows(hipStream_t st, K17Graph g, uint32_t* seen, uint32_t* deg, u64* ctr) {
  if (!g.n_nodes) return;
  hipLaunchKernelGGL(k17_check_rows, dim3(k17_blocks(g.n_nodes)), dim3(K17_BLOCK), 0, st, g, seen, deg, ctr);
}
void launch_k17_successors(hipStream_t st, K17Graph g, const uint32_t* deg, uint32_t* succ, K17State s) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_successors, dim3(k17_blocks(2ull * g.n_polylines)), dim3(K17_BLOCK), 0, st, g, deg, succ, s);
}
void launch_k17_jump(hipStream_t st, uint32_t n_halfedges, K17State in, K17State out) {
  if (!n_halfedges) return;
  hipLaunchKernelGGL(k17_jump, dim3(k17_blocks(n_halfedges)), dim3(K17_BLOCK), 0, st, n_halfedges, in, out);
}
void launch_k17_cut_rings(hipStream_t st, K17Graph g, const uint32_t* succ, K17State s, uint32_t* cut_node, u64* ctr) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_cut_rings, dim3(k17_blocks(2ull * g.n_polylines)), dim3(K17_BLOCK), 0, st, g, succ, s, cut_node, ctr);
}
void launch_k17_heads(hipStream_t st, K17Graph g, const uint32_t* deg, const uint32_t* cut_node, K17State s, uint32_t* head_flag,
                      uint32_t* head_of) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_heads, dim3(k17_blocks(2ull * g.n_polylines)), dim3(K17_BLOCK), 0, st, g, deg, cut_node, s, head_flag, head_of);
}
void launch_k17_chain_sizes(hipStream_t st, K17Graph g, const uint32_t* head_flag, const uint32_t* chain_id, const uint32_t* head_of,
                            const uint32_t* cut_node, K17State s, u64* n_vtx, uint32_t* chain_flags, uint32_t* chain_of_head, u64* ctr) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_chain_sizes, dim3(k17_blocks(g.n_polylines)), dim3(K17_BLOCK), 0, st, g, head_flag, chain_id, head_of, cut_node,
                     s, n_vtx, chain_flags, chain_of_head, ctr);
}
void launch_k17_fill(hipStream_t st, K17Graph g, K17State s, const uint32_t* chain_of_head, const u64* chain_off, uint32_t* chain_node,
                     u64* ctr) {
  if (!g.n_polylines) return;
  hipLaunchKernelGGL(k17_fill, dim3(k17_blocks(2ull * g.n_polylines)), dim3(K17_BLOCK), 0, st, g, s, chain_of_head, chain_off, chain_node,
                     ctr);
}
void launch_k17_simplify(hipStream_t st, const float* node_X, uint64_t n_chains, const u64* chain_off, const uint32_t* chain_node,
                         float maxsq, uint32_t* region, uint32_t* n_front, uint32_t* n_back, u64* n_kept) {
  if (!n_chains) return;
  const unsigned blocks = (unsigned)std::min<uint64_t>(n_chains, K17_SIMPLIFY_MAX_BLOCKS);
  hipLaunchKernelGGL(k17_simplify, dim3(blocks), dim3(64), 0, st, node_X, n_chains, chain_off, chain_node, maxsq, region, n_front, n_back,
                     n_kept);
}
void launch_k17_compact(hipStream_t st, uint64_t n_chains, const u64* chain_off, const uint32_t* region, const uint32_t* n_front,
                        const uint32_t* n_back, const u64* s_off, uint32_t* s_node) {
  if (!n_chains) return;
  const unsigned blocks = (unsigned)std::min<uint64_t>((n_chains + 3) / 4, 8192);
  hipLaunchKernelGGL(k17_compact, dim3(blocks), dim3(K17_BLOCK), 0, st, n_chains, chain_off, region, n_front, n_back, s_off, s_node);
}
void launch_k17_length(hipStream_t st, const float* node_X, uint64_t n_chains, const u64* s_off, const uint32_t* s_node, float* length) {
  if (!n_chains) return;
  hipLaunchKernelGGL(k17_length, dim3(k17_blocks(n_chains)), dim3(K17_BLOCK), 0, st, node_X, n_chains, s_off, s_node, length);
}

}  // namespace eg3d
