// eg3d_k19_edgemap.hip — K19: the edge maps of the source images (include/eg3d/edgemap.hh). Every rule is a function of
// eg3d_edgemap_core.h; what is here is where the values come from and where they go.
//
// A workgroup of 256 lanes owns a tile of 32 x 32 pixels of one view (blockIdx.z: the view, blockIdx.x / .y: the tile; a
// view with fewer tiles than the largest leaves the surplus workgroups idle). It stages the tile and the frame its stage
// needs in LDS, with the border rule of the stage applied on the way in, so that every later read is an LDS read without
// a case distinction:
//   k19_smooth    frame 2, indices folded (reflect-101): the horizontal sums of 36 rows, then the vertical sums of 32
//   k19_classify  frame 2 = 1 (Sobel, borders replicated) + 1 (the neighbours of the suppression): the Sobel pair and the
//                 magnitude of 34 x 34 pixels (0 outside the image), then direction, keep rule and class of 32 x 32
// Both read either grey values or the images themselves (E1 applied on the way in): the first stage of a call, whichever
// it is, reads the images, and no grey image is written for it.
//   k19_hysteresis frame 1 of classes (none outside the image): strong spreads over weak to the tile's fixed point in LDS.
//                 Lanes read and write the same LDS bytes without order inside a sweep; a byte only ever goes from weak
//                 to strong, a sweep that turned nothing has read the final values, so the fixed point does not depend on it.
//                 Across workgroups: a tile reads its frame from global memory, where the neighbours may be writing in
//                 the same launch — it sees the old class or the new one, both of them classes of the final set's past —
//                 and whoever changed anything marks its neighbours for the next launch. Only what a launch left behind is
//                 relied on: the launch that changes nothing read nothing that was being written.
//   k19_mask      one lane per 4 classes: strong -> 1, the rest -> 0, in place
// Every load is bounded by the fold, the clamp or an in-image test; every store by an in-image test; a tile index by the
// view's own tile counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "eg3d_k19_edgemap.h"

namespace eg3d {
using namespace edgemap;
using u64 = unsigned long long;

namespace {
constexpr int T = K19_TILE;
constexpr int kIn = T + 4;   // a staged side with frame 2
constexpr int kMid = T + 2;  // ... with frame 1

// the workgroup's view and the tile's first pixel; false: the view has no such tile
__device__ inline bool k19_tile(const K19Views& vs, uint32_t view_base, K19View* V, int* x0, int* y0) {
  *V = vs.views[view_base + blockIdx.z];
  *x0 = (int)blockIdx.x * T;
  *y0 = (int)blockIdx.y * T;
  return *x0 < V->w && *y0 < V->h;
}

template <bool RGB>
__device__ inline int k19_value(const uint8_t* src, const K19View& V, int y, int x) {
  const size_t i = (size_t)V.off + (size_t)y * (size_t)V.w + (size_t)x;
  if (RGB) return grey(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
  return src[i];
}
__device__ inline int k19_clamp(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }
}  // namespace

template <bool RGB>
__global__ void __launch_bounds__(K19_BLOCK) k19_smooth(K19Views vs, uint32_t view_base, const uint8_t* src, uint8_t* dst) {
  K19View V;
  int x0, y0;
  if (!k19_tile(vs, view_base, &V, &x0, &y0)) return;
  __shared__ uint8_t s_in[kIn][kIn];
  __shared__ uint16_t s_h[kIn][T];
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < kIn * kIn; i += K19_BLOCK) {
    const int ly = i / kIn, lx = i % kIn;
    s_in[ly][lx] = (uint8_t)k19_value<RGB>(src, V, fold101(y0 + ly - kSmoothHalo, V.h), fold101(x0 + lx - kSmoothHalo, V.w));
  }
  __syncthreads();
  for (int i = tid; i < kIn * T; i += K19_BLOCK) {
    const int ly = i / T, lx = i % T;
    s_h[ly][lx] = (uint16_t)binom5(s_in[ly][lx], s_in[ly][lx + 1], s_in[ly][lx + 2], s_in[ly][lx + 3], s_in[ly][lx + 4]);
  }
  __syncthreads();
  for (int i = tid; i < T * T; i += K19_BLOCK) {
    const int ly = i / T, lx = i % T, y = y0 + ly, x = x0 + lx;
    if (y < V.h && x < V.w)
      dst[(size_t)V.off + (size_t)y * (size_t)V.w + (size_t)x] =
          (uint8_t)smooth_round(binom5(s_h[ly][lx], s_h[ly + 1][lx], s_h[ly + 2][lx], s_h[ly + 3][lx], s_h[ly + 4][lx]));
  }
}

template <bool RGB>
__global__ void __launch_bounds__(K19_BLOCK) k19_classify(K19Views vs, uint32_t view_base, const uint8_t* src, int l2, uint32_t low,
                                                          uint32_t high, uint8_t* cls, u64* ctr) {
  K19View V;
  int x0, y0;
  if (!k19_tile(vs, view_base, &V, &x0, &y0)) return;
  __shared__ uint8_t s_in[kIn][kIn];
  __shared__ uint32_t s_m[kMid][kMid];  // the magnitude
  __shared__ uint32_t s_g[kMid][kMid];  // gx in the low half, gy in the high half (each fits 16 bits signed)
  __shared__ unsigned int s_cnt[2];
  const int tid = (int)threadIdx.x;
  if (tid < 2) s_cnt[tid] = 0;
  for (int i = tid; i < kIn * kIn; i += K19_BLOCK) {
    const int ly = i / kIn, lx = i % kIn;
    s_in[ly][lx] = (uint8_t)k19_value<RGB>(src, V, k19_clamp(y0 + ly - 2, V.h), k19_clamp(x0 + lx - 2, V.w));
  }
  __syncthreads();
  for (int i = tid; i < kMid * kMid; i += K19_BLOCK) {
    const int my = i / kMid, mx = i % kMid, y = y0 + my - 1, x = x0 + mx - 1;
    uint32_t m = 0, g = 0;
    if (y >= 0 && y < V.h && x >= 0 && x < V.w) {
      int q[3][3];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) q[r][c] = s_in[my + r][mx + c];
      const int gx = sobel_x(q), gy = sobel_y(q);
      m = magnitude(gx, gy, l2 != 0);
      g = ((uint32_t)gx & 0xffffu) | ((uint32_t)gy << 16);
    }
    s_m[my][mx] = m;
    s_g[my][mx] = g;
  }
  __syncthreads();
  unsigned int n_cand = 0, n_strong = 0;
  for (int i = tid; i < T * T; i += K19_BLOCK) {
    const int ly = i / T, lx = i % T, y = y0 + ly, x = x0 + lx;
    if (y >= V.h || x >= V.w) continue;
    const uint32_t g = s_g[ly + 1][lx + 1], m = s_m[ly + 1][lx + 1];
    const int gx = (int)(int16_t)(g & 0xffffu), gy = (int)(int16_t)(g >> 16);
    const int d = nms_direction(gx, gy), dr = nms_dr(d), dc = nms_dc(d);
    const bool kept = nms_keep(d, m, s_m[ly + 1 + dr][lx + 1 + dc], s_m[ly + 1 - dr][lx + 1 - dc]);
    const uint8_t k = classify(kept, m, low, high);
    cls[(size_t)V.off + (size_t)y * (size_t)V.w + (size_t)x] = k;
    n_cand += k != kNone;
    n_strong += k == kStrong;
  }
  if (n_cand) atomicAdd(&s_cnt[0], n_cand);
  if (n_strong) atomicAdd(&s_cnt[1], n_strong);
  __syncthreads();
  if (tid == 0) {
    if (s_cnt[0]) atomicAdd(&ctr[K19C_CANDIDATES], (u64)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&ctr[K19C_STRONG], (u64)s_cnt[1]);
  }
}

__global__ void __launch_bounds__(K19_BLOCK) k19_hysteresis(K19Views vs, uint32_t view_base, uint8_t* cls, uint8_t* dirty_in,
                                                            uint8_t* dirty_out, unsigned int* changed) {
  K19View V;
  int x0, y0;
  if (!k19_tile(vs, view_base, &V, &x0, &y0)) return;
  const int ntx = (int)k19_tiles(V.w), nty = (int)k19_tiles(V.h);
  const size_t tile = (size_t)V.tile_off + (size_t)blockIdx.y * (size_t)ntx + blockIdx.x;
  if (!dirty_in[tile]) return;  // (the same byte for every lane of the workgroup)
  __shared__ uint8_t s[kMid][kMid + 2];
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < kMid * kMid; i += K19_BLOCK) {
    const int my = i / kMid, mx = i % kMid, y = y0 + my - 1, x = x0 + mx - 1;
    s[my][mx] = (y >= 0 && y < V.h && x >= 0 && x < V.w) ? cls[(size_t)V.off + (size_t)y * (size_t)V.w + (size_t)x] : (uint8_t)kNone;
  }
  __syncthreads();
  // a lane's pixels: column tid % 32, rows tid / 32 + 8 k
  const int lx = tid % T + 1, ly0 = tid / T + 1;
  constexpr int kPer = T * T / K19_BLOCK, kStep = K19_BLOCK / T;
  bool turned[kPer];
  for (int k = 0; k < kPer; k++) turned[k] = false;
  for (;;) {
    int any = 0;
    for (int k = 0; k < kPer; k++) {
      const int ly = ly0 + k * kStep;
      if (s[ly][lx] != kWeak) continue;
      const bool reached = s[ly - 1][lx - 1] == kStrong || s[ly - 1][lx] == kStrong || s[ly - 1][lx + 1] == kStrong || s[ly][lx - 1] == kStrong ||
                           s[ly][lx + 1] == kStrong || s[ly + 1][lx - 1] == kStrong || s[ly + 1][lx] == kStrong || s[ly + 1][lx + 1] == kStrong;
      if (reached) {
        s[ly][lx] = kStrong;
        turned[k] = true;
        any = 1;
      }
    }
    if (!__syncthreads_or(any)) break;
  }
  int mine = 0;
  for (int k = 0; k < kPer; k++)
    if (turned[k]) {
      // (a pixel that turned was weak, so it lies inside the image)
      cls[(size_t)V.off + (size_t)(y0 + ly0 - 1 + k * kStep) * (size_t)V.w + (size_t)(x0 + lx - 1)] = kStrong;
      mine = 1;
    }
  const int tile_changed = __syncthreads_or(mine);
  if (tid == 0) {
    dirty_in[tile] = 0;
    if (tile_changed) {
      atomicAdd(changed, 1u);
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const int ty = (int)blockIdx.y + dy, tx = (int)blockIdx.x + dx;
          if ((dy || dx) && ty >= 0 && ty < nty && tx >= 0 && tx < ntx) dirty_out[(size_t)V.tile_off + (size_t)ty * (size_t)ntx + (size_t)tx] = 1;
        }
    }
  }
}

__global__ void __launch_bounds__(K19_BLOCK) k19_mask(uint8_t* cls, u64 n, u64* ctr) {
  const u64 n_words = n / 4, stride = (u64)gridDim.x * K19_BLOCK;
  uint32_t* words = reinterpret_cast<uint32_t*>(cls);  // (the array starts an allocation: aligned)
  unsigned int edges = 0;
  for (u64 i = (u64)blockIdx.x * K19_BLOCK + threadIdx.x; i < n_words; i += stride) {
    const uint32_t w = words[i];
    // a byte is 0, 1 or 2: bit 1 of each byte says strong
    const uint32_t m = (w >> 1) & 0x01010101u;
    words[i] = m;
    edges += (unsigned int)__popc(m);
  }
  if (blockIdx.x == 0 && threadIdx.x < (unsigned int)(n - 4 * n_words)) {
    const u64 i = 4 * n_words + threadIdx.x;
    const uint8_t m = cls[i] == kStrong;
    cls[i] = m;
    edges += m;
  }
  __shared__ unsigned int s_edges;
  if (threadIdx.x == 0) s_edges = 0;
  __syncthreads();
  if (edges) atomicAdd(&s_edges, edges);
  __syncthreads();
  if (threadIdx.x == 0 && s_edges) atomicAdd(&ctr[K19C_EDGES], (u64)s_edges);
}

namespace {
// one launch per K19_VIEWS_PER_LAUNCH views: the grid's third dimension is bounded
template <typename F>
void for_view_chunks(const K19Views& v, F launch) {
  for (uint32_t base = 0; base < v.n_views; base += K19_VIEWS_PER_LAUNCH)
    launch(base, dim3(v.max_tx, v.max_ty, std::min<uint32_t>(K19_VIEWS_PER_LAUNCH, v.n_views - base)));
}
}  // namespace

void launch_k19_smooth(hipStream_t st, K19Views v, bool from_rgb, const uint8_t* src, uint8_t* dst) {
  for_view_chunks(v, [&](uint32_t base, dim3 grid) {
    if (from_rgb)
      hipLaunchKernelGGL(k19_smooth<true>, grid, dim3(K19_BLOCK), 0, st, v, base, src, dst);
    else
      hipLaunchKernelGGL(k19_smooth<false>, grid, dim3(K19_BLOCK), 0, st, v, base, src, dst);
  });
}

void launch_k19_classify(hipStream_t st, K19Views v, bool from_rgb, const uint8_t* src, bool l2, uint32_t low, uint32_t high, uint8_t* cls,
                         u64* ctr) {
  for_view_chunks(v, [&](uint32_t base, dim3 grid) {
    if (from_rgb)
      hipLaunchKernelGGL(k19_classify<true>, grid, dim3(K19_BLOCK), 0, st, v, base, src, l2 ? 1 : 0, low, high, cls, ctr);
    else
      hipLaunchKernelGGL(k19_classify<false>, grid, dim3(K19_BLOCK), 0, st, v, base, src, l2 ? 1 : 0, low, high, cls, ctr);
  });
}

void launch_k19_hysteresis(hipStream_t st, K19Views v, uint8_t* cls, uint8_t* dirty_in, uint8_t* dirty_out, unsigned int* changed) {
  for_view_chunks(v, [&](uint32_t base, dim3 grid) {
    hipLaunchKernelGGL(k19_hysteresis, grid, dim3(K19_BLOCK), 0, st, v, base, cls, dirty_in, dirty_out, changed);
  });
}

void launch_k19_mask(hipStream_t st, uint8_t* cls, u64 n, u64* ctr) {
  const u64 blocks = std::min<u64>(4096, std::max<u64>(1, (n / 4 + K19_BLOCK - 1) / K19_BLOCK));
  hipLaunchKernelGGL(k19_mask, dim3((unsigned int)blocks), dim3(K19_BLOCK), 0, st, cls, n, ctr);
}

}  // namespace eg3d
