// eg3d_k1_k2_refpoints.hip — gfx950 kernels of stage A of the refpoint -> epipolar match -> triangulate path.
//
// Phase pipeline (DESIGN.md "Kernels"):
//   k_seed_prep       1 lane / seed       view map of the track, (seed,entry) of every track entry
//   k1_count_raw      1 lane / (seed,entry)  upper bound of candidate polylines (sizes the slots)
//   k1_seed_candidates 1 WAVE / (seed,entry) k-way merge of the 30 px grid cells into batches of 64 candidate ids +
//                                           closest-point scan of a batch's segments as one flat sequence
//   k_task_fill       1 lane / (seed,entry)  enumerates (seed, start view, start hit) tasks; sums K1's byte counts
//   k2_epipolar_hits  1 WAVE / task         epiline x the segments of all candidate polylines of a list (flat),
//                                           ballot/popcount ordered compaction (count pass + fill pass)
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ prep -------
__global__ void k_seed_prep(SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base, uint32_t* sv_seed,
                            int32_t* map_view, uint32_t* map_entry, uint32_t* map_n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seeds) return;
  uint32_t seed = seed_begin + i;
  uint32_t t0 = sd.trk_off[seed], t1 = sd.trk_off[seed + 1];
  for (uint32_t e = t0; e < t1; e++) sv_seed[e - sv_base] = seed;
  map_n[i] = build_seed_view_map(sd.trk_view + t0, t1 - t0, map_view + (t0 - sv_base), map_entry + (t0 - sv_base));
}

__global__ void k1_count_raw(DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                             uint32_t* raw_cnt) {
  uint32_t sv = blockIdx.x * blockDim.x + threadIdx.x;
  if (sv >= n_sv) return;
  uint32_t seed = sv_seed[sv];
  uint32_t t0 = sd.trk_off[seed], k = sd.trk_off[seed + 1] - t0;
  int32_t view = sd.trk_view[sv_base + sv];
  float px, py;
  seed_obs_in_view(sd, t0, k, view, px, py);
  CellWindow w = cell_window(30.0f, s.width, s.height, s.g30_w, s.g30_h, px, py);
  uint32_t n = 0;
  if (w.c1 >= w.c0) {
    const size_t base = (size_t)view * (size_t)(s.g30_w * s.g30_h);
    for (int r = w.r0; r <= w.r1; r++)
      n += s.g30_off[base + (size_t)r * s.g30_w + w.c1 + 1] - s.g30_off[base + (size_t)r * s.g30_w + w.c0];
  }
  raw_cnt[sv] = n;
}

// ------------------------------------------------------------------ K1 ---------
// One wavefront per (seed, track entry). Lanes 0..8 each own one grid cell of the (shrunk)
// 3x3 window and k-way-merge the ascending id lists (wave-min of the heads) so candidates
// come out ascending and unique, 64 at a time; the segments of such a batch are scanned as one
// flat sequence over the 64 lanes and the first closest segment of every candidate falls out of
// an LDS minimum (below). Outputs go to the slot [raw_off[sv], raw_off[sv+1]) sized by
// k1_count_raw. (Reference: PLGEdgeManager::detect_nearby_intersections_and_correspondences_plgp,
// plg_edge_manager.cpp:261-300, its per-view polyline search polyLine_2d_map_search.cpp:46-77.)
__global__ void __launch_bounds__(256) k1_seed_candidates(DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv,
                                                         const uint32_t* sv_seed, const uint32_t* raw_off,
                                                         uint32_t* cand_pl, Obs* start_hits, uint32_t* cand_cnt,
                                                         uint32_t* start_cnt, uint32_t* sv_vtx) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_sv) return;
  const uint32_t sv = wave;
  const uint32_t seed = sv_seed[sv];
  const uint32_t t0 = sd.trk_off[seed], k = sd.trk_off[seed + 1] - t0;
  const int32_t view = sd.trk_view[sv_base + sv];
  float px, py;
  seed_obs_in_view(sd, t0, k, view, px, py);
  CellWindow w = cell_window(30.0f, s.width, s.height, s.g30_w, s.g30_h, px, py);
  uint32_t a = 0, b = 0;
  if (w.c1 >= w.c0) {
    const int ncols = w.c1 - w.c0 + 1, nrows = w.r1 - w.r0 + 1;
    if ((int)lane < ncols * nrows) {
      const int r = w.r0 + (int)lane / ncols, c = w.c0 + (int)lane % ncols;
      const size_t cell = (size_t)view * (size_t)(s.g30_w * s.g30_h) + (size_t)r * s.g30_w + c;
      a = s.g30_off[cell];
      b = s.g30_off[cell + 1];
    }
  }
  const uint32_t out_base = raw_off[sv];
  uint32_t nc = 0, ns = 0;
  uint32_t nvtx = 0;
  // Candidates are taken in batches of up to 64 ids (phase A: the k-way merge, one wave-minimum per id, the lanes' list
  // heads loaded eight at a time); the segments of a whole batch are then scanned as ONE flat sequence (phase B) — a
  // pass per candidate paid the dependent look-ups id -> vertex range -> vertices and three wave reductions per
  // candidate with ~25 of 64 lanes busy. The first closest segment of a candidate (smallest distance, then smallest
  // index) is the minimum of the 64-bit keys (distance bits : segment) in the candidate's LDS slot: squared distances
  // are >= +0, so their bit patterns order like the values; NaN / infinite distances are never submitted (the plain
  // scan's `d < best` with best = +inf).
  __shared__ unsigned long long k1_best[4][64];
  unsigned long long* const slot = k1_best[threadIdx.x >> 6];
  const uint32_t gview = s.view_pl_off[view];
  const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  uint32_t h0 = 0xffffffffu, h1 = 0xffffffffu, h2 = 0xffffffffu, h3 = 0xffffffffu, h4 = 0xffffffffu, h5 = 0xffffffffu,
           h6 = 0xffffffffu, h7 = 0xffffffffu;
  uint32_t hn = 0;  // ids of this lane's list held in h0..h7
  for (;;) {
    uint32_t my_id = 0xffffffffu, nb = 0;
    while (nb < 64) {
      if (hn == 0 && a < b) {  // refill: up to eight ids of the lane's cell list, their loads in flight together
        const uint32_t r = b - a;
        h0 = s.g30_ids[a];
        h1 = r > 1 ? s.g30_ids[a + 1] : 0xffffffffu;
        h2 = r > 2 ? s.g30_ids[a + 2] : 0xffffffffu;
        h3 = r > 3 ? s.g30_ids[a + 3] : 0xffffffffu;
        h4 = r > 4 ? s.g30_ids[a + 4] : 0xffffffffu;
        h5 = r > 5 ? s.g30_ids[a + 5] : 0xffffffffu;
        h6 = r > 6 ? s.g30_ids[a + 6] : 0xffffffffu;
        h7 = r > 7 ? s.g30_ids[a + 7] : 0xffffffffu;
        hn = r > 8 ? 8 : r;
        a += hn;
      }
      const uint32_t head = hn ? h0 : 0xffffffffu;
      const uint32_t m = wave_min_u32_dpp(head);
      if (m == 0xffffffffu) break;
      if (head == m) {
        h0 = h1, h1 = h2, h2 = h3, h3 = h4, h4 = h5, h5 = h6, h6 = h7, h7 = 0xffffffffu;
        hn--;
      }
      if (lane == nb) my_id = m;
      nb++;
    }
    if (nb == 0) break;
    uint32_t my_a = 0, my_n = 0;
    if (lane < nb) {
      const uint32_t v0 = s.pl_vtx_off[gview + my_id], v1 = s.pl_vtx_off[gview + my_id + 1];
      my_a = v0;
      my_n = v1 - v0;
    }
    const uint32_t my_ns = my_n >= 2u ? my_n - 1u : 0u;
    nvtx += (uint32_t)lane_bcast(wave_incl_scan((int)my_n), 63);
    const uint32_t incl = (uint32_t)wave_incl_scan((int)my_ns);
    const uint32_t total = (uint32_t)lane_bcast((int)incl, 63);
    slot[lane] = ~0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < total; base += 64) {
      const uint32_t f = base + lane;
      uint32_t pos = 0;  // owner of flat segment f: the first lane whose inclusive count exceeds f
#pragma unroll
      for (uint32_t step = 32; step; step >>= 1) {
        const uint32_t v = (uint32_t)__shfl((int)incl, (int)(pos + step - 1), 64);
        if (v <= f) pos += step;
      }
      const uint32_t o_incl = (uint32_t)__shfl((int)incl, (int)pos, 64);
      const uint32_t o_ns = (uint32_t)__shfl((int)my_ns, (int)pos, 64);
      const uint32_t o_a = (uint32_t)__shfl((int)my_a, (int)pos, 64);
      if (f < total) {
        const uint32_t j = f - (o_incl - o_ns);
        const f2 v0 = s.vtx[o_a + j], v1 = s.vtx[o_a + j + 1];
        float qx, qy;
        const float d = seg_closest(px, py, v0.x, v0.y, v1.x, v1.y, qx, qy);
        if (d < __builtin_huge_valf())
          atomicMin(&slot[pos], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)j);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned long long key = slot[lane];
    const bool valid = lane < nb && key != ~0ull;  // no finite distance (degenerate polyline): never a candidate
    const float dmin = __uint_as_float((uint32_t)(key >> 32));
    const uint32_t jmin = (uint32_t)key;
    const bool is_start = valid && dmin <= 100.0f;
    const bool is_cand = valid && dmin <= 900.0f;
    const unsigned long long mc = __ballot(is_cand), ms = __ballot(is_start);
    if (is_cand) cand_pl[out_base + nc + __popcll(mc & lt_mask)] = my_id;
    if (is_start) {
      const f2 v0 = s.vtx[my_a + jmin], v1 = s.vtx[my_a + jmin + 1];
      Obs o;
      o.view = view;
      o.pl = my_id;
      o.seg = jmin;
      (void)seg_closest(px, py, v0.x, v0.y, v1.x, v1.y, o.x, o.y);  // the winning segment's closest point again: same inputs, same bits
      start_hits[out_base + ns + __popcll(ms & lt_mask)] = o;
    }
    nc += __popcll(mc);
    ns += __popcll(ms);
    __builtin_amdgcn_wave_barrier();
    if (nb < 64) break;
  }
  if (lane == 0) {
    cand_cnt[sv] = nc;
    start_cnt[sv] = ns;
    // the vertices this entry's scans touched (algorithmic bytes): summed by k_task_fill, one atomic per
    // wave of entries — one atomic per entry on the one counter serialised at the memory side and was 3/4 of this
    // kernel's time (0.51 -> 0.13 ms on C3')
    sv_vtx[sv] = nvtx;
  }
}

__global__ void k_task_fill(SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                            const uint32_t* start_cnt, const uint32_t* task_off, uint32_t* task_seed,
                            uint32_t* task_entry, uint32_t* task_hit, uint32_t* task_k, const uint32_t* sv_vtx,
                            Counters* ctr) {
  uint32_t sv = blockIdx.x * blockDim.x + threadIdx.x;
  {  // K1's vertex counts -> the byte counter, one atomic per wave of entries
    unsigned long long v = sv < n_sv ? (unsigned long long)sv_vtx[sv] : 0ull;
    for (int d = 32; d; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&ctr->bytes, 8ull * v);
  }
  if (sv >= n_sv) return;
  const uint32_t seed = sv_seed[sv];
  const uint32_t t0 = sd.trk_off[seed], k = sd.trk_off[seed + 1] - t0;
  const uint32_t entry = sv_base + sv - t0;
  const uint32_t n = start_cnt[sv], base = task_off[sv];
  for (uint32_t h = 0; h < n; h++) {
    task_seed[base + h] = seed;
    task_entry[base + h] = entry;
    task_hit[base + h] = h;
    task_k[base + h] = k;
  }
}

// ------------------------------------------------------------------ K2 ---------
// One wavefront per task, ONE pass. For every other track entry: epipolar line of the start hit, then all 64 lanes test
// consecutive segments of each candidate polyline; hits inside the detection radius are compacted in segment order with
// __ballot + popcount. Where the hits of a task land in `hits` is decided only once the task knows how many it has, so
// the sweep over the lists writes them to a per-wave LDS stage of `cap` <= EG3D_K2_STAGE_MAX hits; the four tasks of a
// workgroup then claim their regions together, in task order, with ONE atomicAdd on the context's cursor
// (Counters::hits_used), and every wave copies its stage out behind its claim. (One atomicAdd per task was measured first:
// C3' has 119 k tasks per step, the returning atomics on the one address went through the memory side one at a time, and
// the kernel took 1.47 ms - as long as both passes of the two-pass form - with 41 % fewer instructions.) A task that outgrows the
// stage (or has more than 64 lists: the staged form keeps the count of list i in lane i) has been counted by that sweep
// all the same; it claims, then sweeps again and writes straight to its region (DIRECT). The order of the tasks' regions
// in `hits` depends on timing: everything downstream addresses hits through (list_ptr[l], list_cnt[l]) only.
// A claim that ends beyond hits_cap writes no hit; the host sees the cursor in its next read-back, before anything has
// read `hits`, enlarges the buffer and launches K2 again (run_stage_b).
struct K2Task {
  uint32_t t0, k, sv0, lo, lane;
  int32_t start_view;
  Obs hit;
  float detsq;
  unsigned long long lt_mask;
};
// DIRECT=false: hit number p of the task -> dst[p] (the LDS stage) while p < limit; count of list i -> list_cnt and lane
// i & 63's my_cnt. DIRECT=true: dst = the task's region of `hits`, first hit of list i -> list_ptr. Returns the task's hits.
template <bool DIRECT>
__device__ __forceinline__ uint32_t k2_sweep(const DevScene& s, const SeedsDev& sd, const K2Task& T, const uint32_t* raw_off,
                                             const uint32_t* cand_pl, const uint32_t* cand_cnt, Obs* dst, uint32_t limit,
                                             uint32_t base, uint32_t* list_cnt, uint32_t* list_ptr, uint32_t& my_cnt) {
  const uint32_t lane = T.lane, t0 = T.t0;
  uint32_t tot = 0;
  for (uint32_t i = 0; i < T.k; i++) {
    const int32_t cur_view = sd.trk_view[t0 + i];
    uint32_t cnt = 0;
    if (DIRECT && lane == 0) list_ptr[T.lo + i] = base + tot;
    if (cur_view == T.start_view) {
      cnt = 1;
      if (lane == 0 && tot < limit) {
        Obs o = T.hit;
        o.view = cur_view;
        dst[tot] = o;
      }
    } else {
      float la, lb, lc;
      if (epiline(s.F, s.F_valid, s.n_views, T.start_view, cur_view, T.hit.x, T.hit.y, la, lb, lc)) {
        const float sx = sd.trk_xy[2 * (t0 + i)], sy = sd.trk_xy[2 * (t0 + i) + 1];
        const uint32_t cbase = raw_off[T.sv0 + i], ncand = cand_cnt[T.sv0 + i];
        // The segments of up to 64 candidate polylines are dealt to the lanes as ONE flat sequence (candidate-major,
        // segment-minor = the order of the per-candidate loops): polylines average ~25 vertices, so a pass per
        // candidate left 60 % of the lanes idle and paid its dependent look-ups (candidate id -> vertex range ->
        // vertices) once per candidate; here the look-ups of all candidates are in flight together.
        const uint32_t gview = s.view_pl_off[cur_view];
        for (uint32_t c0 = 0; c0 < ncand; c0 += 64) {
          const uint32_t c = c0 + lane;
          uint32_t my_id = 0, my_a = 0, my_ns = 0;
          if (c < ncand) {
            my_id = cand_pl[cbase + c];
            const uint32_t a = s.pl_vtx_off[gview + my_id], b = s.pl_vtx_off[gview + my_id + 1];
            my_a = a;
            my_ns = (b - a) >= 2u ? (b - a) - 1u : 0u;
          }
          const uint32_t incl = (uint32_t)wave_incl_scan((int)my_ns);
          const uint32_t total = (uint32_t)lane_bcast((int)incl, 63);
          const uint32_t excl = incl - my_ns;
          // four chunks of 64 flat segments per trip: their owner searches and vertex loads are independent and in
          // flight together (one chunk at a time, a wave waited out one memory latency per chunk)
          constexpr int U = 4;
          for (uint32_t fb = 0; fb < total; fb += 64 * U) {
            f2 v0[U], v1[U];
            uint32_t oid[U], seg[U];
            bool in[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
              const uint32_t f = fb + 64u * u + lane;
              in[u] = f < total;
              oid[u] = seg[u] = 0;
              v0[u].x = v0[u].y = v1[u].x = v1[u].y = 0.f;
              if (fb + 64u * u < total) {  // wave-uniform
                uint32_t pos = 0;  // owner of flat segment f: the first lane whose inclusive count exceeds f
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1) {
                  const uint32_t v = (uint32_t)__shfl((int)incl, (int)(pos + step - 1), 64);
                  if (v <= f) pos += step;
                }
                const uint32_t o_excl = (uint32_t)__shfl((int)excl, (int)pos, 64);
                const uint32_t o_a = (uint32_t)__shfl((int)my_a, (int)pos, 64);
                oid[u] = (uint32_t)__shfl((int)my_id, (int)pos, 64);
                if (in[u]) {
                  seg[u] = f - o_excl;
                  v0[u] = s.vtx[o_a + seg[u]];
                  v1[u] = s.vtx[o_a + seg[u] + 1];
                }
              }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
              if (fb + 64u * u >= total) break;  // wave-uniform
              bool ok = false;
              float hx = 0.f, hy = 0.f;
              if (in[u] && seg_line_hit(v1[u].x, v1[u].y, v0[u].x, v0[u].y, la, lb, lc, hx, hy))
                ok = dist2(sx, sy, hx, hy) <= T.detsq;
              const unsigned long long mask = __ballot(ok);
              const uint32_t p = tot + cnt + __popcll(mask & T.lt_mask);
              if (ok && p < limit) {
                Obs o;
                o.view = cur_view;
                o.pl = oid[u];
                o.seg = seg[u];
                o.x = hx;
                o.y = hy;
                dst[p] = o;
              }
              cnt += __popcll(mask);
            }
          }
        }
      }
    }
    if (!DIRECT) {
      if (lane == 0) list_cnt[T.lo + i] = cnt;
      if (lane == (i & 63u)) my_cnt = cnt;
    }
    tot += cnt;
  }
  return tot;
}

__global__ void __launch_bounds__(256) k2_epipolar_hits(DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_tasks,
                                                       const uint32_t* task_seed, const uint32_t* task_entry,
                                                       const uint32_t* task_hit, const uint32_t* task_list_off,
                                                       const uint32_t* raw_off, const uint32_t* cand_pl,
                                                       const uint32_t* cand_cnt, const Obs* start_hits,
                                                       uint32_t* list_cnt, uint32_t* list_ptr, Obs* hits,
                                                       uint32_t hits_cap, uint32_t cap, Counters* ctr) {
  __shared__ Obs stage_all[4][EG3D_K2_STAGE_MAX];
  __shared__ uint32_t wave_total[4];
  __shared__ unsigned long long block_base;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t t = blockIdx.x * 4u + w;
  const bool live = t < n_tasks;  // (wave-uniform; the waves past the last task only take part in the claim)
  Obs* stage = stage_all[w];
  K2Task T;
  T.lane = threadIdx.x & 63;
  uint32_t limit = 0, total = 0, my_cnt = 0;
  if (live) {
    const uint32_t seed = task_seed[t], ea = task_entry[t], h = task_hit[t];
    T.t0 = sd.trk_off[seed];
    T.k = sd.trk_off[seed + 1] - T.t0;
    T.sv0 = T.t0 - sv_base;
    T.hit = start_hits[raw_off[T.sv0 + ea] + h];
    T.start_view = sd.trk_view[T.t0 + ea];
    float ix, iy;
    seed_obs_in_view(sd, T.t0, T.k, T.start_view, ix, iy);
    const float radius = dist(ix, iy, T.hit.x, T.hit.y) * 3.0f;
    T.detsq = radius * radius;
    T.lo = task_list_off[t];
    T.lt_mask = (T.lane == 0) ? 0ull : (~0ull >> (64 - T.lane));
    limit = T.k <= 64u ? cap : 0u;
    total = k2_sweep<false>(s, sd, T, raw_off, cand_pl, cand_cnt, stage, limit, 0u, list_cnt, list_ptr, my_cnt);
  }
  if (T.lane == 0) wave_total[w] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long n = (unsigned long long)wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    block_base = n ? atomicAdd(&ctr->hits_used, n) : 0ull;
  }
  __syncthreads();
  if (!live) return;
  unsigned long long base = block_base;
  for (uint32_t v = 0; v < w; v++) base += wave_total[v];
  const bool fits = base + total <= (unsigned long long)hits_cap;
  if (total <= limit) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (fits)
      for (uint32_t j = T.lane; j < total; j += 64) hits[base + j] = stage[j];
    const uint32_t excl = (uint32_t)wave_incl_scan((int)my_cnt) - my_cnt;
    if (T.lane < T.k) list_ptr[T.lo + T.lane] = (uint32_t)base + excl;
  } else if (fits) {
    (void)k2_sweep<true>(s, sd, T, raw_off, cand_pl, cand_cnt, hits + base, 0xffffffffu, (uint32_t)base, list_cnt, list_ptr, my_cnt);
  }
}

void launch_seed_prep(hipStream_t st, SeedsDev sd, uint32_t seed_begin, uint32_t n_seeds, uint32_t sv_base,
                      uint32_t* sv_seed, int32_t* map_view, uint32_t* map_entry, uint32_t* map_n) {
  if (!n_seeds) return;
  hipLaunchKernelGGL(k_seed_prep, blocks_for(n_seeds, 256), dim3(256), 0, st, sd, seed_begin, n_seeds, sv_base, sv_seed,
                     map_view, map_entry, map_n);
}
void launch_k1_count_raw(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                         uint32_t* raw_cnt) {
  if (!n_sv) return;
  hipLaunchKernelGGL(k1_count_raw, blocks_for(n_sv, 256), dim3(256), 0, st, s, sd, sv_base, n_sv, sv_seed, raw_cnt);
}
void launch_k1(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
               const uint32_t* raw_off, uint32_t* cand_pl, Obs* start_hits, uint32_t* cand_cnt, uint32_t* start_cnt,
               uint32_t* sv_vtx) {
  if (!n_sv) return;
  hipLaunchKernelGGL(k1_seed_candidates, blocks_for((uint64_t)n_sv * 64, 256), dim3(256), 0, st, s, sd, sv_base, n_sv,
                     sv_seed, raw_off, cand_pl, start_hits, cand_cnt, start_cnt, sv_vtx);
}
void launch_task_fill(hipStream_t st, SeedsDev sd, uint32_t sv_base, uint32_t n_sv, const uint32_t* sv_seed,
                      const uint32_t* start_cnt, const uint32_t* task_off, uint32_t* task_seed, uint32_t* task_entry,
                      uint32_t* task_hit, uint32_t* task_k, const uint32_t* sv_vtx, Counters* ctr) {
  if (!n_sv) return;
  hipLaunchKernelGGL(k_task_fill, blocks_for(n_sv, 256), dim3(256), 0, st, sd, sv_base, n_sv, sv_seed, start_cnt,
                     task_off, task_seed, task_entry, task_hit, task_k, sv_vtx, ctr);
}
void launch_k2(hipStream_t st, DevScene s, SeedsDev sd, uint32_t sv_base, uint32_t n_tasks, const uint32_t* task_seed,
               const uint32_t* task_entry, const uint32_t* task_hit, const uint32_t* task_list_off, const uint32_t* raw_off,
               const uint32_t* cand_pl, const uint32_t* cand_cnt, const Obs* start_hits, uint32_t* list_cnt, uint32_t* list_ptr,
               Obs* hits, uint32_t hits_cap, uint32_t stage_cap, Counters* ctr) {
  if (!n_tasks) return;
  hipLaunchKernelGGL(k2_epipolar_hits, blocks_for((uint64_t)n_tasks * 64, 256), dim3(256), 0, st, s, sd, sv_base, n_tasks,
                     task_seed, task_entry, task_hit, task_list_off, raw_off, cand_pl, cand_cnt, start_hits, list_cnt,
                     list_ptr, hits, hits_cap, std::min<uint32_t>(std::max<uint32_t>(stage_cap, 1u), EG3D_K2_STAGE_MAX), ctr);
}

}  // namespace eg3d
