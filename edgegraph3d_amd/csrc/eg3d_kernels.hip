// eg3d_kernels.hip — gfx950 kernels of the refpoint -> epipolar match -> triangulate path.
//
// Phase pipeline (DESIGN.md "Kernels"):
//   k_seed_prep       1 lane / seed       view map of the track, (seed,entry) of every track entry
//   k1_count_raw      1 lane / (seed,entry)  upper bound of candidate polylines (sizes the slots)
//   k1_seed_candidates 1 WAVE / (seed,entry) k-way merge of the 30 px grid cells into batches of 64 candidate ids +
//                                           closest-point scan of a batch's segments as one flat sequence
//   k_task_fill       1 lane / (seed,entry)  enumerates (seed, start view, start hit) tasks; sums K1's byte counts
//   k2_epipolar_hits  1 WAVE / task         epiline x the segments of all candidate polylines of a list (flat),
//                                           ballot/popcount ordered compaction (count pass + fill pass)
//   k_task_setup      1 lane / task         3-view selection, hypothesis count
//   k3a_orient, k3a_follow_spec  1 lane / hypothesis, 1 lane / list — the wave SERVES its lanes' triangulation requests
//                                           densely from 64 slots in LDS (eg3d_k3a_engine.h)
//   k3s_select        1 lane / task         uniqueness rule -> chain seeds
//   k3b_expand        1 WAVE / chain        expand-all-views (wave-cooperative Gauss-Newton; eg3d_k3b_expand.h)
//   k4_emit           1 WAVE / chain        ordered SoA output (wave prefix sum of obs counts, flat coalesced copy)
//   k5_gn_filter      1 lane / point        config 5, FP32 Gauss-Newton outlier filter
// Pipelines 1-2 extractor, stage A' feeding the same task_setup..k4 stages:
//   k_n1_samples      1 lane / polyline     a sample every 20 px (count pass + fill pass), 1 task each
//   k_n1_hits         1 lane / task        epiline x the set's polylines of every view (wave-uniform scan), all hits
//   (both <., MATCHED = true> when the caller's matches manager holds intervals: samples and hits inside one are left out,
//    eg3d_matched_core.h; k_n1_check_intervals, 1 lane / polyline, checks the interval table before anything reads it)
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_dev_coopgn.h"
#include "eg3d_kernels.h"

namespace eg3d {

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

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

// ------------------------------------------------------------------ K0 ---------
// Uniform-grid construction on the device (round 6). Behaviour reproduced: PolyLine2DMap ctor +
// polyline::get_intersectedcells_2dmap_set (matching/plg_matching/polyLine_2d_map.cpp:40-58, plgs/polyline_graph_2d.cpp:
// 555-577,819-835): every polyline is sampled from its start every cell / (1.414 + 0.1) px (Euclidean stepping: the walk of
// eg3d_dev_geom.h, the one the kernels use everywhere), samples on a cell boundary are dropped, and each remaining sample's
// cell lists the polyline once. Own design: one lane walks one polyline and emits 64-bit keys (view, cell, polyline) — first
// counted, then written behind an exclusive scan —, a radix sort + unique of the keys IS the per-cell ascending id list,
// and one pass over the unique keys writes the CSR offsets. (host/grid_build.cpp is the same statement for one view on the
// host: the tests compare the two, and both with the oracle.)
#define EG3D_K0_PL_BITS 19 /* a view holds <= 524 288 polylines (eg3d_create refuses more) */
static_assert(EG3D_K0_PL_BITS == EG3D_K0_PL_BITS_HOST, "key layout of the grid builder");
template <bool FILL>
__global__ void k0_grid_pairs(DevScene s, uint32_t n_pl, float cell_dim, int map_w, int map_h, uint32_t* cnt, const uint32_t* off,
                              unsigned long long* keys, uint32_t* dropped) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_pl) return;
  const uint32_t a = s.pl_vtx_off[g], b = s.pl_vtx_off[g + 1];
  uint32_t count = 0;
  if (b - a >= 2) {  // (an invalidated polyline has no vertices on the device)
    uint32_t lo = 0, hi = (uint32_t)s.n_views;  // view of polyline g: last v with view_pl_off[v] <= g
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s.view_pl_off[mid] <= g) lo = mid; else hi = mid;
    }
    const unsigned long long cell_base = (unsigned long long)lo * (unsigned long long)((uint32_t)map_w * (uint32_t)map_h);
    const unsigned long long pl_local = g - s.view_pl_off[lo];
    PlRef pl;
    pl.v = s.vtx + a;
    pl.n = b - a;
    pl.start = s.pl_start[g];
    pl.end = s.pl_end[g];
    const float step = (float)(cell_dim / (1.414 + 0.1));
    const uint32_t direction = pl.end;  // get_other_end(start): end, which equals start for loops (the walk stops at once: Q8)
    const uint32_t base = FILL ? off[g] : 0u;
    bool have_prev = false, pushed = false;
    int32_t prev_c = 0, prev_r = 0;
    uint32_t n_dropped = 0;
    auto visit = [&](const PlPt& p) {
      const CellCoord cc = cell_of(cell_dim, p.x, p.y);
      if (cc.bx || cc.by) return;
      if (have_prev && pushed && cc.col == prev_c && cc.row == prev_r) return;
      if (cc.col < 0 || cc.col >= map_w || cc.row < 0 || cc.row >= map_h) {
        n_dropped++;  // the reference indexes out of bounds here; inputs must keep vertices inside the image
      } else {
        if (FILL) keys[base + count] = ((cell_base + (unsigned long long)(cc.row * map_w + cc.col)) << EG3D_K0_PL_BITS) | pl_local;
        count++;
        pushed = true;
      }
      prev_c = cc.col;
      prev_r = cc.row;
      have_prev = true;
    };
    PlPt cur;
    cur.seg = 0;
    cur.x = pl.v[0].x;
    cur.y = pl.v[0].y;
    visit(cur);
    for (;;) {
      PlPt nx;
      const uint32_t w = walk_by_distance(pl, cur, direction, step, nx);
      visit(nx);
      cur = nx;
      if (w & WALK_EXTREME) break;
    }
    if (!FILL && n_dropped) atomicAdd(dropped, n_dropped);
  }
  if (!FILL) cnt[g] = count;
}
// unique sorted keys -> CSR over (view, cell): off[c] = first key whose cell is >= c, ids = the polyline ids
__global__ void k0_grid_csr(const unsigned long long* keys, uint32_t n, uint32_t total_cells, uint32_t* off, uint32_t* ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const uint32_t cell = (uint32_t)(k >> EG3D_K0_PL_BITS);
  ids[i] = (uint32_t)(k & ((1ull << EG3D_K0_PL_BITS) - 1ull));
  const uint32_t first = i ? (uint32_t)(keys[i - 1] >> EG3D_K0_PL_BITS) + 1u : 0u;
  for (uint32_t c = first; c <= cell; c++) off[c] = i;
  if (i == n - 1)
    for (uint32_t c = cell + 1; c <= total_cells; c++) off[c] = n;
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


// ------------------------------------------------------------------ N1 ---------
// Pipelines 1-2 extractor, stage A (polyline_matching.cpp:153-208 with :45-73): every polyline of a
// set is sampled every 20 px from its start towards its end; each sample is one task whose V lists
// are the hits of its epipolar line on the set's polylines of the other views (all hits, no
// radius; the list of its own view is the sample itself).
__device__ __forceinline__ uint32_t n1_row_of_item(const uint32_t* row_off, uint32_t n_rows, uint32_t item) {
  uint32_t lo = 0, hi = n_rows;  // largest row with row_off[row] <= item (empty rows skipped by <=)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row_off[mid] <= item)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// MATCHED: the caller's PLGMatchesManager holds intervals (eg3d_match_polyline_sets_matched). The lane owns one polyline:
// it loads the bounds of its row of the interval table once and, when the row is empty, does exactly what the MATCHED =
// false form does. Otherwise every 20 px sample is put to is_matched (eg3d_matched_core.h): a matched one is no task, and
// the walk goes on from the end of the interval that holds it (polyline_matching.cpp:175,186-189). Every sample of such
// a polyline must lie strictly further along it than the one before (walk_progresses) — the reference spins where it
// does not; here the polyline stops and CTR_N1_NO_PROGRESS is raised. The count pass and the fill pass run the same walk.
template <bool MATCHED>
struct N1Matched {};  // nothing: the MATCHED = false instantiations carry no argument of it
template <>
struct N1Matched<true> {
  IvTable iv;
  uint32_t* skip_cnt;  // may be null; count pass: [n_items] samples skipped (k_n1_samples), [n_tasks] hits dropped (k_n1_hits)
};
template <bool FILL, bool MATCHED>
__global__ void k_n1_samples(DevScene s, SetsDev sets, uint32_t n_rows, uint32_t item_begin, uint32_t n_items,
                             uint32_t* sample_cnt, const uint32_t* sample_off, Obs* samples, uint32_t* task_seed,
                             uint32_t* task_entry, uint32_t* task_hit, uint32_t* task_list_off, uint32_t* task_row0,
                             Counters* ctr, N1Matched<MATCHED> mt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const uint32_t item = item_begin + i;
  const uint32_t row = n1_row_of_item(sets.row_off, n_rows, item);
  const int view = (int)(row % sets.n_views);
  const uint32_t pl_id = sets.pl_ids[item];
  const PlRef pl = polyline_of(s, view, pl_id);
  uint32_t n = 0;
  if (pl.n >= 2) {
    PlPt p, q;
    p.seg = 0;
    p.x = pl.v[0].x;
    p.y = pl.v[0].y;
    const uint32_t base = FILL ? sample_off[i] : 0u;
    IvRow iv;
    iv.n = 0;
    uint32_t skipped = 0;
    bool first = true;
    PlPt last = p;
    if constexpr (MATCHED) iv = iv_row(mt.iv, s.view_pl_off[view] + pl_id);
    for (;;) {
      const uint32_t w = walk_by_distance(pl, p, pl.end, 20.0f, q);
      if (w & WALK_BAD_DIR) atomicOr(&ctr->flags, 8u);
      if (w & WALK_EXTREME) break;
      if constexpr (MATCHED) {
        if (iv.n) {
          if (!first && !walk_progresses(pl.v, last, q)) {
            atomicOr(&ctr->flags, CTR_N1_NO_PROGRESS);
            break;
          }
          first = false;
          last = q;
          const int32_t k = is_matched(iv, pl.v, q);
          if (k >= 0) {  // jump to the interval's end
            skipped++;
            p.seg = iv.end_seg[k];
            p.x = iv.end_xy[2 * k];
            p.y = iv.end_xy[2 * k + 1];
            continue;
          }
        }
      }
      if (FILL) {
        const uint32_t t = base + n;
        Obs o;
        o.view = view;
        o.pl = pl_id;
        o.seg = q.seg;
        o.x = q.x;
        o.y = q.y;
        samples[t] = o;
        task_seed[t] = t;
        task_entry[t] = (uint32_t)view;
        task_hit[t] = 0;
        task_list_off[t] = t * sets.n_views;
        task_row0[t] = (row / sets.n_views) * sets.n_views;  // first row of the task's set
      }
      n++;
      p = q;
    }
    if constexpr (MATCHED) {
      if (!FILL && mt.skip_cnt) mt.skip_cnt[i] = skipped;
    }
  } else if constexpr (MATCHED) {
    if (!FILL && mt.skip_cnt) mt.skip_cnt[i] = 0;
  }
  if (!FILL) sample_cnt[i] = n;
}

// One LANE per task, 64 consecutive tasks per wavefront. Consecutive tasks are consecutive samples of the same
// polylines, so almost always the whole wave works on ONE set: its lanes are grouped by set, and for every view the
// group scans the set's polylines of that view together — polyline ids, descriptors and vertices are wave-uniform
// (scalar loads, one fetch for 64 tasks), each lane tests the segment against ITS OWN epipolar line and appends its
// hits to ITS OWN list, in polyline and segment order by construction. (Round 1-3 launched one wavefront per
// (task, view) — 64 lanes across the segments, ballot compaction — i.e. 25 waves per task that each fetch the same
// few polylines again: 55.7 ms of the 370 ms C3' sets step; this form: 3.2 ms.)
// MATCHED: a hit inside a held interval of the polyline it lies on is dropped (polyline_matching.cpp:65). The polyline
// scanned is wave-uniform, so the bounds of its row of the interval table are too: read once per polyline on the scalar
// path, and the whole test is skipped for an empty row (the common case). Only a lane that has a hit searches the row.
template <bool FILL, bool MATCHED>
__global__ void __launch_bounds__(256) k_n1_hits(DevScene s, SetsDev sets, uint32_t n_tasks, const Obs* samples,
                                                const uint32_t* task_row0, uint32_t* list_cnt,
                                                const uint32_t* list_ptr, Obs* hits, Counters* ctr,
                                                N1Matched<MATCHED> mt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool have = t < n_tasks;
  const uint32_t V = sets.n_views;
  Obs smp;
  smp.view = 0;
  smp.pl = smp.seg = 0;
  smp.x = smp.y = 0.0f;
  uint32_t row0 = 0xffffffffu;
  if (have) {
    smp = samples[t];
    row0 = task_row0[t];
  }
  unsigned long long bytes = 0;
  uint32_t dropped = 0;
  unsigned long long todo = __ballot(have);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t set_row0 = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)row0, leader, 64));
    const bool mine = have && row0 == set_row0;
    todo &= ~__ballot(mine);
    for (uint32_t cur_view = 0; cur_view < V; cur_view++) {
      const size_t w = (size_t)t * V + cur_view;  // list index = task * V + view
      uint32_t cnt = 0;
      bool scan = false;
      float la = 0.0f, lb = 0.0f, lc = 0.0f;
      uint32_t wbase = 0;
      if (mine) {
        if ((uint32_t)smp.view == cur_view) {
          cnt = 1;
          if (FILL) hits[list_ptr[w]] = smp;
        } else {
          scan = epiline(s.F, s.F_valid, s.n_views, (int)smp.view, (int)cur_view, smp.x, smp.y, la, lb, lc);
          if (FILL && scan) wbase = list_ptr[w];
        }
      }
      if (__any(scan)) {
        const uint32_t row = set_row0 + cur_view;
        const uint32_t c0 = sets.row_off[row], c1 = sets.row_off[row + 1];
        for (uint32_t c = c0; c < c1; c++) {
          const uint32_t pl_id = sets.pl_ids[c];
          const PlRef pl = polyline_of(s, (int)cur_view, pl_id);
          if (scan) bytes += 8ull * pl.n;
          if constexpr (!MATCHED) {
            for (uint32_t ii = 1; ii < pl.n; ii++) {
              const f2 v1 = pl.v[ii], v0 = pl.v[ii - 1];
              float hx = 0.f, hy = 0.f;
              if (scan && seg_line_hit(v1.x, v1.y, v0.x, v0.y, la, lb, lc, hx, hy)) {  // (v[i], v[i-1]), tagged i-1: Q10
                if (FILL) {
                  Obs o;
                  o.view = cur_view;
                  o.pl = pl_id;
                  o.seg = ii - 1;
                  o.x = hx;
                  o.y = hy;
                  hits[wbase + cnt] = o;
                }
                cnt++;
              }
            }
          } else {
            IvRow iv;
            iv.n = 0;
            {
              const uint32_t g = s.view_pl_off[cur_view] + pl_id;  // wave-uniform, as the two offsets
              const uint64_t r0 = mt.iv.off[g], r1 = mt.iv.off[g + 1];
              if (r1 != r0) iv = iv_row_at(mt.iv, r0, r1);
            }
            // A hit on a polyline that holds intervals is not judged where it is found — each lane finds its hit on another
            // segment, and the row search with its dependent loads would run once per such segment, for one lane at a time —
            // but kept as the lane's PENDING hit and judged when the lane finds its next one on this polyline (rare) or in
            // the turn behind the last segment, where every lane that has one judges it in the same pass. The list order is
            // unchanged: a pending hit is settled before anything behind it is appended.
            bool pend = false;
            uint32_t pseg = 0;
            float px = 0.f, py = 0.f;
            const uint32_t n_it = iv.n ? pl.n + 1 : pl.n;  // (one more turn settles the last pending hit)
            for (uint32_t ii = 1; ii < n_it; ii++) {
              float hx = 0.f, hy = 0.f;
              bool hit = false;
              if (ii < pl.n) {
                const f2 v1 = pl.v[ii], v0 = pl.v[ii - 1];
                hit = scan && seg_line_hit(v1.x, v1.y, v0.x, v0.y, la, lb, lc, hx, hy);  // (v[i], v[i-1]), tagged i-1: Q10
              }
              uint32_t oseg = ii - 1;
              float ox = hx, oy = hy;
              bool out = hit;
              if (iv.n) {
                out = false;
                if (pend && (hit || ii == pl.n)) {  // the one place a hit is judged
                  PlPt ph;
                  ph.seg = pseg;
                  ph.x = px;
                  ph.y = py;
                  pend = false;
                  if (is_matched(iv, pl.v, ph) >= 0) {
                    dropped++;
                  } else {
                    out = true;
                    oseg = pseg;
                    ox = px;
                    oy = py;
                  }
                }
                if (hit) {
                  pend = true;
                  pseg = ii - 1;
                  px = hx;
                  py = hy;
                }
              }
              if (out) {
                if (FILL) {
                  Obs o;
                  o.view = cur_view;
                  o.pl = pl_id;
                  o.seg = oseg;
                  o.x = ox;
                  o.y = oy;
                  hits[wbase + cnt] = o;
                }
                cnt++;
              }
            }
          }
        }
      }
      if (!FILL && mine) list_cnt[w] = cnt;
    }
  }
  if constexpr (MATCHED) {
    if (!FILL && have && mt.skip_cnt) mt.skip_cnt[t] = dropped;
  }
  if (!FILL) {  // algorithmic bytes: the vertices every (task, view) list scanned
    for (int d = 32; d; d >>= 1) bytes += (unsigned long long)__shfl_xor((long long)bytes, d, 64);
    if ((threadIdx.x & 63u) == 0 && bytes) atomicAdd(&ctr->bytes, bytes);
  }
}

// ------------------------------------------------------------------ tasks ------
__global__ void k_task_setup(StageAView a, const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n,
                             TaskDesc* tasks, uint32_t* n_hyp) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_tasks) return;
  TaskDesc d;
  task_setup(a, t, map_view, map_entry, map_n, d);
  tasks[t] = d;
  n_hyp[t] = d.n_hyp;
}

__device__ __forceinline__ uint32_t find_owner(const uint32_t* off, uint32_t n, uint32_t x) {
  // largest t in [0,n) with off[t] <= x (off ascending, off[n] > x)
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ K3a --------
// Hypothesis evaluation: eg3d_k3a_engine.h (k3a_orient, k3a_follow_spec), included below; what it computes is stated
// sequentially by evaluate_hypothesis in eg3d_dev_follow.h (the host simulation of the tests runs that).
#ifndef EG3D_K3A_WAVES
#define EG3D_K3A_WAVES 2 /* waves/SIMD the register allocation of K3a aims at: 256 VGPRs, nothing spills (at 3: 168 VGPRs,
                            86-102 spilled; same speed on C3', K3a 1.50 -> 1.30 ms on C2, half the L2<->fabric traffic) */
#endif
// (which hypotheses are compatible is decided where it is asked, by k3s_select: hyp_compatible in eg3d_dev_follow.h)

}  // namespace eg3d
#include "eg3d_k3a_engine.h"
namespace eg3d {

// ------------------------------------------------------------------ K3s --------
__global__ void k3s_select(uint32_t n_tasks, const uint32_t* hyp_off, const HypResult* res, ChainSeed* seeds_out,
                           uint32_t* valid) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  ChainSeed cs;
  cs.task = t;
  cs.winner = 0;
  cs.pts2_src = 0xffffffffu;
  cs.n1 = 0;
  cs.n2 = 0;
  bool ok = false;
  if (hyp_off[t + 1] > hyp_off[t]) ok = select_task(res, hyp_off[t], hyp_off[t + 1], cs);
  seeds_out[t] = cs;
  valid[t] = ok ? 1u : 0u;
}
__global__ void k_compact_chains(uint32_t n_tasks, const ChainSeed* per_task, const uint32_t* valid,
                                 const uint32_t* chain_off, ChainSeed* chains) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tasks) return;
  if (valid[t]) chains[chain_off[t]] = per_task[t];
}

// ------------------------------------------------------------------ K3b --------
// The expand stage: eg3d_k3b_expand.h.
}  // namespace eg3d
#include "eg3d_k3b_expand.h"
namespace eg3d {

// ------------------------------------------------------------------ K4 ---------
// One wavefront per chain, in OUTPUT order: the chain's packed record (k3b_expand) becomes its slice
// of the ordered SoA cloud. Lanes take consecutive points; the observation offset of each point is
// the chain's base plus a wave prefix sum of the per-point counts; the observations of the record are
// already one flat range, so lane f copies observation f: coalesced 16-byte reads, coalesced rows in
// every output array.
__global__ void __launch_bounds__(64) k4_emit(const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                                              StageBuf stage, const ChainOut* outs, const uint32_t* point_off,
                                              const uint32_t* obs_off_in, uint64_t point_base, uint64_t obs_base,
                                              uint32_t key0_base, float* X, eg3d_off_t* obs_off, int32_t* obs_view,
                                              uint32_t* obs_pl, uint32_t* obs_seg, float* obs_xy, uint32_t* key) {
  const uint32_t j = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const ChainOut co = outs[j];
  const StagePt* spt = stage.pts + co.spt;
  const Obs* sob = stage.obs + co.sobs;
  const TaskDesc d = tasks[chains[j].task];
  const uint64_t pbase = point_base + point_off[j];
  const uint64_t obase = obs_base + obs_off_in[j];
  uint32_t run = 0;  // observations of the points before this group of 64
  for (uint32_t i0 = 0; i0 < co.n_points; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool act = i < co.n_points;
    StagePt p;
    p.nobs = 0;
    p.X[0] = p.X[1] = p.X[2] = 0.f;
    if (act) p = spt[i];
    const uint32_t incl = (uint32_t)wave_incl_scan((int)p.nobs);  // inclusive wave scan of the observation counts
    const uint32_t total = lane_bcast(incl, 63);
    if (act) {
      const uint64_t pi = pbase + i;
      X[3 * pi] = p.X[0];
      X[3 * pi + 1] = p.X[1];
      X[3 * pi + 2] = p.X[2];
      obs_off[pi] = (eg3d_off_t)(obase + run + (incl - p.nobs));
      key[4 * pi] = d.seed + key0_base;
      key[4 * pi + 1] = d.entry;
      key[4 * pi + 2] = d.hit;
      key[4 * pi + 3] = i;
    }
    run += total;
  }
  for (uint32_t f = lane; f < co.n_obs; f += 64) {
    const Obs po = sob[f];
    const uint64_t o = obase + f;
    obs_view[o] = po.view;
    obs_pl[o] = po.pl;
    obs_seg[o] = po.seg;
    *(f2*)(obs_xy + 2 * o) = f2{po.x, po.y};
  }
}

// ------------------------------------------------------------------ K5 ---------
// One lane per point, one block per 256 consecutive points. The block's operands are staged in LDS
// with coalesced loads first: the 3x4 part of every camera matrix (V <= 256) and the block's
// observations, which are one contiguous slice of the CSR (<= K5_OBS_CAP of them; k ~ U[3,10] gives
// ~1.5k). A lane then walks ITS list through ds_reads — lane-strided reads of the CSR straight from
// HBM touch ~7x the cache lines they use, and the per-observation camera matrix is a 48-byte gather.
// Blocks whose slice or rig does not fit fall back to the HBM operands (same arithmetic).
// What bounds it is arithmetic, not memory: the filter's convergence test |d mse| < 5e-10 on FP32 values
// of ~0.25 only fires when the mean-square error repeats EXACTLY, so most points run many of the 30
// iterations, each 2 passes x k rows x (8 correctly rounded FP32 divisions + 60 FP64 multiply-adds and
// conversions). Measured alternatives (same bits, slower): persistent lanes with a flattened
// per-row state machine and a global work counter — the end-of-pass step then diverges on almost every
// trip (4.4 ms vs 3.2 ms per 1 M points).
// Round 6 — lane occupancy (tools/c5_iterations.py: on the 1 M-point workload 62 % of the points run all 30 passes, the
// others stop after 4-10, and k spans 3..10; with points taken in input order a wavefront keeps 0.71 of its lanes busy by
// passes and only 0.41 by residual rows, because every pass runs as long as the longest list among its 64 lanes). The
// block's points are therefore SORTED BY k in LDS (counting sort) before lanes take them: a wavefront's lists have (nearly)
// the same length. 2.83 -> 2.17 ms per 1 M points, vector instructions 1.78e9 -> 1.18e9, measured active-lane fraction
// 0.61 (profiles/r06_c5_rocprof_summary.txt). A point's arithmetic does not depend on the lane that runs it, so the output
// is bit for bit what one lane per point in input order produces.
// Measured and dropped: packing the points still running after 6 / 10 passes into the block's first wavefronts (state
// through LDS, order kept; gauss_newton_f32_span makes the iteration resumable): 2.37 / 2.21 ms against 2.17 without —
// a block of 4 wavefronts rarely empties a whole one (0.62 x 256 points = 2.5 wavefronts), and the freed lanes of a
// partly empty wavefront cost nothing extra.
#define K5_BLOCK 256
#define K5_OBS_CAP 2816
#define K5_VIEW_CAP 256
#define K5_KBUCKETS 65 /* list lengths 0..63 and "64 or more" */
// The body has two instantiations. <uint32_t, true>: host clouds as eg3d_gn_filter uploads them (32-bit offsets with a
// sentinel, validated on the host; ext is empty). <uint64_t, false>: device-resident clouds as the match path leaves them
// (eg3d_device_edgepoints: 64-bit offsets, the last point ends at ext.n_obs), which nothing has validated: a list that
// does not lie inside [0, n_obs] in ascending order, or a view id outside the rig, raises a bit of *ext.flags and the
// point is skipped (no operand is read through a bad index). This form also takes the optional keep mask (a masked
// point takes bucket 0 of the counting sort and costs no arithmetic) and accumulates the histogram of the inliers' list
// lengths where the verdict and k are in registers: LDS bins per block and one 64-bit atomic per non-empty bin for rigs
// of <= K5_VIEW_CAP views, global atomics otherwise (block-uniform). ext.hist has n_views + 2 bins: [k] for k <= n_views,
// [n_views + 1] for longer lists.
#define K5_SKIP 0x8000u /* s_perm: the point is masked out or malformed */
template <typename OffT, bool SENTINEL>
__global__ void __launch_bounds__(K5_BLOCK) k5_gn_filter(const float* cam_P, int n_views, const float* X,
                                                        const OffT* obs_off, const int32_t* obs_view,
                                                        const float* obs_xy, uint64_t n, float gn_max_mse,
                                                        int legacy_abs, float* X_out, uint8_t* inlier,
                                                        K5Ext<SENTINEL> ext) {
  typedef const __attribute__((address_space(3))) float* lds_fp;
  typedef const __attribute__((address_space(3))) int32_t* lds_ip;
  __shared__ float sP[K5_VIEW_CAP * 12];
  __shared__ int32_t sV[K5_OBS_CAP];
  __shared__ float sXY[2 * K5_OBS_CAP];
  __shared__ uint32_t s_cnt[K5_KBUCKETS], s_base[K5_KBUCKETS];
  __shared__ uint16_t s_perm[K5_BLOCK];
  __shared__ uint32_t s_hist[SENTINEL ? 1 : K5_VIEW_CAP + 2];  // (never referenced by the host-cloud form: no LDS there)
  const uint64_t p0 = (uint64_t)blockIdx.x * K5_BLOCK;
  const uint64_t p1 = p0 + K5_BLOCK < n ? p0 + K5_BLOCK : n;
  const uint32_t np = (uint32_t)(p1 - p0);
  // end of point i's list
  auto off_end = [&](uint64_t i) -> OffT {
    if constexpr (SENTINEL)
      return obs_off[i + 1];
    else
      return i + 1 < n ? obs_off[i + 1] : (OffT)ext.n_obs;
  };
  const OffT o0 = obs_off[p0], o1 = off_end(p1 - 1);
  // the block's slice: a 64-bit difference on device clouds, held in 32 bits once it is known to fit the staging area
  bool fits;
  if constexpr (SENTINEL)
    fits = (uint32_t)(o1 - o0) <= K5_OBS_CAP;
  else
    fits = o0 <= o1 && o1 <= ext.n_obs && o1 - o0 <= (OffT)K5_OBS_CAP;
  const uint32_t m = (uint32_t)(o1 - o0);
  const uint32_t t = threadIdx.x;
  const bool staged = n_views <= K5_VIEW_CAP && fits;  // block-uniform
  if (staged) {
    for (uint32_t q = t; q < (uint32_t)n_views * 12u; q += K5_BLOCK) sP[q] = cam_P[(q / 12u) * 16u + q % 12u];
    if constexpr (SENTINEL) {
      for (uint32_t q = t; q < m; q += K5_BLOCK) sV[q] = obs_view[o0 + q];
    } else {
      bool bad_view = false;
      for (uint32_t q = t; q < m; q += K5_BLOCK) {
        const int32_t v = obs_view[o0 + q];
        const bool bad = (uint32_t)v >= (uint32_t)n_views;
        bad_view |= bad;
        sV[q] = bad ? 0 : v;
      }
      if (bad_view) atomicOr(ext.flags, K5_FLAG_BAD_VIEW);
    }
    for (uint32_t q = t; q < 2u * m; q += K5_BLOCK) sXY[q] = obs_xy[2 * (size_t)o0 + q];
  }
  if (t < K5_KBUCKETS) s_cnt[t] = 0;
  if constexpr (!SENTINEL) {
    if (n_views <= K5_VIEW_CAP)
      for (uint32_t q = t; q < (uint32_t)n_views + 2u; q += K5_BLOCK) s_hist[q] = 0;
  }
  __syncthreads();
  // ---- (1) counting sort of the block's points by list length (the order inside a bucket is whatever the LDS atomics
  // give: it decides which lane runs a point, not what the point computes)
  uint32_t kb = 0, rank = 0;
  bool skip = false;
  if (t < np) {
    if constexpr (SENTINEL) {
      const uint32_t k = obs_off[p0 + t + 1] - obs_off[p0 + t];
      kb = k < K5_KBUCKETS - 1 ? k : K5_KBUCKETS - 1;
    } else {
      const OffT a = obs_off[p0 + t], b = off_end(p0 + t);
      bool bad = !(a <= b && b <= ext.n_obs && b - a <= (OffT)K5_MAX_LIST) || (staged && !(a >= o0 && b <= o1));
      if (!bad && !staged) {  // operands come straight from HBM: no view id may index past the rig's cameras
        bool bad_view = false;
        for (OffT q = a; q < b; q++) bad_view |= (uint32_t)obs_view[q] >= (uint32_t)n_views;
        if (bad_view) atomicOr(ext.flags, K5_FLAG_BAD_VIEW);
        bad = bad_view;
      } else if (bad) {
        atomicOr(ext.flags, K5_FLAG_BAD_OFFSETS);
      }
      skip = bad || (ext.keep && !ext.keep[p0 + t]);
      const OffT k = skip ? 0 : b - a;
      kb = k < K5_KBUCKETS - 1 ? (uint32_t)k : K5_KBUCKETS - 1;
    }
    rank = atomicAdd(&s_cnt[kb], 1u);
  }
  __syncthreads();
  if (t < K5_KBUCKETS) {
    uint32_t base = 0;
    for (uint32_t q = 0; q < t; q++) base += s_cnt[q];
    s_base[t] = base;
  }
  __syncthreads();
  if constexpr (SENTINEL) {
    if (t < np) s_perm[s_base[kb] + rank] = (uint16_t)t;
  } else {
    if (t < np) s_perm[s_base[kb] + rank] = (uint16_t)(t | (skip ? K5_SKIP : 0u));
  }
  __syncthreads();
  // ---- lane t takes the t-th point of the sorted order
  auto run_span = [&](uint32_t j, GnF32State& st, int it0, int it1) -> int {
    const uint64_t i = p0 + j;
    const OffT a = obs_off[i], b = off_end(i);
    if (staged)
      return gauss_newton_f32_span((lds_fp)&sP[0], 12, (lds_ip)&sV[0] + (a - o0), (lds_fp)&sXY[0] + 2 * (a - o0), (int)(b - a),
                                   st, legacy_abs != 0, it0, it1);
    return gauss_newton_f32_span(cam_P, 16, obs_view + a, obs_xy + 2 * (size_t)a, (int)(b - a), st, legacy_abs != 0, it0, it1);
  };
  auto finish = [&](uint32_t j, const GnF32State& st, int r) -> bool {  // gauss_newton.cpp:130-133: accepted on the last mse, converged or not
    const uint64_t i = p0 + j;
    const bool ok = r != GN_F32_FAILED && st.last_mse < gn_max_mse;
    const float x0 = X[3 * i], x1 = X[3 * i + 1], x2 = X[3 * i + 2];
    inlier[i] = ok ? 1 : 0;
    X_out[3 * i] = ok ? st.X[0] : x0;
    X_out[3 * i + 1] = ok ? st.X[1] : x1;
    X_out[3 * i + 2] = ok ? st.X[2] : x2;
    return ok;
  };
  if constexpr (SENTINEL) {
    if (t < np) {
      const uint32_t j = s_perm[t];
      const uint64_t i = p0 + j;
      GnF32State st;
      st.X[0] = X[3 * i];
      st.X[1] = X[3 * i + 1];
      st.X[2] = X[3 * i + 2];
      st.last_mse = 0;
      finish(j, st, run_span(j, st, 0, 30));
    }
  } else {
    const bool lds_bins = n_views <= K5_VIEW_CAP;  // block-uniform
    if (t < np) {
      const uint32_t pj = s_perm[t];
      const uint32_t j = pj & (K5_SKIP - 1u);
      const uint64_t i = p0 + j;
      GnF32State st;
      st.X[0] = X[3 * i];
      st.X[1] = X[3 * i + 1];
      st.X[2] = X[3 * i + 2];
      st.last_mse = 0;
      if (pj & K5_SKIP) {
        inlier[i] = 0;
        X_out[3 * i] = st.X[0];
        X_out[3 * i + 1] = st.X[1];
        X_out[3 * i + 2] = st.X[2];
      } else if (finish(j, st, run_span(j, st, 0, 30))) {
        const OffT k = off_end(i) - obs_off[i];
        const uint32_t bin = k <= (OffT)n_views ? (uint32_t)k : (uint32_t)n_views + 1u;
        if (lds_bins)
          atomicAdd(&s_hist[bin], 1u);
        else
          atomicAdd(ext.hist + bin, 1ull);
      }
    }
    if (lds_bins) {
      __syncthreads();
      for (uint32_t q = t; q < (uint32_t)n_views + 2u; q += K5_BLOCK) {
        const uint32_t c = s_hist[q];
        if (c) atomicAdd(ext.hist + q, (unsigned long long)c);
      }
    }
  }
}

// ------------------------------------------------------------------ K6 ---------
// Order-preserving stream compaction of a device-resident cloud (all seven arrays), three launches:
//   k6_compact_count    1 lane / point, K6_BLOCK points per block: surviving points and observations of the block
//   k6_compact_scan     one workgroup: exclusive scan of the block totals, both columns 64-bit, totals appended
//   k6_compact_scatter  1 WAVE / 64 source points (shaped like k4_emit): __ballot + popcount rank the surviving points,
//                       wave_incl_scan gives their observation offsets; then the lanes stride over the wave's contiguous
//                       DESTINATION observation range and each finds its source point by a binary search over the <= 64
//                       offsets the wave holds in LDS — the stores of the five observation arrays are coalesced rows, the
//                       loads are coalesced within every surviving list.
// A list that is not an ascending range inside [0, n_obs], or longer than K5_MAX_LIST, drops its point and raises
// K5_FLAG_BAD_OFFSETS in the count pass (the host then fails the call before anything is scattered).
struct K6Pt {
  bool surv;
  uint32_t k;
  uint64_t a;
};
__device__ __forceinline__ K6Pt k6_point(const CloudView& in, const uint8_t* keep, int32_t min_obs, uint64_t i, bool* bad) {
  K6Pt p{false, 0, 0};
  if (i >= in.n_points) return p;
  const uint64_t a = in.obs_off[i], b = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
  if (!(a <= b && b <= in.n_obs && b - a <= (uint64_t)K5_MAX_LIST)) {
    *bad = true;
    return p;
  }
  p.a = a;
  p.k = (uint32_t)(b - a);
  p.surv = (!keep || keep[i]) && (min_obs < 0 || p.k > (uint32_t)min_obs);
  return p;
}
__global__ void __launch_bounds__(K6_BLOCK) k6_compact_count(CloudView in, const uint8_t* keep, int32_t min_obs,
                                                            unsigned long long* blk, uint32_t* flags) {
  __shared__ uint32_t s_p[K6_BLOCK / 64], s_o[K6_BLOCK / 64];
  const uint32_t t = threadIdx.x, w = t >> 6;
  bool bad = false;
  const K6Pt p = k6_point(in, keep, min_obs, (uint64_t)blockIdx.x * K6_BLOCK + t, &bad);
  if (bad) atomicOr(flags, K5_FLAG_BAD_OFFSETS);
  const uint32_t np = (uint32_t)__popcll(__ballot(p.surv));
  const uint32_t no = lane_bcast((uint32_t)wave_incl_scan((int)(p.surv ? p.k : 0u)), 63);  // <= 64 x 2^24
  if ((t & 63u) == 0) {
    s_p[w] = np;
    s_o[w] = no;
  }
  __syncthreads();
  if (t == 0) {
    unsigned long long sp = 0, so = 0;
    for (uint32_t q = 0; q < K6_BLOCK / 64; q++) {
      sp += s_p[q];
      so += s_o[q];
    }
    blk[2 * (uint64_t)blockIdx.x] = sp;
    blk[2 * (uint64_t)blockIdx.x + 1] = so;
  }
}
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long u = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += u;
  }
  return v;
}
__global__ void __launch_bounds__(1024) k6_compact_scan(uint64_t n_blocks, unsigned long long* blk) {
  __shared__ unsigned long long s_p[16], s_o[16];
  const uint32_t t = threadIdx.x, w = t >> 6;
  unsigned long long base_p = 0, base_o = 0;
  for (uint64_t c0 = 0; c0 < n_blocks; c0 += 1024) {
    const uint64_t i = c0 + t;
    const unsigned long long vp = i < n_blocks ? blk[2 * i] : 0, vo = i < n_blocks ? blk[2 * i + 1] : 0;
    const unsigned long long ip = wave_incl_scan_u64(vp), io = wave_incl_scan_u64(vo);
    if ((t & 63u) == 63u) {
      s_p[w] = ip;
      s_o[w] = io;
    }
    __syncthreads();
    unsigned long long pre_p = 0, pre_o = 0, tot_p = 0, tot_o = 0;
    for (uint32_t q = 0; q < 16; q++) {
      if (q < w) {
        pre_p += s_p[q];
        pre_o += s_o[q];
      }
      tot_p += s_p[q];
      tot_o += s_o[q];
    }
    if (i < n_blocks) {
      blk[2 * i] = base_p + pre_p + ip - vp;
      blk[2 * i + 1] = base_o + pre_o + io - vo;
    }
    base_p += tot_p;
    base_o += tot_o;
    __syncthreads();
  }
  if (t == 0) {
    blk[2 * n_blocks] = base_p;
    blk[2 * n_blocks + 1] = base_o;
  }
}
template <bool NT, typename T>
__device__ __forceinline__ T k6_load(const T* p) {
  if constexpr (NT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}
template <bool NT>
__global__ void __launch_bounds__(K6_BLOCK) k6_compact_scatter(CloudView in, const uint8_t* keep, const float* X_new,
                                                              int32_t min_obs, const unsigned long long* blk, CloudOut out) {
  __shared__ uint32_t s_p[K6_BLOCK / 64], s_o[K6_BLOCK / 64];
  __shared__ uint32_t s_incl[K6_BLOCK / 64][64];  // inclusive sums of the surviving lists of the wave's points
  __shared__ uint64_t s_src[K6_BLOCK / 64][64];   // first source observation of the point minus its exclusive sum
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
  const uint64_t i = (uint64_t)blockIdx.x * K6_BLOCK + t;
  bool bad = false;
  const K6Pt p = k6_point(in, keep, min_obs, i, &bad);
  const unsigned long long mask = __ballot(p.surv);
  const uint32_t prank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  const uint32_t ks = p.surv ? p.k : 0u;
  const uint32_t incl = (uint32_t)wave_incl_scan((int)ks);
  const uint32_t wave_obs = lane_bcast(incl, 63);
  s_incl[w][lane] = incl;
  s_src[w][lane] = p.a - (uint64_t)(incl - ks);
  if (lane == 0) {
    s_p[w] = (uint32_t)__popcll(mask);
    s_o[w] = wave_obs;
  }
  __syncthreads();
  uint64_t pbase = blk[2 * (uint64_t)blockIdx.x], obase = blk[2 * (uint64_t)blockIdx.x + 1];
  for (uint32_t q = 0; q < w; q++) {
    pbase += s_p[q];
    obase += s_o[q];
  }
  if (p.surv) {
    const uint64_t d = pbase + prank;
    const float* xs = X_new ? X_new : in.X;
    out.X[3 * d] = k6_load<NT>(xs + 3 * i);
    out.X[3 * d + 1] = k6_load<NT>(xs + 3 * i + 1);
    out.X[3 * d + 2] = k6_load<NT>(xs + 3 * i + 2);
    out.obs_off[d] = obase + (incl - ks);
    out.key[4 * d] = k6_load<NT>(in.key + 4 * i);
    out.key[4 * d + 1] = k6_load<NT>(in.key + 4 * i + 1);
    out.key[4 * d + 2] = k6_load<NT>(in.key + 4 * i + 2);
    out.key[4 * d + 3] = k6_load<NT>(in.key + 4 * i + 3);
  }
  for (uint32_t f = lane; f < wave_obs; f += 64) {
    uint32_t lo = 0, hi = 63;  // the first lane whose inclusive sum exceeds f (it exists: f < s_incl[w][63])
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_incl[w][mid] > f)
        hi = mid;
      else
        lo = mid + 1;
    }
    const uint64_t so = s_src[w][lo] + f, o = obase + f;
    out.obs_view[o] = k6_load<NT>(in.obs_view + so);
    out.obs_pl[o] = k6_load<NT>(in.obs_pl + so);
    out.obs_seg[o] = k6_load<NT>(in.obs_seg + so);
    *(unsigned long long*)(out.obs_xy + 2 * o) = k6_load<NT>((const unsigned long long*)(in.obs_xy + 2 * so));  // (x, y) as one 8-byte word
  }
}

// ------------------------------------------------------------------ K7 ---------
// The 3 px de-duplication of a device-resident cloud (filter_3d_points_close_2d_array; eg3d_host_filter_close_2d is the
// sequential statement). The first point that touches a cell is always kept (nothing before it occupied the cell), so a
// cell is occupied before point i exactly when a point before i has an observation in it, and
//   keep[i] = some observation of i lies in a valid cell whose SMALLEST touching point index is i.
// Two order-independent passes over a claim map first[n_views x w x h] of point indices (0xFFFFFFFF = untouched):
//   k7_dedup_claim  1 lane / observation: atomicMin(first[cell], index_base + owning point)
//   k7_dedup_keep   8 lanes / point: keep = any observation whose cell holds index_base + point; kept points counted
// The outcome of atomicMin does not depend on arrival order, so the mask is deterministic. Claims persist between calls:
// with index_base = the number of points of the earlier clouds, a cloud is deduplicated against all of them.
// The cell of an observation as cell_of in host/post_steps.cpp: a true float division (correctly rounded in this build),
// the range test written so that NaN fails, truncation toward zero (a coordinate in (-3, 0) lands in cell 0), the range
// test again on the integers. Returns false for an observation without a cell.
__device__ __forceinline__ bool k7_cell(const K7Map& m, int32_t v, float x, float y, uint64_t* cell) {
  const float fx = x / 3.0f, fy = y / 3.0f;
  if (v < 0 || v >= m.n_views || !(fx > -1.0f) || !(fy > -1.0f) || !(fx < (float)m.w) || !(fy < (float)m.h)) return false;
  const int cx = (int)fx, cy = (int)fy;
  if (cx < 0 || cy < 0 || cx >= m.w || cy >= m.h) return false;
  *cell = ((uint64_t)v * (uint64_t)m.h + (uint64_t)cy) * (uint64_t)m.w + (uint64_t)cx;
  return true;
}
// The last point of [lo, hi) whose offset is <= j (lo's is): the owner of observation j, empty lists before it skipped.
// Reads obs_off inside [lo, hi) only, whatever the offsets hold.
__device__ __forceinline__ uint64_t k7_owner(const eg3d_off_t* obs_off, uint64_t lo, uint64_t hi, uint64_t j) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (obs_off[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// Adjacent lanes take adjacent observations: obs_view and the 8-byte (x, y) words load coalesced. The owning point: the
// wave searches the whole offset array once for its first observation (every lane the same addresses), stages the next
// 64 offsets in LDS, and a lane counts how many of them are <= its observation (6 LDS probes). A wave's 64 observations
// span more than 64 points only across empty lists; such a lane falls back to the search over the whole array.
__global__ void __launch_bounds__(K7_BLOCK) k7_dedup_claim(CloudView in, K7Map m, uint32_t index_base) {
  __shared__ uint64_t s_off[K7_BLOCK / 64][64];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
  const uint64_t j0 = (uint64_t)blockIdx.x * K7_BLOCK + (uint64_t)w * 64, j = j0 + lane;
  uint64_t p0 = 0;
  if (j0 < in.n_obs) {
    p0 = k7_owner(in.obs_off, 0, in.n_points, j0);
    const uint64_t q = p0 + 1 + lane;
    s_off[w][lane] = q < in.n_points ? in.obs_off[q] : ~0ull;
  }
  __syncthreads();
  if (j >= in.n_obs) return;
  uint32_t lo = 0, hi = 64;  // the number of staged offsets <= j
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_off[w][mid] <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  uint64_t p = p0 + lo;
  if (lo == 64) p = k7_owner(in.obs_off, p, in.n_points, j);
  if (p == 0 && in.obs_off[0] > j) return;  // (an observation in front of the first list belongs to no point)
  const int32_t v = in.obs_view[j];
  const unsigned long long xy = *(const unsigned long long*)(in.obs_xy + 2 * j);
  uint64_t cell;
  if (!k7_cell(m, v, __uint_as_float((uint32_t)xy), __uint_as_float((uint32_t)(xy >> 32)), &cell)) return;
  const uint32_t id = index_base + (uint32_t)p;
  // most observations are not the first of their cell: an entry only ever decreases, so one that already reads <= id
  // cannot be lowered by this lane and the atomic is skipped (measured: DESIGN_LOG.md, "Dedup on the device")
  if (m.first[cell] <= id) return;
  atomicMin(m.first + cell, id);
}
// 8 lanes per point, 32 points per block: the lists of a C2 / C3' cloud hold 3 to 9 observations, so a group covers its
// list in one or two strides, the 8 groups of a wave read 8 adjacent lists (one contiguous stretch of obs_view / obs_xy),
// and the verdict is one ballot. Against 1 lane / observation + a per-point OR this needs no second owner search and no
// zeroed mask, and writes every byte of the mask exactly once; against 1 lane / point its loads are contiguous per wave
// rather than strided by list. A list that is not an ascending range inside [0, n_obs] raises K5_FLAG_BAD_OFFSETS and
// drops its point. Kept points: ballot + popcount per wave, LDS per block, one atomic per block.
__global__ void __launch_bounds__(K7_BLOCK) k7_dedup_keep(CloudView in, K7Map m, uint32_t index_base, uint8_t* keep,
                                                         unsigned long long* n_kept, uint32_t* flags) {
  __shared__ uint32_t s_n[K7_BLOCK / 64];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u, sub = lane & 7u;
  const uint64_t i = (uint64_t)blockIdx.x * (K7_BLOCK / 8) + (t >> 3);
  bool hit = false;
  if (i < in.n_points) {
    const uint64_t a = in.obs_off[i], b = i + 1 < in.n_points ? in.obs_off[i + 1] : in.n_obs;
    if (!(a <= b && b <= in.n_obs)) {
      if (sub == 0) atomicOr(flags, K5_FLAG_BAD_OFFSETS);
    } else {
      const uint32_t id = index_base + (uint32_t)i;
      for (uint64_t j = a + sub; j < b && !hit; j += 8) {
        const int32_t v = in.obs_view[j];
        const unsigned long long xy = *(const unsigned long long*)(in.obs_xy + 2 * j);
        uint64_t cell;
        if (k7_cell(m, v, __uint_as_float((uint32_t)xy), __uint_as_float((uint32_t)(xy >> 32)), &cell)) hit = m.first[cell] == id;
      }
    }
  }
  const unsigned long long any = __ballot(hit);
  const bool kept = ((any >> (lane & ~7u)) & 0xffull) != 0;
  if (sub == 0 && i < in.n_points) keep[i] = kept ? 1 : 0;
  const uint32_t n = (uint32_t)__popcll(__ballot(kept && sub == 0));
  if (lane == 0) s_n[w] = n;
  __syncthreads();
  if (t == 0) {
    uint32_t sum = 0;
    for (uint32_t q = 0; q < K7_BLOCK / 64; q++) sum += s_n[q];
    if (sum) atomicAdd(n_kept, (unsigned long long)sum);
  }
}

// Exclusive scans of 32-bit counts wrap silently when the total passes 2^32. The counts are
// non-negative, so a wrapped scan is exactly one whose output decreases somewhere: this check runs
// after every scan and ORs into a device flag word that k_publish hands to the host (and clears).
__global__ void k_scan_check(const uint32_t* out, uint64_t n_plus_one, uint32_t* wrapped) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 < n_plus_one && out[i + 1] < out[i]) atomicOr(wrapped, 1u);
}
void launch_scan_check(hipStream_t st, const uint32_t* out, uint64_t n_plus_one, uint32_t* wrapped) {
  hipLaunchKernelGGL(k_scan_check, dim3((unsigned)((n_plus_one + 255) / 256)), dim3(256), 0, st, out, n_plus_one, wrapped);
}

// Small device -> host read-backs (scan totals, counters) without a driver round trip: one wavefront
// copies the listed device words into a mailbox in pinned, GPU-mapped host memory and then stores
// the sequence number the host thread is polling for (system-scope release after system fences).
__global__ void __launch_bounds__(64) k_publish(PubArgs a, uint32_t* mbox, uint32_t seq) {
  uint32_t at = 2;  // [0] sequence number, [1] unused, payload from [2]
  for (int i = 0; i < a.n; i++) {
    for (uint32_t w = threadIdx.x; w < a.words[i]; w += 64) mbox[at + w] = a.src[i][w];
    at += a.words[i];
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < a.n_clear; i++) *a.clear[i] = 0;
    __threadfence_system();
    __hip_atomic_store(mbox, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
void launch_publish(hipStream_t st, const PubArgs& a, uint32_t* mbox_dev, uint32_t seq) {
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, a, mbox_dev, seq);
}

// ------------------------------------------------------------ launch wrappers --
static inline dim3 blocks_for(uint64_t n, uint32_t per_block) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

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
void launch_n1_samples(hipStream_t st, bool fill, DevScene s, SetsDev sets, uint32_t n_rows, uint32_t item_begin,
                       uint32_t n_items, uint32_t* sample_cnt, const uint32_t* sample_off, Obs* samples,
                       uint32_t* task_seed, uint32_t* task_entry, uint32_t* task_hit, uint32_t* task_list_off,
                       uint32_t* task_row0, Counters* ctr, const IvTable* matched, uint32_t* skip_cnt) {
  if (!n_items) return;
  const dim3 grid = blocks_for(n_items, 64);
  if (matched) {
    N1Matched<true> mt;
    mt.iv = *matched;
    mt.skip_cnt = skip_cnt;
    if (fill)
      hipLaunchKernelGGL((k_n1_samples<true, true>), grid, dim3(64), 0, st, s, sets, n_rows, item_begin, n_items,
                         sample_cnt, sample_off, samples, task_seed, task_entry, task_hit, task_list_off, task_row0, ctr, mt);
    else
      hipLaunchKernelGGL((k_n1_samples<false, true>), grid, dim3(64), 0, st, s, sets, n_rows, item_begin, n_items,
                         sample_cnt, sample_off, samples, task_seed, task_entry, task_hit, task_list_off, task_row0, ctr, mt);
    return;
  }
  if (fill)
    hipLaunchKernelGGL((k_n1_samples<true, false>), grid, dim3(64), 0, st, s, sets, n_rows, item_begin,
                       n_items, sample_cnt, sample_off, samples, task_seed, task_entry, task_hit, task_list_off,
                       task_row0, ctr, N1Matched<false>());
  else
    hipLaunchKernelGGL((k_n1_samples<false, false>), grid, dim3(64), 0, st, s, sets, n_rows, item_begin,
                       n_items, sample_cnt, sample_off, samples, task_seed, task_entry, task_hit, task_list_off,
                       task_row0, ctr, N1Matched<false>());
}
void launch_n1_hits(hipStream_t st, bool fill, DevScene s, SetsDev sets, uint32_t n_tasks, const Obs* samples,
                    const uint32_t* task_row0, uint32_t* list_cnt, const uint32_t* list_ptr, Obs* hits, Counters* ctr,
                    const IvTable* matched, uint32_t* drop_cnt) {
  if (!n_tasks) return;
  const dim3 grid = blocks_for(n_tasks, 256);
  if (matched) {
    N1Matched<true> mt;
    mt.iv = *matched;
    mt.skip_cnt = drop_cnt;
    if (fill)
      hipLaunchKernelGGL((k_n1_hits<true, true>), grid, dim3(256), 0, st, s, sets, n_tasks, samples, task_row0, list_cnt,
                         list_ptr, hits, ctr, mt);
    else
      hipLaunchKernelGGL((k_n1_hits<false, true>), grid, dim3(256), 0, st, s, sets, n_tasks, samples, task_row0, list_cnt,
                         list_ptr, hits, ctr, mt);
    return;
  }
  if (fill)
    hipLaunchKernelGGL((k_n1_hits<true, false>), grid, dim3(256), 0, st, s, sets, n_tasks, samples, task_row0,
                       list_cnt, list_ptr, hits, ctr, N1Matched<false>());
  else
    hipLaunchKernelGGL((k_n1_hits<false, false>), grid, dim3(256), 0, st, s, sets, n_tasks, samples, task_row0,
                       list_cnt, list_ptr, hits, ctr, N1Matched<false>());
}
// one lane per row of the interval table (= per polyline of the scene): check_interval_row; *bad |= 1 where it fails
__global__ void k_n1_check_intervals(DevScene s, IvTable iv, uint64_t total, uint32_t n_pl, uint32_t* bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_pl) return;
  if (!check_interval_row(iv, total, g, s.pl_vtx_off[g + 1] - s.pl_vtx_off[g])) atomicOr(bad, 1u);
}
void launch_n1_check_intervals(hipStream_t st, DevScene s, IvTable iv, uint64_t total, uint32_t n_pl, uint32_t* bad) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k_n1_check_intervals, blocks_for(n_pl, 256), dim3(256), 0, st, s, iv, total, n_pl, bad);
}
void launch_task_setup(hipStream_t st, StageAView a, const int32_t* map_view, const uint32_t* map_entry,
                       const uint32_t* map_n, TaskDesc* tasks, uint32_t* n_hyp) {
  if (!a.n_tasks) return;
  hipLaunchKernelGGL(k_task_setup, blocks_for(a.n_tasks, 256), dim3(256), 0, st, a, map_view, map_entry, map_n, tasks,
                     n_hyp);
}
// K3a as a request/serve engine (eg3d_k3a_engine.h): one wavefront per block
void launch_k3a_engine(hipStream_t st, uint32_t orient_waves, uint32_t follow_waves, uint32_t lanes_per_wave, DevScene s,
                       StageAView a, const TaskDesc* tasks, const uint32_t* hyp_off, uint32_t n_hyp, HypResult* res,
                       HPoint* follow_scratch, uint32_t hyp_cap, HPoint* arena, uint32_t arena_cap, Counters* ctr,
                       uint32_t* queue3, uint32_t* items) {
  if (!n_hyp) return;
  hipLaunchKernelGGL(k3a_orient, dim3(orient_waves), dim3(64), 0, st, s, a, tasks, hyp_off, n_hyp, res, hyp_cap, arena,
                     arena_cap, ctr, queue3, lanes_per_wave, items, queue3 + 2);
  hipLaunchKernelGGL(k3a_follow_spec, dim3(follow_waves), dim3(64), 0, st, s, res, follow_scratch, hyp_cap, arena, arena_cap, ctr, queue3 + 1, lanes_per_wave, items, queue3 + 2);
}
void launch_k3s(hipStream_t st, uint32_t n_tasks, const uint32_t* hyp_off, const HypResult* res, ChainSeed* per_task,
                uint32_t* valid) {
  if (!n_tasks) return;
  hipLaunchKernelGGL(k3s_select, blocks_for(n_tasks, 256), dim3(256), 0, st, n_tasks, hyp_off, res, per_task, valid);
}
void launch_compact_chains(hipStream_t st, uint32_t n_tasks, const ChainSeed* per_task, const uint32_t* valid,
                           const uint32_t* chain_off, ChainSeed* chains) {
  if (!n_tasks) return;
  hipLaunchKernelGGL(k_compact_chains, blocks_for(n_tasks, 256), dim3(256), 0, st, n_tasks, per_task, valid, chain_off,
                     chains);
}
#ifdef EG3D_GN_COUNTERS
int gn_dbg_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gn_dbg), sizeof(unsigned long long) * 128) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[128] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_gn_dbg), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
// Three instantiations (round 4), see TeamWaveT: small scenes (50.6 k -> 45 k instructions, 116 instead of 262 spilled
// vector registers), general, many views.
static_assert(EG3D_STAGE_VTX_HOST == EG3D_STAGE_VTX, "the host's small-scene rule must match the side walks' staging capacity");
static_assert(EG3D_GN_PACK_MAX >= EG3D_SMALL_SCENE_VIEWS_HOST, "a small scene's solves must fit a packed round");
static_assert(2 * EG3D_SMALL_SCENE_VIEWS_HOST + 8 <= EG3D_COOP_ROWS && 2 * (EG3D_SMALL_SCENE_VIEWS_HOST + 1) + 8 > EG3D_COOP_ROWS,
              "EG3D_SMALL_SCENE_VIEWS_HOST must be the last view count whose N-view step lists fit LDS");
static constexpr auto k3b_expand_small = k3b_expand_t<EG3D_K3B_WAVES, 0, 0>;
static constexpr auto k3b_expand = k3b_expand_t<EG3D_K3B_WAVES, 0, 1>;
#ifndef EG3D_MANY_WAVES
#define EG3D_MANY_WAVES EG3D_K3B_WAVES /* waves per SIMD of the many-views build (fewer = more registers for kept chunks) */
#endif
static constexpr auto k3b_expand_many = k3b_expand_t<EG3D_MANY_WAVES, EG3D_MANY_KEEP, 2>;
int k3b_blocks_per_cu() {  // the largest residency of the builds sizes the slot pools
  int best = 0;
  for (int k = 0; k < 3; k++) {
    int n = 0;
    const void* f = k == 0 ? (const void*)k3b_expand_small : k == 1 ? (const void*)k3b_expand : (const void*)k3b_expand_many;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 64, 0) != hipSuccess || n < 1) return 0;
    best = n > best ? n : best;
  }
  return best;
}
void launch_pool_init(hipStream_t st, SlotPools pools) {
  hipLaunchKernelGGL(k_pool_init, dim3(8), dim3(256), 0, st, pools);
}
void launch_k3b(hipStream_t st, DevScene s, StageAView a, const TaskDesc* tasks, const ChainSeed* chains,
                uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L,
                unsigned char* slices, SlotPools pools, StageBuf stage, ChainOut* outs, uint32_t* out_points,
                uint32_t* out_obs, Counters* ctr, const uint32_t* order, int scene_class) {
  if (!n_chains) return;
  if (scene_class == 0)
    hipLaunchKernelGGL(k3b_expand_small, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
  else if (scene_class == 2)
    hipLaunchKernelGGL(k3b_expand_many, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
  else
    hipLaunchKernelGGL(k3b_expand, dim3(n_chains), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res,
                       arena, map_view, map_entry, map_n, L, slices, pools, stage, outs, out_points, out_obs, ctr, order);
}
}  // namespace eg3d
// The lane-per-chain engine is a second, slower form of the expand stage: compiled only into builds made with
// -DEG3D_WITH_K3C_ENGINE (edgegraph3d_amd/build.py build_hip_engine -> variants/libeg3d_engine.so); the product libraries
// do not carry it. Its state machine (eg3d_chain_sm.h) stays checked on the host by tests/hostsim.
#ifdef EG3D_WITH_K3C_ENGINE
#include "eg3d_k3c_engine.h"
#endif
namespace eg3d {
#ifdef EG3D_WITH_K3C_ENGINE
// The expand stage as a lane-per-chain engine (eg3d_k3c_engine.h): n_waves single-wavefront blocks whose first
// lanes_per_wave lanes each own a working slice (slices: [n_waves * lanes_per_wave] x L.total bytes) and take chains from
// the launch's queue (*queue zeroed by the caller) until it is empty. long_gn = 0: scenes whose solves all fit a packed
// round of the solver (<= 32 rows); a longer request raises CTR_LONG_REFUSED and the host repeats the launch with 1.
static constexpr auto k3c_engine_short = k3c_engine_t<false>;
static constexpr auto k3c_engine_long = k3c_engine_t<true>;
int k3c_blocks_per_cu() {
  int a = 0, b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, (const void*)k3c_engine_short, 64, 0) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k3c_engine_long, 64, 0) != hipSuccess) return 0;
  return a < b ? a : b;
}
void launch_k3c(hipStream_t st, uint32_t n_waves, uint32_t lanes_per_wave, DevScene s, StageAView a, const TaskDesc* tasks,
                const ChainSeed* chains, uint32_t n_chains, const uint32_t* hyp_off, const HypResult* res, const HPoint* arena,
                const int32_t* map_view, const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L, unsigned char* slices,
                StageBuf stage, ChainOut* outs, uint32_t* out_points, uint32_t* out_obs, Counters* ctr, const uint32_t* order,
                uint32_t* queue, int long_gn) {
  if (!n_chains) return;
  if (long_gn)
    hipLaunchKernelGGL(k3c_engine_long, dim3(n_waves), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res, arena,
                       map_view, map_entry, map_n, L, slices, stage, outs, out_points, out_obs, ctr, order, queue, lanes_per_wave);
  else
    hipLaunchKernelGGL(k3c_engine_short, dim3(n_waves), dim3(64), 0, st, s, a, tasks, chains, n_chains, hyp_off, res, arena,
                       map_view, map_entry, map_n, L, slices, stage, outs, out_points, out_obs, ctr, order, queue, lanes_per_wave);
}
#endif  // EG3D_WITH_K3C_ENGINE
#if defined(EG3D_WITH_K3C_ENGINE) && (defined(EG3D_SECTION_TIMING) || defined(EG3D_K3C_TIMING))
int k3c_dbg_read(unsigned long long* out, int reset) {  // out[128]: g_k3c_dbg[32] then g_k3c_prof[96]
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_k3c_dbg), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_k3c_prof), sizeof(unsigned long long) * 96) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[96] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_k3c_dbg), z, sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_k3c_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
void launch_k0_pairs(hipStream_t st, bool fill, DevScene s, uint32_t n_pl, float cell_dim, int map_w, int map_h, uint32_t* cnt,
                     const uint32_t* off, unsigned long long* keys, uint32_t* dropped) {
  if (!n_pl) return;
  if (fill)
    hipLaunchKernelGGL(k0_grid_pairs<true>, blocks_for(n_pl, 64), dim3(64), 0, st, s, n_pl, cell_dim, map_w, map_h, cnt, off, keys, dropped);
  else
    hipLaunchKernelGGL(k0_grid_pairs<false>, blocks_for(n_pl, 64), dim3(64), 0, st, s, n_pl, cell_dim, map_w, map_h, cnt, off, keys, dropped);
}
void launch_k0_csr(hipStream_t st, const unsigned long long* keys, uint32_t n, uint32_t total_cells, uint32_t* off, uint32_t* ids) {
  if (!n) return;
  hipLaunchKernelGGL(k0_grid_csr, blocks_for(n, 256), dim3(256), 0, st, keys, n, total_cells, off, ids);
}
void launch_collect_overflow(hipStream_t st, const ChainOut* outs, const uint32_t* order, uint32_t n, uint32_t* redo,
                             uint32_t* n_redo, Counters* ctr) {
  if (!n) return;
  hipLaunchKernelGGL(k_collect_overflow, blocks_for(n, 256), dim3(256), 0, st, outs, order, n, redo, n_redo, ctr);
}
void launch_chain_cost(hipStream_t st, StageAView a, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                       uint32_t* cost, uint32_t* idx) {
  if (!n_chains) return;
  hipLaunchKernelGGL(k_chain_cost, blocks_for(n_chains, 256), dim3(256), 0, st, a, tasks, chains, n_chains, cost, idx);
}
void launch_k4(hipStream_t st, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains, StageBuf stage,
               const ChainOut* outs, const uint32_t* point_off, const uint32_t* obs_off_in, uint64_t point_base,
               uint64_t obs_base, uint32_t key0_base, float* X, eg3d_off_t* obs_off, int32_t* obs_view, uint32_t* obs_pl,
               uint32_t* obs_seg, float* obs_xy, uint32_t* key) {
  if (!n_chains) return;
  hipLaunchKernelGGL(k4_emit, dim3(n_chains), dim3(64), 0, st, tasks, chains, n_chains, stage, outs, point_off,
                     obs_off_in, point_base, obs_base, key0_base, X, obs_off, obs_view, obs_pl, obs_seg, obs_xy, key);
}
void launch_k5(hipStream_t st, const float* cam_P, int n_views, const float* X, const uint32_t* obs_off,
               const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
               uint8_t* inlier) {
  if (!n) return;
  hipLaunchKernelGGL((k5_gn_filter<uint32_t, true>), blocks_for(n, K5_BLOCK), dim3(K5_BLOCK), 0, st, cam_P, n_views, X, obs_off,
                     obs_view, obs_xy, n, gn_max_mse, legacy_abs, X_out, inlier, K5Host{});
}
void launch_k5_device(hipStream_t st, const float* cam_P, int n_views, const float* X, const eg3d_off_t* obs_off,
                      const int32_t* obs_view, const float* obs_xy, uint64_t n, float gn_max_mse, int legacy_abs, float* X_out,
                      uint8_t* inlier, K5Dev ext) {
  if (!n) return;
  hipLaunchKernelGGL((k5_gn_filter<eg3d_off_t, false>), blocks_for(n, K5_BLOCK), dim3(K5_BLOCK), 0, st, cam_P, n_views, X,
                     obs_off, obs_view, obs_xy, n, gn_max_mse, legacy_abs, X_out, inlier, ext);
}
void launch_compact_count(hipStream_t st, CloudView in, const uint8_t* keep, int32_t min_obs, unsigned long long* blk,
                          uint32_t* flags) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k6_compact_count, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, min_obs, blk, flags);
}
void launch_compact_scan(hipStream_t st, uint64_t n_blocks, unsigned long long* blk) {
  hipLaunchKernelGGL(k6_compact_scan, dim3(1), dim3(1024), 0, st, n_blocks, blk);
}
void launch_compact_scatter(hipStream_t st, CloudView in, const uint8_t* keep, const float* X_new, int32_t min_obs,
                            const unsigned long long* blk, CloudOut out, bool nt) {
  if (!in.n_points) return;
  if (nt)
    hipLaunchKernelGGL(k6_compact_scatter<true>, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, X_new,
                       min_obs, blk, out);
  else
    hipLaunchKernelGGL(k6_compact_scatter<false>, blocks_for(in.n_points, K6_BLOCK), dim3(K6_BLOCK), 0, st, in, keep, X_new,
                       min_obs, blk, out);
}
void launch_dedup_claim(hipStream_t st, CloudView in, K7Map m, uint32_t index_base) {
  if (!in.n_points || !in.n_obs) return;
  hipLaunchKernelGGL(k7_dedup_claim, blocks_for(in.n_obs, K7_BLOCK), dim3(K7_BLOCK), 0, st, in, m, index_base);
}
void launch_dedup_keep(hipStream_t st, CloudView in, K7Map m, uint32_t index_base, uint8_t* keep, unsigned long long* n_kept,
                       uint32_t* flags) {
  if (!in.n_points) return;
  hipLaunchKernelGGL(k7_dedup_keep, blocks_for(in.n_points, K7_BLOCK / 8), dim3(K7_BLOCK), 0, st, in, m, index_base, keep,
                     n_kept, flags);
}

}  // namespace eg3d
