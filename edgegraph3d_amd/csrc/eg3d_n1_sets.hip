// eg3d_n1_sets.hip — gfx950 kernels of the pipelines 1-2 extractor, stage A' feeding the same
// task_setup..k4 stages as the refpoint path:
//   k_n1_samples      1 lane / polyline     a sample every 20 px (count pass + fill pass), 1 task each
//   k_n1_hits         1 lane / task        epiline x the set's polylines of every view (wave-uniform scan), all hits
//   (both <., MATCHED = true> when the caller's matches manager holds intervals: samples and hits inside one are left out,
//    eg3d_matched_core.h; k_n1_check_intervals, 1 lane / polyline, checks the interval table before anything reads it)
// All arithmetic follows the contract in DESIGN.md (no FMA contraction: -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eg3d_dev_pipeline.h"
#include "eg3d_kernels.h"

namespace eg3d {

// ------------------------------------------------------------------ N1 ---------
// Pipelines 1-2 extractor, stage A (polyline_matching.cpp:153-208 with :45-73): every polyline of a
// set is sampled every 20 px from its start towards its end; each sample is one task whose V lists
// are the hits of its epipolar line on the set's polylines of the other views (all hits, no
// radius; the list of its own view is the sample itself).
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
  const uint32_t row = find_owner(sets.row_off, n_rows, item);  // (empty rows skipped by its <=)
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

// one lane per row of the interval table (= per polyline of the scene): check_interval_row; *bad |= 1 where it fails
__global__ void k_n1_check_intervals(DevScene s, IvTable iv, uint64_t total, uint32_t n_pl, uint32_t* bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_pl) return;
  if (!check_interval_row(iv, total, g, s.pl_vtx_off[g + 1] - s.pl_vtx_off[g])) atomicOr(bad, 1u);
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
void launch_n1_check_intervals(hipStream_t st, DevScene s, IvTable iv, uint64_t total, uint32_t n_pl, uint32_t* bad) {
  if (!n_pl) return;
  hipLaunchKernelGGL(k_n1_check_intervals, blocks_for(n_pl, 256), dim3(256), 0, st, s, iv, total, n_pl, bad);
}

}  // namespace eg3d
