// eg3d_unit_plan.h — how the range of one eg3d_match_* call is cut into units (the sub-batches run_pipelined puts on the
// lanes), as plain functions of their inputs: no HIP, no context, so tests/unitplan/unit_plan_check.cpp runs them without a
// GPU. Top to bottom: UnitRange; cut_by_weight, the balanced cut; plan_seed_units for a seed range; cut_bounded for runs of
// polyline sets and for item ranges. Every planner returns units that cover [b, e) contiguously, each non-empty.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// (hidden, like the rest of what the drivers share: eg3d_api_internal.h)
namespace eg3d { namespace api __attribute__((visibility("hidden"))) {

struct UnitRange {
  uint32_t b, e;
  double w;
};
// Cuts [b, e) into contiguous units of (nearly) equal weight; cum[i] = weight of items [0, i) (ascending).
template <typename Cum>
std::vector<UnitRange> cut_by_weight(uint32_t b, uint32_t e, uint32_t n_units, Cum cum, double ramp = 1.0) {
  std::vector<UnitRange> out;
  if (b >= e) return out;
  n_units = std::max(1u, std::min(n_units, e - b));
  const double w0 = (double)cum(b), w1 = (double)cum(e);
  // unit i gets a share proportional to ramp^i (1 = equal units; < 1 = the later units are smaller)
  double share_all = 0, share_done = 0, r = 1.0;
  for (uint32_t k = 0; k < n_units; k++, r *= ramp) share_all += r;
  r = 1.0;
  uint32_t at = b;
  for (uint32_t k = 1; k <= n_units && at < e; k++) {
    uint32_t end = e;
    share_done += r;
    r *= ramp;
    if (k < n_units) {
      const double target = w0 + (w1 - w0) * share_done / share_all;
      uint32_t lo = at + 1, hi = e;  // first index whose prefix weight reaches the target (at least one item per unit)
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((double)cum(mid) < target) lo = mid + 1; else hi = mid;
      }
      end = std::min(e - (n_units - k), std::max(at + 1, lo));  // leave an item for each unit still to come
    }
    out.push_back({at, end, (double)cum(end) - (double)cum(at)});
    at = end;
  }
  return out;
}

// Units of the seed range [b, e); trk_off is the seeds' track CSR (its host copy), `units` the caller's EG3D_PIPELINE_UNITS
// (0 = chosen here), `ramp` its EG3D_UNIT_RAMP. One lane: batches of 16 384 seeds (one expand launch each), as before round 6.
// Several lanes: at least one unit per lane when the range is worth cutting (>= 128 seeds per unit), never more than
// 16 384 seeds per unit, balanced by the sum of track lengths (the same weight the multi-GPU sharding uses).
inline std::vector<UnitRange> plan_seed_units(const std::vector<uint32_t>& trk_off, uint32_t b, uint32_t e, int lanes, int units,
                                              double ramp) {
  const uint32_t SEED_BATCH = 16384, MIN_UNIT = 128;
  const uint32_t n = e - b;
  auto cum = [&](uint32_t i) { return (double)trk_off[i] + 1e-3 * (double)i; };  // (+ a little per seed: seeds without tracks still count)
  if (lanes <= 1 && !units) {
    std::vector<UnitRange> out;
    for (uint32_t s0 = b; s0 < e; s0 += SEED_BATCH) {
      const uint32_t s1 = std::min(e, s0 + SEED_BATCH);
      out.push_back({s0, s1, cum(s1) - cum(s0)});
    }
    return out;
  }
  uint32_t n_units = units ? (uint32_t)units : std::min<uint32_t>((uint32_t)lanes, n / MIN_UNIT);
  n_units = std::max(n_units, (n + SEED_BATCH - 1) / SEED_BATCH);
  std::vector<UnitRange> out = cut_by_weight(b, e, std::max(1u, n_units), cum, ramp);
  // (balancing by weight can leave a unit of many short tracks above the batch bound: cut such a unit again)
  for (size_t i = 0; i < out.size();) {
    if (out[i].e - out[i].b > SEED_BATCH) {
      const uint32_t mid = out[i].b + (out[i].e - out[i].b) / 2, end = out[i].e;
      out[i] = {out[i].b, mid, cum(mid) - cum(out[i].b)};
      out.insert(out.begin() + (long)i + 1, {mid, end, cum(end) - cum(mid)});
    } else {
      i++;
    }
  }
  return out;
}

// Units of [b, e) whose weight is bounded: prefix(i) = the 32-bit weight of items [.., i) (polyline ids in front of set i,
// samples in front of item i; ascending). `want` balanced pieces (cut_by_weight, + a little per item: empty ones count),
// each then cut into greedy runs of at most `bound`; a single item above the bound stays alone.
template <typename Prefix>
std::vector<UnitRange> cut_bounded(uint32_t b, uint32_t e, uint32_t want, Prefix prefix, uint32_t bound) {
  auto cum = [&](uint32_t i) { return (double)prefix(i) + 1e-3 * (double)i; };
  std::vector<UnitRange> out;
  for (const UnitRange& r : cut_by_weight(b, e, want, cum))
    for (uint32_t i0 = r.b; i0 < r.e;) {
      uint32_t i1 = i0 + 1;
      while (i1 < r.e && (uint32_t)prefix(i1 + 1) - (uint32_t)prefix(i0) <= bound) i1++;
      out.push_back({i0, i1, cum(i1) - cum(i0)});
      i0 = i1;
    }
  return out;
}

}}  // namespace eg3d::api
