// unit_plan_check.cpp — runs the unit planners of edgegraph3d_amd/csrc/eg3d_unit_plan.h on one case from stdin, without a
// GPU (tests/test_unit_plan.py). Input: kind b e lanes units ramp bound n, then the n entries of the prefix array
// (seeds: trk_off; bounded: prefix(i) = entry i). Output: one "b e" line per unit.
//   seeds    plan_seed_units(prefix, b, e, lanes, units, ramp)
//   bounded  cut_bounded(b, e, units ? units : lanes, prefix, bound), as eg3d_match_polyline_sets / _items call it
#include <cstdio>
#include <iostream>
#include <string>

#include "eg3d_unit_plan.h"

int main() {
  std::string kind;
  uint32_t b = 0, e = 0, bound = 0;
  int lanes = 0, units = 0;
  double ramp = 1.0;
  size_t n = 0;
  if (!(std::cin >> kind >> b >> e >> lanes >> units >> ramp >> bound >> n)) return 2;
  std::vector<uint32_t> prefix(n);
  for (uint32_t& v : prefix)
    if (!(std::cin >> v)) return 2;
  if (b > e || (size_t)e >= n) return 2;  // (every planner reads prefix[b .. e])
  std::vector<eg3d::api::UnitRange> out;
  if (kind == "seeds")
    out = eg3d::api::plan_seed_units(prefix, b, e, lanes, units, ramp);
  else if (kind == "bounded")
    out = eg3d::api::cut_bounded(b, e, units ? (uint32_t)units : (uint32_t)lanes, [&](uint32_t i) { return prefix[i]; }, bound);
  else
    return 2;
  for (const eg3d::api::UnitRange& u : out) printf("%u %u\n", u.b, u.e);
  return 0;
}
