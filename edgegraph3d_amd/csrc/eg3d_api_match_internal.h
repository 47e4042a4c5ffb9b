// eg3d_api_match_internal.h — what the files of the match path share: eg3d_api_match.hip (the seed path's stage A, a call
// as units on lanes), eg3d_api_match_stage_b.hip (stage B), eg3d_api_match_sets.hip (the polyline-set path) and
// eg3d_api_candidates.hip (the stage-A dumps); eg3d_api_sets.hip includes it for the two calls on item ranges. Top to
// bottom: a batch's state; where a call's units put their output (RawVec, HostOut, CallSink, UnitTurn); then, file by file,
// what each of them defines for the others. Host only; the unit planners are in eg3d_unit_plan.h.
#pragma once
#include <sys/mman.h>

#include <condition_variable>
#include <functional>
#include <shared_mutex>

#include "eg3d_api_internal.h"
#include "eg3d_unit_plan.h"

EG3D_API_BEGIN
// One batch (a unit of a call, or a stage-A dump) from stage A to stage B: the seed range, the totals each step read back,
// and the view of stage A's arrays that stage B and the kernels take.
struct BatchState {
  uint32_t b, e, n_seeds, sv_base, n_sv, n_tasks, n_lists, n_hits, n_hyp, n_chains, total_raw;
  uint32_t key0_base;  // added to key[0] of every point (polyline-set path: samples before this batch)
  bool k2_single_pass;  // seed path: K2 claimed its hits from the cursor of b_ctr; hits_cap slots were there (k2_settle)
  uint32_t hits_cap;
  StageAView a;
  SeedsDev sd;
};

// Caller-bound output arrays: malloc/realloc'ed runs that are handed to the caller as they are
// (eg3d_free_edgepoints frees them) — no zero-fill on growth, no final copy.
template <typename T>
struct RawVec {
  T* p = nullptr;
  size_t n = 0, cap = 0;
  RawVec() = default;
  RawVec(const RawVec&) = delete;
  RawVec& operator=(const RawVec&) = delete;
  ~RawVec() { free(p); }
  bool reserve(size_t nc) {  // keeps the contents
    if (nc <= cap) return true;
    T* q;
    const size_t bytes = sizeof(T) * nc;
    if (!p && bytes >= (size_t)(4u << 20)) {
      // large result arrays: 2 MiB-aligned and advised as huge pages — the first touch of a fresh 0.45 GB cloud
      // in 4 KiB pages costs 110 k page faults (measured: the host copy ran at 11-15 GB/s whatever the thread
      // count; 60-80 GB/s with huge pages). Untouched capacity costs nothing, so multi-chunk results reserve
      // their estimated total up front: growing such a block later is the slow case.
      void* m = nullptr;
      if (posix_memalign(&m, (size_t)2 << 20, bytes) != 0) return false;
      (void)madvise(m, bytes, MADV_HUGEPAGE);
      q = (T*)m;
    } else {
      q = (T*)realloc(p, bytes);
      if (!q) return false;
    }
    p = q;
    cap = nc;
    return true;
  }
  bool grow_to(size_t want) {  // keeps the contents
    if (want > cap && !reserve(std::max(want, cap + cap / 2 + 64))) return false;
    n = want;
    return true;
  }
  size_t size() const { return n; }
  T* data() { return p; }
  T& operator[](size_t i) { return p[i]; }
  T* release() {
    T* r = p ? p : (T*)malloc(sizeof(T));
    p = nullptr;
    n = cap = 0;
    return r;
  }
};

// What one unit (a sub-batch of a call: a seed range or a run of polyline sets) adds to the call's totals.
struct HostOut {
  uint64_t n_points = 0, n_obs = 0, n_tasks = 0, n_hyp = 0, n_chains = 0;
  uint32_t flags = 0;
  uint64_t bytes_algorithmic = 0, bytes_vertices = 0;
  float ms[7] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t max_chain_ticks = 0;  // the slowest chain of the expand launches (constant-rate clock)
  int pieces = 0;  // (unit, chunk) pieces placed
};

// Where the units of ONE eg3d_match_* call put their output. Units are computed concurrently on the context's lanes
// (run_pipelined) but PLACED strictly in unit order — the call's cloud is the concatenation of its units' clouds in seed /
// set order, byte for byte what a single batch produces (seeds are independent: plg_matching_from_refpoints.cpp:83-104).
// The order is kept by a turnstile: a unit may place (learn its offsets, reserve its part of the destination) only when
// every earlier unit has placed everything.
//   host calls (device_only == 0): a unit's arrays cross PCIe into its lane's pinned staging area as soon as its k4_emit is
//     done, whatever its turn; once it holds the turn it reserves [p0, p0 + np) x [o0, o0 + no) of the caller-bound arrays,
//     passes the turn on, and copies staging -> destination while the later units are still computing.
//   device-only calls: the unit waits for its turn BEFORE k4_emit, which then writes straight into the owner's output
//     buffers at the unit's offsets (eg3d_last_device_output sees one whole cloud, as before).
struct CallSink {
  eg3d_ctx* owner = nullptr;
  int device_only = 0;
  std::mutex mu;
  std::condition_variable cv;
  uint32_t turn = 0;  // the unit that places next
  bool failed = false;
  int rc = EG3D_OK;
  std::string err;
  // destination of a host call; dst_mu: copiers hold it shared, a (rare) growth of the arrays holds it exclusively
  RawVec<float> X, xy;
  RawVec<uint32_t> pl, seg, key;
  RawVec<uint64_t> off;
  RawVec<int32_t> view;
  std::shared_mutex dst_mu;
  uint64_t n_points = 0, n_obs = 0;          // placed so far
  double weight_total = 0, weight_placed = 0;  // share of the call placed so far (sizes the destination's first allocation)
  int lanes_active = 1;                      // lanes working on the call (shares the host copy threads among them)
  bool keyed_by_sample = false;              // polyline-set calls: key[0] = sample index of the CALL ...
  uint32_t key0_next = 0;                    // ... = samples of the units placed so far + the sample's index in its unit
  HostOut tot;
  void unit_tasks(uint32_t n) {  // (holding the turn)
    if (keyed_by_sample) key0_next += n;
  }

  bool acquire(uint32_t u) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return failed || turn == u; });
    return !failed;
  }
  void release(uint32_t u) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (turn == u) turn = u + 1;
    }
    cv.notify_all();
  }
  void fail(int code, const std::string& text) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!failed) {
        failed = true;
        rc = code;
        err = text;
      }
    }
    cv.notify_all();
  }
  // (holding the turn) reserve np points / no observations of the host destination; w = this piece's share of the call
  bool place_host(uint64_t np, uint64_t no, double w, uint64_t& p0, uint64_t& o0) {
    p0 = n_points;
    o0 = n_obs;
    const uint64_t need_p = p0 + np, need_o = o0 + no;
    if (need_p + 1 > off.cap || need_o > view.cap) {
      // estimated size of the whole call from the share placed so far (virtual until touched; a block that has to grow
      // later is the slow case, so the estimate is generous)
      double f = 1.0;
      if (weight_total > weight_placed + w && weight_placed + w > 0) f = 1.5 * weight_total / (weight_placed + w);
      const size_t rp = (size_t)std::max<double>((double)need_p, f * (double)need_p) + 1;
      const size_t ro = (size_t)std::max<double>((double)need_o, f * (double)need_o) + 1;
      std::unique_lock<std::shared_mutex> lk(dst_mu);
      if (!X.reserve(rp * 3) || !off.reserve(rp + 1) || !key.reserve(rp * 4) || !view.reserve(ro) || !pl.reserve(ro) ||
          !seg.reserve(ro) || !xy.reserve(ro * 2))
        return false;
    }
    n_points = need_p;
    n_obs = need_o;
    weight_placed += w;
    return true;
  }
  void add(const HostOut& h) {
    std::lock_guard<std::mutex> lk(mu);
    tot.n_tasks += h.n_tasks;
    tot.n_hyp += h.n_hyp;
    tot.n_chains += h.n_chains;
    tot.flags |= h.flags;
    tot.bytes_algorithmic += h.bytes_algorithmic;
    tot.pieces += h.pieces;
    tot.max_chain_ticks = std::max(tot.max_chain_ticks, h.max_chain_ticks);
    for (int k = 0; k < 7; k++) tot.ms[k] += h.ms[k];
  }
};

// A unit's pass through the turnstile (it may take the turn several times: once per chunk of an expand stage cut by
// EG3D_MAX_SCRATCH_MB; it passes the turn on exactly once).
struct UnitTurn {
  CallSink& S;
  uint32_t u;
  double weight;       // the unit's share of the call (sum of track lengths / polylines)
  bool held = false, passed = false;
  bool more_parts = false;  // the unit is run as several parts (eg3d_match_polyline_items: a unit cut in two and redone) and
                            // the part in progress is not its last: its tasks are counted, the turn stays with the unit
  bool take() {
    if (held) return true;
    if (passed) return false;
    if (S.owner->tune.test_fail_unit == (int)u + 1) {  // (tests: the failure path of the turnstile)
      g_err = "eg3d: unit failure requested by EG3D_TEST_FAIL_UNIT";
      return false;
    }
    held = S.acquire(u);
    return held;
  }
  void pass() {
    if (passed) return;
    if (!held && !S.acquire(u)) {  // (failed call: nobody waits for a turn any more)
      passed = true;
      return;
    }
    S.release(u);
    held = false;
    passed = true;
  }
  // The unit's last piece is placed: under the turn its tasks are counted into the call (CallSink::unit_tasks), then the
  // turn goes to the next unit. false: the turn could not be taken (another unit of the call failed: its error is the call's).
  bool finish(uint32_t n_tasks) {
    if (!take()) return false;
    S.unit_tasks(n_tasks);
    if (!more_parts) pass();
    return true;
  }
};

// ---- eg3d_api_match.hip ----------------------------------------------------------------------------------------------------
// Stage A of the seed path, queued on the context's stream: K1 + task enumeration + K2 for seeds [B.b, B.e) of a zeroed B.
int run_stage_a(eg3d_ctx* c, BatchState& B);
// K2's verdict on the size of b_hits from the cursor value `used`; *again: K2 was queued again with room.
int k2_settle(eg3d_ctx* c, BatchState& B, unsigned long long used, bool* again);
// B.a from the batch as it stands (a batch of the polyline-set path sets dense_k afterwards).
void fill_stage_a_view(const eg3d_ctx* c, BatchState& B);
// One call = units on lanes: run(lane, unit index, turn, stats) -> status computes one unit; match_call makes the call's
// sink, runs the units (run_pipelined), takes the call's time and hands out the result.
using UnitRunner = std::function<int(eg3d_ctx*, uint32_t, UnitTurn&, HostOut&)>;
int match_call(eg3d_ctx* c, int device_only, bool keyed_by_sample, const std::vector<UnitRange>& units, int lanes,
               eg3d_edgepoints* out, eg3d_stage_times* times, const UnitRunner& run, uint32_t key0_start = 0);
int lanes_for(const eg3d_ctx* c, int device_only);  // lanes of a call when eg3d_set_pipelining / EG3D_PIPELINE_LANES chose none

// ---- eg3d_api_match_stage_b.hip --------------------------------------------------------------------------------------------
// Stage B on the StageAView in B: run_stage_b = count_hypotheses, then run_stage_b_counted (a caller that judges the
// unit's totals first enters there). The output goes to the call's sink in unit order (T), counts and times to H.
int count_hypotheses(eg3d_ctx* c, BatchState& B);
int run_stage_b_counted(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H);
int run_stage_b(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H);

// ---- eg3d_api_match_sets.hip -----------------------------------------------------------------------------------------------
// The caller's matched_polyline_intervals for the duration of ONE call: host arrays are uploaded into the DevBufs
// (released with the call), device arrays are read in place. active: the table holds at least one interval.
struct MatchedCall {
  DevBuf off, sseg, sxy, eseg, exy, bad;
  IvTable dev{};
  bool active = false;
};
int prepare_matched(eg3d_ctx* c, const eg3d_matched_intervals* m, MatchedCall& M);  // every check of `m`, then the upload
// How a call on host polyline sets begins: "<who>: bad arguments" / "<who>: too many rows" (nothing is touched), then,
// once the call has a device, the scene's checks of the sets and their upload (sd: the resident sets).
int open_sets_call(const char* who, const eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e, const void* out);
int prepare_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, SetsDev& sd);
// Stage A of the extractor over items [item_b, item_e) of the resident sets (an item is one entry of pl_ids; a run of whole
// sets is the items of its rows), queued on the context's stream; B is zeroed first.
int run_items_stage_a(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows_total, uint32_t item_b, uint32_t item_e,
                      const IvTable* matched, DevBuf* skip_cnt, DevBuf* drop_cnt, BatchState& B);
// ---- the extractor on item ranges (include/eg3d_sets_device.h; the entry points are in eg3d_api_sets.hip) -----------------
// `sets` is resident and checked, n_rows = n_sets * V, [item_b, item_e) lies inside it.
// count_item_samples: the count pass of k_n1_samples alone over the range, as ONE launch on the context's stream — under
// the intervals of `m` when given. counts_host (may be null) receives the n counts, prefix (may be null) their n + 1
// exclusive prefix sums.
int count_item_samples(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e,
                       const eg3d_matched_intervals* m, uint32_t* counts_host, std::vector<uint32_t>* prefix);
// match_items_call: the cloud of the items' samples, key[0] = sample index within the range + sample_base. Units are item
// ranges cut by the sample counts; c->items_units tells how many, c->items_redone how many of them were cut in two and redone.
int match_items_call(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e, uint32_t sample_base,
                     const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out, eg3d_stage_times* times);
EG3D_API_END
