// eg3d_api_match.hip — the match pipeline of the C ABI (include/eg3d.h): eg3d_match_resident / _refpoints / _polyline_sets,
// the device view of the last call, eg3d_set_pipelining, eg3d_candidates_run. Top to bottom: the D2H ring; stage A; where a
// call's units put their output (CallSink, UnitTurn); stage B as its steps, with run_stage_b as their list; the two kinds of
// batch; one call = units on lanes (run_pipelined); the entry points. Host orchestration only: no kernel and no hipCUB here
// (the scans and the sort of the chain costs are helpers of eg3d_api.hip, declared in eg3d_api_internal.h).
#include <sys/mman.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <shared_mutex>
#include <thread>

#include "eg3d_api_internal.h"
#include "eg3d_host_copy.h"

// D2H ring of a context: EG3D_D2H_RING pinned buffers of `ring_chunk` bytes (run_stage_b) — 16 MB each for a cloud worth it,
// 2 MB each for small ones (pinning memory costs ~0.2 ms per MB: the big ring is a fifth of a small scene's whole call).
// Allocated by the thread that drives the context, normally right after the expand launch, whose run time hides the pinning
// (the cloud's size is then an estimate from the number of chains; a ring that turns out too small for a big cloud is
// replaced once, at copy time).
#ifndef EG3D_D2H_CHUNK
#define EG3D_D2H_CHUNK ((size_t)16 << 20)
#endif
#define EG3D_D2H_CHUNK_SMALL ((size_t)2 << 20)
#define EG3D_D2H_BIG_CLOUD ((size_t)96 << 20) /* bytes of a unit's cloud from which the 16 MB buffers pay */
#ifndef EG3D_D2H_RING
#define EG3D_D2H_RING 4
#endif
static int ensure_d2h_ring(eg3d_ctx* c, size_t cloud_bytes) {
  const size_t want = cloud_bytes >= EG3D_D2H_BIG_CLOUD ? EG3D_D2H_CHUNK : EG3D_D2H_CHUNK_SMALL;
  if (c->pinned && c->ring_chunk >= want) return EG3D_OK;
  if (c->pinned) (void)hipHostFree(c->pinned);
  c->pinned = nullptr;
  c->ring_chunk = c->pinned_cap = 0;
  HIP_TRY(hipHostMalloc(&c->pinned, want * EG3D_D2H_RING, hipHostMallocDefault));
  c->ring_chunk = want;
  c->pinned_cap = want * EG3D_D2H_RING;
  return EG3D_OK;
}

namespace {

struct BatchState {
  uint32_t b, e, n_seeds, sv_base, n_sv, n_tasks, n_lists, n_hits, n_hyp, n_chains, total_raw;
  uint32_t key0_base;  // added to key[0] of every point (polyline-set path: samples before this batch)
  bool k2_single_pass;  // seed path: K2 claimed its hits from the cursor of b_ctr; hits_cap slots were there (k2_settle)
  uint32_t hits_cap;
  StageAView a;
  SeedsDev sd;
};

// K2 of the seed path, queued on the stream: b_hits with room for B.hits_cap hits, the cursor zeroed.
int launch_stage_a_k2(eg3d_ctx* c, BatchState& B) {
  hipStream_t st = c->stream;
  BUF_TRY(c->b_hits.ensure(sizeof(Obs) * ((size_t)B.hits_cap + 1)));
  B.a.hits = c->b_hits.as<Obs>();
  HIP_TRY(hipMemsetAsync(&c->b_ctr.as<Counters>()->hits_used, 0, sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(c->ea[2], st));
  launch_k2(st, c->ds, B.sd, B.sv_base, B.n_tasks, c->b_task_seed.as<uint32_t>(), c->b_task_entry.as<uint32_t>(),
            c->b_task_hit.as<uint32_t>(), c->b_task_list_off.as<uint32_t>(), c->b_raw_off.as<uint32_t>(),
            c->b_cand_pl.as<uint32_t>(), c->b_cand_cnt.as<uint32_t>(), c->b_start_hits.as<Obs>(), c->b_list_cnt.as<uint32_t>(),
            c->b_list_ptr.as<uint32_t>(), c->b_hits.as<Obs>(), B.hits_cap, c->tune.k2_stage_cap, c->b_ctr.as<Counters>());
  HIP_TRY(hipEventRecord(c->eb[2], st));
  return EG3D_OK;
}

// The view of stage A's arrays that stage B and the kernels take, from the batch as it stands. The seed path's batch has
// its tracks in B.sd; the polyline-set path's (a zeroed B.sd, B.b and B.sv_base: no tracks) sets dense_k afterwards.
void fill_stage_a_view(const eg3d_ctx* c, BatchState& B) {
  StageAView& a = B.a;
  a.trk_off = B.sd.trk_off;
  a.trk_view = B.sd.trk_view;
  a.trk_xy = B.sd.trk_xy;
  a.seed_begin = B.b;
  a.sv_base = B.sv_base;
  a.n_tasks = B.n_tasks;
  a.task_seed = c->b_task_seed.as<uint32_t>();
  a.task_entry = c->b_task_entry.as<uint32_t>();
  a.task_hit = c->b_task_hit.as<uint32_t>();
  a.task_list_off = c->b_task_list_off.as<uint32_t>();
  a.list_ptr = c->b_list_ptr.as<uint32_t>();
  a.list_cnt = c->b_list_cnt.as<uint32_t>();
  a.hits = c->b_hits.as<Obs>();
}

// Stage A: K1 + task enumeration + K2. Leaves everything on the device.
int run_stage_a(eg3d_ctx* c, BatchState& B) {
  hipStream_t st = c->stream;
  B.n_seeds = B.e - B.b;
  B.sv_base = c->seeds->trk_off[B.b];
  B.n_sv = c->seeds->trk_off[B.e] - B.sv_base;
  B.sd = c->seeds->dev();
  const uint32_t n_sv = B.n_sv;
  for (DevBuf* w : {&c->b_sv_seed, &c->b_map_view, &c->b_map_entry, &c->b_raw_cnt, &c->b_raw_off, &c->b_cand_cnt, &c->b_start_cnt,
                     &c->b_task_off})  // (one 32-bit word per track entry)
    BUF_TRY(w->ensure(sizeof(uint32_t) * (n_sv + 1)));
  BUF_TRY(c->b_map_n.ensure(sizeof(uint32_t) * (B.n_seeds + 1)));
  BUF_TRY(c->b_ctr.ensure(sizeof(Counters)));
  HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, sizeof(Counters), st));
  launch_seed_prep(st, B.sd, B.b, B.n_seeds, B.sv_base, c->b_sv_seed.as<uint32_t>(), c->b_map_view.as<int32_t>(),
                   c->b_map_entry.as<uint32_t>(), c->b_map_n.as<uint32_t>());
  HIP_TRY(hipMemsetAsync(c->b_raw_cnt.as<uint32_t>() + n_sv, 0, sizeof(uint32_t), st));
  launch_k1_count_raw(st, c->ds, B.sd, B.sv_base, n_sv, c->b_sv_seed.as<uint32_t>(), c->b_raw_cnt.as<uint32_t>());
  BUF_TRY(scan_total_u32(c, c->b_raw_cnt.as<uint32_t>(), c->b_raw_off.as<uint32_t>(), n_sv + 1, B.total_raw, "candidate slots"));
  BUF_TRY(c->b_cand_pl.ensure(sizeof(uint32_t) * (B.total_raw + 1)));
  BUF_TRY(c->b_start_hits.ensure(sizeof(Obs) * (B.total_raw + 1)));
  HIP_TRY(hipMemsetAsync(c->b_start_cnt.as<uint32_t>() + n_sv, 0, sizeof(uint32_t), st));
  HIP_TRY(hipEventRecord(c->ea[1], st));
  launch_k1(st, c->ds, B.sd, B.sv_base, n_sv, c->b_sv_seed.as<uint32_t>(), c->b_raw_off.as<uint32_t>(),
            c->b_cand_pl.as<uint32_t>(), c->b_start_hits.as<Obs>(), c->b_cand_cnt.as<uint32_t>(),
            c->b_start_cnt.as<uint32_t>(), c->b_raw_cnt.as<uint32_t>() /* dead after its scan: reused for K1's vertex counts */);
  HIP_TRY(hipEventRecord(c->eb[1], st));
  BUF_TRY(scan_total_u32(c, c->b_start_cnt.as<uint32_t>(), c->b_task_off.as<uint32_t>(), n_sv + 1, B.n_tasks, "tasks"));
  const uint32_t nt = B.n_tasks;
  for (DevBuf* w : {&c->b_task_seed, &c->b_task_entry, &c->b_task_hit, &c->b_task_k, &c->b_task_list_off})
    BUF_TRY(w->ensure(sizeof(uint32_t) * (nt + 1)));
  HIP_TRY(hipMemsetAsync(c->b_task_k.as<uint32_t>() + nt, 0, sizeof(uint32_t), st));
  launch_task_fill(st, B.sd, B.sv_base, n_sv, c->b_sv_seed.as<uint32_t>(), c->b_start_cnt.as<uint32_t>(),
                   c->b_task_off.as<uint32_t>(), c->b_task_seed.as<uint32_t>(), c->b_task_entry.as<uint32_t>(),
                   c->b_task_hit.as<uint32_t>(), c->b_task_k.as<uint32_t>(), c->b_raw_cnt.as<uint32_t>(), c->b_ctr.as<Counters>());
  BUF_TRY(scan_total_u32(c, c->b_task_k.as<uint32_t>(), c->b_task_list_off.as<uint32_t>(), nt + 1, B.n_lists, "hit lists"));
  BUF_TRY(c->b_list_cnt.ensure(sizeof(uint32_t) * (B.n_lists + 1)));
  BUF_TRY(c->b_list_ptr.ensure(sizeof(uint32_t) * (B.n_lists + 1)));
  HIP_TRY(hipMemsetAsync(c->b_list_cnt.as<uint32_t>() + B.n_lists, 0, sizeof(uint32_t), st));
  // b_hits: what the earlier calls of this context needed per list, or a first guess (C3' has 2.6 hits per list); K2
  // finds out whether it was enough (k2_settle)
  const uint64_t want = c->tune.hits_cap0 && !c->learned.hits_learned ? c->tune.hits_cap0 : (uint64_t)((double)B.n_lists * c->learned.hits_per_list) + 4096;
  B.hits_cap = (uint32_t)std::min<uint64_t>(want, 0xffffffffull);
  B.k2_single_pass = true;
  B.n_hits = 0;
  BUF_TRY(launch_stage_a_k2(c, B));
  fill_stage_a_view(c, B);
  return EG3D_OK;
}

// K2's verdict on the size of b_hits, from the cursor value `used` a read-back brought (B.k2_single_pass). Enough: notes
// what the next call should reserve, *again = false. Not enough: enlarges b_hits to what K2 asked for plus a margin and
// queues K2 again; nothing has read the hits yet, and whatever was derived from the list counts is queued again by the caller.
int k2_settle(eg3d_ctx* c, BatchState& B, unsigned long long used, bool* again) {
  *again = false;
  if (used > 0xffffffffull) return wrapped_error("epipolar hits");
  if (used <= B.hits_cap) {
    B.n_hits = (uint32_t)used;
    if (B.n_lists) c->learned.hits_per_list = std::max(c->learned.hits_per_list, 1.0625 * (double)used / (double)B.n_lists);
    c->learned.hits_learned = true;
    return EG3D_OK;
  }
  if (c->tune.trace_arena)
    fprintf(stderr, "eg3d: epipolar hits: %llu claimed of %u: the buffer is enlarged and K2 runs again\n", used, B.hits_cap);
  B.hits_cap = (uint32_t)std::min<unsigned long long>(used + used / 16 + 64, 0xffffffffull);
  *again = true;
  return launch_stage_a_k2(c, B);
}

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

// ---- stage B: task setup, K3a, K3s, K3b + K4 in chunks --------------------------------------------------------------------
// Consumes the StageAView in B (from the seed path's stage A or from the polyline-set sampler); the output goes to the
// call's sink in unit order (T), the unit's counts and times to H. run_stage_b, below its steps, is the list of them.

// Task setup + hypothesis offsets.
// The number of hypotheses and K2's cursor (seed path) come back in ONE read-back. A b_hits that was too small shows
// here, before anything has read a hit: K2 runs again with room (k2_settle), and the task setup behind it.
int count_hypotheses(eg3d_ctx* c, BatchState& B) {
  hipStream_t st = c->stream;
  const uint32_t nt = B.n_tasks;
  BUF_TRY(c->b_tasks.ensure(sizeof(TaskDesc) * (nt + 1)));
  BUF_TRY(c->b_nhyp.ensure(sizeof(uint32_t) * (nt + 1)));
  BUF_TRY(c->b_hyp_off.ensure(sizeof(uint32_t) * (nt + 1)));
  for (;;) {
    HIP_TRY(hipMemsetAsync(c->b_nhyp.as<uint32_t>() + nt, 0, sizeof(uint32_t), st));
    launch_task_setup(st, B.a, c->b_map_view.as<int32_t>(), c->b_map_entry.as<uint32_t>(), c->b_map_n.as<uint32_t>(),
                      c->b_tasks.as<TaskDesc>(), c->b_nhyp.as<uint32_t>());
    BUF_TRY(scan_queue_u32(c, c->b_nhyp.as<uint32_t>(), c->b_hyp_off.as<uint32_t>(), nt + 1, 0));
    Readback rb(c);
    const int it = rb.add(c->b_hyp_off.as<uint32_t>() + nt, 1);
    const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 1);
    const int ih = B.k2_single_pass ? rb.add(&c->b_ctr.as<Counters>()->hits_used, 2) : -1;
    rb.clear_after(c->b_scanchk.as<uint32_t>());
    BUF_TRY(rb.run());
    bool again = false;
    if (ih >= 0) {
      unsigned long long used;
      memcpy(&used, rb.item(ih), sizeof(used));
      BUF_TRY(k2_settle(c, B, used, &again));
    }
    if (again) continue;
    if (*rb.item(iw)) return wrapped_error("hypotheses");
    B.n_hyp = *rb.item(it);
    return EG3D_OK;
  }
}

// K3a, K3s and the chain scan: follows the hypotheses into the arena, selects per task, leaves the B.n_chains chains of the
// unit compacted in b_chains.
int follow_and_select(eg3d_ctx* c, BatchState& B, HostOut& H) {
  hipStream_t st = c->stream;
  const uint32_t nt = B.n_tasks;
  // ---- K3a
  BUF_TRY(c->b_res.ensure(sizeof(HypResult) * (B.n_hyp + 1)));
  // K3a engine (eg3d_k3a_engine.h): single-wavefront blocks; the lanes of a wave that take work are limited when there
  // is little of it, so that each working lane gets more of the wave's 64 request slots
  const uint32_t eng_waves_max = c->n_simd * (uint32_t)(c->tune.k3a_engine_waves > 0 ? c->tune.k3a_engine_waves : 2);
  uint32_t eng_lanes = 64;
  if (c->tune.k3a_engine_lanes > 0)
    eng_lanes = (uint32_t)std::min(64, c->tune.k3a_engine_lanes);
  else
    while (eng_lanes > 8 && (uint64_t)eng_waves_max * (eng_lanes / 2) >= B.n_hyp) eng_lanes /= 2;
  const uint32_t eng_waves = std::max<uint32_t>(1, std::min<uint32_t>(eng_waves_max, (B.n_hyp + eng_lanes - 1) / eng_lanes));
  BUF_TRY(c->b_fscratch.ensure(sizeof(HPoint) * std::min<uint32_t>(c->learned.hyp_cap, EG3D_K3A_STAGE_POINTS) * ((size_t)eng_waves * 64)));
  BUF_TRY(c->b_queue.ensure(4 * sizeof(uint32_t)));
  BUF_TRY(c->b_items.ensure(sizeof(uint32_t) * 2 * ((size_t)B.n_hyp + 1)));
  // hypothesis arena: 16 points per hypothesis to start with (the seed path uses 0.4-11.6, the polyline-set path 23-24: its
  // first call overflows once), more once an attempt of this context has overflowed (it is redone with room)
  uint32_t arena_cap = std::max<uint32_t>(1u << 16, std::min<uint64_t>((uint64_t)((double)B.n_hyp * c->learned.arena_per_hyp) + 1, 1ull << 26));
  if (c->tune.arena_cap0) arena_cap = c->tune.arena_cap0;  // tests: force the overflow-and-retry path
  Counters hc;
  BUF_TRY(c->b_cs_task.ensure(sizeof(ChainSeed) * (nt + 1)));
  BUF_TRY(c->b_valid.ensure(sizeof(uint32_t) * (nt + 1)));
  BUF_TRY(c->b_chain_off.ensure(sizeof(uint32_t) * (nt + 1)));
  for (int attempt = 0;; attempt++) {
    BUF_TRY(c->b_arena.ensure(sizeof(HPoint) * (size_t)arena_cap));
    HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, 2 * sizeof(uint32_t), st));  // arena_used, flags (keep bytes)
    HIP_TRY(hipEventRecord(c->ea[3], st));
    HIP_TRY(hipMemsetAsync(c->b_queue.p, 0, 4 * sizeof(uint32_t), st));
    launch_k3a_engine(st, eng_waves, eng_waves, eng_lanes, c->ds, B.a, c->b_tasks.as<TaskDesc>(), c->b_hyp_off.as<uint32_t>(),
                      B.n_hyp, c->b_res.as<HypResult>(), c->b_fscratch.as<HPoint>(), c->learned.hyp_cap, c->b_arena.as<HPoint>(),
                      arena_cap, c->b_ctr.as<Counters>(), c->b_queue.as<uint32_t>(), c->b_items.as<uint32_t>());
    HIP_TRY(hipEventRecord(c->eb[3], st));
    // ---- K3s and the chain scan are queued right behind K3a; K3a's counters (arena overflow?) and the
    // number of chains come back in ONE read-back. An overflowing attempt is redone from K3a.
    HIP_TRY(hipMemsetAsync(c->b_valid.as<uint32_t>() + nt, 0, sizeof(uint32_t), st));
    HIP_TRY(hipEventRecord(c->ea[4], st));
    launch_k3s(st, nt, c->b_hyp_off.as<uint32_t>(), c->b_res.as<HypResult>(), c->b_cs_task.as<ChainSeed>(),
               c->b_valid.as<uint32_t>());
    BUF_TRY(scan_queue_u32(c, c->b_valid.as<uint32_t>(), c->b_chain_off.as<uint32_t>(), nt + 1, 0));
    Readback rb(c);
    const int ic = rb.add(c->b_ctr.p, sizeof(Counters) / 4);
    const int it = rb.add(c->b_chain_off.as<uint32_t>() + nt, 1);
    const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 1);
    rb.clear_after(c->b_scanchk.as<uint32_t>());
    BUF_TRY(rb.run());
    memcpy(&hc, rb.item(ic), sizeof(Counters));
    if (c->tune.trace_arena)
      fprintf(stderr, "eg3d: hypothesis arena: %u hypotheses, %u points used of %u (%.2f per hypothesis)%s\n", B.n_hyp,
              hc.arena_used, arena_cap, B.n_hyp ? (double)hc.arena_used / B.n_hyp : 0.0,
              (hc.flags & CTR_ARENA_OVERFLOW) ? " OVERFLOW" : "");
    if (!(hc.flags & CTR_ARENA_OVERFLOW)) {
      if (*rb.item(iw)) return wrapped_error("chains");
      B.n_chains = *rb.item(it);
      break;
    }
    if (attempt >= 6) {
      g_err = "eg3d: hypothesis arena overflow";
      return EG3D_ERR_CAPACITY;
    }
    arena_cap = std::max<uint32_t>(arena_cap * 2, hc.arena_used + (hc.arena_used >> 2));
    if (B.n_hyp) c->learned.arena_per_hyp = std::max(c->learned.arena_per_hyp, 1.25 * (double)arena_cap / (double)B.n_hyp);
  }
  H.flags |= (hc.flags & 0xffu);
  c->k3a_walks_served += hc.k3a_walks_served;
  c->k3a_walk_passes += hc.k3a_walk_passes;
  BUF_TRY(c->b_chains.ensure(sizeof(ChainSeed) * (B.n_chains + 1)));
  launch_compact_chains(st, nt, c->b_cs_task.as<ChainSeed>(), c->b_valid.as<uint32_t>(), c->b_chain_off.as<uint32_t>(),
                        c->b_chains.as<ChainSeed>());
  HIP_TRY(hipEventRecord(c->eb[4], st));
  return EG3D_OK;
}

// What the chunk loop of run_stage_b carries from one expand launch to the next: the chunk, the launch as prepare_expand
// sized it, what launch_expand read back.
struct ExpandState {
  uint32_t c0 = 0, nc = 0;  // the chunk: chains [c0, c0 + nc) of the unit
  // A launch in which some chains outgrew their working slices is followed by a RELAUNCH OF THOSE CHAINS ONLY with larger
  // slices (redo_n of the chunk's nc chains, listed in b_redo[redo_buf]); the others keep their packed results.
  // (Until round 6 the whole chunk was launched again: the first call on a many-view scene ran its expand stage four times —
  // C4: 6.8 s against 1.75 s warm.)
  uint32_t redo_n = 0;
  int redo_buf = 0;
  uint64_t stage_lim_pts = ~0ull, stage_lim_obs = ~0ull;  // EG3D_STAGE_CAP0: what the kernel is told the staging area holds
  // the launch
  ChainLayout L{};
  bool engine = false;  // the lane-per-chain engine (eng_waves x eng_lanes) instead of k3b_expand on the slot pools
  uint32_t eng_waves = 0, eng_lanes = 64;
  SlotPools pools{};
  StageBuf stage{};
  uint32_t n_launch = 0;
  const uint32_t* launch_order = nullptr;
  // what came back
  Counters hc{};
  uint32_t np = 0, no = 0;
  unsigned long long stage_used[2] = {0, 0};
  float ms_expand = 0, ms_emit = 0;
};

// device copy of the byte counter before the chunk
uint32_t* saved_bytes(eg3d_ctx* c) { return c->b_scanchk.as<uint32_t>() + 4; }

// the expand stage's two forms: one wavefront per chain on XCD-affine slots (k3b_expand), or the lane-per-chain
// engine (k3c_engine): n_waves single-wave blocks whose first eng_lanes lanes own a working slice each. Only builds made
// with -DEG3D_WITH_K3C_ENGINE carry the engine; in the others no context selects it (eg3d_create refuses EG3D_K3B_ENGINE=1).
#ifdef EG3D_WITH_K3C_ENGINE
bool engine_selected(const eg3d_ctx* c) { return c->tune.k3b_engine != 0; }
int size_engine(eg3d_ctx* c, ExpandState& X) {
  hipStream_t st = c->stream;
  const ChainLayout& L = X.L;
  const uint32_t per_simd = (uint32_t)(c->tune.k3c_waves > 0 ? c->tune.k3c_waves : std::max(1, c->k3c_per_cu / 4));
  const uint32_t waves_max = c->n_simd * per_simd;
  // owning lanes per wave: 8 by measurement (C3': 2 / 4 / 8 / 16 / 32 / 64 lanes -> 111 / 105 / 103 / 149 / 252 / 397 ms —
  // more lanes buy no parallelism in the lane-private phases and add resident chains, DESIGN_LOG.md round 5)
  X.eng_lanes = c->tune.k3c_lanes > 0 ? (uint32_t)std::min(64, c->tune.k3c_lanes) : 8u;
  X.eng_waves = std::max<uint32_t>(1, std::min<uint32_t>(waves_max, (X.nc + X.eng_lanes - 1) / X.eng_lanes));
  // one working slice per owning lane: keep the arena within 16 GB (many-view scenes have slices of ~1 MB)
  while (X.eng_waves > 64 && L.total * (size_t)X.eng_waves * X.eng_lanes > ((size_t)16 << 30)) X.eng_waves /= 2;
  BUF_TRY(c->b_cscratch.ensure(L.total * (size_t)X.eng_waves * X.eng_lanes));
  BUF_TRY(c->b_queue.ensure(4 * sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(c->b_queue.p, 0, 4 * sizeof(uint32_t), st));
  return EG3D_OK;
}
void launch_engine(eg3d_ctx* c, const BatchState& B, const ExpandState& X) {
  launch_k3c(c->stream, X.eng_waves, X.eng_lanes, c->ds, B.a, c->b_tasks.as<TaskDesc>(), c->b_chains.as<ChainSeed>() + X.c0, X.nc,
             c->b_hyp_off.as<uint32_t>(), c->b_res.as<HypResult>(), c->b_arena.as<HPoint>(), c->b_map_view.as<int32_t>(),
             c->b_map_entry.as<uint32_t>(), c->b_map_n.as<uint32_t>(), X.L, c->b_cscratch.as<unsigned char>(), X.stage,
             c->b_couts.as<ChainOut>(), c->b_cpts.as<uint32_t>(), c->b_cobs.as<uint32_t>(), c->b_ctr.as<Counters>(),
             c->b_order.as<uint32_t>(), c->b_queue.as<uint32_t>(),
             (c->tune.k3b_full || c->learned.k3b_long_latched || (c->V > EG3D_SMALL_SCENE_VIEWS_HOST && !c->tune.assume_short)) ? 1 : 0);
}
#else
bool engine_selected(const eg3d_ctx*) { return false; }
int size_engine(eg3d_ctx*, ExpandState&) { return EG3D_OK; }
void launch_engine(eg3d_ctx*, const BatchState&, const ExpandState&) {}
#endif

// Everything one expand launch needs, queued or allocated: the chunk and its layout, the slot pools (or the engine's grid),
// the staging area, the per-chain output counters, the launch order. A relaunch of the chains listed in b_redo (X.redo_n)
// keeps the chunk, the staging area and the order's buffers of the launch before it.
int prepare_expand(eg3d_ctx* c, const BatchState& B, ExpandState& X) {
  hipStream_t st = c->stream;
  // capacities can grow between chunks (overflow -> retry below), so the layout is per chunk
  X.L = chain_layout(c->learned.chain_cap, c->learned.pool_cap, (uint32_t)c->V);
  const ChainLayout& L = X.L;
  if (!X.redo_n) {
    const size_t max_scratch = c->tune.max_scratch, left = B.n_chains - X.c0;
    X.nc = (uint32_t)std::min<size_t>(left, std::max<size_t>(1, max_scratch ? std::min<size_t>(left, max_scratch / L.total) : left));
  }
  const uint32_t nc = X.nc;
  BUF_TRY(ensure_mailbox(c));
  if (!X.redo_n)
    HIP_TRY(hipMemcpyAsync(saved_bytes(c), &c->b_ctr.as<Counters>()->bytes, sizeof(unsigned long long),
                           hipMemcpyDeviceToDevice, st));
  X.engine = engine_selected(c);
  if (X.engine) {
    BUF_TRY(size_engine(c, X));
  } else {
    SlotPools& pools = X.pools;
    BUF_TRY(c->b_cscratch.ensure(L.total * 8 * (size_t)c->slots_per_xcd));
    pools.slots_per_xcd = c->slots_per_xcd;
    pools.ring_n = 1;
    while (pools.ring_n <= c->slots_per_xcd) pools.ring_n <<= 1;
    pools.stride = 32 + pools.ring_n;
    BUF_TRY(c->b_pools.ensure(sizeof(uint32_t) * 8 * (size_t)pools.stride));
    pools.base = c->b_pools.as<uint32_t>();
    launch_pool_init(st, pools);
  }
  // staging area: what the previous launches needed, or a first guess (an overflowing launch is repeated once
  // with the exact need, which the output scans report). A relaunch of some chains appends to the area as it is.
  if (!X.redo_n) {
    const uint64_t guess_pts = 96ull * nc;
    const uint64_t per_pt = (uint64_t)std::min(100, std::max(8, c->V / 2));
    // (EG3D_STAGE_CAP0, tests: until the context has learned a need the area holds that few points, whatever is allocated)
    const bool cap0 = c->tune.stage_cap0 && !c->learned.stage_cap_pts;
    X.stage_lim_pts = cap0 ? (uint64_t)c->tune.stage_cap0 : ~0ull;
    X.stage_lim_obs = cap0 ? (uint64_t)c->tune.stage_cap0 * per_pt : ~0ull;
    const uint64_t want_pts = cap0 ? X.stage_lim_pts : std::max<uint64_t>(c->learned.stage_cap_pts, guess_pts);
    // (the first guess is capped at 8 GB of observations: a launch that needs more reports its exact need and is
    // repeated once — better than reserving tens of GB per context on a guess for a many-view scene)
    const uint64_t want_obs = cap0 ? X.stage_lim_obs
                                   : std::max<uint64_t>(c->learned.stage_cap_obs, std::min<uint64_t>(guess_pts * per_pt, (8ull << 30) / sizeof(Obs)));
    BUF_TRY(c->b_stage_pts.ensure(sizeof(StagePt) * (size_t)want_pts));
    BUF_TRY(c->b_stage_obs.ensure(sizeof(Obs) * (size_t)want_obs));
    BUF_TRY(c->b_stage_used.ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->b_stage_used.p, 0, 2 * sizeof(unsigned long long), st));
  }
  StageBuf& stage = X.stage;
  stage.pts = c->b_stage_pts.as<StagePt>();
  stage.obs = c->b_stage_obs.as<Obs>();
  stage.cap_pts = std::min<uint64_t>(c->b_stage_pts.cap / sizeof(StagePt), X.stage_lim_pts);
  stage.cap_obs = std::min<uint64_t>(c->b_stage_obs.cap / sizeof(Obs), X.stage_lim_obs);
  stage.used = c->b_stage_used.as<unsigned long long>();
  BUF_TRY(c->b_couts.ensure(sizeof(ChainOut) * (nc + 1)));
  // (per chain: its points and observations and their scans; the cost, its index and the sorted pair of the launch order)
  for (DevBuf* w : {&c->b_cpts, &c->b_cobs, &c->b_cpoff, &c->b_cooff, &c->b_cost, &c->b_cidx, &c->b_cost2, &c->b_order})
    BUF_TRY(w->ensure(sizeof(uint32_t) * (nc + 1)));
  HIP_TRY(hipMemsetAsync(c->b_cpts.as<uint32_t>() + nc, 0, sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(c->b_cobs.as<uint32_t>() + nc, 0, sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, 2 * sizeof(uint32_t), st));
  // longest-first launch order of this chunk's chains (sort by estimated cost, descending)
  X.n_launch = X.redo_n ? X.redo_n : nc;
  X.launch_order = X.redo_n ? c->b_redo[X.redo_buf].as<uint32_t>() : c->b_order.as<uint32_t>();
  if (!X.redo_n) {
    launch_chain_cost(st, B.a, c->b_tasks.as<TaskDesc>(), c->b_chains.as<ChainSeed>() + X.c0, nc, c->b_cost.as<uint32_t>(),
                      c->b_cidx.as<uint32_t>());
    BUF_TRY(sort_pairs_desc_u32(c, c->b_cost.as<uint32_t>(), c->b_cost2.as<uint32_t>(), c->b_cidx.as<uint32_t>(),
                                c->b_order.as<uint32_t>(), nc));
    if (!c->tune.use_lpt)  // identity order (diagnostic): chain j runs in block j
      HIP_TRY(hipMemcpyAsync(c->b_order.p, c->b_cidx.p, sizeof(uint32_t) * nc, hipMemcpyDeviceToDevice, st));
  }
  return EG3D_OK;
}

// The launch, the two output scans behind it, and what they and the kernel's counters say: X.hc, X.np, X.no, X.stage_used.
int launch_expand(eg3d_ctx* c, const BatchState& B, bool device_only, ExpandState& X) {
  hipStream_t st = c->stream;
  const uint32_t nc = X.nc;
  HIP_TRY(hipEventRecord(c->ea[5], st));
  // scene class of the launch: solves of more than 32 rows (EG3D_GN_PACK_MAX) need the builds with the solver's
  // long-request path. Few views normally means none (one observation per view), and the smaller builds run; a point
  // that repeats a view can exceed it — the kernel then raises CTR_LONG_REFUSED and the chunk is redone with the general
  // build (k3b_full latched for the context), like the capacity overflows below.
  const bool general = c->tune.k3b_full || c->learned.k3b_long_latched || c->max_pl_vtx > EG3D_STAGE_VTX_HOST;
  if (X.engine)
    launch_engine(c, B, X);
  else
    launch_k3b(st, c->ds, B.a, c->b_tasks.as<TaskDesc>(), c->b_chains.as<ChainSeed>() + X.c0, X.n_launch,
               c->b_hyp_off.as<uint32_t>(), c->b_res.as<HypResult>(), c->b_arena.as<HPoint>(),
               c->b_map_view.as<int32_t>(), c->b_map_entry.as<uint32_t>(), c->b_map_n.as<uint32_t>(), X.L,
               c->b_cscratch.as<unsigned char>(), X.pools, X.stage, c->b_couts.as<ChainOut>(), c->b_cpts.as<uint32_t>(),
               c->b_cobs.as<uint32_t>(), c->b_ctr.as<Counters>(), X.launch_order,
               general ? 1 : (c->V > EG3D_SMALL_SCENE_VIEWS_HOST && !c->tune.assume_short) ? 2 : 0);
  HIP_TRY(hipEventRecord(c->eb[5], st));
  if (!device_only)  // (first host call of this lane: pinned while the expand kernel runs; ~50 points of ~12 observations per chain)
    BUF_TRY(ensure_d2h_ring(c, (size_t)nc * 50u * (36u + 20u * (size_t)std::min(c->V, 12))));
  // the two output scans are queued right behind K3b; its counters (capacity overflow?) and both totals
  // come back in ONE read-back
  BUF_TRY(scan_queue_u32(c, c->b_cpts.as<uint32_t>(), c->b_cpoff.as<uint32_t>(), nc + 1, 0));
  BUF_TRY(scan_queue_u32(c, c->b_cobs.as<uint32_t>(), c->b_cooff.as<uint32_t>(), nc + 1, 1));
  Readback rb(c);
  const int ic = rb.add(c->b_ctr.p, sizeof(Counters) / 4);
  const int ip = rb.add(c->b_cpoff.as<uint32_t>() + nc, 1);
  const int io = rb.add(c->b_cooff.as<uint32_t>() + nc, 1);
  const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 2);
  const int iu = rb.add(c->b_stage_used.p, 4);  // what the launches of this chunk have packed (two 64-bit counters)
  rb.clear_after(c->b_scanchk.as<uint32_t>());
  rb.clear_after(c->b_scanchk.as<uint32_t>() + 1);
  BUF_TRY(rb.run());
  memcpy(&X.hc, rb.item(ic), sizeof(Counters));
  X.np = *rb.item(ip);
  X.no = *rb.item(io);
  memcpy(X.stage_used, rb.item(iu), sizeof(X.stage_used));
  const bool overflow = X.hc.flags & (EG3D_FLAG_CHAIN_OVERFLOW | EG3D_FLAG_OBS_OVERFLOW);
  if (!overflow && rb.item(iw)[0]) return wrapped_error("edge-points of one chunk");
  if (!overflow && rb.item(iw)[1]) return wrapped_error("observations of one chunk");
  return EG3D_OK;
}

// What a launch is followed by: the chunk's emit (done), every chain of the chunk again (redo_chunk), or the chains
// listed in b_redo[X.redo_buf] again (redo_listed). Either redo keeps X.c0.
enum class Expand { done, redo_chunk, redo_listed };

// Every chain of the chunk again: the byte counter goes back to its value before the chunk.
int redo_whole_chunk(eg3d_ctx* c, ExpandState& X, bool drain) {
  X.redo_n = 0;
  HIP_TRY(hipMemcpyAsync(&c->b_ctr.as<Counters>()->bytes, saved_bytes(c), sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                         c->stream));
  if (drain) HIP_TRY(hipStreamSynchronize(c->stream));
  return EG3D_OK;
}

// The verdict on the launch X describes, from its counters and totals; what a redo needs (the latched build, the learned
// staging need, the doubled capacities, the list of chains) is in place when it returns.
int judge_expand(eg3d_ctx* c, HostOut& H, ExpandState& X, Expand* verdict) {
  hipStream_t st = c->stream;
  const Counters& hc = X.hc;
  const StageBuf& stage = X.stage;
  const uint32_t nc = X.nc, np = X.np, no = X.no;
  const bool overflow = hc.flags & (EG3D_FLAG_CHAIN_OVERFLOW | EG3D_FLAG_OBS_OVERFLOW);
  *verdict = Expand::redo_chunk;
  if (hc.flags & CTR_LONG_REFUSED) {
    // a point of a few-views scene carries more than 32 observations (a view repeated on a track): valid input — the
    // general build solves it. Latch it for the context, restore the byte counter and redo this chunk.
    if (c->learned.k3b_long_latched) {
      g_err = "eg3d: internal: the general build of the expand kernel refused a solve";
      return EG3D_ERR_HIP;
    }
    c->learned.k3b_long_latched = true;
    if (c->tune.trace_arena) fprintf(stderr, "eg3d: expand launch of %u chains redone: a solve of more than 32 rows -> general build\n", nc);
    return redo_whole_chunk(c, X, true);
  }
  if (hc.flags & CTR_SLOT_STARVED) {
    g_err = "eg3d: internal: the expand kernel found no free working slice (slot pool smaller than the residency)";
    return EG3D_ERR_HIP;
  }
  // (the area holds what every launch of the chunk packed — after a relaunch of some chains also their discarded first
  // attempts — so it is the packed totals, not the cloud's, that must fit)
  if (!overflow && (np > stage.cap_pts || no > stage.cap_obs || X.stage_used[0] > stage.cap_pts || X.stage_used[1] > stage.cap_obs)) {
    // the staging area was too small for this launch: its chains were counted but not all packed. Size it
    // for what they need (kept for later calls) and repeat the launch.
    if (c->tune.trace_arena)
      fprintf(stderr, "eg3d: expand launch of %u chains redone: staging area %zu points / %zu observations, needed %u / %u\n", nc,
              (size_t)stage.cap_pts, (size_t)stage.cap_obs, np, no);
    c->learned.stage_cap_pts = std::max<uint64_t>(c->learned.stage_cap_pts, std::max<uint64_t>(np, X.stage_used[0]) + np / 16 + 64);
    c->learned.stage_cap_obs = std::max<uint64_t>(c->learned.stage_cap_obs, std::max<uint64_t>(no, X.stage_used[1]) + no / 16 + 64);
    return redo_whole_chunk(c, X, true);  // (every chain of the chunk again: what was packed does not fit the area as it is)
  }
  // a chain outgrew its working slice: enlarge the capacities (kept for later calls) and redo
  // this chunk; results of the overflowing attempt are discarded
  const bool can_grow = ((hc.flags & EG3D_FLAG_CHAIN_OVERFLOW) && c->learned.chain_cap < 8192) ||
                        ((hc.flags & EG3D_FLAG_OBS_OVERFLOW) && c->learned.pool_cap < (1u << 20));
  if (!can_grow) {  // nothing overflowed — or what did cannot grow any further: the call ends with the flag raised
    X.redo_n = 0;
    *verdict = Expand::done;
    return EG3D_OK;
  }
  if (hc.flags & EG3D_FLAG_CHAIN_OVERFLOW) c->learned.chain_cap *= 2;
  if (hc.flags & EG3D_FLAG_OBS_OVERFLOW) c->learned.pool_cap *= 2;
  H.flags |= hc.flags & 0xffu & ~(uint32_t)(EG3D_FLAG_CHAIN_OVERFLOW | EG3D_FLAG_OBS_OVERFLOW);  // what the chains that keep their results raised
  {
    float t_launch = 0;  // (the launch is over: its counters have been read back)
    HIP_TRY(hipEventElapsedTime(&t_launch, c->ea[5], c->eb[5]));
    X.ms_expand += t_launch;
  }
  uint32_t n_again = 0;
  if (!X.engine) {
    // list the chains of this launch that overflowed (and take their share of the byte counter back)
    const int nb = X.redo_n ? 1 - X.redo_buf : 0;
    BUF_TRY(c->b_redo[nb].ensure(sizeof(uint32_t) * (nc + 1)));
    BUF_TRY(c->b_queue.ensure(4 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->b_queue.p, 0, 4 * sizeof(uint32_t), st));
    launch_collect_overflow(st, c->b_couts.as<ChainOut>(), X.launch_order, X.n_launch, c->b_redo[nb].as<uint32_t>(),
                            c->b_queue.as<uint32_t>(), c->b_ctr.as<Counters>());
    Readback rb(c);
    const int in = rb.add(c->b_queue.p, 1);
    BUF_TRY(rb.run());
    n_again = *rb.item(in);
    X.redo_buf = nb;
  }
  if (c->tune.trace_arena)
    fprintf(stderr, "eg3d: expand launch of %u chains: %u outgrew their slices (flags %u); relaunching %s with %u points / %u "
                    "observation slots per chain\n", X.n_launch, n_again, hc.flags & 3u, n_again ? "those" : "the chunk", c->learned.chain_cap, c->learned.pool_cap);
  if (!n_again) return redo_whole_chunk(c, X, false);  // (the engine form, or nothing listed: the whole chunk again)
  X.redo_n = n_again;
  *verdict = Expand::redo_listed;
  return EG3D_OK;
}

// ---- K4 + placement of this chunk. Device-only calls keep the WHOLE cloud of the call in the OWNER's output buffers
// (unit after unit, chunk after chunk, global observation offsets), so that eg3d_last_device_output is complete whatever
// the cutting — the RCCL gather reads it: the chunk waits for its unit's turn, then k4_emit writes at the call's running
// offsets. Calls that copy to the host emit into the lane's own buffers (chunk-local offsets, rebased on the host below)
// and start the D2H at once; the turn is only needed to learn where the chunk goes in the caller's arrays.
int emit_chunk(eg3d_ctx* c, const BatchState& B, UnitTurn& T, HostOut& H, const ExpandState& X, bool last_chunk) {
  hipStream_t st = c->stream;
  CallSink& S = T.S;
  const uint32_t np = X.np, no = X.no;
  const bool accumulate = S.device_only != 0;
  eg3d_ctx* const oc = accumulate ? S.owner : c;  // whose output buffers k4_emit writes
  size_t P0 = 0, O0 = 0;
  uint32_t key0 = 0;
  if (accumulate) {
    if (!T.take()) return EG3D_ERR_HIP;  // another unit of the call failed: its error is the call's
    P0 = (size_t)S.n_points;
    O0 = (size_t)S.n_obs;
    key0 = S.key0_next + B.key0_base;
  }
  BUF_TRY(oc->o_X.ensure_keep(sizeof(float) * 3 * (P0 + np + 1), sizeof(float) * 3 * P0, st));
  BUF_TRY(oc->o_off.ensure_keep(sizeof(eg3d_off_t) * (P0 + np + 1), sizeof(eg3d_off_t) * P0, st));
  BUF_TRY(oc->o_key.ensure_keep(sizeof(uint32_t) * 4 * (P0 + np + 1), sizeof(uint32_t) * 4 * P0, st));
  BUF_TRY(oc->o_view.ensure_keep(sizeof(int32_t) * (O0 + no + 1), sizeof(int32_t) * O0, st));
  BUF_TRY(oc->o_pl.ensure_keep(sizeof(uint32_t) * (O0 + no + 1), sizeof(uint32_t) * O0, st));
  BUF_TRY(oc->o_seg.ensure_keep(sizeof(uint32_t) * (O0 + no + 1), sizeof(uint32_t) * O0, st));
  BUF_TRY(oc->o_xy.ensure_keep(sizeof(float) * 2 * (O0 + no + 1), sizeof(float) * 2 * O0, st));
  HIP_TRY(hipEventRecord(c->ea[6], st));
  c->learned.stage_cap_pts = std::max<uint64_t>(c->learned.stage_cap_pts, (uint64_t)np + np / 16);  // sizing hint of the next launch
  c->learned.stage_cap_obs = std::max<uint64_t>(c->learned.stage_cap_obs, (uint64_t)no + no / 16);
  launch_k4(st, c->b_tasks.as<TaskDesc>(), c->b_chains.as<ChainSeed>() + X.c0, X.nc, X.stage,
            c->b_couts.as<ChainOut>(), c->b_cpoff.as<uint32_t>(), c->b_cooff.as<uint32_t>(), P0, O0, key0,
            oc->o_X.as<float>(), oc->o_off.as<eg3d_off_t>(), oc->o_view.as<int32_t>(), oc->o_pl.as<uint32_t>(),
            oc->o_seg.as<uint32_t>(), oc->o_xy.as<float>(), oc->o_key.as<uint32_t>());
  HIP_TRY(hipEventRecord(c->eb[6], st));
  H.flags |= (X.hc.flags & 0xffu);
  H.bytes_vertices = X.hc.bytes;  // running total of this batch (K1 + K3b so far)
  H.max_chain_ticks = std::max(H.max_chain_ticks, X.hc.max_chain_ticks);
  if (accumulate) {
    HIP_TRY(hipStreamSynchronize(st));  // k4_emit has written: the next piece may grow / write the owner's buffers
    S.n_points += np;
    S.n_obs += no;
    if (last_chunk && !T.finish(B.n_tasks)) return EG3D_ERR_HIP;
  }
  return EG3D_OK;
}

// A host call's chunk, emitted into the lane's own buffers, goes to the caller's arrays:
// D2H through the lane's RING of pinned buffers (EG3D_D2H_RING of EG3D_D2H_CHUNK bytes, allocated once — behind the
// first expand launch, see ensure_d2h_ring): the seven arrays are cut into pieces of at most one buffer; a piece
// crosses PCIe into a free buffer (async, an event behind it) and is copied on by a few host threads into the
// caller's pageable memory while the next pieces are crossing. (A pageable hipMemcpy runs at ~2 GB/s and made the
// copy 3x the compute time on the dtu006-shaped workload. Until round 6 a whole unit was staged at once: pinning
// that much memory — 0.57 GB for C3' — cost the FIRST call of a context 110-160 ms, twice its kernels.)
int copy_chunk_to_host(eg3d_ctx* c, const BatchState& B, UnitTurn& T, const ExpandState& X, bool last_chunk) {
  hipStream_t st = c->stream;
  CallSink& S = T.S;
  const uint32_t np = X.np, no = X.no, nc = X.nc;
  const double w_piece = T.weight * (double)nc / (double)std::max(1u, B.n_chains);
  const size_t sz[7] = {sizeof(float) * 3 * np, sizeof(eg3d_off_t) * np,   sizeof(uint32_t) * 4 * np, sizeof(int32_t) * no,
                        sizeof(uint32_t) * no,  sizeof(uint32_t) * no,      sizeof(float) * 2 * no};
  const char* src[7] = {(const char*)c->o_X.p,  (const char*)c->o_off.p, (const char*)c->o_key.p, (const char*)c->o_view.p,
                        (const char*)c->o_pl.p, (const char*)c->o_seg.p, (const char*)c->o_xy.p};
  struct Piece {
    int k;
    size_t at, bytes;
  };
  std::vector<Piece> pieces;
  size_t total = 0;
  // (the big observation arrays first)
  static const int order[7] = {6, 3, 4, 5, 2, 1, 0};
  for (int i = 0; i < 7; i++) total += sz[i];
  BUF_TRY(ensure_d2h_ring(c, total));
  const size_t CH = c->ring_chunk;
  for (int i = 0; i < 7; i++) {
    const int k = order[i];
    for (size_t at = 0; at < sz[k]; at += CH) pieces.push_back({k, at, std::min<size_t>(CH, sz[k] - at)});
  }
#ifdef EG3D_COPY_TIMING
  const auto tc0 = std::chrono::steady_clock::now();
#endif
  size_t issued = 0, done = 0;
  auto issue = [&]() -> int {  // the next piece into its ring buffer
    const Piece& q = pieces[issued];
    const int slot = (int)(issued % EG3D_D2H_RING);
    HIP_TRY(hipMemcpyAsync((char*)c->pinned + (size_t)slot * CH, src[q.k] + q.at, q.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(c->ecopy[slot], st));
    issued++;
    return EG3D_OK;
  };
  // the first pieces cross PCIe whatever the unit's turn ...
  while (issued < pieces.size() && issued < EG3D_D2H_RING) BUF_TRY(issue());
  // ... where they go is known once every earlier unit has placed its output
  if (!T.take()) return EG3D_ERR_HIP;
  uint64_t p0 = 0, o0 = 0;
  const bool placed = S.place_host(np, no, w_piece, p0, o0);
  const uint32_t key0_host = S.key0_next + B.key0_base;
  if (last_chunk) T.finish(B.n_tasks);  // the later units place (and copy) while this one copies
  if (!placed) {
    g_err = "eg3d: out of host memory for the edge-point cloud";
    return EG3D_ERR_ARG;
  }
#ifdef EG3D_COPY_TIMING
  const auto tc1 = std::chrono::steady_clock::now();
#endif
  {
    std::shared_lock<std::shared_mutex> lk(S.dst_mu);
    char* dst[7] = {(char*)(S.X.data() + p0 * 3), (char*)(S.off.data() + p0), (char*)(S.key.data() + p0 * 4),
                    (char*)(S.view.data() + o0),  (char*)(S.pl.data() + o0),  (char*)(S.seg.data() + o0),
                    (char*)(S.xy.data() + o0 * 2)};
    while (done < pieces.size()) {
      const Piece& q = pieces[done];
      const int slot = (int)(done % EG3D_D2H_RING);
      HIP_TRY(hipEventSynchronize(c->ecopy[slot]));
      eg3d::copy_mt(dst[q.k] + q.at, (char*)c->pinned + (size_t)slot * CH, q.bytes,
                    c->tune.copy_threads > 0 ? c->tune.copy_threads : std::max(2, EG3D_COPY_THREADS / std::max(1, S.lanes_active)),
                    (size_t)1 << 20);
      done++;
      if (issued < pieces.size()) BUF_TRY(issue());  // the buffer just emptied takes the next piece
    }
    if (o0) {
      uint64_t* off = S.off.data();
      for (size_t i = p0; i < p0 + np; i++) off[i] += (uint64_t)o0;
    }
    if (key0_host) {  // polyline-set calls: key[0] counts the samples of the whole call
      uint32_t* key = S.key.data();
      for (size_t i = p0; i < p0 + np; i++) key[4 * i] += key0_host;
    }
  }
#ifdef EG3D_COPY_TIMING
  const auto tc2 = std::chrono::steady_clock::now();
  fprintf(stderr, "chunk: p0 %zu o0 %zu np %u no %u nc %u  ", (size_t)p0, (size_t)o0, np, no, nc);
  fprintf(stderr, "copy timing: %.1f MB in %zu pieces  first pieces + turn %.2f ms  D2H + host copy %.2f ms\n", total / 1e6, pieces.size(),
          std::chrono::duration<double, std::milli>(tc1 - tc0).count(),
          std::chrono::duration<double, std::milli>(tc2 - tc1).count());
#endif
  return EG3D_OK;
}

// The chunk is out: its launch and emit times, its counts.
int close_chunk(eg3d_ctx* c, HostOut& H, ExpandState& X) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, c->ea[5], c->eb[5]));
  X.ms_expand += t;
  HIP_TRY(hipEventElapsedTime(&t, c->ea[6], c->eb[6]));
  X.ms_emit += t;
  H.n_points += X.np;
  H.n_obs += X.no;
  H.pieces++;
  c->last_np = X.np;  // (the owner's view of the whole call is set when the call ends)
  c->last_no = X.no;
  c->last_nc = X.nc;
  return EG3D_OK;
}

// Stage times and counts of the unit.
int stage_times_and_counts(eg3d_ctx* c, const BatchState& B, HostOut& H, const ExpandState& X) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  float t = 0;
  for (int k = 1; k <= 4; k++) {
    if ((k == 2 && !B.n_tasks) || (k == 3 && !B.n_hyp) || (k == 4 && !B.n_tasks)) continue;
    HIP_TRY(hipEventElapsedTime(&t, c->ea[k], c->eb[k]));
    H.ms[k] += t;
  }
  H.ms[5] += X.ms_expand;
  H.ms[6] += X.ms_emit;
  if (!B.n_chains) {
    Counters hc;
    HIP_TRY(hipMemcpy(&hc, c->b_ctr.p, sizeof(Counters), hipMemcpyDeviceToHost));
    H.bytes_vertices = hc.bytes;
  }
  H.bytes_algorithmic += H.bytes_vertices;
  H.bytes_vertices = 0;
  H.n_tasks += B.n_tasks;
  H.n_hyp += B.n_hyp;
  c->last_nhyp = B.n_hyp;
  H.n_chains += B.n_chains;
  return EG3D_OK;
}

// (the steps behind count_hypotheses: a caller that judges the unit's totals first — run_items_part — enters here)
int run_stage_b_counted(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H);
int run_stage_b(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H) {
  BUF_TRY(count_hypotheses(c, B));
  return run_stage_b_counted(c, B, T, H);
}
int run_stage_b_counted(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H) {
  const bool device_only = T.S.device_only != 0;
  BUF_TRY(follow_and_select(c, B, H));
  // ---- K3b + K4. One launch takes all the chains of the batch: their working slices are slots of a fixed arena
  // (8 XCDs x slots_per_xcd), so nothing grows with the number of chains but the staging area the finished chains
  // are packed into. (EG3D_MAX_SCRATCH_MB, a test knob, still cuts the chains into several launches.)
  ExpandState X;
  while (X.c0 < B.n_chains) {
    BUF_TRY(prepare_expand(c, B, X));
    BUF_TRY(launch_expand(c, B, device_only, X));
    Expand verdict;
    BUF_TRY(judge_expand(c, H, X, &verdict));
    if (verdict != Expand::done) continue;  // the same chunk again, whole or the chains listed: c0 stays
    const bool last_chunk = X.c0 + X.nc >= B.n_chains;
    BUF_TRY(emit_chunk(c, B, T, H, X, last_chunk));
    if (!device_only) {
      if (X.np)
        BUF_TRY(copy_chunk_to_host(c, B, T, X, last_chunk));
      else if (last_chunk && !T.finish(B.n_tasks))
        return EG3D_ERR_HIP;
    }
    BUF_TRY(close_chunk(c, H, X));
    X.c0 += X.nc;
  }
  if (!B.n_chains && !T.finish(B.n_tasks)) return EG3D_ERR_HIP;  // a unit without chains still takes its turn
  return stage_times_and_counts(c, B, H, X);
}

int run_batch(eg3d_ctx* c, uint32_t b, uint32_t e, UnitTurn& T, HostOut& H) {
  BatchState B;
  memset(&B, 0, sizeof(B));
  B.b = b;
  B.e = e;
  BUF_TRY(run_stage_a(c, B));
  BUF_TRY(run_stage_b(c, B, T, H));
  // per seed 12 + k*12 + k*64 + k(k-1)*72 (the vertices touched and the output were
  // added by stage B)
  for (uint32_t sd_i = b; sd_i < e; sd_i++) {
    const uint64_t k = c->seeds->trk_off[sd_i + 1] - c->seeds->trk_off[sd_i];
    H.bytes_algorithmic += 12 + k * 12 + k * 64 + k * (k - 1) * 72;
  }
  return EG3D_OK;
}

// Pipelines 1-2 extractor, stage A: sample the polylines of sets [set_b, set_e) and
// collect the epipolar hits of every sample; then the common stage B. `sets` is already on the
// device; h_row_off is its host copy of the row offsets.
// `matched` (null: none) is the caller's interval table on the device: samples and hits inside a held interval are left out
// (k_n1_samples / k_n1_hits <., true>); skip_cnt / drop_cnt (may be null) receive the per-polyline / per-task counts of them.
// (the kernels work on items — entries [item_b, item_e) of pl_ids; a run of whole sets is the items of its rows)
int run_items_stage_a(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows_total, uint32_t item_b, uint32_t item_e,
                      const IvTable* matched, DevBuf* skip_cnt, DevBuf* drop_cnt, BatchState& B) {
  hipStream_t st = c->stream;
  const uint32_t V = (uint32_t)c->V;
  memset(&B, 0, sizeof(B));
  B.key0_base = 0;  // (key[0] = sample index of the CALL: the sink adds the samples of the units before this one)
  const uint32_t n_items = item_e - item_b;
  BUF_TRY(c->b_ctr.ensure(sizeof(Counters)));
  HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, sizeof(Counters), st));
  BUF_TRY(c->b_raw_cnt.ensure(sizeof(uint32_t) * (n_items + 1)));
  BUF_TRY(c->b_raw_off.ensure(sizeof(uint32_t) * (n_items + 1)));
  HIP_TRY(hipMemsetAsync(c->b_raw_cnt.as<uint32_t>() + n_items, 0, sizeof(uint32_t), st));
  HIP_TRY(hipEventRecord(c->ea[1], st));
  if (matched && skip_cnt) BUF_TRY(skip_cnt->ensure(sizeof(uint32_t) * (n_items + 1)));
  launch_n1_samples(st, false, c->ds, sets, n_rows_total, item_b, n_items, c->b_raw_cnt.as<uint32_t>(), nullptr, nullptr,
                    nullptr, nullptr, nullptr, nullptr, nullptr, c->b_ctr.as<Counters>(), matched,
                    matched && skip_cnt ? skip_cnt->as<uint32_t>() : nullptr);
  BUF_TRY(scan_total_u32(c, c->b_raw_cnt.as<uint32_t>(), c->b_raw_off.as<uint32_t>(), n_items + 1, B.n_tasks, "samples"));
  const uint32_t nt = B.n_tasks;
  if ((uint64_t)nt * V > 0x7fffffffull) {
    g_err = "eg3d_match_polyline_sets: too many samples in one batch of sets";
    return EG3D_ERR_CAPACITY;
  }
  BUF_TRY(c->b_start_hits.ensure(sizeof(Obs) * (nt + 1)));  // the samples
  for (DevBuf* w : {&c->b_task_seed, &c->b_task_entry, &c->b_task_hit, &c->b_task_k /* first row of the task's set */,
                     &c->b_task_list_off})
    BUF_TRY(w->ensure(sizeof(uint32_t) * (nt + 1)));
  launch_n1_samples(st, true, c->ds, sets, n_rows_total, item_b, n_items, nullptr, c->b_raw_off.as<uint32_t>(),
                    c->b_start_hits.as<Obs>(), c->b_task_seed.as<uint32_t>(), c->b_task_entry.as<uint32_t>(),
                    c->b_task_hit.as<uint32_t>(), c->b_task_list_off.as<uint32_t>(), c->b_task_k.as<uint32_t>(),
                    c->b_ctr.as<Counters>(), matched, nullptr);
  {
    const uint32_t last = nt * V;
    HIP_TRY(hipMemcpyAsync(c->b_task_list_off.as<uint32_t>() + nt, &last, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // `last` leaves scope
  }
  if (matched) {  // (stage B clears the flags: a walk that did not advance is reported here)
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, &c->b_ctr.as<Counters>()->flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags & CTR_N1_NO_PROGRESS) {
      g_err = "eg3d_match_polyline_sets_matched: the walk does not advance past a matched interval: the intervals do not "
              "belong to this scene";
      return EG3D_ERR_ARG;
    }
  }
  HIP_TRY(hipEventRecord(c->eb[1], st));
  B.n_lists = nt * V;
  BUF_TRY(c->b_list_cnt.ensure(sizeof(uint32_t) * ((size_t)B.n_lists + 1)));
  BUF_TRY(c->b_list_ptr.ensure(sizeof(uint32_t) * ((size_t)B.n_lists + 1)));
  HIP_TRY(hipMemsetAsync(c->b_list_cnt.as<uint32_t>() + B.n_lists, 0, sizeof(uint32_t), st));
  HIP_TRY(hipEventRecord(c->ea[2], st));
  if (matched && drop_cnt) BUF_TRY(drop_cnt->ensure(sizeof(uint32_t) * (nt + 1)));
  launch_n1_hits(st, false, c->ds, sets, nt, c->b_start_hits.as<Obs>(), c->b_task_k.as<uint32_t>(),
                 c->b_list_cnt.as<uint32_t>(), nullptr, nullptr, c->b_ctr.as<Counters>(), matched,
                 matched && drop_cnt ? drop_cnt->as<uint32_t>() : nullptr);
  BUF_TRY(scan_total_u32(c, c->b_list_cnt.as<uint32_t>(), c->b_list_ptr.as<uint32_t>(), (size_t)B.n_lists + 1, B.n_hits,
                         "epipolar hits"));
  BUF_TRY(c->b_hits.ensure(sizeof(Obs) * ((size_t)B.n_hits + 1)));
  launch_n1_hits(st, true, c->ds, sets, nt, c->b_start_hits.as<Obs>(), c->b_task_k.as<uint32_t>(),
                 c->b_list_cnt.as<uint32_t>(), c->b_list_ptr.as<uint32_t>(), c->b_hits.as<Obs>(), c->b_ctr.as<Counters>(),
                 matched, nullptr);
  HIP_TRY(hipEventRecord(c->eb[2], st));
  return EG3D_OK;
}

int run_sets_stage_a(eg3d_ctx* c, const SetsDev& sets, const uint32_t* h_row_off, uint32_t n_rows_total, uint32_t set_b,
                     uint32_t set_e, const IvTable* matched, DevBuf* skip_cnt, DevBuf* drop_cnt, BatchState& B) {
  const uint32_t V = (uint32_t)c->V;
  return run_items_stage_a(c, sets, n_rows_total, h_row_off[(size_t)set_b * V], h_row_off[(size_t)set_e * V], matched, skip_cnt,
                           drop_cnt, B);
}

// One unit of a polyline-set call, items [item_b, item_e): stage A above, then the common stage B.
// `wrapped` (null: the unit runs or the call fails, as eg3d_match_polyline_sets does): the caller can cut the unit. The
// unit's 32-bit totals — samples x views, epipolar hits, hypotheses — are all known before the first chain is followed;
// where one does not fit (or exceeds wrap_limit, EG3D_TEST_ITEM_WRAP; 0 = no such limit), *wrapped is set and EG3D_OK
// returned with nothing placed, nothing counted into H and the turn untouched.
int run_items_batch(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows_total, uint32_t item_b, uint32_t item_e,
                    const IvTable* matched, UnitTurn& T, HostOut& H, uint32_t wrap_limit = 0, bool* wrapped = nullptr) {
  hipStream_t st = c->stream;
  const uint32_t V = (uint32_t)c->V;
  BatchState B;
  {
    const int rc = run_items_stage_a(c, sets, n_rows_total, item_b, item_e, matched, nullptr, nullptr, B);
    if (wrapped) {
      *wrapped = rc == EG3D_ERR_CAPACITY ||
                 (rc == EG3D_OK && wrap_limit && ((uint64_t)B.n_tasks * V > wrap_limit || B.n_hits > wrap_limit));
      if (*wrapped) return EG3D_OK;
    }
    BUF_TRY(rc);
  }
  const uint32_t nt = B.n_tasks;
  // every sample of the unit lies inside a held interval: nothing to launch, the unit only takes its turn
  if (matched && !nt) return T.finish(0) ? EG3D_OK : EG3D_ERR_HIP;
  // identity view map: one row of V entries shared by every sample (StageAView::dense_k)
  {
    std::vector<int32_t> mv(V);
    std::vector<uint32_t> me(V);
    for (uint32_t j = 0; j < V; j++) {
      mv[j] = (int32_t)j;
      me[j] = j;
    }
    BUF_TRY(upload(c->b_map_view, mv.data(), V, st));
    BUF_TRY(upload(c->b_map_entry, me.data(), V, st));
    BUF_TRY(c->b_map_n.ensure(sizeof(uint32_t)));
    HIP_TRY(hipStreamSynchronize(st));
  }
  fill_stage_a_view(c, B);  // (no tracks, seed_begin = sv_base = 0: B was zeroed)
  B.a.dense_k = V;
  if (wrapped) {
    const int rc = count_hypotheses(c, B);
    *wrapped = rc == EG3D_ERR_CAPACITY || (rc == EG3D_OK && wrap_limit && B.n_hyp > wrap_limit);
    if (*wrapped) return EG3D_OK;
    BUF_TRY(rc);
    BUF_TRY(run_stage_b_counted(c, B, T, H));
  } else {
    BUF_TRY(run_stage_b(c, B, T, H));
  }
  // per sample: its coordinates, V camera matrices, V-1 fundamental matrices (the scanned vertices
  // and the output were added by the kernels)
  H.bytes_algorithmic += (uint64_t)nt * (8 + (uint64_t)V * 64 + (uint64_t)(V - 1) * 72);
  return EG3D_OK;
}

int run_sets_batch(eg3d_ctx* c, const SetsDev& sets, const uint32_t* h_row_off, uint32_t n_rows_total, uint32_t set_b,
                   uint32_t set_e, const IvTable* matched, UnitTurn& T, HostOut& H) {
  const uint32_t V = (uint32_t)c->V;
  return run_items_batch(c, sets, n_rows_total, h_row_off[(size_t)set_b * V], h_row_off[(size_t)set_e * V], matched, T, H);
}

template <typename T>
T* dup_to_malloc(const std::vector<T>& v, size_t extra = 0) {
  T* p = (T*)malloc(sizeof(T) * std::max<size_t>(1, v.size() + extra));
  if (!v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}

}  // namespace

// ---- one call = units on lanes ----------------------------------------------------------------------------------------
// The reference's parallel entry point runs the seeds of ONE call on its OpenMP team (plg_matching_from_refpoints.cpp:83-104,
// `#pragma omp parallel for`). The analogue here: a call's range is cut into units (contiguous, balanced by the sum of track
// lengths), the units run concurrently on the context's lanes — internal contexts with their own HIP stream, work buffers
// and host thread — and their clouds are concatenated in unit order (CallSink). What that buys on one GPU: the candidate /
// hypothesis stages and the D2H copy of one unit overlap the expand stage of another, and the thin tail of one expand launch
// (a few long chains on an otherwise empty GPU) is filled by the next unit's chains.
// A lane takes the owner's current seeds and what the owner has learned (run_pipelined gives back what the lanes learned:
// it serves all of them, capacities only grow). Lane 0 is the owner itself.
static void lane_share_inputs(eg3d_ctx* owner, eg3d_ctx* l) {
  l->seeds = owner->seeds;
  l->learned.merge(owner->learned);
}
static int ensure_lanes(eg3d_ctx* c, int n) {
  if (c->lanes.empty()) c->lanes.push_back(c);
  while ((int)c->lanes.size() < n) {
    const StreamPrio prio = !c->tune.lane_priorities ? StreamPrio::plain : c->lanes.size() == 1 ? StreamPrio::middle : StreamPrio::least;
    eg3d_ctx* l = nullptr;
    BUF_TRY(clone_ctx(c, prio, &l));  // (whole or not at all: nothing below can fail)
    l->is_lane = true;
    l->tune.lanes = 1;
    c->lanes.push_back(l);
  }
  return EG3D_OK;
}

struct UnitRange {
  uint32_t b, e;
  double w;
};
// Cuts [b, e) into contiguous units of (nearly) equal weight; cum[i] = weight of items [0, i) (ascending).
template <typename Cum>
static std::vector<UnitRange> cut_by_weight(uint32_t b, uint32_t e, uint32_t n_units, Cum cum, double ramp = 1.0) {
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

// Runs the units on up to n_lanes lanes (the calling thread drives lane 0). run(lane, unit index, turn, stats) -> status.
template <typename Run>
static int run_pipelined(eg3d_ctx* c, CallSink& S, const std::vector<UnitRange>& units, int n_lanes, Run run) {
  const uint32_t n_units = (uint32_t)units.size();
  n_lanes = (int)std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)std::max(1, n_lanes), n_units));
  BUF_TRY(ensure_lanes(c, n_lanes));
  S.lanes_active = n_lanes;
  for (int l = 0; l < n_lanes; l++) lane_share_inputs(c, c->lanes[(size_t)l]);
  for (const UnitRange& u : units) S.weight_total += u.w;
  std::atomic<uint32_t> next{0};
  auto worker = [&](eg3d_ctx* lane) {
    if (hipSetDevice(lane->device) != hipSuccess) {
      S.fail(EG3D_ERR_HIP, "eg3d: hipSetDevice failed on a pipeline thread");
      return;
    }
    for (uint32_t u; (u = next.fetch_add(1)) < n_units;) {
      UnitTurn T{S, u, units[u].w};
      HostOut H;
      const int rc = run(lane, u, T, H);
      if (rc != EG3D_OK) {
        S.fail(rc, g_err);  // (this thread's message; the first failure of the call is the one reported)
        return;
      }
      T.pass();
      S.add(H);
    }
  };
  std::vector<std::thread> th;
  try {
    for (int l = 1; l < n_lanes; l++) th.emplace_back(worker, c->lanes[(size_t)l]);
  } catch (...) {  // no more threads: the lanes that did start (and this thread) take all units
  }
  worker(c);
  for (auto& t : th) t.join();
  for (int l = 0; l < n_lanes; l++) c->learned.merge(c->lanes[(size_t)l]->learned);
  if (S.failed) {
    g_err = S.err;
    return S.rc;
  }
  return EG3D_OK;
}

extern "C" void eg3d_free_edgepoints(eg3d_edgepoints* e);
static int finish_match(eg3d_ctx* c, CallSink& S, float total, eg3d_edgepoints* out, eg3d_stage_times* times) {
  const HostOut& H = S.tot;
  const int device_only = S.device_only;
  out->n_points = S.n_points;
  out->n_obs = S.n_obs;
  out->n_tasks = H.n_tasks;
  out->n_hypotheses = H.n_hyp;
  out->n_chains = H.n_chains;
  out->flags = H.flags;
  c->last_chunks = H.pieces;
  c->last_accumulated = device_only != 0;
  if (!device_only) {
    c->host_calls++;
    c->last_host_cloud_bytes = 36 * S.n_points + 20 * S.n_obs;
  }
  if (device_only) {
    c->last_np = S.n_points;
    c->last_no = S.n_obs;
  }
  if (!device_only) {
    const size_t npts = (size_t)S.n_points;
    if (!S.off.reserve(npts + 1)) {
      g_err = "eg3d: out of host memory for the edge-point cloud";
      return EG3D_ERR_ARG;
    }
    S.off[npts] = S.n_obs;
    out->X = S.X.release();
    out->obs_off = S.off.release();
    out->obs_view = S.view.release();
    out->obs_pl = S.pl.release();
    out->obs_seg = S.seg.release();
    out->obs_xy = S.xy.release();
    out->key = S.key.release();
    out->_owner = (void*)1;
  }
  if (times) {
    times->ms_total = total;
    times->ms_candidates = H.ms[1];
    times->ms_epipolar = H.ms[2];
    times->ms_hypotheses = H.ms[3];
    times->ms_select = H.ms[4];
    times->ms_expand = H.ms[5];
    times->ms_emit = H.ms[6];
    times->bytes_algorithmic = H.bytes_algorithmic + 12 * S.n_points + 20 * S.n_obs;
    times->ms_slowest_chain = c->wall_clock_khz > 0 ? (float)((double)H.max_chain_ticks / (double)c->wall_clock_khz) : 0.0f;
  }
  if (H.flags & (EG3D_FLAG_CHAIN_OVERFLOW | EG3D_FLAG_OBS_OVERFLOW | EG3D_FLAG_HYP_OVERFLOW)) {
    g_err = "eg3d: a device-side capacity was exceeded (flags in out->flags)";
    const uint32_t flags = out->flags;
    eg3d_free_edgepoints(out);  // an error return owns nothing the caller would have to free
    out->flags = flags;
    return EG3D_ERR_CAPACITY;
  }
  return EG3D_OK;
}

extern "C" int eg3d_set_pipelining(eg3d_ctx* c, int lanes, int units) {
  if (!c || lanes < 0 || units < 0) {
    g_err = "eg3d_set_pipelining: bad arguments";
    return EG3D_ERR_ARG;
  }
  c->tune.lanes = std::min(16, lanes);
  c->tune.units = std::min(4096, units);
  return EG3D_OK;
}

static int lanes_for(const eg3d_ctx* c, int device_only) {
  if (c->tune.lanes > 0) return c->tune.lanes;
  // by measurement (round 6): cutting a call buys nothing on the device — every expand launch lasts at least as
  // long as its slowest chain and the launches of a call's units run nearly first-in-first-out — but it hides most of the
  // D2H copy of a host call (C3' 64 -> 54 ms). Lanes have a price when they are created (streams, work buffers, pinned
  // rings: +50-90 ms on the call that creates them, seconds on a 200-view scene), so the FIRST host call of a context — a
  // one-shot caller's only call — runs on the context alone; a context that is called again is worth the lanes.
  if (device_only) return 1;
  // every lane owns a full slot arena (the residency of the expand kernel x the slice size): on many-view scenes that is
  // 17 GB per lane (C4) for a 3 % gain with the copy and a loss without — such scenes stay on the context alone
  const size_t arena = chain_layout(c->learned.chain_cap, c->learned.pool_cap, (uint32_t)c->V).total * 8 * (size_t)c->slots_per_xcd;
  if (arena > ((size_t)4 << 30)) return 1;
  // ... and a small cloud has no copy worth hiding (C3-real, 0.3 MB: 3.3 ms uncut, 5.1 ms on three lanes)
  return c->host_calls > 0 && c->last_host_cloud_bytes >= ((uint64_t)4 << 20) ? Tunables::kHostCallLanes : 1;
}

// Units of a seed range. One lane: batches of 16 384 seeds (one expand launch each), as before round 6. Several lanes:
// at least one unit per lane when the range is worth cutting (>= 128 seeds per unit), never more than 16 384 seeds per unit,
// balanced by the sum of track lengths (the same weight the multi-GPU sharding uses).
static std::vector<UnitRange> plan_seed_units(const eg3d_ctx* c, uint32_t b, uint32_t e, int lanes) {
  const uint32_t SEED_BATCH = 16384, MIN_UNIT = 128;
  const uint32_t n = e - b;
  const std::vector<uint32_t>& trk = c->seeds->trk_off;
  auto cum = [&](uint32_t i) { return (double)trk[i] + 1e-3 * (double)i; };  // (+ a little per seed: seeds without tracks still count)
  if (lanes <= 1 && !c->tune.units) {
    std::vector<UnitRange> out;
    for (uint32_t s0 = b; s0 < e; s0 += SEED_BATCH) {
      const uint32_t s1 = std::min(e, s0 + SEED_BATCH);
      out.push_back({s0, s1, cum(s1) - cum(s0)});
    }
    return out;
  }
  uint32_t n_units = c->tune.units ? (uint32_t)c->tune.units : std::min<uint32_t>((uint32_t)lanes, n / MIN_UNIT);
  n_units = std::max(n_units, (n + SEED_BATCH - 1) / SEED_BATCH);
  std::vector<UnitRange> out = cut_by_weight(b, e, std::max(1u, n_units), cum, c->tune.unit_ramp);
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

// What eg3d_match_resident and eg3d_match_polyline_sets do with their units: the call's sink, the units on the lanes
// (run(lane, unit index, turn, stats) -> status computes one), the call's time, the result. keyed_by_sample: key[0] of a
// point is the sample index of the CALL (polyline sets), not a seed id; key0_start is then the index of the call's first
// sample (eg3d_match_polyline_items: the samples of the item ranges before this one).
template <typename Run>
static int match_call(eg3d_ctx* c, int device_only, bool keyed_by_sample, const std::vector<UnitRange>& units, int lanes,
                      eg3d_edgepoints* out, eg3d_stage_times* times, Run run, uint32_t key0_start = 0) {
  CallSink S;
  S.owner = c;
  S.device_only = device_only;
  S.keyed_by_sample = keyed_by_sample;
  S.key0_next = key0_start;
  c->last_np = c->last_no = 0;
  c->last_chunks = 0;
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipEventRecord(c->ea[7], c->stream));  // the context's own events: nothing to leak on an error path
  if (!units.empty()) BUF_TRY(run_pipelined(c, S, units, lanes, run));
  HIP_TRY(hipEventRecord(c->eb[7], c->stream));
  HIP_TRY(hipEventSynchronize(c->eb[7]));
  float total = 0;
  HIP_TRY(hipEventElapsedTime(&total, c->ea[7], c->eb[7]));
  // (several lanes: the context's own stream saw one of them only — the call's wall time is the total)
  if (units.size() > 1 && lanes > 1)
    total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return finish_match(c, S, total, out, times);
}

extern "C" int eg3d_match_resident(eg3d_ctx* c, uint32_t b, uint32_t e, int device_only, eg3d_edgepoints* out,
                                   eg3d_stage_times* times) {
  if (!c || !out || b > e || e > c->seeds->n_seeds) {
    g_err = "eg3d_match_resident: bad arguments (seeds uploaded?)";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  memset(out, 0, sizeof(*out));
  const int lanes = lanes_for(c, device_only);
  const std::vector<UnitRange> units = plan_seed_units(c, b, e, lanes);
  return match_call(c, device_only, false, units, lanes, out, times, [&](eg3d_ctx* lane, uint32_t u, UnitTurn& T, HostOut& H) {
    return run_batch(lane, units[u].b, units[u].e, T, H);
  });
}

extern "C" int eg3d_last_device_output(eg3d_ctx* c, eg3d_device_edgepoints* out) {
  if (!c || !out) {
    g_err = "eg3d_last_device_output: bad arguments";
    return EG3D_ERR_ARG;
  }
  out->n_points = c->last_np;
  out->n_obs = c->last_no;
  out->X = c->o_X.as<float>();
  out->obs_off = c->o_off.as<eg3d_off_t>();
  out->obs_view = c->o_view.as<int32_t>();
  out->obs_pl = c->o_pl.as<uint32_t>();
  out->obs_seg = c->o_seg.as<uint32_t>();
  out->obs_xy = c->o_xy.as<float>();
  out->key = c->o_key.as<uint32_t>();
  out->complete = (c->last_accumulated || c->last_chunks <= 1) ? 1 : 0;
  return EG3D_OK;
}

extern "C" int eg3d_match_refpoints(eg3d_ctx* c, const eg3d_seeds* seeds, uint32_t b, uint32_t e, int device_only,
                                    eg3d_edgepoints* out, eg3d_stage_times* times) {
  int rc = eg3d_upload_seeds(c, seeds);
  if (rc != EG3D_OK) return rc;
  return eg3d_match_resident(c, b, e, device_only, out, times);
}

extern "C" int eg3d_check_polyline_sets(const eg3d_polyline_sets* ps, int32_t n_views) {
  if (!ps || !ps->row_off || n_views < 1) {
    g_err = "eg3d_check_polyline_sets: bad arguments";
    return EG3D_ERR_ARG;
  }
  const uint64_t n_rows = (uint64_t)ps->n_sets * (uint64_t)n_views;
  if (n_rows > 0xffffffffull) {
    g_err = "eg3d_match_polyline_sets: too many rows";
    return EG3D_ERR_ARG;
  }
  if (ps->row_off[n_rows] && !ps->pl_ids) {
    g_err = "eg3d_match_polyline_sets: pl_ids is null";
    return EG3D_ERR_ARG;
  }
  for (uint64_t r = 0; r < n_rows; r++) {
    if (ps->row_off[r + 1] < ps->row_off[r]) {
      g_err = "eg3d_match_polyline_sets: row_off is not ascending";
      return EG3D_ERR_ARG;
    }
    // a row is the reference's set<ulong>: strictly ascending, no repeats (a repeated id would be sampled and scanned
    // twice — an input the reference cannot produce)
    for (uint32_t k = ps->row_off[r] + 1; k < ps->row_off[r + 1]; k++)
      if (ps->pl_ids[k] <= ps->pl_ids[k - 1]) {
        g_err = "eg3d_match_polyline_sets: polyline ids of a row are not strictly ascending";
        return EG3D_ERR_ARG;
      }
  }
  return EG3D_OK;
}

// The caller's matched_polyline_intervals for the duration of ONE call: host arrays are uploaded into the DevBufs here
// (released with the call), device arrays are read in place. Everything is checked before anything is indexed with it:
// what needs no scene on the host for host arrays (their total sizes the upload), then check_interval_row, one lane per
// row, for both kinds. active: the table holds at least one interval.
namespace {
struct MatchedCall {
  DevBuf off, sseg, sxy, eseg, exy, bad;
  IvTable dev{};
  bool active = false;
};
int bad_matched(const char* what) {
  g_err = std::string("eg3d_match_polyline_sets_matched: ") + what;
  return EG3D_ERR_ARG;
}
int prepare_matched(eg3d_ctx* c, const eg3d_matched_intervals* m, MatchedCall& M) {
  if (!m) return EG3D_OK;
  if (m->struct_size != sizeof(eg3d_matched_intervals)) return bad_matched("struct_size is not sizeof(eg3d_matched_intervals)");
  const uint32_t V = (uint32_t)c->V;
  uint32_t n_pl = 0;
  HIP_TRY(hipMemcpy(&n_pl, c->ds.view_pl_off + V, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (m->n_scene_polylines != n_pl) return bad_matched("n_scene_polylines is not the scene's number of polylines");
  if (!m->iv_off) return bad_matched("iv_off is null");
  hipStream_t st = c->stream;
  uint64_t total = 0;
  if (m->on_device) {
    HIP_TRY(hipMemcpy(&total, m->iv_off + n_pl, sizeof(uint64_t), hipMemcpyDeviceToHost));
    M.dev.off = m->iv_off;
    M.dev.start_seg = m->iv_start_seg;
    M.dev.start_xy = m->iv_start_xy;
    M.dev.end_seg = m->iv_end_seg;
    M.dev.end_xy = m->iv_end_xy;
  } else {
    total = m->iv_off[n_pl];
    for (uint32_t g = 0; g < n_pl; g++)
      if (m->iv_off[g] > m->iv_off[g + 1] || m->iv_off[g + 1] > total) return bad_matched("iv_off is not ascending");
  }
  if (total && (!m->iv_start_seg || !m->iv_start_xy || !m->iv_end_seg || !m->iv_end_xy))
    return bad_matched("an interval array is null");
  if (!m->on_device) {
    BUF_TRY(upload(M.off, m->iv_off, (size_t)n_pl + 1, st));
    BUF_TRY(upload(M.sseg, m->iv_start_seg, total, st));
    BUF_TRY(upload(M.sxy, m->iv_start_xy, 2 * total, st));
    BUF_TRY(upload(M.eseg, m->iv_end_seg, total, st));
    BUF_TRY(upload(M.exy, m->iv_end_xy, 2 * total, st));
    M.dev.off = M.off.as<uint64_t>();
    M.dev.start_seg = M.sseg.as<uint32_t>();
    M.dev.start_xy = M.sxy.as<float>();
    M.dev.end_seg = M.eseg.as<uint32_t>();
    M.dev.end_xy = M.exy.as<float>();
  }
  BUF_TRY(M.bad.ensure(sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(M.bad.p, 0, sizeof(uint32_t), st));
  launch_n1_check_intervals(st, c->ds, M.dev, total, n_pl, M.bad.as<uint32_t>());
  uint32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, M.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (also: the table is resident before any lane reads it)
  if (bad)
    return bad_matched("the intervals fail their checks (offsets ascending, segment indices inside their polyline, start "
                       "segments strictly ascending within a row)");
  M.active = total != 0;
  return EG3D_OK;
}
// the checks and the upload of the sets, shared by the calls on polyline sets; `who` names the entry point in errors
int prepare_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, SetsDev& sd);
}  // namespace

static int match_sets_call(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                           const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out, eg3d_stage_times* times) {
  if (!c || !ps || !out || !ps->row_off || set_b > set_e || set_e > ps->n_sets) {
    g_err = "eg3d_match_polyline_sets: bad arguments";
    return EG3D_ERR_ARG;
  }
  if ((uint64_t)ps->n_sets * (uint64_t)c->V > 0xffffffffull) {
    g_err = "eg3d_match_polyline_sets: too many rows";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  MatchedCall M;
  BUF_TRY(prepare_matched(c, m, M));  // (before `out` is touched)
  const IvTable* matched = M.active ? &M.dev : nullptr;
  memset(out, 0, sizeof(*out));
  SetsDev sd;
  BUF_TRY(prepare_sets(c, ps, sd));
  const uint32_t V = (uint32_t)c->V;
  const uint32_t n_rows = ps->n_sets * V;
  const int lanes = lanes_for(c, device_only);
  // units = runs of whole sets, bounded by the number of polylines (every sample owns V lists); with several lanes at
  // least one unit per lane, balanced by the number of polylines
  const uint32_t max_items = V >= 64 ? 2048u : 16384u;
  std::vector<UnitRange> units;
  {
    auto cum = [&](uint32_t i) { return (double)ps->row_off[(size_t)i * V] + 1e-3 * (double)i; };
    const uint32_t want = c->tune.units ? (uint32_t)c->tune.units : (uint32_t)lanes;
    for (const UnitRange& r : cut_by_weight(set_b, set_e, want, cum))
      for (uint32_t s0 = r.b; s0 < r.e;) {  // (a unit above the bound is cut into runs of whole sets within it)
        uint32_t s1 = s0 + 1;
        while (s1 < r.e && ps->row_off[(size_t)(s1 + 1) * V] - ps->row_off[(size_t)s0 * V] <= max_items) s1++;
        units.push_back({s0, s1, cum(s1) - cum(s0)});
        s0 = s1;
      }
  }
  return match_call(c, device_only, true, units, lanes, out, times, [&](eg3d_ctx* lane, uint32_t u, UnitTurn& T, HostOut& H) {
    return run_sets_batch(lane, sd, ps->row_off, n_rows, units[u].b, units[u].e, matched, T, H);
  });
}

extern "C" int eg3d_match_polyline_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                        int device_only, eg3d_edgepoints* out, eg3d_stage_times* times) {
  return match_sets_call(c, ps, set_b, set_e, nullptr, device_only, out, times);
}

extern "C" int eg3d_match_polyline_sets_matched(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                                const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out,
                                                eg3d_stage_times* times) {
  return match_sets_call(c, ps, set_b, set_e, m, device_only, out, times);
}

// ---- the extractor on item ranges (include/eg3d_sets_device.h; the entry points are in eg3d_api_sets.hip) -----------------
// The count pass of k_n1_samples over items [item_b, item_b + n_items) on the context's stream: the counts in b_raw_cnt,
// their exclusive scan in b_raw_off (n_items + 1 words), the total on the host.
static int count_items(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t n_items, const IvTable* matched,
                       uint32_t& total) {
  hipStream_t st = c->stream;
  BUF_TRY(c->b_ctr.ensure(sizeof(Counters)));
  HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, sizeof(Counters), st));
  BUF_TRY(c->b_raw_cnt.ensure(sizeof(uint32_t) * ((size_t)n_items + 1)));
  BUF_TRY(c->b_raw_off.ensure(sizeof(uint32_t) * ((size_t)n_items + 1)));
  HIP_TRY(hipMemsetAsync(c->b_raw_cnt.as<uint32_t>() + n_items, 0, sizeof(uint32_t), st));
  launch_n1_samples(st, false, c->ds, sets, n_rows, item_b, n_items, c->b_raw_cnt.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, c->b_ctr.as<Counters>(), matched, nullptr);
  BUF_TRY(scan_total_u32(c, c->b_raw_cnt.as<uint32_t>(), c->b_raw_off.as<uint32_t>(), (size_t)n_items + 1, total, "samples"));
  HIP_TRY(hipStreamSynchronize(st));
  if (matched) {
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, &c->b_ctr.as<Counters>()->flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags & CTR_N1_NO_PROGRESS) return bad_matched("the walk does not advance past a matched interval: the intervals do not belong to this scene");
  }
  return EG3D_OK;
}

int eg3d::api::count_item_samples(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e,
                                  const eg3d_matched_intervals* m, uint32_t* counts_host, std::vector<uint32_t>* prefix) {
  HIP_TRY(hipSetDevice(c->device));
  MatchedCall M;
  BUF_TRY(prepare_matched(c, m, M));
  const uint32_t n_items = item_e - item_b;
  uint32_t total = 0;
  BUF_TRY(count_items(c, sets, n_rows, item_b, n_items, M.active ? &M.dev : nullptr, total));
  if (counts_host && n_items) HIP_TRY(hipMemcpy(counts_host, c->b_raw_cnt.p, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost));
  if (prefix) {
    prefix->resize((size_t)n_items + 1);
    HIP_TRY(hipMemcpy(prefix->data(), c->b_raw_off.p, sizeof(uint32_t) * ((size_t)n_items + 1), hipMemcpyDeviceToHost));
  }
  return EG3D_OK;
}

int eg3d::api::match_items_call(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e,
                                uint32_t sample_base, const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out,
                                eg3d_stage_times* times) {
  HIP_TRY(hipSetDevice(c->device));
  MatchedCall M;
  BUF_TRY(prepare_matched(c, m, M));  // (before `out` is touched)
  const IvTable* matched = M.active ? &M.dev : nullptr;
  memset(out, 0, sizeof(*out));
  c->items_units = 0;
  const uint32_t V = (uint32_t)c->V, n_items = item_e - item_b;
  // one count pass for the range; its prefix sums, read back, are what the units are cut by
  uint32_t total = 0;
  std::vector<uint32_t> pre((size_t)n_items + 1, 0);
  BUF_TRY(count_items(c, sets, n_rows, item_b, n_items, matched, total));
  HIP_TRY(hipMemcpy(pre.data(), c->b_raw_off.p, sizeof(uint32_t) * ((size_t)n_items + 1), hipMemcpyDeviceToHost));
  if ((uint64_t)sample_base + total > 0xffffffffull) {
    g_err = "eg3d_match_polyline_items: sample_base + the samples of the range does not fit key[0]";
    return EG3D_ERR_CAPACITY;
  }
  const int lanes = lanes_for(c, device_only);
  // units = item ranges of at most unit_samples samples (every sample owns V lists); with several lanes at least one unit
  // per lane, balanced by the samples. A set larger than a unit is cut inside; only a single polyline stays whole.
  const uint32_t unit_samples = c->tune.item_unit_samples ? c->tune.item_unit_samples : (V >= 64 ? 1u << 15 : 1u << 18);
  std::vector<UnitRange> units;
  {
    auto cum = [&](uint32_t i) { return (double)pre[i - item_b] + 1e-3 * (double)i; };  // (+ a little per item: empty ones count)
    const uint32_t want = c->tune.units ? (uint32_t)c->tune.units : (uint32_t)lanes;
    for (const UnitRange& r : cut_by_weight(item_b, item_e, want, cum))
      for (uint32_t i0 = r.b; i0 < r.e;) {
        uint32_t i1 = i0 + 1;
        while (i1 < r.e && pre[i1 + 1 - item_b] - pre[i0 - item_b] <= unit_samples) i1++;
        units.push_back({i0, i1, cum(i1) - cum(i0)});
        i0 = i1;
      }
  }
  c->items_units = (uint32_t)units.size();
  // A unit whose 32-bit totals wrap is cut in two by its samples and redone, down to one item: the parts run one after the
  // other on the unit's lane and under the unit's turn (UnitTurn::more_parts), so the cloud's bytes do not depend on it.
  std::atomic<uint32_t> redone{0};
  const uint32_t wrap_limit = c->tune.test_item_wrap;
  std::function<int(eg3d_ctx*, uint32_t, uint32_t, bool, UnitTurn&, HostOut&)> part = [&](eg3d_ctx* lane, uint32_t b, uint32_t e,
                                                                                           bool last, UnitTurn& T, HostOut& H) -> int {
    T.more_parts = !last;
    bool wrapped = false;
    BUF_TRY(run_items_batch(lane, sets, n_rows, b, e, matched, T, H, wrap_limit, &wrapped));
    if (!wrapped) return EG3D_OK;
    if (e - b <= 1) {
      g_err = "eg3d_match_polyline_items: the samples x views, epipolar hits or hypotheses of a single polyline exceed 2^32-1";
      return EG3D_ERR_CAPACITY;
    }
    redone.fetch_add(1);
    const uint32_t half = pre[b - item_b] + (pre[e - item_b] - pre[b - item_b]) / 2;
    uint32_t mid = b + 1;
    while (mid < e - 1 && pre[mid - item_b] < half) mid++;
    BUF_TRY(part(lane, b, mid, false, T, H));
    return part(lane, mid, e, last, T, H);
  };
  const int rc = match_call(
      c, device_only, true, units, lanes, out, times,
      [&](eg3d_ctx* lane, uint32_t u, UnitTurn& T, HostOut& H) { return part(lane, units[u].b, units[u].e, true, T, H); },
      sample_base);
  c->items_redone = redone.load();
  return rc;
}

namespace {
int prepare_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, SetsDev& sd) {
  const uint32_t V = (uint32_t)c->V;
  const uint32_t n_rows = ps->n_sets * V;
  const uint32_t n_ids = ps->row_off[n_rows];
  {
    std::vector<uint32_t> vpo(V + 1);
    HIP_TRY(hipMemcpy(vpo.data(), c->ds.view_pl_off, sizeof(uint32_t) * (V + 1), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < n_rows; r++) {
      if (ps->row_off[r + 1] < ps->row_off[r]) {
        g_err = "eg3d_match_polyline_sets: row_off is not ascending";
        return EG3D_ERR_ARG;
      }
      const uint32_t npl = vpo[r % V + 1] - vpo[r % V];
      for (uint32_t k = ps->row_off[r]; k < ps->row_off[r + 1]; k++)
        if (ps->pl_ids[k] >= npl) {
          g_err = "eg3d_match_polyline_sets: polyline id out of range";
          return EG3D_ERR_ARG;
        }
    }
  }
  {
    const int rc = eg3d_check_polyline_sets(ps, c->V);  // (the checks that need no scene: rows are sets)
    if (rc != EG3D_OK) return rc;
  }
  BUF_TRY(upload(c->b_sets_off, ps->row_off, (size_t)n_rows + 1, c->stream));
  BUF_TRY(upload(c->b_sets_ids, ps->pl_ids, n_ids, c->stream));
  sd.n_views = V;
  sd.row_off = c->b_sets_off.as<uint32_t>();
  sd.pl_ids = c->b_sets_ids.as<uint32_t>();
  HIP_TRY(hipStreamSynchronize(c->stream));  // the sets are resident before any lane reads them
  return EG3D_OK;
}
}  // namespace

// Stage A of the extractor alone, the whole range as ONE batch on the context's own stream.
extern "C" int eg3d_polyline_set_candidates(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                            const eg3d_matched_intervals* m, eg3d_set_candidates* out) {
  if (!c || !ps || !out || !ps->row_off || set_b > set_e || set_e > ps->n_sets) {
    g_err = "eg3d_polyline_set_candidates: bad arguments";
    return EG3D_ERR_ARG;
  }
  if ((uint64_t)ps->n_sets * (uint64_t)c->V > 0xffffffffull) {
    g_err = "eg3d_polyline_set_candidates: too many rows";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  MatchedCall M;
  BUF_TRY(prepare_matched(c, m, M));
  const IvTable* matched = M.active ? &M.dev : nullptr;
  memset(out, 0, sizeof(*out));
  SetsDev sd;
  BUF_TRY(prepare_sets(c, ps, sd));
  const uint32_t V = (uint32_t)c->V;
  DevBuf skip_cnt, drop_cnt;
  BatchState B;
  BUF_TRY(run_sets_stage_a(c, sd, ps->row_off, ps->n_sets * V, set_b, set_e, matched, &skip_cnt, &drop_cnt, B));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const uint32_t nt = B.n_tasks;
  const uint32_t n_items = ps->row_off[(size_t)set_e * V] - ps->row_off[(size_t)set_b * V];
  std::vector<Obs> samples(nt + 1), hits((size_t)B.n_hits + 1);
  std::vector<uint32_t> list_ptr((size_t)B.n_lists + 1), skipped(n_items + 1), dropped(nt + 1);
  if (nt) HIP_TRY(hipMemcpy(samples.data(), c->b_start_hits.p, sizeof(Obs) * nt, hipMemcpyDeviceToHost));
  if (B.n_hits) HIP_TRY(hipMemcpy(hits.data(), c->b_hits.p, sizeof(Obs) * B.n_hits, hipMemcpyDeviceToHost));
  // (list_ptr is the exclusive scan of the counts, its last entry the total: the lists lie in (task, view) order)
  HIP_TRY(hipMemcpy(list_ptr.data(), c->b_list_ptr.p, sizeof(uint32_t) * ((size_t)B.n_lists + 1), hipMemcpyDeviceToHost));
  if (matched && n_items) HIP_TRY(hipMemcpy(skipped.data(), skip_cnt.p, sizeof(uint32_t) * n_items, hipMemcpyDeviceToHost));
  if (matched && nt) HIP_TRY(hipMemcpy(dropped.data(), drop_cnt.p, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost));
  std::vector<int32_t> t_view(nt);
  std::vector<uint32_t> t_pl(nt), t_seg(nt), h_pl(B.n_hits), h_seg(B.n_hits);
  std::vector<float> t_xy((size_t)nt * 2), h_xy((size_t)B.n_hits * 2);
  std::vector<uint64_t> list_off((size_t)B.n_lists + 1);
  for (uint32_t i = 0; i < nt; i++) {
    t_view[i] = (int32_t)samples[i].view;
    t_pl[i] = samples[i].pl;
    t_seg[i] = samples[i].seg;
    t_xy[2 * (size_t)i] = samples[i].x;
    t_xy[2 * (size_t)i + 1] = samples[i].y;
  }
  for (uint32_t i = 0; i < B.n_hits; i++) {
    h_pl[i] = hits[i].pl;
    h_seg[i] = hits[i].seg;
    h_xy[2 * (size_t)i] = hits[i].x;
    h_xy[2 * (size_t)i + 1] = hits[i].y;
  }
  for (size_t l = 0; l <= B.n_lists; l++) list_off[l] = list_ptr[l];
  if (matched) {
    for (uint32_t i = 0; i < n_items; i++) out->n_samples_skipped += skipped[i];
    for (uint32_t i = 0; i < nt; i++) out->n_hits_filtered += dropped[i];
  }
  out->n_tasks = nt;
  out->task_view = dup_to_malloc(t_view);
  out->task_pl = dup_to_malloc(t_pl);
  out->task_seg = dup_to_malloc(t_seg);
  out->task_xy = dup_to_malloc(t_xy);
  out->list_off = dup_to_malloc(list_off);
  out->hit_pl = dup_to_malloc(h_pl);
  out->hit_seg = dup_to_malloc(h_seg);
  out->hit_xy = dup_to_malloc(h_xy);
  out->_owner = (void*)1;
  return EG3D_OK;
}

extern "C" void eg3d_free_set_candidates(eg3d_set_candidates* c) {
  if (!c) return;
  for (void* p : {(void*)c->task_view, (void*)c->task_pl, (void*)c->task_seg, (void*)c->task_xy, (void*)c->list_off,
                  (void*)c->hit_pl, (void*)c->hit_seg, (void*)c->hit_xy})
    free(p);
  memset(c, 0, sizeof(*c));
}

extern "C" void eg3d_free_edgepoints(eg3d_edgepoints* e) {
  if (!e) return;
  for (void* p : {(void*)e->X, (void*)e->obs_off, (void*)e->obs_view, (void*)e->obs_pl, (void*)e->obs_seg, (void*)e->obs_xy, (void*)e->key})
    free(p);
  memset(e, 0, sizeof(*e));
}

extern "C" int eg3d_candidates_run(eg3d_ctx* c, const eg3d_seeds* seeds, uint32_t b, uint32_t e, eg3d_candidates* out) {
  if (!c || !seeds || !out || b > e || e > seeds->n_seeds) {
    g_err = "eg3d_candidates_run: bad arguments";
    return EG3D_ERR_ARG;
  }
  int rc = eg3d_upload_seeds(c, seeds);
  if (rc != EG3D_OK) return rc;
  memset(out, 0, sizeof(*out));
  BatchState B;
  memset(&B, 0, sizeof(B));
  B.b = b;
  B.e = e;
  BUF_TRY(run_stage_a(c, B));
  for (bool again = true; again;) {
    unsigned long long used = 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(&used, &c->b_ctr.as<Counters>()->hits_used, sizeof(used), hipMemcpyDeviceToHost));
    BUF_TRY(k2_settle(c, B, used, &again));
  }
  const uint32_t n_sv = B.n_sv, nt = B.n_tasks;
  std::vector<uint32_t> raw_off(n_sv + 1), cand_cnt(n_sv + 1), start_cnt(n_sv + 1), cand_pl(B.total_raw + 1),
      task_seed(nt + 1), task_entry(nt + 1), task_hit(nt + 1), task_list_off(nt + 1), list_cnt(B.n_lists + 1),
      list_ptr(B.n_lists + 1);
  std::vector<Obs> start_hits(B.total_raw + 1), hits(B.n_hits + 1);
#define DL(vec, buf, n) \
  if (n) HIP_TRY(hipMemcpy(vec.data(), c->buf.p, sizeof(vec[0]) * (n), hipMemcpyDeviceToHost))
  DL(raw_off, b_raw_off, n_sv + 1);
  DL(cand_cnt, b_cand_cnt, n_sv);
  DL(start_cnt, b_start_cnt, n_sv);
  DL(cand_pl, b_cand_pl, B.total_raw);
  DL(start_hits, b_start_hits, B.total_raw);
  DL(task_seed, b_task_seed, nt);
  DL(task_entry, b_task_entry, nt);
  DL(task_hit, b_task_hit, nt);
  DL(task_list_off, b_task_list_off, nt + 1);
  DL(list_cnt, b_list_cnt, B.n_lists);
  DL(list_ptr, b_list_ptr, B.n_lists);
  DL(hits, b_hits, B.n_hits);
#undef DL
  std::vector<uint32_t> o_cand_off(1, 0), o_cand_pl, o_start_off(1, 0), o_start_pl, o_start_seg, o_task_sv(nt),
      o_hit_pl(B.n_hits), o_hit_seg(B.n_hits);
  std::vector<float> o_start_xy, o_hit_xy((size_t)B.n_hits * 2);
  for (uint32_t sv = 0; sv < n_sv; sv++) {
    for (uint32_t i = 0; i < cand_cnt[sv]; i++) o_cand_pl.push_back(cand_pl[raw_off[sv] + i]);
    o_cand_off.push_back((uint32_t)o_cand_pl.size());
    for (uint32_t i = 0; i < start_cnt[sv]; i++) {
      const Obs& o = start_hits[raw_off[sv] + i];
      o_start_pl.push_back(o.pl);
      o_start_seg.push_back(o.seg);
      o_start_xy.push_back(o.x);
      o_start_xy.push_back(o.y);
    }
    o_start_off.push_back((uint32_t)o_start_pl.size());
  }
  for (uint32_t t = 0; t < nt; t++) o_task_sv[t] = c->seeds->trk_off[task_seed[t]] - B.sv_base + task_entry[t];
  // the tasks' regions of b_hits lie in the order the tasks claimed them: gathered here in (task, list) order, the CSR
  // from the counts
  std::vector<uint32_t> list_off(B.n_lists + 1, 0);
  for (uint32_t l = 0, h = 0; l < B.n_lists; l++) {
    for (uint32_t i = 0; i < list_cnt[l]; i++, h++) {
      const Obs& o = hits[list_ptr[l] + i];
      o_hit_pl[h] = o.pl;
      o_hit_seg[h] = o.seg;
      o_hit_xy[2 * h] = o.x;
      o_hit_xy[2 * h + 1] = o.y;
    }
    list_off[l + 1] = h;
  }
  task_hit.resize(nt);
  task_list_off.resize(nt + 1);
  out->n_sv = n_sv;
  out->cand_off = dup_to_malloc(o_cand_off);
  out->cand_pl = dup_to_malloc(o_cand_pl);
  out->start_off = dup_to_malloc(o_start_off);
  out->start_pl = dup_to_malloc(o_start_pl);
  out->start_seg = dup_to_malloc(o_start_seg);
  out->start_xy = dup_to_malloc(o_start_xy);
  out->n_tasks = nt;
  out->task_sv = dup_to_malloc(o_task_sv);
  out->task_hit = dup_to_malloc(task_hit);
  out->task_list_off = dup_to_malloc(task_list_off);
  out->list_off = dup_to_malloc(list_off);
  out->hit_pl = dup_to_malloc(o_hit_pl);
  out->hit_seg = dup_to_malloc(o_hit_seg);
  out->hit_xy = dup_to_malloc(o_hit_xy);
  out->_owner = (void*)1;
  return EG3D_OK;
}

extern "C" void eg3d_free_candidates(eg3d_candidates* c) {
  if (!c) return;
  for (void* p : {(void*)c->cand_off, (void*)c->cand_pl, (void*)c->start_off, (void*)c->start_pl, (void*)c->start_seg,
                  (void*)c->start_xy, (void*)c->task_sv, (void*)c->task_hit, (void*)c->task_list_off, (void*)c->list_off,
                  (void*)c->hit_pl, (void*)c->hit_seg, (void*)c->hit_xy})
    free(p);
  memset(c, 0, sizeof(*c));
}

