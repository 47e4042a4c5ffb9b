// eg3d_api_match.hip — the match pipeline of the C ABI (include/eg3d.h) on seeds, and what every match call is made of:
// eg3d_match_resident / _refpoints, the device view of the last call, eg3d_set_pipelining, eg3d_free_edgepoints. Top to
// bottom: stage A of the seed path and its batch (run_batch); one call = units on lanes (ensure_lanes, run_pipelined,
// finish_match, lanes_for, match_call); the entry points. Stage B is in eg3d_api_match_stage_b.hip, the calls on polyline
// sets in eg3d_api_match_sets.hip, the stage-A dumps in eg3d_api_candidates.hip; eg3d_api_match_internal.h holds what they
// share (BatchState, CallSink, UnitTurn), eg3d_unit_plan.h how a range is cut into units. Host orchestration only: no kernel
// and no hipCUB here (the scans are helpers of eg3d_api.hip, declared in eg3d_api_internal.h).
#include <atomic>
#include <cstdio>
#include <thread>

#include "eg3d_api_match_internal.h"

EG3D_API_BEGIN

// K2 of the seed path, queued on the stream: b_hits with room for B.hits_cap hits, the cursor zeroed.
static int launch_stage_a_k2(eg3d_ctx* c, BatchState& B) {
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

static int run_batch(eg3d_ctx* c, uint32_t b, uint32_t e, UnitTurn& T, HostOut& H) {
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

// Runs the units on up to n_lanes lanes (the calling thread drives lane 0). run(lane, unit index, turn, stats) -> status.
static int run_pipelined(eg3d_ctx* c, CallSink& S, const std::vector<UnitRange>& units, int n_lanes, const UnitRunner& run) {
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

int lanes_for(const eg3d_ctx* c, int device_only) {
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

// What eg3d_match_resident and eg3d_match_polyline_sets do with their units: the call's sink, the units on the lanes
// (run(lane, unit index, turn, stats) -> status computes one), the call's time, the result. keyed_by_sample: key[0] of a
// point is the sample index of the CALL (polyline sets), not a seed id; key0_start is then the index of the call's first
// sample (eg3d_match_polyline_items: the samples of the item ranges before this one).
int match_call(eg3d_ctx* c, int device_only, bool keyed_by_sample, const std::vector<UnitRange>& units, int lanes,
               eg3d_edgepoints* out, eg3d_stage_times* times, const UnitRunner& run, uint32_t key0_start) {
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

EG3D_API_END

extern "C" int eg3d_set_pipelining(eg3d_ctx* c, int lanes, int units) {
  if (!c || lanes < 0 || units < 0) {
    g_err = "eg3d_set_pipelining: bad arguments";
    return EG3D_ERR_ARG;
  }
  c->tune.lanes = std::min(16, lanes);
  c->tune.units = std::min(4096, units);
  return EG3D_OK;
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
  const std::vector<UnitRange> units = plan_seed_units(c->seeds->trk_off, b, e, lanes, c->tune.units, c->tune.unit_ramp);
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

extern "C" void eg3d_free_edgepoints(eg3d_edgepoints* e) {
  if (!e) return;
  for (void* p : {(void*)e->X, (void*)e->obs_off, (void*)e->obs_view, (void*)e->obs_pl, (void*)e->obs_seg, (void*)e->obs_xy, (void*)e->key})
    free(p);
  memset(e, 0, sizeof(*e));
}
