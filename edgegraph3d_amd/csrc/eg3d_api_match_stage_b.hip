// eg3d_api_match_stage_b.hip — stage B of every match call, seeds and polyline sets alike: from a batch's StageAView to its
// part of the call's cloud. Top to bottom: the D2H ring of a context; the steps — count_hypotheses, follow_and_select, the
// expand launch (ExpandState; the engine's pair; prepare_expand, launch_expand, the verdict of judge_expand), emit_chunk,
// copy_chunk_to_host, close_chunk, stage_times_and_counts — and run_stage_b[_counted] as their list. Host orchestration
// only: no kernel and no hipCUB here (the scans and the sort of the chain costs are helpers of eg3d_api.hip, declared in
// eg3d_api_internal.h); BatchState, HostOut and the turnstile (CallSink, UnitTurn) are in eg3d_api_match_internal.h.
#include <cstdio>

#include "eg3d_api_match_internal.h"
#include "eg3d_host_copy.h"

EG3D_API_BEGIN

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
static int follow_and_select(eg3d_ctx* c, BatchState& B, HostOut& H) {
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
static uint32_t* saved_bytes(eg3d_ctx* c) { return c->b_scanchk.as<uint32_t>() + 4; }

// the expand stage's two forms: one wavefront per chain on XCD-affine slots (k3b_expand), or the lane-per-chain
// engine (k3c_engine): n_waves single-wave blocks whose first eng_lanes lanes own a working slice each. Only builds made
// with -DEG3D_WITH_K3C_ENGINE carry the engine; in the others no context selects it (eg3d_create refuses EG3D_K3B_ENGINE=1).
#ifdef EG3D_WITH_K3C_ENGINE
static bool engine_selected(const eg3d_ctx* c) { return c->tune.k3b_engine != 0; }
static int size_engine(eg3d_ctx* c, ExpandState& X) {
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
static void launch_engine(eg3d_ctx* c, const BatchState& B, const ExpandState& X) {
  launch_k3c(c->stream, X.eng_waves, X.eng_lanes, c->ds, B.a, c->b_tasks.as<TaskDesc>(), c->b_chains.as<ChainSeed>() + X.c0, X.nc,
             c->b_hyp_off.as<uint32_t>(), c->b_res.as<HypResult>(), c->b_arena.as<HPoint>(), c->b_map_view.as<int32_t>(),
             c->b_map_entry.as<uint32_t>(), c->b_map_n.as<uint32_t>(), X.L, c->b_cscratch.as<unsigned char>(), X.stage,
             c->b_couts.as<ChainOut>(), c->b_cpts.as<uint32_t>(), c->b_cobs.as<uint32_t>(), c->b_ctr.as<Counters>(),
             c->b_order.as<uint32_t>(), c->b_queue.as<uint32_t>(),
             (c->tune.k3b_full || c->learned.k3b_long_latched || (c->V > EG3D_SMALL_SCENE_VIEWS_HOST && !c->tune.assume_short)) ? 1 : 0);
}
#else
static bool engine_selected(const eg3d_ctx*) { return false; }
static int size_engine(eg3d_ctx*, ExpandState&) { return EG3D_OK; }
static void launch_engine(eg3d_ctx*, const BatchState&, const ExpandState&) {}
#endif

// Everything one expand launch needs, queued or allocated: the chunk and its layout, the slot pools (or the engine's grid),
// the staging area, the per-chain output counters, the launch order. A relaunch of the chains listed in b_redo (X.redo_n)
// keeps the chunk, the staging area and the order's buffers of the launch before it.
static int prepare_expand(eg3d_ctx* c, const BatchState& B, ExpandState& X) {
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
static int launch_expand(eg3d_ctx* c, const BatchState& B, bool device_only, ExpandState& X) {
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
static int redo_whole_chunk(eg3d_ctx* c, ExpandState& X, bool drain) {
  X.redo_n = 0;
  HIP_TRY(hipMemcpyAsync(&c->b_ctr.as<Counters>()->bytes, saved_bytes(c), sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                         c->stream));
  if (drain) HIP_TRY(hipStreamSynchronize(c->stream));
  return EG3D_OK;
}

// The verdict on the launch X describes, from its counters and totals; what a redo needs (the latched build, the learned
// staging need, the doubled capacities, the list of chains) is in place when it returns.
static int judge_expand(eg3d_ctx* c, HostOut& H, ExpandState& X, Expand* verdict) {
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
static int emit_chunk(eg3d_ctx* c, const BatchState& B, UnitTurn& T, HostOut& H, const ExpandState& X, bool last_chunk) {
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
static int copy_chunk_to_host(eg3d_ctx* c, const BatchState& B, UnitTurn& T, const ExpandState& X, bool last_chunk) {
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
static int close_chunk(eg3d_ctx* c, HostOut& H, ExpandState& X) {
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
static int stage_times_and_counts(eg3d_ctx* c, const BatchState& B, HostOut& H, const ExpandState& X) {
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

// (the steps behind count_hypotheses: a caller that judges the unit's totals first — run_items_batch — enters here)
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
int run_stage_b(eg3d_ctx* c, BatchState& B, UnitTurn& T, HostOut& H) {
  BUF_TRY(count_hypotheses(c, B));
  return run_stage_b_counted(c, B, T, H);
}

EG3D_API_END
