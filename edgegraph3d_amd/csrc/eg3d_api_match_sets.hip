// eg3d_api_match_sets.hip — the polyline-set path of the match pipeline (pipelines 1-2 extractor):
// eg3d_check_polyline_sets, eg3d_match_polyline_sets[_matched] on host sets, and the two calls on item ranges of resident
// sets behind eg3d_api_sets.hip (count_item_samples, match_items_call). Top to bottom: stage A of the extractor (its
// count pass, the refusal of intervals that are not the scene's, run_items_stage_a) and one unit, run_items_batch; what a
// call's inputs go through (eg3d_check_polyline_sets, prepare_matched, open_sets_call, prepare_sets); the calls. Stage B
// and the units on lanes are the seed path's (eg3d_api_match_internal.h), the cuts eg3d_unit_plan.h's. Host orchestration
// only: the kernels are in eg3d_n1_sets.hip.
#include <atomic>

#include "eg3d_api_match_internal.h"

EG3D_API_BEGIN

static int bad_matched(const char* what) {
  g_err = std::string("eg3d_match_polyline_sets_matched: ") + what;
  return EG3D_ERR_ARG;
}

// The count pass of k_n1_samples over items [item_b, item_b + n_items), queued on the context's stream behind a zeroed
// b_ctr: the counts in b_raw_cnt, their exclusive scan in b_raw_off (n_items + 1 words), the total on the host. `begin`
// (null: none) is recorded behind the memsets, in front of the launch; skip_cnt (may be null) receives the per-item counts
// of samples left out under `matched`.
static int count_pass(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t n_items, const IvTable* matched,
                      hipEvent_t begin, DevBuf* skip_cnt, uint32_t& total) {
  hipStream_t st = c->stream;
  BUF_TRY(c->b_ctr.ensure(sizeof(Counters)));
  HIP_TRY(hipMemsetAsync(c->b_ctr.p, 0, sizeof(Counters), st));
  BUF_TRY(c->b_raw_cnt.ensure(sizeof(uint32_t) * ((size_t)n_items + 1)));
  BUF_TRY(c->b_raw_off.ensure(sizeof(uint32_t) * ((size_t)n_items + 1)));
  HIP_TRY(hipMemsetAsync(c->b_raw_cnt.as<uint32_t>() + n_items, 0, sizeof(uint32_t), st));
  if (begin) HIP_TRY(hipEventRecord(begin, st));
  if (matched && skip_cnt) BUF_TRY(skip_cnt->ensure(sizeof(uint32_t) * ((size_t)n_items + 1)));
  launch_n1_samples(st, false, c->ds, sets, n_rows, item_b, n_items, c->b_raw_cnt.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, c->b_ctr.as<Counters>(), matched,
                    matched && skip_cnt ? skip_cnt->as<uint32_t>() : nullptr);
  return scan_total_u32(c, c->b_raw_cnt.as<uint32_t>(), c->b_raw_off.as<uint32_t>(), (size_t)n_items + 1, total, "samples");
}

// A walk of k_n1_samples under `matched` that did not advance raised CTR_N1_NO_PROGRESS in b_ctr (the stream is idle; stage
// B clears the flags, so it is read before): the intervals are another scene's, and the call is refused.
static int refuse_no_progress(eg3d_ctx* c) {
  uint32_t flags = 0;
  HIP_TRY(hipMemcpy(&flags, &c->b_ctr.as<Counters>()->flags, sizeof(flags), hipMemcpyDeviceToHost));
  if (flags & CTR_N1_NO_PROGRESS)
    return bad_matched("the walk does not advance past a matched interval: the intervals do not belong to this scene");
  return EG3D_OK;
}

// Stage A of the extractor: sample the polylines of items [item_b, item_e) — entries of pl_ids; a run of whole sets is the
// items of its rows — and collect the epipolar hits of every sample. `sets` is already on the device.
// `matched` (null: none) is the caller's interval table on the device: samples and hits inside a held interval are left out
// (k_n1_samples / k_n1_hits <., true>); skip_cnt / drop_cnt (may be null) receive the per-polyline / per-task counts of them.
int run_items_stage_a(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows_total, uint32_t item_b, uint32_t item_e,
                      const IvTable* matched, DevBuf* skip_cnt, DevBuf* drop_cnt, BatchState& B) {
  hipStream_t st = c->stream;
  const uint32_t V = (uint32_t)c->V;
  memset(&B, 0, sizeof(B));
  B.key0_base = 0;  // (key[0] = sample index of the CALL: the sink adds the samples of the units before this one)
  const uint32_t n_items = item_e - item_b;
  BUF_TRY(count_pass(c, sets, n_rows_total, item_b, n_items, matched, c->ea[1], skip_cnt, B.n_tasks));
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
  if (matched) BUF_TRY(refuse_no_progress(c));
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

// One unit of a polyline-set call, items [item_b, item_e): stage A above, then the common stage B.
// `wrapped` (null: the unit runs or the call fails, as eg3d_match_polyline_sets does): the caller can cut the unit. The
// unit's 32-bit totals — samples x views, epipolar hits, hypotheses — are all known before the first chain is followed;
// where one does not fit (or exceeds wrap_limit, EG3D_TEST_ITEM_WRAP; 0 = no such limit), *wrapped is set and EG3D_OK
// returned with nothing placed, nothing counted into H and the turn untouched.
static int run_items_batch(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows_total, uint32_t item_b, uint32_t item_e,
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

EG3D_API_END

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

EG3D_API_BEGIN

// The caller's matched_polyline_intervals for the duration of ONE call (MatchedCall): host arrays are uploaded into the
// DevBufs here, device arrays are read in place. Everything is checked before anything is indexed with it: what needs no
// scene on the host for host arrays (their total sizes the upload), then check_interval_row, one lane per row, for both kinds.
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

int open_sets_call(const char* who, const eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e, const void* out) {
  if (!c || !ps || !out || !ps->row_off || set_b > set_e || set_e > ps->n_sets) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if ((uint64_t)ps->n_sets * (uint64_t)c->V > 0xffffffffull) {
    g_err = std::string(who) + ": too many rows";
    return EG3D_ERR_ARG;
  }
  return EG3D_OK;
}

// the checks and the upload of the sets, shared by the calls on host polyline sets (behind open_sets_call: the rows fit)
int prepare_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, SetsDev& sd) {
  const uint32_t V = (uint32_t)c->V;
  const uint32_t n_rows = ps->n_sets * V;
  const uint32_t n_ids = ps->row_off[n_rows];
  if (n_ids && !ps->pl_ids) {  // (before any id is read)
    g_err = "eg3d_match_polyline_sets: pl_ids is null";
    return EG3D_ERR_ARG;
  }
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
  BUF_TRY(eg3d_check_polyline_sets(ps, c->V));  // (the checks that need no scene: rows are sets)
  BUF_TRY(upload(c->b_sets_off, ps->row_off, (size_t)n_rows + 1, c->stream));
  BUF_TRY(upload(c->b_sets_ids, ps->pl_ids, n_ids, c->stream));
  sd.n_views = V;
  sd.row_off = c->b_sets_off.as<uint32_t>();
  sd.pl_ids = c->b_sets_ids.as<uint32_t>();
  HIP_TRY(hipStreamSynchronize(c->stream));  // the sets are resident before any lane reads them
  return EG3D_OK;
}

// eg3d_match_polyline_sets, with the intervals of `m` when given
static int match_sets_call(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                           const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out, eg3d_stage_times* times) {
  BUF_TRY(open_sets_call("eg3d_match_polyline_sets", c, ps, set_b, set_e, out));
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
  // units = runs of whole sets, bounded by the number of polylines (every sample owns V lists: a piece above the bound is
  // cut into runs of whole sets within it); with several lanes at least one unit per lane, balanced by the number of polylines
  const uint32_t max_items = V >= 64 ? 2048u : 16384u;
  const uint32_t* row_off = ps->row_off;
  const std::vector<UnitRange> units = cut_bounded(set_b, set_e, c->tune.units ? (uint32_t)c->tune.units : (uint32_t)lanes,
                                                   [&](uint32_t i) { return row_off[(size_t)i * V]; }, max_items);
  return match_call(c, device_only, true, units, lanes, out, times, [&](eg3d_ctx* lane, uint32_t u, UnitTurn& T, HostOut& H) {
    return run_items_batch(lane, sd, n_rows, row_off[(size_t)units[u].b * V], row_off[(size_t)units[u].e * V], matched, T, H);
  });
}

// ---- the extractor on item ranges (include/eg3d_sets_device.h; the entry points are in eg3d_api_sets.hip) -----------------
// The count pass alone, waited for, and its refusal under `matched`.
static int count_items(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t n_items, const IvTable* matched,
                       uint32_t& total) {
  BUF_TRY(count_pass(c, sets, n_rows, item_b, n_items, matched, nullptr, nullptr, total));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return matched ? refuse_no_progress(c) : EG3D_OK;
}

int count_item_samples(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e,
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

int match_items_call(eg3d_ctx* c, const SetsDev& sets, uint32_t n_rows, uint32_t item_b, uint32_t item_e, uint32_t sample_base,
                     const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out, eg3d_stage_times* times) {
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
  const std::vector<UnitRange> units = cut_bounded(item_b, item_e, c->tune.units ? (uint32_t)c->tune.units : (uint32_t)lanes,
                                                   [&](uint32_t i) { return pre[i - item_b]; }, unit_samples);
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

EG3D_API_END

extern "C" int eg3d_match_polyline_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                        int device_only, eg3d_edgepoints* out, eg3d_stage_times* times) {
  return match_sets_call(c, ps, set_b, set_e, nullptr, device_only, out, times);
}

extern "C" int eg3d_match_polyline_sets_matched(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                                const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out,
                                                eg3d_stage_times* times) {
  return match_sets_call(c, ps, set_b, set_e, m, device_only, out, times);
}

