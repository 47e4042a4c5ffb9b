// eg3d_api_candidates.hip — stage A alone, dumped to the host for tests and diagnostics (include/eg3d.h). Top to bottom:
// eg3d_polyline_set_candidates (the extractor's samples and epipolar hits, run_items_stage_a of eg3d_api_match_sets.hip) and
// its free; eg3d_candidates_run (the seed path's candidates, start hits, tasks and hits, run_stage_a of eg3d_api_match.hip)
// and its free. Each runs its whole range as ONE batch on the context's own stream. Host orchestration only.
#include "eg3d_api_match_internal.h"

EG3D_API_BEGIN
template <typename T>
static T* dup_to_malloc(const std::vector<T>& v, size_t extra = 0) {
  T* p = (T*)malloc(sizeof(T) * std::max<size_t>(1, v.size() + extra));
  if (!v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}
EG3D_API_END

// Stage A of the extractor alone, the whole range as ONE batch on the context's own stream.
extern "C" int eg3d_polyline_set_candidates(eg3d_ctx* c, const eg3d_polyline_sets* ps, uint32_t set_b, uint32_t set_e,
                                            const eg3d_matched_intervals* m, eg3d_set_candidates* out) {
  BUF_TRY(open_sets_call("eg3d_polyline_set_candidates", c, ps, set_b, set_e, out));
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
  const uint32_t item_b = ps->row_off[(size_t)set_b * V], item_e = ps->row_off[(size_t)set_e * V];
  BUF_TRY(run_items_stage_a(c, sd, ps->n_sets * V, item_b, item_e, matched, &skip_cnt, &drop_cnt, B));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const uint32_t nt = B.n_tasks;
  const uint32_t n_items = item_e - item_b;
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

