// eg3d_api_polymatch.hip — polyline matching by closeness to the reference points (K9, eg3d_k9_polymatch.hip)
#include "eg3d_api_internal.h"

extern "C" void eg3d_free_polyline_matches(eg3d_polyline_matches* m) {
  if (!m) return;
  free(m->refpoints);
  free(m->row_off);
  free(m->pl_ids);
  memset(m, 0, sizeof(*m));
}

// `forced` (tests): per-entry results that take the place of the search's, host arrays of n_sv entries each
struct K9Forced {
  const uint32_t* cnt;
  const uint32_t* pl;
  const float* dist;
};
static int polymatch_impl(eg3d_ctx* c, const eg3d_seeds* seeds, uint32_t b, uint32_t e, const K9Forced* forced,
                          eg3d_polyline_matches* out, eg3d_polymatch_stats* stats) {
  static const char who[] = "eg3d_match_polylines_closeness";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_polymatch_stats", stats->struct_size, sizeof(eg3d_polymatch_stats)));
  SeedRange r;
  BUF_TRY(open_seed_range(c, who, seeds, b, e, out, &eg3d_ctx::k9_ctr, &eg3d_ctx::k9_svseed, &r));  // k9_ctr: [0] flags, [1] nodes, [2] sets
  hipStream_t st = c->stream;
  const uint32_t V = (uint32_t)c->V, NP = c->n_pl, n_seeds = r.n_seeds, sv_base = r.sv_base, n_sv = r.n_sv;
  c->rs_k9.valid = false;  // (k9_rowoff / k9_plids are rewritten: eg3d_polyline_matches_device views them once this call is through)
  uint32_t n_acc = 0, n_nodes = 0, n_sets = 0;
  float ms_search = 0, ms_comp = 0, ms_copy = 0;
  if (r.active) {
    const K9Grid& g10 = r.g10;
    const SeedsDev& sd = r.sd;
    uint32_t* ctr = c->k9_ctr.as<uint32_t>();
    // ---- the search
    BUF_TRY(c->k9_cnt.ensure(sizeof(uint32_t) * n_sv));
    BUF_TRY(c->k9_pl.ensure(sizeof(uint32_t) * n_sv));
    BUF_TRY(c->k9_dist.ensure(sizeof(float) * n_sv));
    const K9Entries ent{c->k9_cnt.as<uint32_t>(), c->k9_pl.as<uint32_t>(), c->k9_dist.as<float>()};
    HIP_TRY(hipEventRecord(c->ea[0], st));  // ms_search: the search kernel alone
    if (!forced) {
      launch_k9_close_polylines(st, c->ds, g10, sd, sv_base, n_sv, c->k9_svseed.as<uint32_t>(), ent);
      HIP_TRY(hipGetLastError());
    } else {
      HIP_TRY(hipMemcpyAsync(ent.cnt, forced->cnt, sizeof(uint32_t) * n_sv, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(ent.pl, forced->pl, sizeof(uint32_t) * n_sv, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(ent.dist, forced->dist, sizeof(float) * n_sv, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));  // (pageable host arrays of the caller)
    }
    HIP_TRY(hipEventRecord(c->eb[0], st));
    // ---- the rule, the match graph, its components and their order
    BUF_TRY(c->k9_acc.ensure(sizeof(uint32_t) * ((size_t)n_seeds + 1)));
    BUF_TRY(c->k9_accoff.ensure(sizeof(uint32_t) * ((size_t)n_seeds + 1)));
    BUF_TRY(c->k9_first.ensure(8 * (size_t)NP));
    BUF_TRY(c->k9_ckey.ensure(8 * (size_t)NP));
    BUF_TRY(c->k9_parent.ensure(4 * (size_t)NP));
    BUF_TRY(c->k9_root.ensure(4 * (size_t)NP));
    BUF_TRY(c->k9_rank.ensure(4 * (size_t)NP));
    for (int k = 0; k < 2; k++) BUF_TRY(c->k9_key[k].ensure(8 * (size_t)NP));
    const K9Graph g{c->k9_first.as<unsigned long long>(), c->k9_parent.as<uint32_t>(), c->k9_root.as<uint32_t>(),
                    c->k9_ckey.as<unsigned long long>(), c->k9_rank.as<uint32_t>()};
    unsigned long long* key[2] = {c->k9_key[0].as<unsigned long long>(), c->k9_key[1].as<unsigned long long>()};
    HIP_TRY(hipEventRecord(c->ea[1], st));
    launch_k9_init(st, NP, g);
    launch_k9_refpoint_rule(st, c->ds, sd, b, n_seeds, sv_base, ent, c->k9_acc.as<uint32_t>(), g);
    launch_k9_flatten(st, NP, g, ctr + 1);
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, g.ckey, key[0], NP));
    launch_k9_rank(st, key[0], NP, g, ctr + 2);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_queue_u32(c, c->k9_acc.as<uint32_t>(), c->k9_accoff.as<uint32_t>(), (size_t)n_seeds + 1, 0));
    {
      Readback rb(c);
      const int ic = rb.add(ctr + 1, 2);
      const int ia = rb.add(c->k9_accoff.as<uint32_t>() + n_seeds, 1);
      const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 1);
      rb.clear_after(c->b_scanchk.as<uint32_t>());
      BUF_TRY(rb.run());
      if (*rb.item(iw)) return wrapped_error("accepted reference points");
      n_nodes = rb.item(ic)[0];
      n_sets = rb.item(ic)[1];
      n_acc = *rb.item(ia);
    }
    if ((uint64_t)n_sets * V >= 0xffffffffull) {
      g_err = "eg3d_match_polylines_closeness: the result has more than 2^32-2 rows (sets x views)";
      return EG3D_ERR_CAPACITY;
    }
    BUF_TRY(c->k9_ref.ensure(sizeof(uint32_t) * std::max<size_t>(n_acc, 1)));
    BUF_TRY(c->k9_rowoff.ensure(sizeof(uint32_t) * ((size_t)n_sets * V + 1)));
    BUF_TRY(c->k9_plids.ensure(sizeof(uint32_t) * std::max<size_t>(n_nodes, 1)));
    launch_k9_compact(st, c->k9_acc.as<uint32_t>(), c->k9_accoff.as<uint32_t>(), b, n_seeds, c->k9_ref.as<uint32_t>());
    if (n_nodes) {
      launch_k9_node_keys(st, c->ds, NP, g, key[0]);
      HIP_TRY(hipGetLastError());
      BUF_TRY(sort_keys_u64(c, key[0], key[1], NP));
      launch_k0_csr(st, key[1], n_nodes, n_sets * V, c->k9_rowoff.as<uint32_t>(), c->k9_plids.as<uint32_t>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms_search, c->ea[0], c->eb[0]));
    HIP_TRY(hipEventElapsedTime(&ms_comp, c->ea[1], c->eb[1]));
  }
  // ---- the result, library-owned
  const auto t0 = std::chrono::steady_clock::now();
  eg3d_polyline_matches m;
  memset(&m, 0, sizeof(m));
  const size_t n_rows1 = (size_t)n_sets * V + 1;
  BUF_TRY(copy_out(st, who, {{&m.refpoints, c->k9_ref.p, sizeof(uint32_t) * n_acc},
                             {&m.row_off, n_sets ? c->k9_rowoff.p : nullptr, sizeof(uint32_t) * n_rows1},
                             {&m.pl_ids, c->k9_plids.p, sizeof(uint32_t) * n_nodes}}));
  m.n_refpoints = n_acc;
  m.n_sets = n_sets;
  ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = m;
  c->rs_k9.valid = true;
  c->rs_k9.n_sets = n_sets;
  c->rs_k9.n_ids = n_nodes;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_polymatch_stats);
    stats->n_entries = n_sv;
    stats->n_accepted = n_acc;
    stats->n_nodes = n_nodes;
    stats->n_sets = n_sets;
    stats->ms_grid = r.ms_grid;
    stats->ms_search = ms_search;
    stats->ms_components = ms_comp;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}
extern "C" int eg3d_match_polylines_closeness(eg3d_ctx* c, const eg3d_seeds* seeds, uint32_t b, uint32_t e,
                                              eg3d_polyline_matches* out, eg3d_polymatch_stats* stats) {
  return polymatch_impl(c, seeds, b, e, nullptr, out, stats);
}
/* Tests only, not declared in include/eg3d.h (tests/test_gpu_polymatch.py).
 * eg3d_polymatch_test_entries: the per-entry results the last eg3d_match_polylines_closeness call on this context left on the
 * device (n = its stats.n_entries): polylines within 10 px, the first one's id and its distance.
 * eg3d_polymatch_test_rule: the matcher on the uploaded seeds [b, e) with the CALLER's per-entry results (one per track entry
 * of the range; a polyline id must lie inside its view) in place of the search: the rule, the graph and the order alone. */
extern "C" int eg3d_polymatch_test_entries(eg3d_ctx* c, uint32_t n, uint32_t* cnt, uint32_t* pl, float* dist) {
  if (!c || (size_t)n * 4 > c->k9_cnt.cap || (size_t)n * 4 > c->k9_pl.cap || (size_t)n * 4 > c->k9_dist.cap) {
    g_err = "eg3d_polymatch_test_entries: bad arguments";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n) {
    HIP_TRY(hipMemcpy(cnt, c->k9_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pl, c->k9_pl.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dist, c->k9_dist.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  }
  return EG3D_OK;
}
extern "C" int eg3d_polymatch_test_rule(eg3d_ctx* c, uint32_t b, uint32_t e, const uint32_t* cnt, const uint32_t* pl,
                                        const float* dist, eg3d_polyline_matches* out) {
  if (!cnt || !pl || !dist) {
    g_err = "eg3d_polymatch_test_rule: bad arguments";
    return EG3D_ERR_ARG;
  }
  const K9Forced f{cnt, pl, dist};
  return polymatch_impl(c, nullptr, b, e, &f, out, nullptr);
}
