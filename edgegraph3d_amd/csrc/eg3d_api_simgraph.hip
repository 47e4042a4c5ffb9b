// eg3d_api_simgraph.hip — pipeline 1's polyline compatibility graph (K10, eg3d_k10_simgraph.hip)
#include "eg3d_api_internal.h"

// Edge keys one chunk of the clique expansion writes when EG3D_SIMGRAPH_PAIR_BUDGET does not say.
#ifndef EG3D_SIMGRAPH_PAIR_BUDGET_DEFAULT
#define EG3D_SIMGRAPH_PAIR_BUDGET_DEFAULT (1ull << 22)
#endif

extern "C" void eg3d_free_simgraph(eg3d_simgraph* g) {
  if (!g) return;
  void* all[] = {g->node_view, g->node_pl, g->adj_off, g->adj_node, g->adj_w, g->point_weight, g->cp_off, g->cp_view, g->cp_pl,
                 g->cr_off, g->cr_point};
  for (void* p : all) free(p);
  memset(g, 0, sizeof(*g));
}

extern "C" int eg3d_similarity_graph(eg3d_ctx* c, const eg3d_seeds* seeds, uint32_t b, uint32_t e, eg3d_simgraph* out,
                                     eg3d_simgraph_stats* stats) {
  static const char who[] = "eg3d_similarity_graph";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_simgraph_stats", stats->struct_size, sizeof(eg3d_simgraph_stats)));
  SeedRange r;  // k10_ctr: [0] flags, [1] nodes, [2] distinct edges, [3] kept edges
  BUF_TRY(open_seed_range(c, who, seeds, b, e, out, &eg3d_ctx::k10_ctr, &eg3d_ctx::k10_svseed, &r));
  hipStream_t st = c->stream;
  c->k10_valid = false;
  const uint32_t V = (uint32_t)c->V, NP = c->n_pl, n_pts = r.n_seeds, sv_base = r.sv_base, n_sv = r.n_sv;
  const uint64_t budget = c->tune.simgraph_pair_budget ? c->tune.simgraph_pair_budget : EG3D_SIMGRAPH_PAIR_BUDGET_DEFAULT;
  uint32_t n_pair = 0, n_nodes = 0, n_uniq = 0, n_kept = 0, n_chunks = 0;
  uint64_t n_inst = 0;
  float ms_search = 0, ms_graph = 0, ms_weights = 0, ms_copy = 0;
  const SeedsDev& sd = r.sd;
  if (r.active) {
    const K9Grid& g10 = r.g10;
    // ---- the search, list form: count, scan, fill
    BUF_TRY(c->k10_cnt.ensure(sizeof(uint32_t) * ((size_t)n_sv + 1)));
    BUF_TRY(c->k10_off.ensure(sizeof(uint32_t) * ((size_t)n_sv + 1)));
    uint32_t* cnt = c->k10_cnt.as<uint32_t>();
    uint32_t* off = c->k10_off.as<uint32_t>();
    HIP_TRY(hipEventRecord(c->ea[0], st));
    HIP_TRY(hipMemsetAsync(cnt + n_sv, 0, sizeof(uint32_t), st));
    launch_k10_close_list(st, false, c->ds, g10, sd, sv_base, n_sv, c->k10_svseed.as<uint32_t>(), cnt, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_queue_u32(c, cnt, off, (size_t)n_sv + 1, 0));
    {
      Readback rb(c);
      const int it = rb.add(off + n_sv, 1);
      const int iw = rb.add(c->b_scanchk.as<uint32_t>(), 1);
      rb.clear_after(c->b_scanchk.as<uint32_t>());
      BUF_TRY(rb.run());
      if (*rb.item(iw)) return wrapped_error("close polylines");
      n_pair = *rb.item(it);
    }
    for (int k = 0; k < 2; k++) BUF_TRY(c->k10_pair[k].ensure(8 * std::max<size_t>(n_pair, 1)));
    unsigned long long* pair[2] = {c->k10_pair[0].as<unsigned long long>(), c->k10_pair[1].as<unsigned long long>()};
    launch_k10_close_list(st, true, c->ds, g10, sd, sv_base, n_sv, c->k10_svseed.as<uint32_t>(), nullptr, off, pair[0]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[0], st));
    HIP_TRY(hipEventRecord(c->ea[1], st));
    HIP_TRY(hipEventRecord(c->eb[1], st));  // (re-recorded below: both pairs are always defined)
    HIP_TRY(hipEventRecord(c->ea[2], st));
    HIP_TRY(hipEventRecord(c->eb[2], st));
  }
  if (n_pair) {
    // ---- close_polylines, close_refpoints, the weights, the nodes
    HIP_TRY(hipEventRecord(c->ea[1], st));
    const uint32_t vis_words = (V + 31u) / 32u;
    BUF_TRY(c->k10_crkey.ensure(8 * (size_t)n_pair));
    BUF_TRY(c->k10_cpoff.ensure(4 * ((size_t)n_pts + 1)));
    BUF_TRY(c->k10_cpview.ensure(4 * (size_t)n_pair));
    BUF_TRY(c->k10_cppl.ensure(4 * (size_t)n_pair));
    BUF_TRY(c->k10_croff.ensure(4 * ((size_t)NP + 1)));
    BUF_TRY(c->k10_crpoint.ensure(4 * (size_t)n_pair));
    BUF_TRY(c->k10_weight.ensure(4 * (size_t)n_pts));
    BUF_TRY(c->k10_vis.ensure(4 * (size_t)n_pts * vis_words));
    BUF_TRY(c->k10_npairs.ensure(8 * ((size_t)n_pts + 1)));
    BUF_TRY(c->k10_pairoff.ensure(8 * ((size_t)n_pts + 1)));
    for (int k = 0; k < 2; k++) BUF_TRY(c->k10_nkey[k].ensure(8 * (size_t)NP));
    BUF_TRY(c->k10_nodeof.ensure(4 * (size_t)NP));
    BUF_TRY(c->k10_nodeg.ensure(4 * (size_t)NP));
    BUF_TRY(c->k10_nodeview.ensure(4 * (size_t)NP));
    BUF_TRY(c->k10_nodepl.ensure(4 * (size_t)NP));
    uint32_t* ctr = c->k10_ctr.as<uint32_t>();
    unsigned long long* const raw = c->k10_pair[0].as<unsigned long long>();
    unsigned long long* const pair = c->k10_pair[1].as<unsigned long long>();    // point << 32 | g, ascending
    unsigned long long* const crkey = c->k10_crkey.as<unsigned long long>();     // g << 32 | point, ascending
    unsigned long long* const pair_off = c->k10_pairoff.as<unsigned long long>();
    BUF_TRY(sort_keys_u64(c, raw, pair, n_pair));
    launch_k10_pairs(st, c->ds, pair, n_pair, c->k10_cpview.as<uint32_t>(), c->k10_cppl.as<uint32_t>(), raw);
    launch_k10_row_off(st, pair, n_pair, b, n_pts, c->k10_cpoff.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, raw, crkey, n_pair));
    launch_k10_low_words(st, crkey, n_pair, c->k10_crpoint.as<uint32_t>());
    launch_k10_row_off(st, crkey, n_pair, 0, NP, c->k10_croff.as<uint32_t>());
    launch_k10_points(st, sd, b, n_pts, c->k10_cpoff.as<uint32_t>(), c->k10_cpview.as<uint32_t>(), vis_words,
                      c->k10_weight.as<float>(), c->k10_vis.as<uint32_t>(), c->k10_npairs.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u64(c, c->k10_npairs.as<unsigned long long>(), pair_off, (size_t)n_pts + 1));
    launch_k10_node_keys(st, NP, c->k10_croff.as<uint32_t>(), c->k10_crpoint.as<uint32_t>(), c->k10_nkey[0].as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, c->k10_nkey[0].as<unsigned long long>(), c->k10_nkey[1].as<unsigned long long>(), NP));
    launch_k10_nodes(st, c->ds, c->k10_nkey[1].as<unsigned long long>(), NP, c->k10_nodeof.as<uint32_t>(), c->k10_nodeg.as<uint32_t>(),
                     c->k10_nodeview.as<uint32_t>(), c->k10_nodepl.as<uint32_t>(), ctr + 1);
    HIP_TRY(hipGetLastError());
    {
      Readback rb(c);
      const int in = rb.add(ctr + 1, 1);
      const int ip = rb.add(pair_off + n_pts, 2);
      BUF_TRY(rb.run());
      n_nodes = *rb.item(in);
      n_inst = (uint64_t)rb.item(ip)[0] | ((uint64_t)rb.item(ip)[1] << 32);
    }
    K10Graph g;
    g.seed_begin = b;
    g.n_pts = n_pts;
    g.n_pl = NP;
    g.vis_words = vis_words;
    g.pair = pair;
    g.cp_off = c->k10_cpoff.as<uint32_t>();
    g.cr_off = c->k10_croff.as<uint32_t>();
    g.cr_point = c->k10_crpoint.as<uint32_t>();
    g.weight = c->k10_weight.as<float>();
    g.vis = c->k10_vis.as<uint32_t>();
    g.node_g = c->k10_nodeg.as<uint32_t>();
    g.node_view = c->k10_nodeview.as<uint32_t>();
    // ---- the distinct edges: the cliques a chunk of pair instances at a time, each chunk written behind the distinct keys
    // so far (k10_edge[0]), the whole sorted (k10_edge[1]) and made distinct again (k10_edge[0])
    for (uint64_t t0 = 0; t0 < n_inst; t0 += budget) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(budget, n_inst - t0);
      const size_t total = (size_t)n_uniq + n;
      BUF_TRY(c->k10_edge[0].ensure_keep(8 * total, 8 * (size_t)n_uniq, st));
      BUF_TRY(c->k10_edge[1].ensure(8 * total));
      unsigned long long* const ek0 = c->k10_edge[0].as<unsigned long long>();
      unsigned long long* const ek1 = c->k10_edge[1].as<unsigned long long>();
      launch_k10_expand(st, g, pair_off, c->k10_nodeof.as<uint32_t>(), t0, n, ek0 + n_uniq);
      HIP_TRY(hipGetLastError());
      BUF_TRY(sort_keys_u64(c, ek0, ek1, total));
      BUF_TRY(unique_u64(c, ek1, ek0, ctr + 2, total));
      Readback rb(c);
      const int iu = rb.add(ctr + 2, 1);
      BUF_TRY(rb.run());
      n_uniq = *rb.item(iu);
      n_chunks++;
      if (n_uniq >= 0x80000000u) {
        g_err = "eg3d_similarity_graph: the graph has 2^31 or more distinct edges (adjacency offsets are 32-bit)";
        return EG3D_ERR_CAPACITY;
      }
    }
    HIP_TRY(hipEventRecord(c->eb[1], st));
    // ---- the edge weights and the adjacency
    HIP_TRY(hipEventRecord(c->ea[2], st));
    BUF_TRY(c->k10_adjoff.ensure(4 * ((size_t)n_nodes + 1)));
    if (n_uniq) {
      for (int k = 0; k < 2; k++) {
        BUF_TRY(c->k10_dkey[k].ensure(16 * (size_t)n_uniq));
        BUF_TRY(c->k10_dval[k].ensure(8 * (size_t)n_uniq));
      }
      launch_k10_edge_weights(st, g, c->k10_edge[0].as<unsigned long long>(), n_uniq, c->k10_dkey[0].as<unsigned long long>(),
                              c->k10_dval[0].as<uint32_t>(), ctr + 3);
      HIP_TRY(hipGetLastError());
      BUF_TRY(sort_pairs_u64_u32(c, c->k10_dkey[0].as<unsigned long long>(), c->k10_dkey[1].as<unsigned long long>(),
                             c->k10_dval[0].as<uint32_t>(), c->k10_dval[1].as<uint32_t>(), 2 * (size_t)n_uniq));
      Readback rb(c);
      const int ik = rb.add(ctr + 3, 1);
      BUF_TRY(rb.run());
      n_kept = *rb.item(ik);
      BUF_TRY(c->k10_adjnode.ensure(8 * std::max<size_t>(n_kept, 1)));
      launch_k10_low_words(st, c->k10_dkey[1].as<unsigned long long>(), 2 * n_kept, c->k10_adjnode.as<uint32_t>());
    }
    // (directed keys that are not kept sort behind every node's: the offsets look at the kept ones only)
    launch_k10_row_off(st, c->k10_dkey[1].as<unsigned long long>(), 2 * n_kept, 0, n_nodes, c->k10_adjoff.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[2], st));
  }
  if (r.active) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms_search, c->ea[0], c->eb[0]));
    HIP_TRY(hipEventElapsedTime(&ms_graph, c->ea[1], c->eb[1]));
    HIP_TRY(hipEventElapsedTime(&ms_weights, c->ea[2], c->eb[2]));
  }
  // ---- the result, library-owned
  const auto t0 = std::chrono::steady_clock::now();
  eg3d_simgraph m;
  memset(&m, 0, sizeof(m));
  const size_t n_adj = 2 * (size_t)n_kept;
  const auto dev = [&](const DevBuf& w) { return n_pair ? w.p : nullptr; };  // (an empty range: all-zero arrays of their sizes)
  BUF_TRY(copy_out(st, who,
                   {{&m.node_view, dev(c->k10_nodeview), 4 * (size_t)n_nodes}, {&m.node_pl, dev(c->k10_nodepl), 4 * (size_t)n_nodes},
                    {&m.adj_off, dev(c->k10_adjoff), 4 * ((size_t)n_nodes + 1)}, {&m.adj_node, dev(c->k10_adjnode), 4 * n_adj},
                    {&m.adj_w, dev(c->k10_dval[1]), 4 * n_adj}, {&m.point_weight, dev(c->k10_weight), 4 * (size_t)n_pts},
                    {&m.cp_off, dev(c->k10_cpoff), 4 * ((size_t)n_pts + 1)}, {&m.cp_view, dev(c->k10_cpview), 4 * (size_t)n_pair},
                    {&m.cp_pl, dev(c->k10_cppl), 4 * (size_t)n_pair}, {&m.cr_off, dev(c->k10_croff), 4 * ((size_t)NP + 1)},
                    {&m.cr_point, dev(c->k10_crpoint), 4 * (size_t)n_pair}}));
  m.n_nodes = n_nodes;
  m.seed_begin = b;
  m.n_points = n_pts;
  m.n_polylines = NP;
  ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = m;
  c->k10_valid = true;  // (k10_nodeview / k10_nodepl hold the n_nodes nodes: eg3d_sets_from_communities_device reads them there)
  c->k10_nodes = n_nodes;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_simgraph_stats);
    stats->n_entries = n_sv;
    stats->n_nodes = n_nodes;
    stats->n_edges = n_kept;
    stats->n_pair_instances = n_inst;
    stats->n_chunks = n_chunks;
    stats->ms_grid = r.ms_grid;
    stats->ms_search = ms_search;
    stats->ms_graph = ms_graph;
    stats->ms_weights = ms_weights;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}
