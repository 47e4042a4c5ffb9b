// eg3d_api_replay.hip — the PLGMatchesManager replay on a device-resident cloud (K8, eg3d_k8_replay.hip)
#include "../../include/eg3d_host.h"
#include "eg3d_api_internal.h"

static int k8_read_u32(eg3d_ctx* c, const uint32_t* dev, uint64_t* v) {
  uint32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, dev, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *v = h;
  return EG3D_OK;
}
static uint64_t pow2_above(uint64_t n) {  // the smallest power of two > n
  uint64_t p = 1;
  while (p <= n) p <<= 1;
  return p;
}

extern "C" void eg3d_free_graph3d(eg3d_graph3d* g) {
  if (!g) return;
  void* all[] = {g->node_X, g->node_point, g->pl_start, g->pl_end, g->conn_off, g->conn_pl, g->iv_off, g->iv_start_seg,
                 g->iv_start_xy, g->iv_end_seg, g->iv_end_xy};
  for (void* p : all) free(p);
  memset(g, 0, sizeof(*g));
}

extern "C" int eg3d_replay_device(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, eg3d_device_graph3d* out_dev,
                                  eg3d_graph3d* out_host, eg3d_replay_stats* stats) {
  if (stats) BUF_TRY(check_struct_size("eg3d_replay_device", "eg3d_replay_stats", stats->struct_size, sizeof(eg3d_replay_stats)));
  if (!c) {
    g_err = "eg3d_replay_device: bad arguments";
    return EG3D_ERR_ARG;
  }
  eg3d_device_edgepoints d;
  if (cloud)
    d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, &d));
  if (d.n_points >= 0xfffffff0ull) {
    g_err = "eg3d_replay_device: n_points must stay below 0xfffffff0 (node and polyline ids are 32-bit)";
    return EG3D_ERR_CAPACITY;
  }
  BUF_TRY(check_cloud(&d, "eg3d_replay_device", true));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const CloudView in = cloud_view(&d);
  const uint64_t N = d.n_points, NP = c->n_pl, NV = c->n_vtx;

  // ---- the checks, before anything is indexed or written
  BUF_TRY(c->k8_cnt.ensure(16));
  HIP_TRY(hipMemsetAsync(c->k8_cnt.p, 0, 16, st));
  unsigned long long* cnt = c->k8_cnt.as<unsigned long long>();
  launch_k8_pairs(st, in, c->ds, cnt, (uint32_t*)(cnt + 1));
  HIP_TRY(hipGetLastError());
  uint64_t back[2];  // pairs, flags
  HIP_TRY(hipMemcpyAsync(back, cnt, sizeof(back), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t flags = (uint32_t)back[1];
  if (flags & ~K8_FLAG_HOSTONLY) {
    g_err = std::string("eg3d_replay_device: ") +
            (flags & K8_FLAG_BAD_OFFSETS ? "obs_off is not ascending within [0, n_obs]"
             : flags & K8_FLAG_BAD_VIEW  ? "view id out of range"
             : flags & K8_FLAG_BAD_PL    ? "polyline id outside its view"
                                         : "segment index outside its polyline (or a polyline without segments)");
    return EG3D_ERR_ARG;
  }
  if (flags & K8_FLAG_HOSTONLY) {
    g_err = "eg3d_replay_device: a point of a chain pair has a NaN coordinate or x or y == -1 (the reference's invalid-node "
            "rule): replay this cloud with eg3d_host_replay_matches";
    return EG3D_ERR_HOSTONLY;
  }
  const uint64_t n_pairs = back[0];

  uint64_t n_nodes = 0, n_pl = 0, n_conn = 0, n_iv = 0, slots = 0;
  float ms_graph = 0, ms_iv = 0, ms_copy = 0;
  K8Graph g{};
  c->g_valid = false;  // (the result buffers are rewritten from here on; set again with the new view at the end)
  BUF_TRY(c->g_ivoff.ensure(8 * (NP + 1)));
  g.iv_off = c->g_ivoff.as<unsigned long long>();
  if (!n_pairs) {  // an empty cloud, or one-point chains only: the all-zero graph
    BUF_TRY(c->g_conoff.ensure(8));
    g.conn_off = c->g_conoff.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(g.conn_off, 0, 8, st));
    HIP_TRY(hipMemsetAsync(g.iv_off, 0, 8 * (NP + 1), st));
  } else {
    // ---- nodes
    slots = c->tune.replay_table_bits ? std::max<uint64_t>(1ull << c->tune.replay_table_bits, pow2_above(2 * n_pairs))
                                 : pow2_above(std::max<uint64_t>(4 * n_pairs, 63));
    BUF_TRY(c->k8_slot.ensure(4 * slots));
    BUF_TRY(c->k8_last.ensure(4 * slots));
    BUF_TRY(c->k8_firstof.ensure(4 * N));
    BUF_TRY(c->k8_lastof.ensure(4 * N));
    BUF_TRY(c->k8_flag.ensure(4 * (N + 1)));
    BUF_TRY(c->k8_rank.ensure(4 * (N + 1)));
    BUF_TRY(c->k8_plid.ensure(4 * (N + 1)));
    const size_t sort_n = std::max<uint64_t>(N, 2 * n_pairs);  // the pairs' keys by point, then two incidences per polyline
    for (int k = 0; k < 2; k++) {
      BUF_TRY(c->k8_key[k].ensure(8 * sort_n));
      BUF_TRY(c->k8_val[k].ensure(4 * N));
    }
    const K8Table tab{c->k8_slot.as<uint32_t>(), c->k8_last.as<uint32_t>(), slots - 1};
    uint32_t* first_of = c->k8_firstof.as<uint32_t>();
    uint32_t* last_of = c->k8_lastof.as<uint32_t>();
    uint32_t* flag = c->k8_flag.as<uint32_t>();
    uint32_t* rank = c->k8_rank.as<uint32_t>();
    uint32_t* pl_id = c->k8_plid.as<uint32_t>();
    unsigned long long* key[2] = {c->k8_key[0].as<unsigned long long>(), c->k8_key[1].as<unsigned long long>()};
    uint32_t* val[2] = {c->k8_val[0].as<uint32_t>(), c->k8_val[1].as<uint32_t>()};
    HIP_TRY(hipEventRecord(c->ea[0], st));
    HIP_TRY(hipMemsetAsync(tab.slot, 0xFF, 4 * slots, st));
    HIP_TRY(hipMemsetAsync(tab.last, 0, 4 * slots, st));
    HIP_TRY(hipMemsetAsync(flag, 0, 4 * (N + 1), st));
    launch_k8_node_claim(st, in, tab);
    launch_k8_node_resolve(st, in, tab, first_of, flag, last_of);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u32(c, flag, rank, N + 1));
    BUF_TRY(k8_read_u32(c, rank + N, &n_nodes));
    BUF_TRY(c->g_nodeX.ensure(12 * n_nodes));
    BUF_TRY(c->g_nodept.ensure(8 * n_nodes));
    BUF_TRY(c->g_conoff.ensure(8 * (n_nodes + 1)));
    g.node_X = c->g_nodeX.as<float>();
    g.node_point = c->g_nodept.as<unsigned long long>();
    g.conn_off = c->g_conoff.as<unsigned long long>();
    launch_k8_node_write(st, in, first_of, flag, rank, last_of, g, key[0], val[0]);
    HIP_TRY(hipGetLastError());
    // ---- polylines: a stable sort keeps the pairs of one connection in cloud order, the first of a run creates it
    BUF_TRY(sort_pairs_u64_u32(c, key[0], key[1], val[0], val[1], N));
    HIP_TRY(hipMemsetAsync(flag, 0, 4 * (N + 1), st));
    launch_k8_pl_heads(st, key[1], val[1], n_pairs, flag);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u32(c, flag, pl_id, N + 1));
    BUF_TRY(k8_read_u32(c, pl_id + N, &n_pl));
    BUF_TRY(c->g_pls.ensure(4 * n_pl));
    BUF_TRY(c->g_ple.ensure(4 * n_pl));
    BUF_TRY(c->g_conpl.ensure(8 * n_pl));
    g.pl_start = c->g_pls.as<uint32_t>();
    g.pl_end = c->g_ple.as<uint32_t>();
    g.conn_pl = c->g_conpl.as<uint32_t>();
    launch_k8_pl_write(st, in, first_of, rank, flag, pl_id, g, key[0]);
    HIP_TRY(hipGetLastError());
    // ---- connections: the (node, polyline) incidences sorted = every node's polylines in ascending id
    BUF_TRY(sort_keys_u64(c, key[0], key[1], 2 * n_pl));
    launch_k8_conn(st, key[1], 2 * n_pl, n_nodes, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[0], st));
    HIP_TRY(hipMemcpyAsync(&n_conn, g.conn_off + n_nodes, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms_graph, c->ea[0], c->eb[0]));
    // ---- matched intervals: the claim map is indexed by the scene's global segment index
    BUF_TRY(c->k8_map.ensure(8 * std::max<uint64_t>(NV, 1)));
    BUF_TRY(c->k8_sflag.ensure(4 * (NV + 1)));
    BUF_TRY(c->k8_pos.ensure(4 * (NV + 1)));
    unsigned long long* map = c->k8_map.as<unsigned long long>();
    uint32_t* pos = c->k8_pos.as<uint32_t>();
    HIP_TRY(hipEventRecord(c->ea[0], st));
    HIP_TRY(hipMemsetAsync(map, 0xFF, 8 * std::max<uint64_t>(NV, 1), st));
    launch_k8_iv(st, false, in, c->ds, map, pos, g);
    launch_k8_seg_flags(st, map, NV, c->k8_sflag.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u32(c, c->k8_sflag.as<uint32_t>(), pos, NV + 1));
    BUF_TRY(k8_read_u32(c, pos + NV, &n_iv));
    BUF_TRY(c->g_ivss.ensure(4 * n_iv));
    BUF_TRY(c->g_ives.ensure(4 * n_iv));
    BUF_TRY(c->g_ivsxy.ensure(8 * n_iv));
    BUF_TRY(c->g_ivexy.ensure(8 * n_iv));
    g.iv_start_seg = c->g_ivss.as<uint32_t>();
    g.iv_end_seg = c->g_ives.as<uint32_t>();
    g.iv_start_xy = c->g_ivsxy.as<float>();
    g.iv_end_xy = c->g_ivexy.as<float>();
    launch_k8_iv(st, true, in, c->ds, map, pos, g);
    launch_k8_iv_off(st, c->ds, (uint32_t)NP, pos, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->eb[0], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms_iv, c->ea[0], c->eb[0]));
  }

  if (out_host) {
    const auto t0 = std::chrono::steady_clock::now();
    eg3d_graph3d h;
    memset(&h, 0, sizeof(h));
    BUF_TRY(copy_out(st, "eg3d_replay_device",
                     {{&h.node_X, g.node_X, 12 * n_nodes},      {&h.node_point, g.node_point, 8 * n_nodes},
                      {&h.pl_start, g.pl_start, 4 * n_pl},      {&h.pl_end, g.pl_end, 4 * n_pl},
                      {&h.conn_off, g.conn_off, 8 * (n_nodes + 1)}, {&h.conn_pl, g.conn_pl, 4 * n_conn},
                      {&h.iv_off, g.iv_off, 8 * (NP + 1)},      {&h.iv_start_seg, g.iv_start_seg, 4 * n_iv},
                      {&h.iv_start_xy, g.iv_start_xy, 8 * n_iv}, {&h.iv_end_seg, g.iv_end_seg, 4 * n_iv},
                      {&h.iv_end_xy, g.iv_end_xy, 8 * n_iv}}));
    h.n_nodes = h.n_real_nodes = n_nodes;
    h.n_polylines = n_pl;
    h.n_scene_polylines = NP;
    *out_host = h;
    ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  {  // the view of the result: the caller's, and the context's own for eg3d_edge_chains_device(graph == NULL)
    eg3d_device_graph3d& v = c->g_last;
    v.n_nodes = v.n_real_nodes = n_nodes;
    v.n_polylines = n_pl;
    v.n_scene_polylines = NP;
    v.node_X = g.node_X;
    v.node_point = (const uint64_t*)g.node_point;
    v.pl_start = g.pl_start;
    v.pl_end = g.pl_end;
    v.conn_off = (const uint64_t*)g.conn_off;
    v.conn_pl = g.conn_pl;
    v.iv_off = (const uint64_t*)g.iv_off;
    v.iv_start_seg = g.iv_start_seg;
    v.iv_start_xy = g.iv_start_xy;
    v.iv_end_seg = g.iv_end_seg;
    v.iv_end_xy = g.iv_end_xy;
    c->g_valid = true;
    if (out_dev) *out_dev = v;
  }
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_replay_stats);
    stats->n_pairs = n_pairs;
    stats->n_nodes = n_nodes;
    stats->n_polylines = n_pl;
    stats->n_intervals = n_iv;
    stats->table_slots = slots;
    stats->ms_graph = ms_graph;
    stats->ms_intervals = ms_iv;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}
