// eg3d_api_accumulate.hip — the PLGMatchesManager replay that accumulates over the clouds of a run (K8a,
// eg3d_k8a_accumulate.hip; include/eg3d_accumulate.h), and the same accumulator taking the graph of the run that follows in
// place of its cloud (K8m, eg3d_k8m_merge.hip; include/eg3d_replay_merge.h). eg3d_replay_device (eg3d_api_replay.hip) is not
// touched by either.
#include "../../include/eg3d_accumulate.h"
#include "../../include/eg3d_replay_merge.h"
#include "../../include/eg3d_host.h"
#include "eg3d_api_internal.h"
#include "eg3d_k8m_merge.h"

static int ka_read_u32(eg3d_ctx* c, const uint32_t* dev, uint64_t* v) {
  uint32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, dev, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *v = h;
  return EG3D_OK;
}
static uint64_t ka_pow2_above(uint64_t n) {  // the smallest power of two > n
  uint64_t p = 1;
  while (p <= n) p <<= 1;
  return p;
}
// the table size of eg3d_replay_device, for `pairs` pairs
static uint64_t ka_slots_for(const eg3d_ctx* c, uint64_t pairs) {
  return c->tune.replay_table_bits ? std::max<uint64_t>(1ull << c->tune.replay_table_bits, ka_pow2_above(2 * pairs))
                                   : ka_pow2_above(std::max<uint64_t>(4 * pairs, 63));
}

// The state's table, for `more` further pairs (two lookups each; a merged graph counts one per node): rebuilt from node_X when
// the run asks for a larger one. A cloud of p pairs adds at most 2 p nodes and a graph its own, so the table always has more
// than twice as many slots as the state has nodes.
static int ka_table_reserve(eg3d_ctx* c, uint64_t more, K8aTable* t) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  a.tab_pairs += more;
  const uint64_t want = ka_slots_for(c, a.tab_pairs);
  if (want > a.slots) {
    BUF_TRY(a.slot.ensure(4 * want));
    HIP_TRY(hipMemsetAsync(a.slot.p, 0xFF, 4 * want, st));
    a.slots = want;
    launch_k8a_table_insert(st, K8aTable{a.slot.as<uint32_t>(), want - 1}, a.node_X.as<float>(), 0, a.n_nodes);
    HIP_TRY(hipGetLastError());
  }
  *t = K8aTable{a.slot.as<uint32_t>(), a.slots - 1};
  return EG3D_OK;
}
// The claim map over the scene's vertices and the records, which live as long as the state
static int ka_open_intervals(eg3d_ctx* c, K8aRecords* rec) {
  ReplayAcc& a = c->ka;
  const size_t cells = std::max<uint64_t>(c->n_vtx, 1);
  BUF_TRY(a.map.ensure_exact(8 * cells));
  BUF_TRY(a.r_ss.ensure_exact(4 * cells));
  BUF_TRY(a.r_es.ensure_exact(4 * cells));
  BUF_TRY(a.r_sxy.ensure_exact(8 * cells));
  BUF_TRY(a.r_exy.ensure_exact(8 * cells));
  BUF_TRY(a.cnt.ensure(8));
  if (!a.map_ready) {
    HIP_TRY(hipMemsetAsync(a.map.p, 0xFF, 8 * cells, c->stream));
    HIP_TRY(hipMemsetAsync(a.cnt.p, 0, 8, c->stream));
    a.map_ready = true;
  }
  *rec = K8aRecords{a.r_ss.as<uint32_t>(), a.r_es.as<uint32_t>(), a.r_sxy.as<float>(), a.r_exy.as<float>()};
  return EG3D_OK;
}

// The claims of one cloud of `n_pairs` pairs whose points count from `base`. Every failure in here leaves the state invalid
// (the caller marks it so before the call and valid again after it).
static int ka_add_claims(eg3d_ctx* c, const CloudView& in, uint64_t base, uint64_t n_pairs) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  const uint64_t N = in.n_points;
  K8aTable ptab;
  BUF_TRY(ka_table_reserve(c, n_pairs, &ptab));
  // ---- the cloud's own points, grouped by K8's kernels on K8's scratch
  const uint64_t lslots = ka_slots_for(c, n_pairs);
  BUF_TRY(c->k8_slot.ensure(4 * lslots));
  BUF_TRY(c->k8_last.ensure(4 * lslots));
  BUF_TRY(c->k8_firstof.ensure(4 * N));
  BUF_TRY(c->k8_lastof.ensure(4 * N));
  BUF_TRY(c->k8_flag.ensure(4 * (N + 1)));
  BUF_TRY(c->k8_rank.ensure(4 * (N + 1)));
  BUF_TRY(c->k8_plid.ensure(4 * (N + 1)));
  BUF_TRY(a.node_id.ensure(4 * N));
  BUF_TRY(a.is_new.ensure(4 * (N + 1)));
  for (int k = 0; k < 2; k++) {
    BUF_TRY(c->k8_key[k].ensure(8 * N));
    BUF_TRY(c->k8_val[k].ensure(4 * N));
  }
  const K8Table ltab{c->k8_slot.as<uint32_t>(), c->k8_last.as<uint32_t>(), lslots - 1};
  uint32_t* first_of = c->k8_firstof.as<uint32_t>();
  uint32_t* last_of = c->k8_lastof.as<uint32_t>();
  uint32_t* flag = c->k8_flag.as<uint32_t>();
  uint32_t* rank = c->k8_rank.as<uint32_t>();
  uint32_t* pl_id = c->k8_plid.as<uint32_t>();
  uint32_t* node_id = a.node_id.as<uint32_t>();
  uint32_t* is_new = a.is_new.as<uint32_t>();
  u64* key[2] = {c->k8_key[0].as<u64>(), c->k8_key[1].as<u64>()};
  uint32_t* val[2] = {c->k8_val[0].as<uint32_t>(), c->k8_val[1].as<uint32_t>()};
  HIP_TRY(hipMemsetAsync(ltab.slot, 0xFF, 4 * lslots, st));
  HIP_TRY(hipMemsetAsync(ltab.last, 0, 4 * lslots, st));
  HIP_TRY(hipMemsetAsync(flag, 0, 4 * (N + 1), st));
  HIP_TRY(hipMemsetAsync(is_new, 0, 4 * (N + 1), st));
  launch_k8_node_claim(st, in, ltab);
  launch_k8_node_resolve(st, in, ltab, first_of, flag, last_of);
  // ---- settled or new
  launch_k8a_node_lookup(st, in, ptab, a.node_X.as<float>(), flag, node_id, is_new);
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u32(c, is_new, rank, N + 1));
  uint64_t n_new = 0;
  BUF_TRY(ka_read_u32(c, rank + N, &n_new));
  BUF_TRY(a.node_X.ensure_keep(12 * (a.n_nodes + n_new), 12 * a.n_nodes, st));
  BUF_TRY(a.node_point.ensure_keep(8 * (a.n_nodes + n_new), 8 * a.n_nodes, st));
  launch_k8a_node_write(st, in, flag, is_new, rank, last_of, base, a.n_nodes, node_id, a.node_X.as<float>(), a.node_point.as<u64>(), ptab);
  launch_k8a_pair_keys(st, in, first_of, node_id, key[0], val[0]);
  HIP_TRY(hipGetLastError());
  a.n_nodes += n_new;
  // ---- polylines: run heads that the polylines so far do not hold
  BUF_TRY(sort_pairs_u64_u32(c, key[0], key[1], val[0], val[1], N));
  HIP_TRY(hipMemsetAsync(flag, 0, 4 * (N + 1), st));
  launch_k8a_pl_heads(st, key[1], val[1], n_pairs, a.pl_key[a.cur].as<u64>(), a.n_pl, flag);
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u32(c, flag, pl_id, N + 1));
  uint64_t n_new_pl = 0;
  BUF_TRY(ka_read_u32(c, pl_id + N, &n_new_pl));
  if (n_new_pl) {
    const uint64_t total = a.n_pl + n_new_pl;
    BUF_TRY(a.pl_start.ensure_keep(4 * total, 4 * a.n_pl, st));
    BUF_TRY(a.pl_end.ensure_keep(4 * total, 4 * a.n_pl, st));
    BUF_TRY(a.pl_key[a.cur].ensure_keep(8 * total, 8 * a.n_pl, st));
    BUF_TRY(a.pl_key[a.cur ^ 1].ensure(8 * total));
    launch_k8a_pl_write(st, in, first_of, node_id, flag, pl_id, a.n_pl, a.pl_start.as<uint32_t>(), a.pl_end.as<uint32_t>(),
                        a.pl_key[a.cur].as<u64>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, a.pl_key[a.cur].as<u64>(), a.pl_key[a.cur ^ 1].as<u64>(), total));
    a.cur ^= 1;
    a.n_pl = total;
  }
  // ---- matched intervals: the claim map and the records live as long as the state
  K8aRecords rec;
  BUF_TRY(ka_open_intervals(c, &rec));
  launch_k8a_iv(st, false, in, c->ds, base, a.map.as<u64>(), rec, a.cnt.as<u64>());
  launch_k8a_iv(st, true, in, c->ds, base, a.map.as<u64>(), rec, a.cnt.as<u64>());
  HIP_TRY(hipGetLastError());
  uint64_t n_iv = 0;
  HIP_TRY(hipMemcpyAsync(&n_iv, a.cnt.p, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  a.n_iv = n_iv;
  a.n_pairs += n_pairs;
  return EG3D_OK;
}

// The graph of the state into the accumulator's own result buffers; reads the state, writes none of it.
static int ka_materialise(eg3d_ctx* c, K8Graph* out, uint64_t* n_conn) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  const uint64_t NP = c->n_pl, NV = c->n_vtx;
  K8Graph g{};
  g.node_X = a.node_X.as<float>();
  g.node_point = a.node_point.as<u64>();
  g.pl_start = a.pl_start.as<uint32_t>();
  g.pl_end = a.pl_end.as<uint32_t>();
  BUF_TRY(a.iv_off.ensure(8 * (NP + 1)));
  g.iv_off = a.iv_off.as<u64>();
  *n_conn = 0;
  // ---- connections: the (node, polyline) incidences sorted = every node's polylines in ascending id. Nothing but empty
  // clouds and one-point chains so far: none. (A merged graph may bring nodes without polylines — nothing the replay builds,
  // but nothing the checks refuse: they have no connections either.)
  BUF_TRY(a.conn_off.ensure(8 * (a.n_nodes + 1)));
  g.conn_off = a.conn_off.as<u64>();
  if (!a.n_pl) {
    HIP_TRY(hipMemsetAsync(g.conn_off, 0, 8 * (a.n_nodes + 1), st));
  } else {
    for (int k = 0; k < 2; k++) BUF_TRY(c->k8_key[k].ensure(16 * a.n_pl));
    BUF_TRY(a.conn_pl.ensure(8 * a.n_pl));
    g.conn_pl = a.conn_pl.as<uint32_t>();
    launch_k8a_inc(st, g.pl_start, g.pl_end, a.n_pl, c->k8_key[0].as<u64>());
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, c->k8_key[0].as<u64>(), c->k8_key[1].as<u64>(), 2 * a.n_pl));
    launch_k8_conn(st, c->k8_key[1].as<u64>(), 2 * a.n_pl, a.n_nodes, g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n_conn, g.conn_off + a.n_nodes, 8, hipMemcpyDeviceToHost, st));
  }
  // ---- intervals: flags of the claimed cells -> scan -> gather
  if (!a.map_ready) {  // no claim pass has run
    HIP_TRY(hipMemsetAsync(g.iv_off, 0, 8 * (NP + 1), st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = g;
    return EG3D_OK;
  }
  BUF_TRY(c->k8_sflag.ensure(4 * (NV + 1)));
  BUF_TRY(c->k8_pos.ensure(4 * (NV + 1)));
  uint32_t* pos = c->k8_pos.as<uint32_t>();
  launch_k8_seg_flags(st, a.map.as<u64>(), NV, c->k8_sflag.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u32(c, c->k8_sflag.as<uint32_t>(), pos, NV + 1));
  uint64_t n_iv = 0;
  BUF_TRY(ka_read_u32(c, pos + NV, &n_iv));
  if (n_iv != a.n_iv) {
    g_err = "eg3d_replay_accumulate: the claimed cells do not add up to the intervals counted (internal)";
    return EG3D_ERR_HIP;
  }
  BUF_TRY(a.iv_ss.ensure(4 * n_iv));
  BUF_TRY(a.iv_es.ensure(4 * n_iv));
  BUF_TRY(a.iv_sxy.ensure(8 * n_iv));
  BUF_TRY(a.iv_exy.ensure(8 * n_iv));
  g.iv_start_seg = a.iv_ss.as<uint32_t>();
  g.iv_end_seg = a.iv_es.as<uint32_t>();
  g.iv_start_xy = a.iv_sxy.as<float>();
  g.iv_end_xy = a.iv_exy.as<float>();
  const K8aRecords rec{a.r_ss.as<uint32_t>(), a.r_es.as<uint32_t>(), a.r_sxy.as<float>(), a.r_exy.as<float>()};
  launch_k8a_iv_gather(st, a.map.as<u64>(), NV, pos, rec, g);
  launch_k8_iv_off(st, c->ds, (uint32_t)NP, pos, g);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  *out = g;
  return EG3D_OK;
}

// How both entry points end once the claims are in and the state is whole: the graph when it is asked for, the copy, the
// views and the totals. (A failure in here leaves the state whole: materialising reads it only.)
static int ka_answer(eg3d_ctx* c, const char* who, float ms_graph, eg3d_device_graph3d* out_dev, eg3d_graph3d* out_host,
                     eg3d_replay_stats* stats) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  const uint64_t NP = c->n_pl;
  float ms_iv = 0, ms_copy = 0;
  K8Graph g{};
  uint64_t n_conn = 0;
  if (out_dev || out_host) {
    HIP_TRY(hipEventRecord(c->ea[0], st));
    BUF_TRY(ka_materialise(c, &g, &n_conn));
    HIP_TRY(hipEventRecord(c->eb[0], st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms_iv, c->ea[0], c->eb[0]));
  }
  if (out_host) {
    const auto t0 = std::chrono::steady_clock::now();
    eg3d_graph3d h;
    memset(&h, 0, sizeof(h));
    BUF_TRY(copy_out(st, who,
                     {{&h.node_X, g.node_X, 12 * a.n_nodes},      {&h.node_point, g.node_point, 8 * a.n_nodes},
                      {&h.pl_start, g.pl_start, 4 * a.n_pl},      {&h.pl_end, g.pl_end, 4 * a.n_pl},
                      {&h.conn_off, g.conn_off, 8 * (a.n_nodes + 1)}, {&h.conn_pl, g.conn_pl, 4 * n_conn},
                      {&h.iv_off, g.iv_off, 8 * (NP + 1)},        {&h.iv_start_seg, g.iv_start_seg, 4 * a.n_iv},
                      {&h.iv_start_xy, g.iv_start_xy, 8 * a.n_iv}, {&h.iv_end_seg, g.iv_end_seg, 4 * a.n_iv},
                      {&h.iv_end_xy, g.iv_end_xy, 8 * a.n_iv}}));
    h.n_nodes = h.n_real_nodes = a.n_nodes;
    h.n_polylines = a.n_pl;
    h.n_scene_polylines = NP;
    *out_host = h;
    ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (out_dev) {
    out_dev->n_nodes = out_dev->n_real_nodes = a.n_nodes;
    out_dev->n_polylines = a.n_pl;
    out_dev->n_scene_polylines = NP;
    out_dev->node_X = g.node_X;
    out_dev->node_point = (const uint64_t*)g.node_point;
    out_dev->pl_start = g.pl_start;
    out_dev->pl_end = g.pl_end;
    out_dev->conn_off = (const uint64_t*)g.conn_off;
    out_dev->conn_pl = g.conn_pl;
    out_dev->iv_off = (const uint64_t*)g.iv_off;
    out_dev->iv_start_seg = g.iv_start_seg;
    out_dev->iv_start_xy = g.iv_start_xy;
    out_dev->iv_end_seg = g.iv_end_seg;
    out_dev->iv_end_xy = g.iv_end_xy;
  }
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_replay_stats);
    stats->n_pairs = a.n_pairs;
    stats->n_nodes = a.n_nodes;
    stats->n_polylines = a.n_pl;
    stats->n_intervals = a.n_iv;
    stats->table_slots = a.slots;
    stats->ms_graph = ms_graph;
    stats->ms_intervals = ms_iv;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}

extern "C" int eg3d_replay_accumulate(eg3d_ctx* c, const eg3d_device_edgepoints* cloud, int reset, eg3d_device_graph3d* out_dev,
                                      eg3d_graph3d* out_host, eg3d_replay_stats* stats) {
  if (stats) BUF_TRY(check_struct_size("eg3d_replay_accumulate", "eg3d_replay_stats", stats->struct_size, sizeof(eg3d_replay_stats)));
  if (!c) {
    g_err = "eg3d_replay_accumulate: bad arguments";
    return EG3D_ERR_ARG;
  }
  ReplayAcc& a = c->ka;
  if (!a.valid && !reset) {
    g_err = "eg3d_replay_accumulate: an earlier call failed after it began to change the accumulated state: call with reset != 0";
    return EG3D_ERR_ARG;
  }
  eg3d_device_edgepoints d;
  if (cloud)
    d = *cloud;
  else
    BUF_TRY(eg3d_last_device_output(c, &d));
  const uint64_t base = reset ? 0 : a.n_points;
  if (d.n_points >= 0xfffffff0ull || base + d.n_points >= 0xfffffff0ull) {
    g_err = "eg3d_replay_accumulate: the points of the run must stay below 0xfffffff0 (node and polyline ids are 32-bit)";
    return EG3D_ERR_CAPACITY;
  }
  BUF_TRY(check_cloud(&d, "eg3d_replay_accumulate", true));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const CloudView in = cloud_view(&d);
  const uint64_t N = d.n_points;

  // ---- the checks, before anything is indexed or anything of the state is written
  BUF_TRY(c->k8_cnt.ensure(16));
  HIP_TRY(hipMemsetAsync(c->k8_cnt.p, 0, 16, st));
  unsigned long long* cnt = c->k8_cnt.as<unsigned long long>();
  launch_k8_pairs(st, in, c->ds, cnt, (uint32_t*)(cnt + 1));
  HIP_TRY(hipGetLastError());
  uint64_t back[2];  // pairs, flags
  uint32_t ends[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // key of the first and of the last point
  HIP_TRY(hipMemcpyAsync(back, cnt, sizeof(back), hipMemcpyDeviceToHost, st));
  if (N) {
    HIP_TRY(hipMemcpyAsync(ends, in.key, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ends + 4, in.key + 4 * (N - 1), 16, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t flags = (uint32_t)back[1];
  if (flags & ~K8_FLAG_HOSTONLY) {
    g_err = std::string("eg3d_replay_accumulate: ") +
            (flags & K8_FLAG_BAD_OFFSETS ? "obs_off is not ascending within [0, n_obs]"
             : flags & K8_FLAG_BAD_VIEW  ? "view id out of range"
             : flags & K8_FLAG_BAD_PL    ? "polyline id outside its view"
                                         : "segment index outside its polyline (or a polyline without segments)");
    return EG3D_ERR_ARG;
  }
  if (flags & K8_FLAG_HOSTONLY) {
    g_err = "eg3d_replay_accumulate: a point of a chain pair has a NaN coordinate or x or y == -1 (the reference's invalid-node "
            "rule): accumulate this run on the host (eg3d_host_replay_state_add)";
    return EG3D_ERR_HOSTONLY;
  }
  if (N && !reset && a.have_last && ends[0] == a.last_key[0] && ends[1] == a.last_key[1] && ends[2] == a.last_key[2] &&
      ends[3] == a.last_key[3] + 1u) {
    g_err = "eg3d_replay_accumulate: the cloud's first point continues the chain the previous cloud ended on (a cloud is made of "
            "whole chains)";
    return EG3D_ERR_ARG;
  }
  const uint64_t n_pairs = back[0];

  // ---- accepted: from here on a failure invalidates the state
  if (reset) a.clear();
  a.valid = false;
  float ms_graph = 0;
  HIP_TRY(hipEventRecord(c->ea[0], st));
  if (n_pairs) BUF_TRY(ka_add_claims(c, in, base, n_pairs));
  if (N) {
    a.n_points = base + N;
    memcpy(a.last_key, ends + 4, sizeof(a.last_key));
    a.have_last = true;
  }
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipEventElapsedTime(&ms_graph, c->ea[0], c->eb[0]));
  a.valid = true;  // (a failure below leaves the state whole: materialising reads it only)

  return ka_answer(c, "eg3d_replay_accumulate", ms_graph, out_dev, out_host, stats);
}

// The claims of the graph `b` of `n_iv` intervals, whose points count from `base` (eg3d_k8m_merge.hip states the rule). The
// checks have passed; every[] and last_of[] (k8_flag, k8_lastof) were written by k8m_node_group. Every failure in here
// leaves the state invalid, as in ka_add_claims.
static int ka_merge_claims(eg3d_ctx* c, const K8mGraph& b, uint64_t n_iv, uint64_t base) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  const uint64_t NN = b.n_nodes, NL = b.n_pl;
  if (NN) {
    // ---- nodes: every node of b is the first point of its coordinates (they are distinct): settled or new
    K8aTable ptab;
    BUF_TRY(ka_table_reserve(c, NN, &ptab));
    BUF_TRY(c->k8_rank.ensure(4 * (NN + 1)));
    BUF_TRY(a.node_id.ensure(4 * NN));
    BUF_TRY(a.is_new.ensure(4 * (NN + 1)));
    uint32_t* every = c->k8_flag.as<uint32_t>();
    uint32_t* last_of = c->k8_lastof.as<uint32_t>();
    uint32_t* rank = c->k8_rank.as<uint32_t>();
    uint32_t* node_id = a.node_id.as<uint32_t>();
    uint32_t* is_new = a.is_new.as<uint32_t>();
    CloudView in{};  // K8a's node kernels read the points' X and their number, nothing else
    in.X = b.node_X;
    in.n_points = NN;
    HIP_TRY(hipMemsetAsync(is_new, 0, 4 * (NN + 1), st));
    launch_k8a_node_lookup(st, in, ptab, a.node_X.as<float>(), every, node_id, is_new);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u32(c, is_new, rank, NN + 1));
    uint64_t n_new = 0;
    BUF_TRY(ka_read_u32(c, rank + NN, &n_new));
    BUF_TRY(a.node_X.ensure_keep(12 * (a.n_nodes + n_new), 12 * a.n_nodes, st));
    BUF_TRY(a.node_point.ensure_keep(8 * (a.n_nodes + n_new), 8 * a.n_nodes, st));
    launch_k8a_node_write(st, in, every, is_new, rank, last_of, base, a.n_nodes, node_id, a.node_X.as<float>(), a.node_point.as<u64>(), ptab);
    HIP_TRY(hipGetLastError());
    a.n_nodes += n_new;
  }
  if (NL) {
    // ---- polylines: the mapped keys, sorted stably, against the persistent keys
    BUF_TRY(c->k8_flag.ensure(4 * (NL + 1)));  // (every[] is done with)
    BUF_TRY(c->k8_plid.ensure(4 * (NL + 1)));
    for (int k = 0; k < 2; k++) {
      BUF_TRY(c->k8_key[k].ensure(8 * NL));
      BUF_TRY(c->k8_val[k].ensure(4 * NL));
    }
    uint32_t* creates = c->k8_flag.as<uint32_t>();
    uint32_t* pl_id = c->k8_plid.as<uint32_t>();
    u64* key[2] = {c->k8_key[0].as<u64>(), c->k8_key[1].as<u64>()};
    uint32_t* val[2] = {c->k8_val[0].as<uint32_t>(), c->k8_val[1].as<uint32_t>()};
    const uint32_t* node_id = a.node_id.as<uint32_t>();
    launch_k8m_pl_keys(st, b, node_id, key[0], val[0]);
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_pairs_u64_u32(c, key[0], key[1], val[0], val[1], NL));
    HIP_TRY(hipMemsetAsync(creates, 0, 4 * (NL + 1), st));
    launch_k8a_pl_heads(st, key[1], val[1], NL, a.pl_key[a.cur].as<u64>(), a.n_pl, creates);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u32(c, creates, pl_id, NL + 1));
    uint64_t n_new_pl = 0;
    BUF_TRY(ka_read_u32(c, pl_id + NL, &n_new_pl));
    if (n_new_pl) {
      const uint64_t total = a.n_pl + n_new_pl;
      BUF_TRY(a.pl_start.ensure_keep(4 * total, 4 * a.n_pl, st));
      BUF_TRY(a.pl_end.ensure_keep(4 * total, 4 * a.n_pl, st));
      BUF_TRY(a.pl_key[a.cur].ensure_keep(8 * total, 8 * a.n_pl, st));
      BUF_TRY(a.pl_key[a.cur ^ 1].ensure(8 * total));
      launch_k8m_pl_write(st, b, node_id, creates, pl_id, a.n_pl, a.pl_start.as<uint32_t>(), a.pl_end.as<uint32_t>(),
                          a.pl_key[a.cur].as<u64>());
      HIP_TRY(hipGetLastError());
      BUF_TRY(sort_keys_u64(c, a.pl_key[a.cur].as<u64>(), a.pl_key[a.cur ^ 1].as<u64>(), total));
      a.cur ^= 1;
      a.n_pl = total;
    }
  }
  if (n_iv) {
    // ---- matched intervals: the cells nobody holds
    K8aRecords rec;
    BUF_TRY(ka_open_intervals(c, &rec));
    launch_k8m_iv(st, b, c->ds, c->n_pl, n_iv, (u64)base * (u64)c->V, a.map.as<u64>(), rec, a.cnt.as<u64>());
    HIP_TRY(hipGetLastError());
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a.cnt.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    a.n_iv = total;
  }
  return EG3D_OK;
}

extern "C" int eg3d_replay_merge_graph(eg3d_ctx* c, const eg3d_device_graph3d* later, uint64_t later_points, uint64_t later_pairs,
                                       int reset, eg3d_device_graph3d* out_dev, eg3d_graph3d* out_host, eg3d_replay_stats* stats) {
  const char* who = "eg3d_replay_merge_graph";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_replay_stats", stats->struct_size, sizeof(eg3d_replay_stats)));
  if (!c || !later) {
    g_err = "eg3d_replay_merge_graph: bad arguments";
    return EG3D_ERR_ARG;
  }
  ReplayAcc& a = c->ka;
  if (!a.valid && !reset) {
    g_err = "eg3d_replay_merge_graph: an earlier call failed after it began to change the accumulated state: call with reset != 0";
    return EG3D_ERR_ARG;
  }
  const uint64_t base = reset ? 0 : a.n_points;
  if (later_points >= 0xfffffff0ull || base + later_points >= 0xfffffff0ull) {
    g_err = "eg3d_replay_merge_graph: the points of the run must stay below 0xfffffff0 (node and polyline ids are 32-bit)";
    return EG3D_ERR_CAPACITY;
  }
  const uint64_t NN = later->n_nodes, NL = later->n_polylines, NP = c->n_pl;
  auto refuse = [&](const char* why) {
    g_err = std::string("eg3d_replay_merge_graph: ") + why;
    return EG3D_ERR_ARG;
  };
  if (later->n_scene_polylines != NP) return refuse("n_scene_polylines is not the scene's");
  if (NN > later_points || NL > later_points) return refuse("more nodes or polylines than later_points (every node has a point of its own)");
  if (!later->iv_off || (NN && (!later->node_X || !later->node_point)) || (NL && (!later->pl_start || !later->pl_end)))
    return refuse("a null array");
  // the accumulator's own graph (its out_dev views these buffers): what the merge appends to cannot be what it reads
  for (const void* p : {(const void*)later->node_X, (const void*)later->node_point, (const void*)later->pl_start, (const void*)later->pl_end,
                        (const void*)later->iv_off, (const void*)later->iv_start_seg, (const void*)later->iv_end_seg,
                        (const void*)later->iv_start_xy, (const void*)later->iv_end_xy})
    for (const DevBuf* d : {&a.node_X, &a.node_point, &a.pl_start, &a.pl_end, &a.iv_off, &a.iv_ss, &a.iv_es, &a.iv_sxy, &a.iv_exy})
      if (p && d->p && (const char*)p >= (const char*)d->p && (const char*)p < (const char*)d->p + d->cap)
        return refuse("`later` is this accumulator's own graph");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  K8mGraph b{};
  b.n_nodes = NN;
  b.n_pl = NL;
  b.node_X = later->node_X;
  b.node_point = (const u64*)later->node_point;
  b.pl_start = later->pl_start;
  b.pl_end = later->pl_end;
  b.iv_off = (const u64*)later->iv_off;
  b.iv_start_seg = later->iv_start_seg;
  b.iv_start_xy = later->iv_start_xy;
  b.iv_end_seg = later->iv_end_seg;
  b.iv_end_xy = later->iv_end_xy;

  // ---- the checks, before anything of `later` is an index or anything of the state is written. First what stands alone ...
  BUF_TRY(c->k8_cnt.ensure(16));
  HIP_TRY(hipMemsetAsync(c->k8_cnt.p, 0, 16, st));
  uint32_t* flags_dev = c->k8_cnt.as<uint32_t>();
  launch_k8m_check(st, b, c->ds, (uint32_t)NP, later_points, flags_dev);
  HIP_TRY(hipGetLastError());
  uint32_t flags = 0;
  uint64_t n_iv = 0;
  HIP_TRY(hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  auto flag_error = [&](uint32_t f) {
    return refuse(f & K8M_FLAG_BAD_POINT      ? "a node_point that is not below later_points"
                  : f & K8M_FLAG_BAD_ENDPOINT ? "a polyline endpoint that is not a node"
                  : f & K8M_FLAG_BAD_OFFSETS  ? "iv_off does not ascend from 0, or gives a scene polyline more intervals than it has segments"
                  : f & K8M_FLAG_BAD_SEG      ? "an interval's segment outside its scene polyline"
                  : f & K8M_FLAG_SEG_ORDER    ? "start segments of a scene polyline that do not ascend strictly"
                  : f & K8M_FLAG_DUP_NODE     ? "two nodes with equal coordinates"
                                              : "two polylines on one pair of nodes");
  };
  if (flags & ~K8M_FLAG_HOSTONLY) return flag_error(flags);
  if (NP) {  // (ascending from 0 and row by row within the scene's segments: at most one per scene vertex)
    HIP_TRY(hipMemcpyAsync(&n_iv, b.iv_off + NP, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (n_iv && (!b.iv_start_seg || !b.iv_end_seg || !b.iv_start_xy || !b.iv_end_xy)) return refuse("a null array");
  // ... then what indexes with it: the intervals' segments, duplicates among the nodes (K8's scratch table) and the polylines
  const uint64_t lslots = ka_slots_for(c, NN);
  BUF_TRY(c->k8_slot.ensure(4 * lslots));
  BUF_TRY(c->k8_flag.ensure(4 * (NN + 1)));
  BUF_TRY(c->k8_lastof.ensure(4 * std::max<uint64_t>(NN, 1)));
  for (int k = 0; k < 2; k++) {
    BUF_TRY(c->k8_key[k].ensure(8 * std::max<uint64_t>(NL, 1)));
    BUF_TRY(c->k8_val[k].ensure(4 * std::max<uint64_t>(NL, 1)));
  }
  HIP_TRY(hipMemsetAsync(c->k8_slot.p, 0xFF, 4 * lslots, st));
  launch_k8m_iv_check(st, b, c->ds, (uint32_t)NP, n_iv, flags_dev);
  launch_k8m_node_group(st, b, K8aTable{c->k8_slot.as<uint32_t>(), lslots - 1}, c->k8_flag.as<uint32_t>(), c->k8_lastof.as<uint32_t>(),
                        flags_dev);
  launch_k8m_pl_keys(st, b, nullptr, c->k8_key[0].as<u64>(), c->k8_val[0].as<uint32_t>());
  HIP_TRY(hipGetLastError());
  if (NL > 1) {
    BUF_TRY(sort_keys_u64(c, c->k8_key[0].as<u64>(), c->k8_key[1].as<u64>(), NL));
    launch_k8m_pl_dups(st, c->k8_key[1].as<u64>(), NL, flags_dev);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (flags & ~K8M_FLAG_HOSTONLY) return flag_error(flags);
  if ((flags & K8M_FLAG_HOSTONLY) || later->n_real_nodes != NN) {
    g_err = "eg3d_replay_merge_graph: `later` holds wiped or invalid nodes (n_real_nodes != n_nodes, a NaN coordinate, or x or y == -1: "
            "the reference's invalid-node rule): add such a run's clouds on the host (eg3d_host_replay_state_add)";
    return EG3D_ERR_HOSTONLY;
  }

  // ---- accepted: from here on a failure invalidates the state
  if (reset) a.clear();
  a.valid = false;
  float ms_graph = 0;
  HIP_TRY(hipEventRecord(c->ea[0], st));
  BUF_TRY(ka_merge_claims(c, b, n_iv, base));
  a.n_points = base + later_points;
  a.n_pairs += later_pairs;
  if (later_points) a.have_last = false;  // a graph does not carry the key its cloud ended on
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipEventElapsedTime(&ms_graph, c->ea[0], c->eb[0]));
  a.valid = true;

  return ka_answer(c, who, ms_graph, out_dev, out_host, stats);
}

extern "C" int eg3d_replay_accumulated(eg3d_ctx* c, uint64_t* n_points, uint64_t* n_pairs, uint64_t* state_bytes) {
  if (!c) {
    g_err = "eg3d_replay_accumulated: bad arguments";
    return EG3D_ERR_ARG;
  }
  if (!c->ka.valid) {
    g_err = "eg3d_replay_accumulated: an earlier eg3d_replay_accumulate failed after it began to change the state: reset first";
    return EG3D_ERR_ARG;
  }
  if (n_points) *n_points = c->ka.n_points;
  if (n_pairs) *n_pairs = c->ka.n_pairs;
  if (state_bytes) *state_bytes = c->ka.state_bytes();
  return EG3D_OK;
}
