// eg3d_api_accumulate.hip — the PLGMatchesManager replay that accumulates over the clouds of a run (K8a,
// eg3d_k8a_accumulate.hip; include/eg3d_accumulate.h). eg3d_replay_device (eg3d_api_replay.hip) is not touched by it.
#include "../../include/eg3d_accumulate.h"
#include "../../include/eg3d_host.h"
#include "eg3d_api_internal.h"

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

// The claims of one cloud of `n_pairs` pairs whose points count from `base`. Every failure in here leaves the state invalid
// (the caller marks it so before the call and valid again after it).
static int ka_add_claims(eg3d_ctx* c, const CloudView& in, uint64_t base, uint64_t n_pairs) {
  ReplayAcc& a = c->ka;
  hipStream_t st = c->stream;
  const uint64_t N = in.n_points, NV = c->n_vtx;
  // ---- the state's table: rebuilt from node_X when the lookups of the run (two per pair) ask for a larger one
  const uint64_t want = ka_slots_for(c, a.n_pairs + n_pairs);
  if (want > a.slots) {
    BUF_TRY(a.slot.ensure(4 * want));
    HIP_TRY(hipMemsetAsync(a.slot.p, 0xFF, 4 * want, st));
    a.slots = want;
    launch_k8a_table_insert(st, K8aTable{a.slot.as<uint32_t>(), want - 1}, a.node_X.as<float>(), 0, a.n_nodes);
    HIP_TRY(hipGetLastError());
  }
  const K8aTable ptab{a.slot.as<uint32_t>(), a.slots - 1};
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
  const size_t cells = std::max<uint64_t>(NV, 1);
  BUF_TRY(a.map.ensure_exact(8 * cells));
  BUF_TRY(a.r_ss.ensure_exact(4 * cells));
  BUF_TRY(a.r_es.ensure_exact(4 * cells));
  BUF_TRY(a.r_sxy.ensure_exact(8 * cells));
  BUF_TRY(a.r_exy.ensure_exact(8 * cells));
  BUF_TRY(a.cnt.ensure(8));
  if (!a.map_ready) {
    HIP_TRY(hipMemsetAsync(a.map.p, 0xFF, 8 * cells, st));
    HIP_TRY(hipMemsetAsync(a.cnt.p, 0, 8, st));
    a.map_ready = true;
  }
  const K8aRecords rec{a.r_ss.as<uint32_t>(), a.r_es.as<uint32_t>(), a.r_sxy.as<float>(), a.r_exy.as<float>()};
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
  if (!a.n_pairs) {  // nothing but empty clouds and one-point chains so far: the all-zero graph
    BUF_TRY(a.conn_off.ensure(8));
    g.conn_off = a.conn_off.as<u64>();
    HIP_TRY(hipMemsetAsync(g.conn_off, 0, 8, st));
    HIP_TRY(hipMemsetAsync(g.iv_off, 0, 8 * (NP + 1), st));
    *out = g;
    return EG3D_OK;
  }
  // ---- connections: the (node, polyline) incidences sorted = every node's polylines in ascending id
  for (int k = 0; k < 2; k++) BUF_TRY(c->k8_key[k].ensure(16 * a.n_pl));
  BUF_TRY(a.conn_off.ensure(8 * (a.n_nodes + 1)));
  BUF_TRY(a.conn_pl.ensure(8 * a.n_pl));
  g.conn_off = a.conn_off.as<u64>();
  g.conn_pl = a.conn_pl.as<uint32_t>();
  launch_k8a_inc(st, g.pl_start, g.pl_end, a.n_pl, c->k8_key[0].as<u64>());
  HIP_TRY(hipGetLastError());
  BUF_TRY(sort_keys_u64(c, c->k8_key[0].as<u64>(), c->k8_key[1].as<u64>(), 2 * a.n_pl));
  launch_k8_conn(st, c->k8_key[1].as<u64>(), 2 * a.n_pl, a.n_nodes, g);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n_conn, g.conn_off + a.n_nodes, 8, hipMemcpyDeviceToHost, st));
  // ---- intervals: flags of the claimed cells -> scan -> gather
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
  const uint64_t N = d.n_points, NP = c->n_pl;

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
  float ms_graph = 0, ms_iv = 0, ms_copy = 0;
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
    BUF_TRY(copy_out(st, "eg3d_replay_accumulate",
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
