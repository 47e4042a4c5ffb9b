// eg3d_api_edges.hip — the 3-D edge model of a graph3d (include/eg3d/edges.h): the host side of K17
#include <cmath>

#include "eg3d_api_internal.h"
#include "eg3d_edges_core.h"
#include "../../include/eg3d/edges.h"

static int read_ctr(eg3d_ctx* c, u64* back) {
  HIP_TRY(hipMemcpyAsync(back, c->k17[K17B_CTR].p, sizeof(u64) * K17C_COUNT, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return EG3D_OK;
}
static int read_u64(eg3d_ctx* c, const u64* dev, uint64_t* v) {
  u64 h = 0;
  HIP_TRY(hipMemcpyAsync(&h, dev, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *v = h;
  return EG3D_OK;
}
static int refuse(const char* who, const char* what) {
  g_err = std::string(who) + ": " + what;
  return EG3D_ERR_ARG;
}
static K17State state_of(eg3d_ctx* c, int which) {
  DevBuf* b = &c->k17[which ? K17B_STATE1 : K17B_STATE0];
  return K17State{b[0].as<uint32_t>(), b[1].as<uint32_t>(), b[2].as<uint32_t>(), b[3].as<uint32_t>(), b[4].as<uint32_t>()};
}

// What both entry points check before they touch the device.
static int check_call(const char* who, const eg3d_ctx* c, float max_dist, const eg3d_edges_stats* stats) {
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_edges_stats", stats->struct_size, sizeof(eg3d_edges_stats)));
  if (!c) return refuse(who, "bad arguments");
  if (!std::isfinite(max_dist) || !(max_dist >= 0.0f)) return refuse(who, "max_dist must be finite and >= 0");
  return EG3D_OK;
}
static int check_counts(const char* who, uint64_t n_nodes, uint64_t n_polylines) {
  if (n_nodes >= edges::kMaxCount || n_polylines >= edges::kMaxCount) {
    g_err = std::string(who) + ": n_nodes and n_polylines must stay below 2^30 (half-edge ids are 32-bit)";
    return EG3D_ERR_CAPACITY;
  }
  return EG3D_OK;
}

// The checks of the graph's polylines and offsets; after them conn_off[n_nodes] == *n_conn == 2 n_polylines - n_loops is known.
static int check_graph_head(eg3d_ctx* c, const char* who, const K17Graph& g, uint64_t* n_loops, uint64_t* n_conn) {
  hipStream_t st = c->stream;
  BUF_TRY(c->k17[K17B_CTR].ensure(sizeof(u64) * K17C_COUNT));
  u64* ctr = c->k17[K17B_CTR].as<u64>();
  HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(u64) * K17C_COUNT, st));
  launch_k17_check_polylines(st, g, ctr);
  HIP_TRY(hipGetLastError());
  u64 back[K17C_COUNT];
  BUF_TRY(read_ctr(c, back));
  if (back[K17C_FLAGS]) return refuse(who, "a polyline names a node outside [0, n_nodes)");
  *n_loops = back[K17C_LOOPS];
  *n_conn = 2ull * g.n_polylines - back[K17C_LOOPS];
  launch_k17_check_offsets(st, g, *n_conn, ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(read_ctr(c, back));
  if (back[K17C_FLAGS]) return refuse(who, "conn_off does not ascend from 0 to 2 * n_polylines - n_loops");
  return EG3D_OK;
}

static void give_stats(eg3d_edges_stats* stats, eg3d_edges_stats s) {
  if (!stats) return;
  s.struct_size = (uint32_t)sizeof(eg3d_edges_stats);
  *stats = s;
}

// The call proper on a graph whose polylines and offsets are checked: the rows, the trace, the simplification, the copy.
static int run_edges(eg3d_ctx* c, const char* who, const K17Graph& g, uint64_t n_loops, float max_dist, int simplify,
                     eg3d_device_edge_chains* out_dev, eg3d_edge_chain_set* out_host, eg3d_edges_stats* stats, float ms_upload) {
  hipStream_t st = c->stream;
  DevBuf* B = c->k17;
  const uint64_t NN = g.n_nodes, NP = g.n_polylines, H = 2 * NP;
  u64* ctr = B[K17B_CTR].as<u64>();
  u64 back[K17C_COUNT];
  // ---- the rows
  BUF_TRY(B[K17B_SEEN].ensure(4 * std::max<uint64_t>(H, 1)));
  BUF_TRY(B[K17B_DEG].ensure(4 * std::max<uint64_t>(NN, 1)));
  HIP_TRY(hipEventRecord(c->ea[0], st));
  HIP_TRY(hipMemsetAsync(B[K17B_SEEN].p, 0, 4 * std::max<uint64_t>(H, 1), st));
  launch_k17_check_rows(st, g, B[K17B_SEEN].as<uint32_t>(), B[K17B_DEG].as<uint32_t>(), ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(read_ctr(c, back));
  if (back[K17C_FLAGS])
    return refuse(who, "a row of conn names a polyline out of range, one that does not end in that node, or one twice");

  // ---- the trace
  const uint32_t* deg = B[K17B_DEG].as<uint32_t>();
  uint64_t n_chains = 0, n_vertices = 0, n_kept = 0;
  for (int k = K17B_STATE0; k < K17B_STATE0 + 10; k++) BUF_TRY(B[k].ensure(4 * std::max<uint64_t>(H, 1)));
  for (int k : {K17B_SUCC, K17B_CUT, K17B_CHAINOFHEAD}) BUF_TRY(B[k].ensure(4 * std::max<uint64_t>(H, 1)));
  for (int k : {K17B_HEADFLAG, K17B_CHAINID, K17B_HEADOF}) BUF_TRY(B[k].ensure(4 * (NP + 1)));
  uint32_t* succ = B[K17B_SUCC].as<uint32_t>();
  uint32_t* cut = B[K17B_CUT].as<uint32_t>();
  uint32_t* chain_of_head = B[K17B_CHAINOFHEAD].as<uint32_t>();
  uint32_t* head_flag = B[K17B_HEADFLAG].as<uint32_t>();
  uint32_t* chain_id = B[K17B_CHAINID].as<uint32_t>();
  uint32_t* head_of = B[K17B_HEADOF].as<uint32_t>();
  int rounds = 0;  // ceil(log2(2 n_polylines)): a list holds at most n_polylines half-edges
  while ((1ull << rounds) < H) rounds++;
  int cur = 0;
  launch_k17_successors(st, g, deg, succ, state_of(c, cur));
  for (int r = 0; r < rounds; r++, cur ^= 1) launch_k17_jump(st, (uint32_t)H, state_of(c, cur), state_of(c, cur ^ 1));
  launch_k17_cut_rings(st, g, succ, state_of(c, cur), cut, ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(read_ctr(c, back));
  if (back[K17C_RING_HALFEDGES])
    for (int r = 0; r < rounds; r++, cur ^= 1) launch_k17_jump(st, (uint32_t)H, state_of(c, cur), state_of(c, cur ^ 1));
  const K17State s = state_of(c, cur);
  HIP_TRY(hipMemsetAsync(head_flag, 0, 4 * (NP + 1), st));
  HIP_TRY(hipMemsetAsync(chain_of_head, 0xFF, 4 * std::max<uint64_t>(H, 1), st));
  launch_k17_heads(st, g, deg, cut, s, head_flag, head_of);
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u32(c, head_flag, chain_id, NP + 1));
  {
    uint32_t h = 0;
    HIP_TRY(hipMemcpyAsync(&h, chain_id + NP, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    n_chains = h;
  }
  // (from here on the buffers of the result are written: an earlier result is gone)
  BUF_TRY(B[K17B_NVTX].ensure(8 * (n_chains + 1)));
  BUF_TRY(B[K17B_CHAINOFF].ensure(8 * (n_chains + 1)));
  BUF_TRY(B[K17B_CHAINFLAGS].ensure(4 * std::max<uint64_t>(n_chains, 1)));
  u64* n_vtx = B[K17B_NVTX].as<u64>();
  u64* chain_off = B[K17B_CHAINOFF].as<u64>();
  uint32_t* chain_flags = B[K17B_CHAINFLAGS].as<uint32_t>();
  HIP_TRY(hipMemsetAsync(n_vtx, 0, 8 * (n_chains + 1), st));
  launch_k17_chain_sizes(st, g, head_flag, chain_id, head_of, cut, s, n_vtx, chain_flags, chain_of_head, ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u64(c, n_vtx, chain_off, n_chains + 1));
  BUF_TRY(read_u64(c, chain_off + n_chains, &n_vertices));
  BUF_TRY(B[K17B_CHAINNODE].ensure(4 * std::max<uint64_t>(n_vertices, 1)));
  uint32_t* chain_node = B[K17B_CHAINNODE].as<uint32_t>();
  launch_k17_fill(st, g, s, chain_of_head, chain_off, chain_node, ctr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  BUF_TRY(read_ctr(c, back));
  if (back[K17C_FLAGS]) {
    g_err = std::string(who) + ": a traced vertex fell outside its chain";
    return EG3D_ERR_HIP;
  }
  eg3d_edges_stats es{};
  HIP_TRY(hipEventElapsedTime(&es.ms_trace, c->ea[0], c->eb[0]));

  // ---- simplify, length
  const u64* s_off = chain_off;
  const uint32_t* s_node = chain_node;
  n_kept = n_vertices;
  BUF_TRY(B[K17B_LENGTH].ensure(4 * std::max<uint64_t>(n_chains, 1)));
  float* length = B[K17B_LENGTH].as<float>();
  HIP_TRY(hipEventRecord(c->ea[0], st));
  if (simplify && n_chains) {
    BUF_TRY(B[K17B_REGION].ensure(4 * n_vertices));
    BUF_TRY(B[K17B_NF].ensure(4 * n_chains));
    BUF_TRY(B[K17B_NB].ensure(4 * n_chains));
    BUF_TRY(B[K17B_NKEPT].ensure(8 * (n_chains + 1)));
    BUF_TRY(B[K17B_SOFF].ensure(8 * (n_chains + 1)));
    u64* kept = B[K17B_NKEPT].as<u64>();
    HIP_TRY(hipMemsetAsync(kept + n_chains, 0, 8, st));
    launch_k17_simplify(st, g.node_X, n_chains, chain_off, chain_node, max_dist * max_dist, B[K17B_REGION].as<uint32_t>(),
                        B[K17B_NF].as<uint32_t>(), B[K17B_NB].as<uint32_t>(), kept);
    HIP_TRY(hipGetLastError());
    BUF_TRY(scan_u64(c, kept, B[K17B_SOFF].as<u64>(), n_chains + 1));
    BUF_TRY(read_u64(c, B[K17B_SOFF].as<u64>() + n_chains, &n_kept));
    BUF_TRY(B[K17B_SNODE].ensure(4 * std::max<uint64_t>(n_kept, 1)));
    launch_k17_compact(st, n_chains, chain_off, B[K17B_REGION].as<uint32_t>(), B[K17B_NF].as<uint32_t>(), B[K17B_NB].as<uint32_t>(),
                       B[K17B_SOFF].as<u64>(), B[K17B_SNODE].as<uint32_t>());
    s_off = B[K17B_SOFF].as<u64>();
    s_node = B[K17B_SNODE].as<uint32_t>();
  }
  launch_k17_length(st, g.node_X, n_chains, s_off, s_node, length);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipEventElapsedTime(&es.ms_simplify, c->ea[0], c->eb[0]));

  es.ms_copy = ms_upload;
  if (out_host) {
    const auto t0 = std::chrono::steady_clock::now();
    eg3d_edge_chain_set h;
    memset(&h, 0, sizeof(h));
    BUF_TRY(copy_out(st, who,
                     {{&h.chain_off, chain_off, 8 * (n_chains + 1)}, {&h.chain_node, chain_node, 4 * n_vertices},
                      {&h.chain_flags, chain_flags, 4 * n_chains},   {&h.s_off, s_off, 8 * (n_chains + 1)},
                      {&h.s_node, s_node, 4 * n_kept},               {&h.length, length, 4 * n_chains}}));
    h.n_chains = n_chains;
    h.n_vertices = n_vertices;
    h.n_kept = n_kept;
    *out_host = h;
    es.ms_copy += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (out_dev) {
    out_dev->n_chains = n_chains;
    out_dev->n_vertices = n_vertices;
    out_dev->n_kept = n_kept;
    out_dev->chain_off = (const uint64_t*)chain_off;
    out_dev->chain_node = chain_node;
    out_dev->chain_flags = chain_flags;
    out_dev->s_off = (const uint64_t*)s_off;
    out_dev->s_node = s_node;
    out_dev->length = length;
  }
  es.n_chains = n_chains;
  es.n_rings = back[K17C_RINGS];
  es.n_loops_dropped = n_loops;
  es.n_vertices_in = n_vertices;
  es.n_vertices_kept = n_kept;
  es.longest_chain = back[K17C_LONGEST];
  give_stats(stats, es);
  return EG3D_OK;
}

extern "C" void eg3d_free_edge_chains(eg3d_edge_chain_set* ch) {
  if (!ch) return;
  void* all[] = {ch->chain_off, ch->chain_node, ch->chain_flags, ch->s_off, ch->s_node, ch->length};
  for (void* p : all) free(p);
  memset(ch, 0, sizeof(*ch));
}

extern "C" int eg3d_edge_chains_device(eg3d_ctx* c, const eg3d_device_graph3d* graph, float max_dist, int simplify,
                                       eg3d_device_edge_chains* out_dev, eg3d_edge_chain_set* out_host, eg3d_edges_stats* stats) {
  const char* who = "eg3d_edge_chains_device";
  BUF_TRY(check_call(who, c, max_dist, stats));
  eg3d_device_graph3d d;
  if (graph) {
    d = *graph;
  } else {
    if (!c->g_valid) return refuse(who, "graph == NULL on a context without an eg3d_replay_device result");
    d = c->g_last;
  }
  BUF_TRY(check_counts(who, d.n_nodes, d.n_polylines));
  if ((d.n_nodes && !d.node_X) || (d.n_polylines && (!d.pl_start || !d.pl_end)) || !d.conn_off) return refuse(who, "the graph lacks an array");
  HIP_TRY(hipSetDevice(c->device));
  K17Graph g{d.node_X, d.pl_start, d.pl_end, (const u64*)d.conn_off, d.conn_pl, (uint32_t)d.n_nodes, (uint32_t)d.n_polylines};
  uint64_t n_loops = 0, n_conn = 0;
  BUF_TRY(check_graph_head(c, who, g, &n_loops, &n_conn));
  if (n_conn && !d.conn_pl) return refuse(who, "the graph lacks an array");
  return run_edges(c, who, g, n_loops, max_dist, simplify, out_dev, out_host, stats, 0.f);
}

extern "C" int eg3d_edge_chains(eg3d_ctx* c, const eg3d_graph3d* hg, float max_dist, int simplify, eg3d_device_edge_chains* out_dev,
                                eg3d_edge_chain_set* out_host, eg3d_edges_stats* stats) {
  const char* who = "eg3d_edge_chains";
  BUF_TRY(check_call(who, c, max_dist, stats));
  if (!hg) return refuse(who, "bad arguments");
  BUF_TRY(check_counts(who, hg->n_nodes, hg->n_polylines));
  if ((hg->n_nodes && !hg->node_X) || (hg->n_polylines && (!hg->pl_start || !hg->pl_end)) || !hg->conn_off)
    return refuse(who, "the graph lacks an array");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const auto w0 = std::chrono::steady_clock::now();
  const uint64_t NN = hg->n_nodes, NP = hg->n_polylines;
  BUF_TRY(upload(c->k17[K17B_UX], hg->node_X, 3 * NN, st));
  BUF_TRY(upload(c->k17[K17B_UPS], hg->pl_start, NP, st));
  BUF_TRY(upload(c->k17[K17B_UPE], hg->pl_end, NP, st));
  BUF_TRY(upload(c->k17[K17B_UCOFF], hg->conn_off, NN + 1, st));
  K17Graph g{c->k17[K17B_UX].as<float>(), c->k17[K17B_UPS].as<uint32_t>(), c->k17[K17B_UPE].as<uint32_t>(), c->k17[K17B_UCOFF].as<u64>(),
             nullptr, (uint32_t)NN, (uint32_t)NP};
  uint64_t n_loops = 0, n_conn = 0;
  BUF_TRY(check_graph_head(c, who, g, &n_loops, &n_conn));
  // conn_off[n_nodes] == n_conn is established: that many entries of the caller's conn_pl are the table
  if (n_conn && !hg->conn_pl) return refuse(who, "the graph lacks an array");
  BUF_TRY(upload(c->k17[K17B_UCPL], hg->conn_pl, n_conn, st));
  HIP_TRY(hipStreamSynchronize(st));
  g.conn_pl = c->k17[K17B_UCPL].as<uint32_t>();
  const float ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  return run_edges(c, who, g, n_loops, max_dist, simplify, out_dev, out_host, stats, ms_upload);
}
