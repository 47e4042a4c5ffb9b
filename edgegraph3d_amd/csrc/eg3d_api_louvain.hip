// eg3d_api_louvain.hip — pipeline 1's community detection (K11, eg3d_k11_louvain.hip)
#include "eg3d_api_internal.h"

extern "C" void eg3d_free_communities(eg3d_communities* m) {
  if (!m) return;
  free(m->ids);
  memset(m, 0, sizeof(*m));
}

static int k11_read_ctr(eg3d_ctx* c, uint64_t* v) {
  Readback rb(c);
  const int it = rb.add(c->k11[K11B_CTR].p, 2 * K11_N_CTR);
  BUF_TRY(rb.run());
  memcpy(v, rb.item(it), sizeof(uint64_t) * K11_N_CTR);
  return EG3D_OK;
}
// N = inside * M - sum of a_c^2, the squares as four sums of 32-bit limbs
static __int128 k11_numer(const uint64_t* v, uint64_t M) {
  unsigned __int128 sq = 0;
  for (int l = 3; l >= 0; l--) sq = (sq << 32) + v[K11_C_LIMB0 + l];
  return (__int128)((unsigned __int128)v[K11_C_INSIDE] * M) - (__int128)sq;
}
// (key0, vin) -> sorted (key1, val1) -> the distinct keys in key0 with their sums in `sums`; their number in ctr[K11_C_UNIQUE]
static int k11_sort_reduce(eg3d_ctx* c, const unsigned long long* vin, unsigned long long* sums, size_t n) {
  unsigned long long* const key0 = c->k11[K11B_KEY0].as<unsigned long long>();
  unsigned long long* const key1 = c->k11[K11B_KEY1].as<unsigned long long>();
  unsigned long long* const val1 = c->k11[K11B_VAL1].as<unsigned long long>();
  unsigned long long* const n_out = c->k11[K11B_CTR].as<unsigned long long>() + K11_C_UNIQUE;
  BUF_TRY(sort_pairs_u64_u64(c, key0, key1, vin, val1, n));
  BUF_TRY(reduce_by_key_u64(c, key1, val1, key0, sums, n_out, n));
  return EG3D_OK;
}

extern "C" int eg3d_detect_communities(eg3d_ctx* c, const eg3d_simgraph* g, const eg3d_louvain_params* params, eg3d_communities* out,
                                       eg3d_louvain_stats* stats) {
  static const char who[] = "eg3d_detect_communities";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_louvain_stats", stats->struct_size, sizeof(eg3d_louvain_stats)));
  if (params) BUF_TRY(check_struct_size(who, "eg3d_louvain_params", params->struct_size, sizeof(eg3d_louvain_params), "params"));
  if (!c || !g || !out) {
    g_err = "eg3d_detect_communities: bad arguments";
    return EG3D_ERR_ARG;
  }
  const uint32_t n_nodes = g->n_nodes;
  if (n_nodes && !g->adj_off) {
    g_err = "eg3d_detect_communities: adj_off is NULL";
    return EG3D_ERR_ARG;
  }
  const uint32_t nnz0 = n_nodes ? g->adj_off[n_nodes] : 0;
  if (nnz0 && (!g->adj_node || !g->adj_w)) {
    g_err = "eg3d_detect_communities: adj_node or adj_w is NULL";
    return EG3D_ERR_ARG;
  }
  if (n_nodes >= 0x80000000u || nnz0 >= 0x80000000u) {
    g_err = "eg3d_detect_communities: 2^31 nodes or directed entries, or more (the integer sums are sized for fewer)";
    return EG3D_ERR_CAPACITY;
  }
  const uint32_t max_phases = params && params->max_phases ? params->max_phases : 200u;
  const uint32_t max_sweeps = params && params->max_sweeps ? params->max_sweeps : 1000u;
  const double sweep_thr = params && params->sweep_threshold != 0.0 ? params->sweep_threshold : 1e-6;
  const double phase_thr = params && params->phase_threshold != 0.0 ? params->phase_threshold : 1e-6;
  if (!(sweep_thr > 0.0) || !(phase_thr > 0.0)) {
    g_err = "eg3d_detect_communities: a threshold is negative or not a number";
    return EG3D_ERR_ARG;
  }
  c->k11_valid = false;
  const uint32_t log2_slots = c->tune.louvain_log2_slots ? c->tune.louvain_log2_slots : (uint32_t)__builtin_ctz(K11_DEFAULT_SLOTS);
  const auto now = [] { return std::chrono::steady_clock::now(); };
  const auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  uint32_t n_comm = 0, n_phases = 0, n_sweeps = 0;
  uint64_t n_ovf_total = 0, M = 0;
  __int128 N = 0;
  float ms_upload = 0, ms_sweeps = 0, ms_coarsen = 0, ms_copy = 0;
  if (n_nodes) {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    BUF_TRY(ensure_mailbox(c));
    auto t_stage = now();
    DevBuf* const B = c->k11;
    const size_t nv = (size_t)n_nodes + 1, ne = std::max<size_t>(nnz0, 1);
    for (int k : {K11B_OFF0, K11B_OFF1, K11B_C, K11B_T, K11B_SIZE0, K11B_SIZE1, K11B_MEMBER, K11B_MINM, K11B_FLAG, K11B_RANK, K11B_CN,
                  K11B_OVF, K11B_OCNT, K11B_OOFF})
      BUF_TRY(B[k].ensure(4 * nv));
    for (int k : {K11B_K, K11B_A0, K11B_A1, K11B_IDS}) BUF_TRY(B[k].ensure(8 * nv));
    for (int k : {K11B_NBR0, K11B_NBR1, K11B_EROW0, K11B_EROW1, K11B_W}) BUF_TRY(B[k].ensure(4 * ne));
    for (int k : {K11B_Q0, K11B_Q1, K11B_KEY0, K11B_KEY1, K11B_VAL0, K11B_VAL1}) BUF_TRY(B[k].ensure(8 * ne));
    BUF_TRY(B[K11B_CTR].ensure(sizeof(uint64_t) * K11_N_CTR));
    unsigned long long* const ctr = B[K11B_CTR].as<unsigned long long>();
    uint64_t v[K11_N_CTR];
    // ---- the caller's graph and its rules
    HIP_TRY(hipMemcpyAsync(B[K11B_OFF0].p, g->adj_off, 4 * nv, hipMemcpyHostToDevice, st));
    if (nnz0) {
      HIP_TRY(hipMemcpyAsync(B[K11B_NBR0].p, g->adj_node, 4 * (size_t)nnz0, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(B[K11B_W].p, g->adj_w, 4 * (size_t)nnz0, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(uint64_t) * K11_N_CTR, st));
    launch_k11_validate(st, n_nodes, nnz0, B[K11B_OFF0].as<uint32_t>(), B[K11B_NBR0].as<uint32_t>(), B[K11B_W].as<float>(),
                        B[K11B_EROW0].as<uint32_t>(), B[K11B_Q0].as<unsigned long long>(), ctr + K11_C_FLAGS);
    HIP_TRY(hipGetLastError());
    BUF_TRY(k11_read_ctr(c, v));
    if (const uint32_t bad = (uint32_t)v[K11_C_FLAGS]) {
      const char* what = bad & K11_BAD_OFFSETS     ? "adj_off does not start at 0 or does not ascend"
                         : bad & K11_BAD_NEIGHBOUR ? "a neighbour id is not below n_nodes"
                         : bad & K11_SELF_LOOP     ? "a row lists its own node (a self-loop)"
                         : bad & K11_BAD_ORDER     ? "the neighbours of a row are not strictly ascending"
                         : bad & K11_BAD_WEIGHT    ? "a weight is not a finite number in (0, 1]"
                         : bad & K11_ASYMMETRIC    ? "an entry has no reverse entry (the graph is not symmetric)"
                                                   : "the two directions of an edge carry different weight bits";
      g_err = std::string("eg3d_detect_communities: ") + what;
      return EG3D_ERR_ARG;
    }
    int cur = 0;
    const auto csr = [&](int k, uint32_t n, uint32_t nnz) {
      return K11Csr{n, nnz, B[K11B_OFF0 + k].as<uint32_t>(), B[K11B_NBR0 + k].as<uint32_t>(), B[K11B_EROW0 + k].as<uint32_t>(),
                    B[K11B_Q0 + k].as<unsigned long long>()};
    };
    K11Csr G = csr(cur, n_nodes, nnz0);
    unsigned long long* const kdeg = B[K11B_K].as<unsigned long long>();
    uint32_t* C = B[K11B_C].as<uint32_t>();
    uint32_t* T = B[K11B_T].as<uint32_t>();
    uint32_t* const member = B[K11B_MEMBER].as<uint32_t>();
    uint32_t* const Cn = B[K11B_CN].as<uint32_t>();
    launch_k11_members(st, n_nodes, G.off, member);
    launch_k11_degrees(st, G, kdeg, C, ctr + K11_C_TOTAL);
    HIP_TRY(hipGetLastError());
    BUF_TRY(k11_read_ctr(c, v));
    M = v[K11_C_TOTAL];
    const double MM = (double)M * (double)M;
    ms_upload = ms_since(t_stage);
    // Renumbers the partition Cp of G by first appearance (Cn) and composes it into `member`; says whether Cp was the identity.
    const auto renumber = [&](const uint32_t* Cp, uint32_t& n_new, bool& identity) -> int {
      uint32_t* const minm = B[K11B_MINM].as<uint32_t>();
      uint32_t* const rank = B[K11B_RANK].as<uint32_t>();
      HIP_TRY(hipMemsetAsync(minm, 0xFF, 4 * (size_t)G.n, st));
      HIP_TRY(hipMemsetAsync(ctr + K11_C_NOT_IDENTITY, 0, sizeof(uint64_t), st));
      launch_k11_min_member(st, G.n, Cp, minm, ctr);
      launch_k11_first_flags(st, G.n, Cp, minm, G.off, B[K11B_FLAG].as<uint32_t>());
      HIP_TRY(hipGetLastError());
      BUF_TRY(scan_u32(c, B[K11B_FLAG].as<uint32_t>(), rank, (size_t)G.n + 1));
      launch_k11_relabel(st, G.n, Cp, minm, rank, Cn);
      launch_k11_compose(st, n_nodes, Cn, member);
      HIP_TRY(hipGetLastError());
      Readback rb(c);
      const int ic = rb.add(ctr + K11_C_NOT_IDENTITY, 2);
      const int ir = rb.add(rank + G.n, 1);
      BUF_TRY(rb.run());
      identity = rb.item(ic)[0] == 0 && rb.item(ic)[1] == 0;
      n_new = *rb.item(ir);
      return EG3D_OK;
    };
    // a / size of the partition P into buffer pair `into`, and the numerator's sums into the counters
    const auto totals_and_numer = [&](const uint32_t* P, int into) -> int {
      unsigned long long* const a = B[K11B_A0 + into].as<unsigned long long>();
      uint32_t* const size = B[K11B_SIZE0 + into].as<uint32_t>();
      HIP_TRY(hipMemsetAsync(a, 0, 8 * (size_t)G.n, st));
      HIP_TRY(hipMemsetAsync(size, 0, 4 * (size_t)G.n, st));
      HIP_TRY(hipMemsetAsync(ctr + K11_C_INSIDE, 0, 5 * sizeof(uint64_t), st));
      launch_k11_totals(st, G.n, P, kdeg, a, size);
      launch_k11_inside(st, G, P, ctr);
      launch_k11_squares(st, G.n, a, ctr);
      HIP_TRY(hipGetLastError());
      return k11_read_ctr(c, v);
    };
    if (!M) {  // no weight at all: every node with a row alone, numbered in order
      t_stage = now();
      bool identity;
      BUF_TRY(renumber(C, n_comm, identity));
      ms_coarsen += ms_since(t_stage);
    }
    for (uint32_t phase = 1; M && phase <= max_phases; phase++) {
      t_stage = now();
      if (phase > 1) launch_k11_degrees(st, G, kdeg, C, ctr + K11_C_TOTAL);  // (k and C = identity; the total is not read again)
      int ia = 0;  // the buffer pair that holds a / size of C
      BUF_TRY(totals_and_numer(C, ia));
      const __int128 N0 = k11_numer(v, M);
      __int128 Nprev = N0;
      for (uint32_t sweep = 1; sweep <= max_sweeps; sweep++) {
        const K11Part P{C, kdeg, B[K11B_A0 + ia].as<unsigned long long>(), B[K11B_SIZE0 + ia].as<uint32_t>(), M};
        uint32_t* const ovf = B[K11B_OVF].as<uint32_t>();
        HIP_TRY(hipMemsetAsync(ctr + K11_C_CHANGED, 0, 3 * sizeof(uint64_t), st));
        launch_k11_targets(st, G, P, log2_slots, T, ovf, ctr);
        HIP_TRY(hipGetLastError());
        BUF_TRY(k11_read_ctr(c, v));
        if (const uint32_t n_ovf = (uint32_t)v[K11_C_OVF_ROWS]) {
          // rows whose communities do not fit the table: (row, community) keys of all of them, sorted and summed
          const uint32_t n_oe = (uint32_t)v[K11_C_OVF_ENTRIES];
          n_ovf_total += n_ovf;
          launch_k11_ovf_counts(st, G, ovf, n_ovf, B[K11B_OCNT].as<uint32_t>());
          HIP_TRY(hipGetLastError());
          BUF_TRY(scan_u32(c, B[K11B_OCNT].as<uint32_t>(), B[K11B_OOFF].as<uint32_t>(), (size_t)n_ovf + 1));
          launch_k11_ovf_expand(st, G, C, ovf, n_ovf, B[K11B_OOFF].as<uint32_t>(), B[K11B_KEY0].as<unsigned long long>(),
                                B[K11B_VAL0].as<unsigned long long>());
          HIP_TRY(hipGetLastError());
          BUF_TRY(k11_sort_reduce(c, B[K11B_VAL0].as<unsigned long long>(), B[K11B_VAL0].as<unsigned long long>(), n_oe));
          launch_k11_ovf_targets(st, P, ovf, n_ovf, B[K11B_KEY0].as<unsigned long long>(), B[K11B_VAL0].as<unsigned long long>(),
                                 ctr + K11_C_UNIQUE, T, ctr);
          HIP_TRY(hipGetLastError());
        }
        n_sweeps++;
        BUF_TRY(totals_and_numer(T, 1 - ia));
        if (!v[K11_C_CHANGED]) break;  // T == C
        const __int128 Nnew = k11_numer(v, M);
        if ((double)(Nnew - Nprev) < sweep_thr * MM) break;  // (T is dropped)
        std::swap(C, T);
        ia = 1 - ia;
        Nprev = Nnew;
      }
      ms_sweeps += ms_since(t_stage);
      t_stage = now();
      n_phases++;
      N = Nprev;
      bool identity = false;
      BUF_TRY(renumber(C, n_comm, identity));
      const bool last = identity || (double)(Nprev - N0) < phase_thr * MM || phase == max_phases;
      if (!last) {
        // ---- the coarse graph: the entries keyed by (community of the row, community of the neighbour), sorted and summed
        launch_k11_coarse_keys(st, G, Cn, B[K11B_KEY0].as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        BUF_TRY(k11_sort_reduce(c, G.q, B[K11B_Q0 + (1 - cur)].as<unsigned long long>(), G.nnz));
        BUF_TRY(k11_read_ctr(c, v));
        const uint32_t nnz2 = (uint32_t)v[K11_C_UNIQUE];
        launch_k11_split_keys(st, B[K11B_KEY0].as<unsigned long long>(), nnz2, B[K11B_EROW0 + (1 - cur)].as<uint32_t>(),
                              B[K11B_NBR0 + (1 - cur)].as<uint32_t>());
        launch_k10_row_off(st, B[K11B_KEY0].as<unsigned long long>(), nnz2, 0, n_comm, B[K11B_OFF0 + (1 - cur)].as<uint32_t>());
        HIP_TRY(hipGetLastError());
        cur = 1 - cur;
        G = csr(cur, n_comm, nnz2);
      }
      ms_coarsen += ms_since(t_stage);
      if (last) break;
    }
    launch_k11_ids(st, n_nodes, member, B[K11B_IDS].as<int64_t>());
    HIP_TRY(hipGetLastError());
  }
  // ---- the result, library-owned
  const auto t0 = std::chrono::steady_clock::now();
  int64_t* ids = nullptr;
  BUF_TRY(copy_out(c->stream, who, {{&ids, n_nodes ? c->k11[K11B_IDS].p : nullptr, sizeof(int64_t) * n_nodes}}));
  uint32_t n_isolated = 0;
  for (uint32_t i = 0; i < n_nodes; i++) n_isolated += ids[i] < 0;
  ms_copy = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  out->n_nodes = n_nodes;
  out->ids = ids;
  out->n_communities = n_comm;
  c->k11_valid = true;  // (K11B_IDS holds the ids of n_nodes nodes: eg3d_sets_from_communities_device reads them there)
  c->k11_nodes = n_nodes;
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_louvain_stats);
    stats->n_phases = n_phases;
    stats->n_sweeps = n_sweeps;
    stats->n_communities = n_comm;
    stats->n_isolated = n_isolated;
    stats->n_overflow_rows = n_ovf_total;
    stats->total_q = M;
    stats->numer_hi = (uint64_t)((unsigned __int128)N >> 64);
    stats->numer_lo = (uint64_t)(unsigned __int128)N;
    stats->modularity = M ? (double)N / ((double)M * (double)M) : 0.0;
    stats->ms_upload = ms_upload;
    stats->ms_sweeps = ms_sweeps;
    stats->ms_coarsen = ms_coarsen;
    stats->ms_copy = ms_copy;
  }
  return EG3D_OK;
}
