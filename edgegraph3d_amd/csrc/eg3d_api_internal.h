// eg3d_api_internal.h — what the host drivers of the C ABI (eg3d_api*.hip) share: the error string, the device buffer
// type, the knobs, the context and what it shares (Scene, Seeds) or has learned, the small read-backs and one copy of each
// idiom the stages repeat. Host only; no kernel lives here. (What only the files of the match path share — a batch's state,
// a call's sink and turnstile — is in eg3d_api_match_internal.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/eg3d.h"
#include "eg3d_kernels.h"
#include "eg3d_k8_replay.h"
#include "eg3d_k8a_accumulate.h"
#include "eg3d_k9_polymatch.h"
#include "eg3d_k10_simgraph.h"
#include "eg3d_k11_louvain.h"
#include "eg3d_k14_triangulate.h"
#include "eg3d_k15_colour.h"
#include "eg3d_k16_transform.h"
#include "eg3d_k17_edges.h"

// (hidden: what the drivers share is not part of the library's dynamic symbol table)
#define EG3D_API_BEGIN namespace eg3d { namespace api __attribute__((visibility("hidden"))) {
#define EG3D_API_END }}

EG3D_API_BEGIN
// ONE string per thread for the whole library (defined in eg3d_api.hip; eg3d_last_error returns it)
extern thread_local std::string g_err;
EG3D_API_END

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) {                                                                         \
      eg3d::api::g_err = std::string(#expr) + ": " + hipGetErrorString(_e);                         \
      return EG3D_ERR_HIP;                                                                          \
    }                                                                                               \
  } while (0)

#define BUF_TRY(expr)          \
  do {                         \
    int _r = (expr);           \
    if (_r != EG3D_OK) return _r; \
  } while (0)

EG3D_API_BEGIN
// Every device allocation of the library is made and freed here (eg3d_api.hip), which keeps the count of live bytes that
// eg3d_test_live_device_bytes reports. dev_alloc sets g_err; dev_free takes the size the block was allocated with.
int dev_alloc(void** p, size_t bytes);
void dev_free(void* p, size_t bytes);

// A device block that belongs to the object it is a member of: no copies, released with its owner. Every device buffer of
// the library is one — a context's work and result buffers, the scene's and the seeds' arrays (Scene, Seeds), the
// temporaries of a grid build — so no list of them exists anywhere.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap && p) return EG3D_OK;
    return replace(std::max<size_t>(bytes + bytes / 4, 256));
  }
  // exactly `bytes` (no growth reserve): for a buffer whose size is fixed by the scene and may be hundreds of MB
  int ensure_exact(size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    if (p && cap == bytes) return EG3D_OK;
    return replace(bytes);
  }
  // grow, keeping the first `keep` bytes (device-to-device copy on `st`, old block freed once it is done)
  int ensure_keep(size_t bytes, size_t keep, hipStream_t st);
  void release() {
    dev_free(p, cap);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }

 private:
  int replace(size_t want) {
    release();
    BUF_TRY(dev_alloc(&p, want));
    cap = want;
    return EG3D_OK;
  }
};

// Test / tuning knobs, ALL of them, read from the environment ONCE when a context is created (eg3d_create calls from_env; a
// clone copies the struct) — nothing else in the library calls getenv, but for EG3D_TRI_STAGE_OBS, which eg3d_triangulate and
// eg3d_triangulate_device read at every call (include/eg3d_triangulate.h):
//   EG3D_K3A_ENGINE_WAVES=n  wavefronts per SIMD the K3a engine launches (default 2 = what its 256-VGPR build allows)
//   EG3D_K3A_ENGINE_LANES=n  lanes of a K3a wavefront that take work (default: 64, fewer for small batches)
#ifndef EG3D_K3B_ENGINE_DEFAULT
#define EG3D_K3B_ENGINE_DEFAULT 0
#endif
//   EG3D_HYP_CAP=n         tests: points per following direction of the hypothesis stage (default 160; a list that would
//                          outgrow it raises EG3D_FLAG_HYP_OVERFLOW and the call returns EG3D_ERR_CAPACITY)
//   EG3D_SLOTS_PER_XCD=n   tests: working slices of the expand stage per XCD (default: what can be resident + margin)
//   EG3D_TRACE_ARENA=1     print the hypothesis arena's use per batch to stderr
//   EG3D_ARENA_CAP0=n      initial hypothesis arena capacity (tests: forces the overflow-and-retry path)
//   EG3D_K2_STAGE_CAP=n    tests: hits a wave of K2 stages in LDS (1 .. 128, default 128); a task with more sweeps twice
//   EG3D_HITS_CAP0=n       tests: capacity of the epipolar-hit buffer until a K2 launch of the context has fitted (forces the
//                          enlarge-and-run-again path)
//   EG3D_STAGE_CAP0=n      tests: points the staging area of the expand stage holds (and n x the per-point guess of observations)
//                          until an expand launch of the context has told what it needs (forces the size-it-and-repeat path)
//   EG3D_MAX_SCRATCH_MB=n  tests: cut the chains of a batch into several K3b launches of at most n MB / slice size
//                          chains each (default: one launch takes all chains — their working slices are slots)
//   EG3D_NO_LPT=1          launch chains in identity order instead of longest-first (diagnostic)
//   EG3D_K3B_FULL=1        always run the general build of the expand kernel (default: the build for the scene's class —
//                          polylines of <= 512 vertices and <= 28 views: small, >= 29 views: many views; general otherwise)
//   EG3D_K3B_ENGINE=0|1    (builds with -DEG3D_WITH_K3C_ENGINE only: variants/libeg3d_engine.so) expand stage: 1 = the
//                          lane-per-chain engine (k3c_engine, eg3d_k3c_engine.h), 0 = one wavefront per chain (k3b_expand).
//                          EG3D_K3C_WAVES=n waves per SIMD of the engine's grid, EG3D_K3C_LANES=n lanes of a wave that own a
//                          chain (default: as many waves as fit, then as few lanes as cover the chains). A library built
//                          without the engine refuses EG3D_K3B_ENGINE=1 at eg3d_create.
//   EG3D_PIPELINE_LANES=n  sub-batches of ONE eg3d_match_* call kept in flight on internal contexts (default 0 = by the kind of
//                          call: 3 for a call that copies its cloud to the host, 1 for a device-only call; 1 = the call
//                          runs as a single batch on the context's own stream). EG3D_PIPELINE_UNITS=n: sub-batches the call's
//                          range is cut into (default: chosen from the range, see plan_seed_units). eg3d_set_pipelining
//                          overrides both. Chosen by measurement (profiles/r06_experiments/pipelining_*.json):
//   EG3D_UNIT_RAMP=r       unit i of a seed call gets a share ~ r^i of the range (default 0.6: the LAST unit, whose D2H copy
//                          nothing can hide, is the smallest); EG3D_LANE_PRIORITIES=0|1: lane 0's stream high priority, lane
//                          1 normal, the others low (default 1: the earlier units finish — and cross PCIe — first)
//   EG3D_TEST_FAIL_UNIT=k  tests: the k-th unit (1-based) of every pipelined call fails when its turn to place comes
//   EG3D_ITEM_UNIT_SAMPLES=n  eg3d_match_polyline_items: 20 px samples per unit at most (default 262 144; 32 768 from 64 views)
//   EG3D_TEST_ITEM_WRAP=n  tests: eg3d_match_polyline_items treats a unit with more than n samples x views, hits or
//                          hypotheses as one whose 32-bit totals wrap (the cut-in-two-and-redo path)
struct Tunables {
  bool grid_on_host = false;  // EG3D_GRID_ON_HOST=1 (diagnostic / A-B): build the uniform grids with the host builder on threads
                              // (rounds 1-5, and round 6 before K0) instead of on the device
  int lanes = 0, units = 0, test_fail_unit = 0;
  int copy_threads = 0;  // EG3D_COPY_THREADS_PER_LANE: host threads that copy one piece of a cloud from the ring to the caller's
                         // arrays (0 = EG3D_COPY_THREADS shared by the lanes of the call: 16 on one lane, 5 each on three)
  double unit_ramp = 0.6;
  int lane_priorities = 1;
  static constexpr int kHostCallLanes = 3;  // lanes = 0: a host call's default
  int k3a_engine_waves = 0, k3a_engine_lanes = 0;
  int k3b_engine = EG3D_K3B_ENGINE_DEFAULT, k3c_waves = 0, k3c_lanes = 0;
  bool assume_short = false;  // EG3D_K3B_ASSUME_SHORT=1 (tests): start with the few-views builds whatever the view count, so that
                              // the CTR_LONG_REFUSED -> general build retry runs
  bool trace_arena = false;
  bool k3b_full = false;  // EG3D_K3B_FULL=1: always the full expand kernel (diagnostic)
  uint32_t arena_cap0 = 0, hyp_cap = 0;
  uint32_t chain_cap0 = 0, pool_cap0 = 0;  // EG3D_CHAIN_CAP0 / EG3D_POOL_CAP0 (tests): initial points / observation slots per chain,
                                           // small enough to force the relaunch-what-overflowed path several times
  uint32_t k2_stage_cap = EG3D_K2_STAGE_MAX;  // EG3D_K2_STAGE_CAP (tests): hits a wave of K2 stages in LDS, 1 .. EG3D_K2_STAGE_MAX;
                                              // a task with more takes the count-claim-write route
  uint32_t hits_cap0 = 0;  // EG3D_HITS_CAP0 (tests): capacity of the epipolar-hit buffer until a K2 launch of the context has
                           // fitted, small enough to force the enlarge-and-rerun path (0 = the first guess of run_stage_a)
  uint32_t stage_cap0 = 0;  // EG3D_STAGE_CAP0 (tests): points of the expand stage's staging area while the context has learned
                            // nothing (stage_cap_pts == 0), small enough to force the size-it-and-repeat path (0 = the first guess)
  size_t max_scratch = 0;  // 0 = no limit
  uint32_t slots_per_xcd = 0;  // 0 = sized from the occupancy query
  bool use_lpt = true;
  bool compact_nt = false;  // EG3D_COMPACT_NT=1: non-temporal loads of the compaction's source
  bool merge_write_all = false;  // EG3D_MERGE_WRITE_ALL=1 (A-B): eg3d_dedup_merge_claims writes every word back, not
                                     // only the words it lowered (tools/bench_dedup_phases.py measures one against the other)
  int replay_table_bits = 0;  // EG3D_REPLAY_TABLE_BITS (tests): a node table of 2^bits slots, raised to the smallest power of
                              // two above the number of lookups; 0 = the default, about twice that
  uint64_t simgraph_pair_budget = 0;  // EG3D_SIMGRAPH_PAIR_BUDGET (tests): edge keys one chunk of the clique expansion may
                                      // write; 0 = EG3D_SIMGRAPH_PAIR_BUDGET_DEFAULT
  uint32_t louvain_log2_slots = 0;  // EG3D_LOUVAIN_TABLE_SLOTS (tests): slots of the sweep's per-wave LDS table, raised to a
                                    // power of two in 16 .. 1024; 0 = K11_DEFAULT_SLOTS
  uint32_t item_unit_samples = 0;  // EG3D_ITEM_UNIT_SAMPLES: 20 px samples a unit of eg3d_match_polyline_items holds at most (a
                                   // single polyline with more is a unit of its own); 0 = the default of match_items_call
  uint32_t test_item_wrap = 0;  // EG3D_TEST_ITEM_WRAP (tests): a unit of eg3d_match_polyline_items whose samples x views, hits or
                                // hypotheses exceed it is treated as one whose 32-bit totals wrap (cut in two and redone)
  static Tunables from_env() {
    Tunables t;
    if (const char* e = getenv("EG3D_K3A_ENGINE_WAVES")) t.k3a_engine_waves = atoi(e);
    if (const char* e = getenv("EG3D_K3A_ENGINE_LANES")) t.k3a_engine_lanes = atoi(e);
    if (const char* e = getenv("EG3D_K3B_ENGINE")) t.k3b_engine = atoi(e);
    if (const char* e = getenv("EG3D_K3C_WAVES")) t.k3c_waves = atoi(e);
    if (const char* e = getenv("EG3D_K3C_LANES")) t.k3c_lanes = atoi(e);
    if (const char* e = getenv("EG3D_K3B_ASSUME_SHORT")) t.assume_short = e[0] == '1';
    if (const char* e = getenv("EG3D_HYP_CAP")) t.hyp_cap = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("EG3D_ARENA_CAP0")) t.arena_cap0 = (uint32_t)std::max(16, atoi(e));
    if (const char* e = getenv("EG3D_CHAIN_CAP0")) t.chain_cap0 = (uint32_t)std::max(8, atoi(e));
    if (const char* e = getenv("EG3D_POOL_CAP0")) t.pool_cap0 = (uint32_t)std::max(64, atoi(e));
    if (const char* e = getenv("EG3D_K2_STAGE_CAP")) t.k2_stage_cap = (uint32_t)std::min<int>(EG3D_K2_STAGE_MAX, std::max(1, atoi(e)));
    if (const char* e = getenv("EG3D_HITS_CAP0")) t.hits_cap0 = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("EG3D_STAGE_CAP0")) t.stage_cap0 = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("EG3D_MAX_SCRATCH_MB")) t.max_scratch = (size_t)std::max(1, atoi(e)) << 20;
    if (const char* e = getenv("EG3D_NO_LPT")) t.use_lpt = !(e[0] == '1');
    if (const char* e = getenv("EG3D_TRACE_ARENA")) t.trace_arena = e[0] == '1';
    if (const char* e = getenv("EG3D_K3B_FULL")) t.k3b_full = e[0] == '1';
    if (const char* e = getenv("EG3D_SLOTS_PER_XCD")) t.slots_per_xcd = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("EG3D_PIPELINE_LANES")) t.lanes = std::min(16, std::max(0, atoi(e)));
    if (const char* e = getenv("EG3D_TEST_FAIL_UNIT")) t.test_fail_unit = atoi(e);
    if (const char* e = getenv("EG3D_GRID_ON_HOST")) t.grid_on_host = e[0] == '1';
    if (const char* e = getenv("EG3D_COPY_THREADS_PER_LANE")) t.copy_threads = std::min(32, std::max(1, atoi(e)));
    if (const char* e = getenv("EG3D_LANE_PRIORITIES")) t.lane_priorities = atoi(e);
    if (const char* e = getenv("EG3D_UNIT_RAMP")) t.unit_ramp = std::min(16.0, std::max(1.0 / 16.0, atof(e)));
    if (const char* e = getenv("EG3D_PIPELINE_UNITS")) t.units = std::min(4096, std::max(0, atoi(e)));
    if (const char* e = getenv("EG3D_COMPACT_NT")) t.compact_nt = e[0] == '1';
    if (const char* e = getenv("EG3D_MERGE_WRITE_ALL")) t.merge_write_all = e[0] == '1';
    if (const char* e = getenv("EG3D_REPLAY_TABLE_BITS")) t.replay_table_bits = std::min(40, std::max(0, atoi(e)));
    if (const char* e = getenv("EG3D_SIMGRAPH_PAIR_BUDGET")) t.simgraph_pair_budget = std::min(1ull << 31, strtoull(e, nullptr, 10));
    if (const char* e = getenv("EG3D_LOUVAIN_TABLE_SLOTS")) {
      const unsigned long long want = std::min<unsigned long long>(K11_MAX_SLOTS, std::max<unsigned long long>(K11_MIN_SLOTS, strtoull(e, nullptr, 10)));
      while ((1ull << t.louvain_log2_slots) < want) t.louvain_log2_slots++;
    }
    if (const char* e = getenv("EG3D_TEST_ITEM_WRAP")) t.test_item_wrap = (uint32_t)std::min(0xffffffffull, strtoull(e, nullptr, 10));
    if (const char* e = getenv("EG3D_ITEM_UNIT_SAMPLES")) t.item_unit_samples = (uint32_t)std::min(1ull << 30, std::max(1ull, strtoull(e, nullptr, 10)));
    return t;
  }
};

// the device buffers of eg3d_detect_communities (eg3d_ctx::k11)
enum K11Buf { K11B_OFF0, K11B_OFF1, K11B_NBR0, K11B_NBR1, K11B_EROW0, K11B_EROW1, K11B_Q0, K11B_Q1, K11B_W, K11B_K, K11B_C, K11B_T,
              K11B_A0, K11B_A1, K11B_SIZE0, K11B_SIZE1, K11B_MEMBER, K11B_MINM, K11B_FLAG, K11B_RANK, K11B_CN, K11B_OVF, K11B_OCNT,
              K11B_OOFF, K11B_KEY0, K11B_KEY1, K11B_VAL0, K11B_VAL1, K11B_IDS, K11B_CTR, K11B_COUNT };

// the device buffers of eg3d_edge_chains_device / eg3d_edge_chains (eg3d_ctx::k17). Work: the counters, the claimed
// (polyline, end) flags, the degrees, the successors, the cut nodes, the two buffers of the pointer jumping (five arrays
// each: K17State), the chain heads and their scan, the chain sizes, the simplification's regions and counts. U*: the host
// graph of eg3d_edge_chains. Result (valid until the next call of either entry point): CHAINOFF .. LENGTH.
enum K17Buf { K17B_CTR, K17B_SEEN, K17B_DEG, K17B_SUCC, K17B_CUT, K17B_STATE0, K17B_STATE1 = K17B_STATE0 + 5, K17B_HEADFLAG = K17B_STATE1 + 5,
              K17B_CHAINID, K17B_HEADOF, K17B_CHAINOFHEAD, K17B_NVTX, K17B_REGION, K17B_NF, K17B_NB, K17B_NKEPT, K17B_UX, K17B_UPS,
              K17B_UPE, K17B_UCOFF, K17B_UCPL, K17B_CHAINOFF, K17B_CHAINNODE, K17B_CHAINFLAGS, K17B_SOFF, K17B_SNODE, K17B_LENGTH,
              K17B_COUNT };

// What the scene fixes, as plain values and device addresses (no ownership). Scene holds the original; every context
// carries a copy (share_scene), so that the drivers read c->V, c->ds, ... without a second indirection.
struct SceneFacts {
  int device = 0;
  int V = 0, W = 0, H = 0;
  DevScene ds;
  uint32_t n_pl = 0, n_vtx = 0;  // polylines and vertices of the scene as uploaded
  uint32_t max_pl_vtx = 0;       // vertices of the scene's longest valid polyline
  uint32_t gw[2] = {0, 0}, gh[2] = {0, 0};  // the 30 px and 4 px grids
  uint32_t grid_dropped = 0;
  uint32_t n_simd = 0;         // SIMDs of the device (4 per CU): sizes the K3a engine's launch
  int wall_clock_khz = 0;      // rate of wall_clock64() on the device (hipDeviceAttributeWallClockRate)
  uint32_t slots_per_xcd = 0;  // working slices of the expand stage per XCD (b_cscratch: 8 XCDs x slots_per_xcd slices)
  int k3c_per_cu = 0;          // resident blocks per CU of the lane-per-chain engine (occupancy query)
};
// The immutable scene: eg3d_create makes one, the context, its clones and their lanes share it through a shared_ptr, and it
// goes away with the last of them. It owns the device arrays `ds` points into, and the host copies of the grids for
// eg3d_get_grid (per view CSR with view-local offsets). The grids live on the device (K0 builds them there); the copies are
// made by the first eg3d_get_grid call that asks for a cell size — tests do, the hot path never. Index 2 is the 10 px map of
// the polyline matcher (eg3d_match_polylines_closeness): nobody has it until the first such call on any context of the
// family builds it (ensure_grid10, under `mu`).
struct Scene : SceneFacts {
  DevBuf camP, F, Fv, vpo, pvo, vtx, pls, ple, bbo, bb;
  DevBuf g_off[3], g_ids[3];  // 30 px, 4 px, 10 px
  std::mutex mu;              // guards what follows
  bool have[3] = {false, false, false};
  std::vector<std::vector<uint32_t>> h_off[3], h_ids[3];
  bool built10 = false;
  uint32_t w10 = 0, h10 = 0;
  const uint32_t* d_off(int which) const { return g_off[which].as<uint32_t>(); }
  const uint32_t* d_ids(int which) const { return g_ids[which].as<uint32_t>(); }
  uint32_t cells_per_view(int which) const { return which == 2 ? w10 * h10 : gw[which] * gh[which]; }
  ~Scene() { (void)hipSetDevice(device); }  // (the last owner may be on any thread; the buffers go right after this body)
};
// The resident seeds, immutable once uploaded: eg3d_upload_seeds builds a fresh object and swaps the context's pointer, so
// clones and lanes still matching the old seeds are not disturbed; the arrays go away with the last of them.
struct Seeds {
  const int device;
  explicit Seeds(int device_) : device(device_) {}
  uint32_t n_seeds = 0;
  std::vector<uint32_t> trk_off = {0};  // host copy: ranges are cut and checked with it
  DevBuf toff, tview, txy;
  SeedsDev dev() const {  // as the kernels take them
    SeedsDev sd;
    sd.trk_off = toff.as<uint32_t>();
    sd.trk_view = tview.as<int32_t>();
    sd.trk_xy = txy.as<float>();
    return sd;
  }
  ~Seeds() { (void)hipSetDevice(device); }
};
// What a context has learned about the sizes the scene needs (capacities only grow). A clone starts from its parent's by
// one assignment; lanes take the owner's and give theirs back through merge.
struct Learned {
  uint32_t chain_cap = 384, pool_cap = 0, hyp_cap = 160;
  double arena_per_hyp = 16.0;  // hypothesis arena: points per hypothesis to reserve (learned from overflows)
  double hits_per_list = 4.0;   // epipolar-hit buffer: hits per list to reserve (learned from what K2 claimed; run_stage_a)
  bool hits_learned = false;    // a K2 launch of this context (or of one it shares what it learned with) has fitted its buffer
  bool k3b_long_latched = false;  // a launch of a few-views build met a solve of > 32 rows: the general builds from then on
  uint64_t stage_cap_pts = 0, stage_cap_obs = 0;  // staging area of the expand stage (b_stage_*: grow-only)
  // stage_cap_* are copied with the rest at clone time and NOT merged: they are sizing hints only — every context allocates
  // its own staging area and learns its need from its own launches. (hyp_cap is fixed by EG3D_HYP_CAP at eg3d_create.)
  void merge(const Learned& o) {
    chain_cap = std::max(chain_cap, o.chain_cap);
    pool_cap = std::max(pool_cap, o.pool_cap);
    arena_per_hyp = std::max(arena_per_hyp, o.arena_per_hyp);
    hits_per_list = std::max(hits_per_list, o.hits_per_list);
    hits_learned = hits_learned || o.hits_learned;
    k3b_long_latched = k3b_long_latched || o.k3b_long_latched;
  }
};
// The accumulator of eg3d_replay_accumulate (K8a), one per context (a clone starts with an empty one): the running totals,
// the key the last cloud ended on, and the state on the device — O(nodes + polylines + scene vertices), never the points of
// the run. The scratch of a call is K8's (eg3d_ctx::k8_*: nothing of it outlives a call of either entry point); the state
// and the materialised graph are these buffers alone, so eg3d_replay_device and the accumulator do not meet.
struct ReplayAcc {
  bool valid = true;      // false: a call failed after it began to change the state; only reset != 0 is accepted
  bool have_last = false;
  uint32_t last_key[4] = {0, 0, 0, 0};
  uint64_t n_points = 0, n_pairs = 0, n_nodes = 0, n_pl = 0, n_iv = 0, slots = 0;
  uint64_t tab_pairs = 0;  // what the node table is sized for: the pairs of the clouds + the nodes of the merged graphs
                           // (eg3d_replay_merge_graph: a graph's pair count is the caller's word, its nodes are counted)
  bool map_ready = false;  // the claim map is filled with K8_UNCLAIMED (or holds the run's claims)
  int cur = 0;             // pl_key[cur] holds the sorted keys
  DevBuf slot, node_X, node_point, pl_start, pl_end, pl_key[2];  // node table; the append-only arrays; sorted polyline keys
  DevBuf map, r_ss, r_es, r_sxy, r_exy, cnt;                      // claim map, dense records, the interval counter
  DevBuf node_id, is_new;                                         // per point of the current cloud
  DevBuf conn_off, conn_pl, iv_off, iv_ss, iv_sxy, iv_es, iv_exy;  // the graph as last materialised
  void clear() {  // an empty accumulator that keeps its allocations
    valid = true;
    have_last = map_ready = false;
    n_points = n_pairs = n_nodes = n_pl = n_iv = slots = tab_pairs = 0;
    cur = 0;
  }
  size_t state_bytes() const {
    size_t b = 0;
    for (const DevBuf* d : {&slot, &node_X, &node_point, &pl_start, &pl_end, &pl_key[0], &pl_key[1], &map, &r_ss, &r_es, &r_sxy, &r_exy, &cnt})
      b += d->cap;
    return b;
  }
};
EG3D_API_END

// (an internal header: only the eg3d_api*.hip include it, and they are written in these namespaces)
using namespace eg3d;
using namespace eg3d::api;

// A context is four kinds of state, each in one place: the scene it shares (`scene`, with SceneFacts as plain copies), the
// seeds it shares until the next upload (`seeds`), what it was told and what it has learned (`tune`, `learned`), and what
// it owns alone — the stream, the events and every buffer below. eg3d_clone is written in exactly these terms.
struct eg3d_ctx : SceneFacts {
  std::shared_ptr<Scene> scene;  // (set by share_scene alone)
  std::shared_ptr<const Seeds> seeds;  // (never null once the context is made: no seeds = an object with none)
  Tunables tune;
  Learned learned;
  hipStream_t stream = nullptr;
  // work buffers
  DevBuf b_sv_seed, b_map_view, b_map_entry, b_map_n, b_raw_cnt, b_raw_off, b_cand_pl, b_start_hits, b_cand_cnt,
      b_start_cnt, b_task_off, b_task_seed, b_task_entry, b_task_hit, b_task_k, b_task_list_off, b_list_cnt, b_list_ptr,
      b_hits, b_tasks, b_nhyp, b_hyp_off, b_res, b_arena, b_ctr, b_cs_task, b_valid, b_chain_off, b_chains,
      b_cscratch, b_couts, b_cpts, b_cobs, b_cpoff, b_cooff, b_scan_tmp, b_scanchk, b_cost, b_cidx, b_cost2, b_order, b_redo[2];
  // K3a walk service (Counters::k3a_walks_served / k3a_walk_passes) of the units this lane ran since the last
  // eg3d_probe_k3a_walks (test-only builds read them; the figures come with the counters' read-back in any case)
  unsigned long long k3a_walks_served = 0, k3a_walk_passes = 0;
  DevBuf o_X, o_off, o_view, o_pl, o_seg, o_xy, o_key;
  DevBuf f_X, f_off, f_view, f_xy, f_Xo, f_inl;
  // eg3d_gn_filter_device / eg3d_compact_device / eg3d_filter_resident: histogram + flag word, block totals of the
  // compaction, the compacted cloud (valid until the next compaction), X_out / inlier of eg3d_filter_resident
  DevBuf r_hist, r_blk, r_Xo, r_inl, c_X, c_off, c_view, c_pl, c_seg, c_xy, c_key;
  // eg3d_dedup_device / eg3d_dedup_resident: the claim map (this context's own; created on first use), the kept count +
  // flag word, the mask of eg3d_dedup_resident
  DevBuf d_first, d_cnt, d_keep;
  bool dedup_valid = false;   // the claim map holds the claims of the earlier calls (false: it is filled before use)
  DevBuf prim_tmp;  // scratch of the post stages' rocPRIM primitives (prim_call: K8 .. K11; the pipeline's scans keep b_scan_tmp)
  // eg3d_replay_device (K8). Work: counters + flag word, the node table (slot / last), per point the first point of its
  // node, flags, their scans, the last point of a node, the sort buffers, the interval claim map over
  // the scene's segments with its flags and scan. Result (valid until the next replay): the arrays of eg3d_graph3d.
  DevBuf k8_cnt, k8_slot, k8_last, k8_firstof, k8_flag, k8_rank, k8_lastof, k8_plid, k8_key[2], k8_val[2], k8_map, k8_sflag, k8_pos;
  DevBuf g_nodeX, g_nodept, g_pls, g_ple, g_conoff, g_conpl, g_ivoff, g_ivss, g_ivsxy, g_ives, g_ivexy;
  ReplayAcc ka;  // eg3d_replay_accumulate (K8a): the state of the run and its materialised graph
  // eg3d_match_polylines_closeness (K9). Work: entry -> seed, the per-entry search results, the accept flags and their scan,
  // the match graph over the scene's polylines, the sort buffers, counters + flag word. Result on the device: the accepted
  // ids, row_off, pl_ids (copied to the caller's library-owned arrays at the end of the call).
  DevBuf k9_svseed, k9_cnt, k9_pl, k9_dist, k9_acc, k9_accoff, k9_first, k9_parent, k9_root, k9_ckey, k9_rank, k9_key[2], k9_ctr,
      k9_ref, k9_rowoff, k9_plids;
  // eg3d_similarity_graph (K10). Work: entry -> seed, the per-entry counts and their scan, the (point, polyline) pairs and
  // their swapped form (two sort buffers each way), the CSRs and columns of close_polylines / close_refpoints, the weights,
  // the visibility rows, the pair counts and their 64-bit scan, the node tables, the edge keys (k10_edge: the unique list
  // with the current chunk behind it, and the sort's output), the directed keys and weights, counters + flag word.
  DevBuf k10_svseed, k10_cnt, k10_off, k10_pair[2], k10_crkey, k10_cpoff, k10_cpview, k10_cppl, k10_croff, k10_crpoint, k10_weight, k10_vis,
      k10_npairs, k10_pairoff, k10_nkey[2], k10_nodeof, k10_nodeg, k10_nodeview, k10_nodepl, k10_edge[2], k10_dkey[2], k10_dval[2],
      k10_adjoff, k10_adjnode, k10_ctr;
  // eg3d_detect_communities (K11): the graph of the current and of the next phase, the partition and its totals, the
  // renumbering, the overflow rows, two (key, value) sort buffers, the ids, the counters (K11Buf names them).
  DevBuf k11[K11B_COUNT];
  DevBuf b_sets_off, b_sets_ids;  // polyline sets of the current eg3d_match_polyline_sets call
  // include/eg3d_sets_device.h: polyline sets that stay on the device. u_*: the caller's sets of eg3d_upload_polyline_sets
  // and the flag word of their check. k13_*: eg3d_sets_from_communities_device (K13) — the caller's ids, the "named" flags
  // and their scan, two key buffers, counters ([0] max id + 1, [1] flag word, [2] distinct keys), and the result. What the
  // last call of each producer left (ResidentSets; K9's rows are k9_rowoff / k9_plids), and what K10 / K11 left for K13.
  DevBuf u_sets_off, u_sets_ids, u_bad;
  DevBuf k13_ids, k13_flag, k13_pos, k13_key[2], k13_ctr, k13_rowoff, k13_plids;
  struct ResidentSets {
    bool valid = false;
    uint32_t n_sets = 0;
    uint64_t n_ids = 0;
  } rs_upload, rs_k9, rs_k13;
  bool k10_valid = false, k11_valid = false;  // the last eg3d_similarity_graph / eg3d_detect_communities call succeeded ...
  uint32_t k10_nodes = 0, k11_nodes = 0;      // ... on that many nodes (k10_nodeview / k10_nodepl, k11[K11B_IDS])
  uint32_t items_units = 0, items_redone = 0;  // units of the last eg3d_match_polyline_items call; units it cut in two and redid
  // include/eg3d_triangulate.h (K14). k14_rec: the Obs records of the current batch (at most the staging budget, or one
  // track); k14_ctr: the flag word and the three counts; k14_cuts: the batches of the call. k14_off .. k14_flags: the
  // caller's arrays and the results of eg3d_triangulate (the device entry point works in the caller's own arrays).
  DevBuf k14_rec, k14_ctr, k14_cuts, k14_off, k14_view, k14_xy, k14_X0, k14_Xo, k14_valid, k14_flags;
  // include/eg3d_colour.h (K15). k15_img: the uploaded images, one after the other; k15_tab: the K15Image of every view
  // (both this context's alone: a clone starts without); k15_words: one word per observation of the current call;
  // k15_ctr: the flag word and the three counts. k15_off .. k15_flags: the caller's arrays and the results of
  // eg3d_colour_points (the device entry point works in the caller's own arrays).
  DevBuf k15_img, k15_tab, k15_words, k15_ctr, k15_off, k15_view, k15_xy, k15_keep, k15_rgb, k15_flags;
  bool k15_have_images = false;
  uint32_t k15_n_images = 0;
  // include/eg3d_transform.h (K16). k16_ctr: the two counts; k16_X: the caller's points of eg3d_transform_points, transformed
  // in place (the device entry point works in the caller's own arrays).
  DevBuf k16_ctr, k16_X;
  // include/eg3d/edges.h (K17): K17Buf names the buffers. g_last: the view eg3d_replay_device last handed out (g_valid: there
  // is one), which eg3d_edge_chains_device reads when it is given no graph.
  DevBuf k17[K17B_COUNT];
  bool g_valid = false;
  eg3d_device_graph3d g_last{};
  DevBuf b_fscratch, b_queue, b_items;  // K3a following: per-lane staging lists, work-queue heads, the lists to follow
  // K3b: working slices of the resident chains (b_cscratch: 8 XCDs x slots_per_xcd slices), the slot pools,
  // and the staging area finished chains are packed into (sized from the previous launches; grow-only)
  DevBuf b_pools, b_stage_pts, b_stage_obs, b_stage_used;
  hipEvent_t ea[8] = {}, eb[8] = {};  // begin/end events per stage: 1 K1, 2 K2, 3 K3a, 4 K3s, 5 K3b, 6 K4, 0 misc, 7 whole call
  hipEvent_t ecopy[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // D2H of the cloud: one per ring buffer (EG3D_D2H_RING <= 7)
  void* pinned = nullptr;  // the ring of pinned host buffers the D2H copies of a cloud go through (ensure_d2h_ring)
  size_t pinned_cap = 0, ring_chunk = 0;
  // mailbox for the small read-backs of a step (scan totals, counters): pinned host memory mapped into the
  // GPU's address space, written by k_publish, polled by the calling thread (no driver round trip)
  uint32_t* mbox = nullptr;
  uint32_t* mbox_dev = nullptr;
  uint32_t mbox_seq = 0;
  uint64_t last_np = 0, last_no = 0;
  int last_chunks = 0;
  bool last_accumulated = false;  // the output buffers hold the whole cloud of the last call (device-only calls)
  uint32_t last_nc = 0;
  uint32_t last_nhyp = 0;
  // Internal pipelining of ONE call (run_pipelined): lane 0 is this context, lanes 1.. are clones created on first use
  // (own stream / work buffers, shared scene and seeds). A lane is never handed to the caller.
  std::vector<eg3d_ctx*> lanes;
  bool is_lane = false;
  uint32_t host_calls = 0;  // eg3d_match_* calls with device_only == 0 this context has completed (lanes_for)
  uint64_t last_host_cloud_bytes = 0;  // ... and the size of the last one's cloud
};

EG3D_API_BEGIN
inline void share_scene(eg3d_ctx* c, std::shared_ptr<Scene> s) {  // the ONE place a context's copies of SceneFacts are filled
  static_cast<SceneFacts&>(*c) = *s;
  c->scene = std::move(s);
}
// What a context owns alone from its first moment: its stream, of the given priority (`plain`: no priority asked for), the
// 16 timing events and the 7 copy events. Whoever makes a context — eg3d_create, clone_ctx — holds it in a CtxGuard until
// it is whole: every failing exit in between is a plain return, and eg3d_destroy frees what was made.
enum class StreamPrio { plain, greatest, middle, least };
int make_own_resources(eg3d_ctx* c, StreamPrio prio);
using CtxGuard = std::unique_ptr<eg3d_ctx, void (*)(eg3d_ctx*)>;
// eg3d_clone with the stream priority chosen: share the scene, share the seeds, copy `tune` and `learned`, make own
// resources. Public clones are `plain`; the lanes of a call (ensure_lanes) ask for theirs.
int clone_ctx(eg3d_ctx* parent, StreamPrio prio, eg3d_ctx** out);

int scan_exclusive_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one);  // (hipCUB, on c->b_scan_tmp)
// (key, value) pairs by descending key, queued on the stream (hipCUB, on c->b_scan_tmp): the launch order of the expand stage
int sort_pairs_desc_u32(eg3d_ctx* c, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n);
// n elements of host memory into a device buffer made large enough, queued on `st`
template <typename Buf, typename T>
int upload(Buf& b, const T* src, size_t n, hipStream_t st) {
  BUF_TRY(b.ensure(sizeof(T) * std::max<size_t>(n, 1)));
  if (n) HIP_TRY(hipMemcpyAsync(b.p, src, sizeof(T) * n, hipMemcpyHostToDevice, st));
  return EG3D_OK;
}
// ---- small read-backs through the mailbox ----------------------------------------------------------
// b_scanchk: [0..3] "scan wrapped" flag words (ORed by k_scan_check, cleared by k_publish), [4..5] a saved
// 64-bit counter.
int ensure_mailbox(eg3d_ctx* c);
struct Readback {
  eg3d_ctx* c;
  PubArgs a{};
  uint32_t off[6] = {0, 0, 0, 0, 0, 0};
  uint32_t used = 2;
  explicit Readback(eg3d_ctx* c_) : c(c_) {}
  int add(const void* dev, uint32_t words) {  // returns the item's index
    const int i = a.n++;
    a.src[i] = (const uint32_t*)dev;
    a.words[i] = words;
    off[i] = used;
    used += words;
    return i;
  }
  void clear_after(uint32_t* dev) { a.clear[a.n_clear++] = dev; }
  const uint32_t* item(int i) const { return c->mbox + off[i]; }
  // Launch the publish kernel behind everything queued on the stream and wait for its data: a short poll of
  // the mailbox (the common case: the GPU is a few microseconds behind), then a blocking wait for long kernels.
  int run();
};
// Exclusive scan queued on the stream, its wrap check ORed into flag word `slot`; the total is out[n].
int scan_queue_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one, int slot);
int wrapped_error(const char* what);
// Exclusive scan + its total on the host, with overflow detection: phase totals (candidate slots,
// tasks, lists, hits, hypotheses) are 32-bit; a batch whose total does not fit is refused with
// EG3D_ERR_CAPACITY instead of sizing buffers from a wrapped number.
int scan_total_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n_plus_one, uint32_t& total, const char* what);

// The 10 px map of the polyline matcher, built by the first call that needs it on this context or a clone of it and shared
// by all of them from then on (Scene). eg3d_create neither builds nor allocates it.
int ensure_grid10(eg3d_ctx* c, K9Grid* out, float* ms);
CloudView cloud_view(const eg3d_device_edgepoints* d);
int check_cloud(const eg3d_device_edgepoints* d, const char* who, bool all_arrays);
int device_flags_error(const char* who, uint32_t flags);

// ---- the steps of the 3 px dedup (eg3d_api_dedup_phases.hip) --------------------------------------------------------------
// eg3d_dedup_device / eg3d_dedup_resident (eg3d_api_filter.hip) and the phased calls of include/eg3d_dedup_phases.h are
// written in these and nothing else, so that the combined and the phased forms cannot drift apart.
// index_base + n_points must stay below 2^32 - 1 (K7_UNCLAIMED); sets g_err under `who`
int dedup_index_check(const char* who, uint64_t index_base, uint64_t n_points);
uint64_t dedup_n_cells(const eg3d_ctx* c, int* w = nullptr, int* h = nullptr);  // n_views x ceil(W / 3) x ceil(H / 3), as the host step
// The context's map, allocated on first use and filled with K7_UNCLAIMED when `reset` or when it holds no valid claims.
// Leaves dedup_valid FALSE: the caller sets it once its call is known to have completed, so that a failure in between
// leaves a map that the next call refills.
int dedup_map_open(eg3d_ctx* c, bool reset, K7Map* m);
// the kept count and the flag word (d_cnt: 2 x 8 bytes), zeroed on the stream
int dedup_counters_zero(eg3d_ctx* c, unsigned long long** cnt);
// the read-back that ends a pass: [0] a count, [1] the flag word; synchronises the stream. Flags -> EG3D_ERR_ARG under `who`
int dedup_counters_read(eg3d_ctx* c, const char* who, uint64_t* count);

// ---- one copy of each idiom of the post stages ---------------------------------------------------------------------------
// The two-call form of a rocPRIM primitive (eg3d_k8_replay.h .. eg3d_k11_louvain.h): ask for the scratch size, make room
// in `tmp`, call again. A failure is reported under the primitive's `name`.
template <typename... P, typename... A>
int prim_call(hipStream_t st, DevBuf& tmp, const char* name, hipError_t (*prim)(hipStream_t, void*, size_t&, P...), A... a) {
  size_t bytes = 0;
  hipError_t e = prim(st, nullptr, bytes, a...);
  if (e == hipSuccess) {
    BUF_TRY(tmp.ensure(bytes));
    e = prim(st, tmp.p, bytes, a...);
  }
  if (e == hipSuccess) return EG3D_OK;
  g_err = std::string(name) + ": " + hipGetErrorString(e);
  return EG3D_ERR_HIP;
}
#define EG3D_PRIM(c, f) (c)->stream, (c)->prim_tmp, #f, f
using u64 = unsigned long long;
inline int scan_u32(eg3d_ctx* c, const uint32_t* in, uint32_t* out, size_t n) { return prim_call(EG3D_PRIM(c, k8_scan_u32), in, out, n); }
inline int scan_u64(eg3d_ctx* c, const u64* in, u64* out, size_t n) { return prim_call(EG3D_PRIM(c, k10_scan_u64), in, out, n); }
inline int sort_keys_u64(eg3d_ctx* c, const u64* in, u64* out, size_t n) { return prim_call(EG3D_PRIM(c, k8_sort_keys), in, out, n); }
inline int sort_pairs_u64_u32(eg3d_ctx* c, const u64* kin, u64* kout, const uint32_t* vin, uint32_t* vout, size_t n) {
  return prim_call(EG3D_PRIM(c, k8_sort_pairs), kin, kout, vin, vout, n);
}
inline int sort_pairs_u64_u64(eg3d_ctx* c, const u64* kin, u64* kout, const u64* vin, u64* vout, size_t n) {
  return prim_call(EG3D_PRIM(c, k11_sort_pairs), kin, kout, vin, vout, n);
}
inline int unique_u64(eg3d_ctx* c, const u64* in, u64* out, uint32_t* n_out, size_t n) {
  return prim_call(EG3D_PRIM(c, k10_unique), in, out, n_out, n);
}
inline int reduce_by_key_u64(eg3d_ctx* c, const u64* kin, const u64* vin, u64* kout, u64* sums, u64* n_out, size_t n) {
  return prim_call(EG3D_PRIM(c, k11_reduce_by_key), kin, vin, kout, sums, n_out, n);
}

// A caller's stats / params struct must be at least this library's: "<who>: <arg>->struct_size is smaller than ..."
int check_struct_size(const char* who, const char* type_name, size_t got, size_t want, const char* arg = "stats");

// How eg3d_match_polylines_closeness and eg3d_similarity_graph begin: the argument checks (messages prefixed with `who`),
// the optional seed upload, the range check, and — when the range has track entries and the scene polylines (`active`) —
// the 10 px map, the counters `ctr` (4 words, zeroed; [0] flags) and the entry -> seed map `svseed` of launch_k9_prep,
// and the view ids checked before anything indexes with them.
struct SeedRange {
  uint32_t n_seeds = 0, sv_base = 0, n_sv = 0;
  bool active = false;
  K9Grid g10;
  SeedsDev sd;
  float ms_grid = 0;
};
int open_seed_range(eg3d_ctx* c, const char* who, const eg3d_seeds* seeds, uint32_t b, uint32_t e, const void* out,
                    DevBuf eg3d_ctx::*ctr_of, DevBuf eg3d_ctx::*svseed_of, SeedRange* r);

// Library-owned result arrays: each *dst is allocated (at least one byte) and filled from the device on `st`; an array
// with no source or nothing to copy is zero-filled instead. The stream is synchronised even after a failure, so that no
// copy still writes into what is freed; then every array is freed, "<who>: out of host memory" or "<who>: copy to the
// host: <error>" is set and EG3D_ERR_HIP returned.
struct HostCopy {
  void** dst;
  const void* src;
  size_t bytes;
  template <typename T>
  HostCopy(T** d, const void* s, size_t b) : dst((void**)d), src(s), bytes(b) {}
};
int copy_out(hipStream_t st, const char* who, std::initializer_list<HostCopy> items);
EG3D_API_END
