// eg3d_k3b_expand.h — K3b, the expand stage, one wavefront per chain (gfx950 only; included by eg3d_k3_chains.hip,
// which instantiates k3b_expand_t and holds the launch wrappers).
//
// What the stage computes is stated sequentially by expand_chain with TeamSeq in eg3d_dev_expand.h (the host simulation
// of the tests runs that). This file is how the GPU runs it: TeamWaveT, the 64-lane team; the slot pools that lend the
// chains their working slices; k3b_expand_t and the two small kernels around a launch.
#pragma once
#include "eg3d_dev_pipeline.h"

#include "eg3d_dev_coopgn.h"

// The A/B switches of rounds 3-6 are decided and their losing forms deleted; a build that still passes one would time
// the product against itself.
#if defined(EG3D_SIDE_WALK_BATCH) || defined(EG3D_WINDOW_ROUNDS) || defined(EG3D_WAVE_SLOT_STEP) || defined(EG3D_DLT_GRP) || \
    defined(EG3D_DLT_HOT_IN_LDS) || defined(EG3D_REDO_SKIP) || defined(EG3D_PAR_CANDIDATES) || defined(EG3D_PAR_APPEND) ||   \
    defined(EG3D_SPEC_FOLLOW)
#error "The expand kernel's A/B switches (EG3D_SIDE_WALK_BATCH, EG3D_WINDOW_ROUNDS, EG3D_WAVE_SLOT_STEP, EG3D_DLT_GRP, EG3D_DLT_HOT_IN_LDS, EG3D_REDO_SKIP, EG3D_PAR_CANDIDATES, EG3D_PAR_APPEND, EG3D_SPEC_FOLLOW) were removed; this build would be the product. See DESIGN_LOG.md, 'The expand kernel's decided switches are gone'."
#endif

namespace eg3d {

// One WAVEFRONT per chain (block = 64 lanes). Control flow is wave-uniform; the lane-parallel
// sections are (a) the per-view projection + 4 px grid lookup + closest point of every chain
// point and (b) the Gauss-Newton ADD solves of a side walk's candidates (see eg3d_dev_expand.h).
#ifndef EG3D_LOOKAHEAD
#define EG3D_LOOKAHEAD 8 /* steps walked ahead per round (<= 8, and <= 64 / observations of the end point) */
#endif
#ifndef EG3D_LA_RESUME
#define EG3D_LA_RESUME 8 /* look-ahead depth after a redone round (0 = off for the rest of the following call: rounds 3-5). Round 6, light timing build: the sequential N-view steps were 17 % of the chain clocks for 215 k steps against 21 % for the 1.2 M steps of the look-ahead rounds (a step on its own pays a whole DLT stream and a solver batch); A/B 0 / 2 / 4 / 8: C3' 43.7 / 42.5 / 42.3 / 42.4 ms, C2 6.22 / 5.50 / 5.42 / 5.15 ms */
#endif
// GN_KEEP: see gn_round (0 = standard build; 4 = the wide build keeps the rows of up to four chunks in registers)
// SCENE = the class of scenes an instantiation serves (the host picks it per context, launch_k3b):
//   0  small: <= 28 views and polylines of <= 512 vertices — the solver's long-request path (a point has at most one
//      observation per view, so no solve exceeds a packed round) and the side walks over polylines that do not fit
//      the LDS staging area are compiled out;
//   1  general: everything;
//   2  many views (>= 29) and polylines of <= 512 vertices: the N-view step's lists never fit LDS there (2 V + 8 > 64
//      observations), so chain following is always one step at a time — the look-ahead rounds are compiled out —,
//      the speculative central solves are always windowed, and the unstaged side walks are compiled out as in 0.
// What a scene cannot execute is not free in a 45-70 k-instruction kernel: register allocation and the instruction
// cache both see it (C3': 50.4 -> 47.5 ms with SCENE 0; C4: 1828 -> 1732 ms per step in flight with SCENE 2).
template <int GN_KEEP, int SCENE>
struct TeamWaveT {
  static constexpr bool LONG_GN = SCENE != 0;
  static constexpr int kPreIt = (SCENE == 2 || EG3D_GN_PRECHECK_ALL) ? EG3D_GN_PRECHECK_IT : 30;  // eg3d_dev_coopgn.h
  // the N-view step tries its candidates one after the other (stepn_chain reads this): on the wave the slot-based
  // step measured slower, failed speculative candidates run all 30 GN iterations
  static constexpr bool kSlotStep = false;
  static constexpr bool kSpecFollow = SCENE != 2;  // chain following walks ahead, then triangulates the steps together: follow()
  CoopLds* L;
  __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63u); }
  __device__ __forceinline__ int size() const { return 64; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void bind(Chain& c) const {
    if constexpr (SCENE != 2)
      if (c.tmp_cap <= EG3D_COOP_ROWS) c.tmp_a = L->tmp_a;
  }
  __device__ __forceinline__ bool lazy_presolve(const DevScene& s) const {
    if constexpr (SCENE == 2) return true;
    return eg3d::lazy_presolve(s);
  }
  __device__ __forceinline__ int rank(bool flag, int& total) const {
    const unsigned long long m = __ballot(flag);
    total = __popcll(m);
    return __popcll(m & ((1ull << lane()) - 1ull));
  }
  template <class T>
  __device__ __forceinline__ T uni(const T& v) const {
    static_assert(sizeof(T) % 4 == 0, "uni(): whole dwords");
    union {
      T t;
      int w[sizeof(T) / 4];
    } u;
    u.t = v;
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; i++) u.w[i] = __builtin_amdgcn_readfirstlane(u.w[i]);
    return u.t;
  }
  // the 2-view DLT of a uniform section: the first group of 8 lanes runs the decomposition (dlt2_grp8,
  // eg3d_dev_coopgn.h: rows of A and V in registers, only the ordered sums through LDS); the start point is then broadcast.
  // (Two functions where one would do: with the body in dlt() itself the compiler issues dlt2_grp8's multiplications in
  // another order — same instructions, other bytes. Collapse them in a change that is timed against its parent.)
  __device__ __forceinline__ void dlt(const float* P1, float x1, float y1, const float* P2, float x2, float y2,
                                      double X0[3]) const {
    dlt_group0(P1, x1, y1, P2, x2, y2, X0);
  }
  __device__ __forceinline__ void dlt_group0(const float* P1, float x1, float y1, const float* P2, float x2, float y2,
                                             double X0[3]) const {
    __syncthreads();
    double r[3] = {0, 0, 0};
    dlt2_grp8(L->dltg, lane() < 8, P1, x1, y1, P2, x2, y2, r);
    X0[0] = lane_bcast(r[0], 0);
    X0[1] = lane_bcast(r[1], 0);
    X0[2] = lane_bcast(r[2], 0);
    __syncthreads();
  }
  // OR over the lanes of a small flag word (the EG3D_FLAG_* bits 0..4 the expand stage raises): one ballot per bit
  __device__ __forceinline__ uint32_t or_reduce(uint32_t v) const {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t b = 1; b <= 16u; b <<= 1)
      if (__ballot((v & b) != 0)) r |= b;
    return r;
  }
  template <class Pred>
  __device__ __forceinline__ int leading_true(int m, Pred pred) const {
    int cnt = 0;
    for (int j0 = 0; j0 < m; j0 += 64) {
      const int j = j0 + lane();
      const unsigned long long mask = __ballot(j < m && pred(j));
      const unsigned long long inv = ~mask;
      const int lead = inv ? (__ffsll((long long)inv) - 1) : 64;
      cnt += lead;
      if (lead < 64) break;
    }
    return cnt;
  }
  __device__ __forceinline__ uint64_t valid_mask(const Chain& c, int base, int end) const {
    const int k = base + lane();
    return __ballot(k < end && c.cand[k].valid != 0);
  }
  __device__ __forceinline__ int group_size(int n_items) const {
    int g = 1;
    while (g < 16 && g * 2 * n_items <= 64) g <<= 1;
    return g;
  }
  __device__ __forceinline__ void group_best(int G, float& d, PlPt& p) const {
    for (int o = 1; o < G; o <<= 1) {
      const float od = __shfl_xor(d, o);
      const uint32_t os = (uint32_t)__shfl_xor((int)p.seg, o);
      const float ox = __shfl_xor(p.x, o), oy = __shfl_xor(p.y, o);
      if (od < d || (od == d && os < p.seg)) {
        d = od;
        p.seg = os;
        p.x = ox;
        p.y = oy;
      }
    }
  }
  __device__ __forceinline__ uint32_t excl_scan(uint32_t v, uint32_t& total) const {
    const uint32_t pre = (uint32_t)wave_incl_scan((int)v);
    total = lane_bcast(pre, 63);
    return pre - v;
  }
  // Staging for the side walks of ONE attachment (all of them walk the same polyline of the same view): the polyline's
  // vertices (when they fit) and the epipolar lines of the chain points on either side of ci — the lower side
  // (ci-1, ci-2, ... >= lo) in the first half of the staging area, the upper side (ci+1, ... < hi) in the second —
  // copied to LDS once by all lanes. (Round 3 staged per side walk: four times per attachment.)
  static constexpr int kEpiHalf = EG3D_STAGE_EPI / 2;
  __device__ __forceinline__ void walk_stage(const DevScene& s, Chain& c, int view, const PlRef& pl, int lo, int ci,
                                             int hi) const {
    __syncthreads();
    if (pl.n <= EG3D_STAGE_VTX)  // (always, in the small-scene build; the test keeps a stray long polyline from overrunning LDS)
      for (uint32_t i = (uint32_t)lane(); i < pl.n; i += 64) L->walk.vtx[i] = pl.v[i];
    const int n_lo = ci - lo < kEpiHalf ? (ci - lo < 0 ? 0 : ci - lo) : kEpiHalf;
    const int n_hi = hi - ci - 1 < kEpiHalf ? (hi - ci - 1 < 0 ? 0 : hi - ci - 1) : kEpiHalf;
    for (int t = lane(); t < n_lo + n_hi; t += 64) {
      const bool low = t < n_lo;
      const int pt = low ? ci - 1 - t : ci + 1 + (t - n_lo);
      const int slot = low ? t : kEpiHalf + (t - n_lo);
      const ViewCand& ve = c.cand[c.head + pt];
      L->walk.epi[slot][0] = ve.eok ? 1.0f : 0.0f;
      L->walk.epi[slot][1] = ve.ea;
      L->walk.epi[slot][2] = ve.eb;
      L->walk.epi[slot][3] = ve.ec;
    }
    __syncthreads();
  }
  // One side walk from the staged data, walked through address_space(3) pointers (ds_read).
  __device__ __forceinline__ int side_walk(const DevScene& s, Chain& c, int view, const PlRef& pl, const Obs& from,
                                           uint32_t direction, int lo, int ci, int hi, bool towards_start, Pending* out) const {
    typedef const __attribute__((address_space(3))) float* lds_fp;
    typedef const __attribute__((address_space(3))) f2* lds_f2p;
    const int count = towards_start ? ci - lo : hi - ci - 1;
    const bool fits = SCENE != 1 || pl.n <= EG3D_STAGE_VTX;  // scene classes 0 and 2: every polyline fits (host-checked)
    const int staged = count < kEpiHalf ? (count < 0 ? 0 : count) : kEpiHalf;
    const lds_fp epi = (lds_fp)&L->walk.epi[towards_start ? 0 : kEpiHalf][0];
    // next hit of the line towards `direction`, SEGMENT-PARALLEL: lane 0 tests the partial segment
    // from the current position, lane k the k-th whole segment beyond it; the first lane (walking
    // order) whose test reports a hit or a quasi-parallel stop decides — exactly the sequential
    // scan of walk_by_line, one test deep instead of one per segment
    auto walk = [](const auto& p, const PlPt& from, uint32_t dir, float la, float lb, float lc, PlPt& nx) -> uint32_t {
      const bool to_start = dir == p.start;
      if (!to_start && dir != p.end) return WALK_BAD_DIR;  // Q15
      const LineDir ld = line_dir(la, lb);
      const uint32_t lane = threadIdx.x & 63u;
      // candidates in walking order: towards start: 1 + from.seg ; towards end: 1 + (n - 2 - from.seg)
      const uint32_t total = 1u + (to_start ? from.seg : (p.n - 2u - from.seg));
      for (uint32_t k0 = 0; k0 < total; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t r = 0, seg = 0;
        float hx = 0.f, hy = 0.f;
        if (k < total) {
          float x1, y1, x2, y2;
          if (k == 0) {
            x1 = from.x;
            y1 = from.y;
            const uint32_t vi = to_start ? from.seg : from.seg + 1u;
            x2 = p.v[vi].x;
            y2 = p.v[vi].y;
            seg = from.seg;
          } else if (to_start) {
            const uint32_t i = from.seg - (k - 1u);  // segment (v[i], v[i-1]), i >= 1
            x1 = p.v[i].x;
            y1 = p.v[i].y;
            x2 = p.v[i - 1].x;
            y2 = p.v[i - 1].y;
            seg = i - 1u;
          } else {
            const uint32_t i = from.seg + k;  // segment (v[i], v[i+1]), i <= n-2
            x1 = p.v[i].x;
            y1 = p.v[i].y;
            x2 = p.v[i + 1].x;
            y2 = p.v[i + 1].y;
            seg = i;
          }
          r = seg_line_hit_guarded(x1, y1, x2, y2, la, lb, lc, ld, hx, hy);
        }
        const unsigned long long any = __ballot(r != 0);
        if (any) {
          const int f = __ffsll((long long)any) - 1;
          const uint32_t rf = lane_bcast(r, f);
          if (rf & 2u) return WALK_QUASIPARALLEL;
          nx.seg = lane_bcast(seg, f);
          nx.x = lane_bcast(hx, f);
          nx.y = lane_bcast(hy, f);
          return WALK_FOUND;
        }
      }
      return WALK_EXTREME;
    };
    if (fits) {
      PlRefT<lds_f2p> pls;
      pls.v = (lds_f2p)&L->walk.vtx[0];
      pls.n = pl.n;
      pls.start = pl.start;
      pls.end = pl.end;
      return walk_side_candidates_core(s, c, pls, epi, staged, view, from, direction, lo, ci, hi, towards_start, out,
                                       walk);
    }
    if constexpr (SCENE != 1) return 0;  // unreachable in those builds (fits is a constant there)
    return walk_side_candidates_core(s, c, pl, epi, staged, view, from, direction, lo, ci, hi, towards_start, out, walk);
  }
  // The walk phase of the starting observations st0 .. n-1 of an N-view step, SEVERAL CANDIDATES AT ONCE (round 6). The
  // sequential order tries them one after the other and takes the first that keeps >= 3 observations; each try is a
  // pass of the wave in which n - 1 lanes walk — and a following ENDS with a step in which every candidate is tried
  // and dies (4 % of the chain clocks on C3'). Here lane (g, i) of a pass is observation i of candidate st = base + g,
  // 64 / n candidates per pass: every lane of a group advances the group's starting observation itself (the same
  // uniform walk, redundantly), then follows its own observation; the first group in order whose walks keep >= 3
  // wins, its survivors are compacted in observation order exactly as stepn_walks does, and only the diagnostic flags
  // of the candidates up to the winner count (the sequential order never ran the later ones). Returns m (0: all dead).
  __device__ __forceinline__ int stepn_walks_par(const DevScene& s, const Obs* co_all, int n, int st0, const uint32_t* dirs,
                                                 Obs* sel, uint32_t& flags, int& st_used) const {
    const int per = 64 / n;
    if (per < 2) {
      int m = 0;
      for (int st = st0; st < n && m == 0; st++) {
        m = stepn_walks(*this, s, co_all, n, st, dirs, sel, n, flags);
        st_used = st;
      }
      return m;
    }
    const int g = lane() / n, i = lane() - g * n;
    for (int base = st0; base < n; base += per) {
      const int st = base + g;
      const bool valid = g < per && st < n;
      bool dead = true, bad = false, found = false, bad_i = false;
      PlPt q;
      q.seg = 0;
      q.x = q.y = 0.f;
      Obs so, r;
      so.view = 0;
      so.pl = so.seg = 0;
      so.x = so.y = 0.f;
      r = so;
      if (valid) {
        so = co_all[st];
        const PlRef ps = polyline_of(s, so.view, so.pl);
        PlPt p;
        p.seg = so.seg;
        p.x = so.x;
        p.y = so.y;
        const uint32_t w = walk_by_distance(ps, p, dirs[so.view], EG3D_FOLLOW_STEP, q);
        bad = (w & WALK_BAD_DIR) != 0;
        dead = (w & WALK_EXTREME) != 0;
        if (!dead && i != st) {
          const Obs co = co_all[i];
          float la, lb, lc;
          if (epiline(s.F, s.F_valid, s.n_views, so.view, co.view, q.x, q.y, la, lb, lc)) {
            const PlRef pk = polyline_of(s, co.view, co.pl);
            PlPt cp, rp;
            cp.seg = co.seg;
            cp.x = co.x;
            cp.y = co.y;
            const uint32_t wr = walk_by_line(pk, cp, dirs[co.view], la, lb, lc, true, EG3D_FOLLOW_MIN, EG3D_FOLLOW_MAX, rp);
            bad_i = (wr & WALK_BAD_DIR) != 0;
            if (wr & WALK_FOUND) {
              found = true;
              r.view = co.view;
              r.pl = co.pl;
              r.seg = rp.seg;
              r.x = rp.x;
              r.y = rp.y;
            }
          }
        }
      }
      const unsigned long long fm = __ballot(found);
      const unsigned long long gm = ((1ull << n) - 1ull) << (valid ? g * n : 0);  // this lane's group (n <= 32 here)
      const int cnt = valid ? __popcll(fm & gm) : 0;
      const bool alive = valid && !dead && 1 + cnt >= 3;
      const unsigned long long am = __ballot(alive);
      const unsigned long long bm = __ballot(valid && (bad_i || bad));
      const int gw = am ? (__ffsll((long long)am) - 1) / n : per;  // the winning group (per: none in this pass)
      // flags of the candidates the sequential order would have run: groups <= gw
      {
        const int upto = gw < per ? (gw + 1) * n : per * n;
        const unsigned long long lanes = upto >= 64 ? ~0ull : ((1ull << upto) - 1ull);
        if (bm & lanes) flags |= 8u;
      }
      if (gw < per) {
        if (g == gw) {
          if (i == 0) {
            Obs o0;
            o0.view = so.view;
            o0.pl = so.pl;
            o0.seg = q.seg;
            o0.x = q.x;
            o0.y = q.y;
            sel[0] = o0;
          }
          if (found) sel[1 + __popcll(fm & gm & ((1ull << lane()) - 1ull))] = r;
        }
        const int m = 1 + lane_bcast(cnt, gw * n);
        st_used = base + gw;
        __syncthreads();
        return m;
      }
    }
    __syncthreads();
    return 0;
  }
  // append a followed point at the chain's front / back (the checks of follow_front / follow_back)
  __device__ __forceinline__ bool follow_append(Chain& c, bool front, const Obs* list, int m, const float X[3]) const {
    if (front ? (c.head <= 0) : (c.head + c.len >= c.cap_pts)) {
      c.flags |= 1u;
      return false;
    }
    ChainPt np;
    // the new point's block is reserved for m + 1 observations (point_reserve: the smallest power of two >= 4 that holds
    // them), so storing m never relocates it: lane i stores observation i, one barrier at the end (m stores by every lane,
    // as new_point_from_tmp has them: C3' 43.7-43.9 -> 43.4-43.5 ms)
    np.X[0] = X[0];
    np.X[1] = X[1];
    np.X[2] = X[2];
    point_init(np);
    if (!point_reserve(c, np, (uint32_t)m + 1)) return false;
    for (int i = lane(); i < m; i += 64) c.pool[np.off + (uint32_t)i] = list[i];
    np.nobs = (uint32_t)m;
    if (front) {
      c.head--;
      c.pts[c.head] = np;
    } else {
      c.pts[c.head + c.len] = np;
    }
    c.len++;
    __syncthreads();  // the observations were stored by different lanes: visible to all before the next step reads them
    return true;
  }
  // Chain following (follow_direction_vector_start/_end, plg_matching.cpp:771-795) with LOOK-AHEAD.
  // The walks of step t+1 start from the observations step t FOUND, not from its triangulated X,
  // so up to D = 8 steps are walked ahead first (each: the first starting observation whose walks
  // keep >= 3 observations — exactly the candidate the sequential N-view step triangulates first);
  // their D initial DLTs then run side by side on D lanes (one DLT's worth of instructions instead
  // of D) and their D all-observation Gauss-Newton solves as D groups of one cooperative batch.
  // Steps are accepted in order while their triangulation succeeds; the first one that fails goes
  // on as the sequential N-view step does (3-subset fallback, later candidates), and the steps
  // walked beyond it are dropped (their diagnostic flags too). Measured: a following call adds
  // 3.4-4.7 points and >95 % of the triangulations succeed.
  __device__ __forceinline__ int follow(const DevScene& s, Chain& c, bool front) const {
    const uint32_t* dirs = front ? c.start_dirs : c.end_dirs;
    int added = 0;
    // look-ahead depth limit: EG3D_LOOKAHEAD to start with; after a round whose step had to be redone look-ahead
    // resumes at depth EG3D_LA_RESUME (< 2: stays off for the rest of the call) and doubles with every round that is
    // accepted whole
    int d_cap = EG3D_LOOKAHEAD;
    bool look_ahead = true;
    for (;;) {
      const ChainPt& endpt = front ? chain_at(c, 0) : chain_at(c, c.len - 1);
      const int n_end = (int)endpt.nobs;
      int D = n_end > 0 ? EG3D_COOP_ROWS / n_end : 0;
      if (D > d_cap) D = d_cap;
      bool seq = !look_ahead || D < 2 || c.tmp_a != L->tmp_a;  // long observation lists (or lists not in LDS): plain steps
      if (!seq) {
      // ---- stage 1: walk ahead (lists of step j at tmp_a + j * n_end; a step keeps <= n_end obs)
      int Deff = 0;
      uint32_t fl_dead = 0;  // walk flags of the step that died (merged when the following ends there)
      const uint64_t tq0 = EG3D_TICK();
      {
        const Obs* prev = c.pool + endpt.off;
        int nprev = n_end;
        for (int j = 0; j < D; j++) {
          Obs* sel = L->tmp_a + j * n_end;
          uint32_t fl = 0;
          int m = 0;
#ifdef EG3D_ONE_SECTION
          const uint64_t tdd0 = EG3D_TICK();  // light timing build: section 11 = the walks of the step that DIES (every starting observation tried)
#endif
          int st_used = 0;
          // when the first starting observation dies, the others are walked several at a time (against one pass of the
          // wave each: C3' 39.3 -> 38.7 ms, round 6)
          m = stepn_walks(*this, s, prev, nprev, 0, dirs, sel, n_end, fl);  // (nearly every step that lives, lives on its first candidate)
          if (m == 0 && nprev > 1) m = stepn_walks_par(s, prev, nprev, 1, dirs, sel, fl, st_used);
          if (m == 0) {
#ifdef EG3D_ONE_SECTION
            EG3D_SEC_ADD(c.tsec, 11, EG3D_TICK() - tdd0);
#endif
            fl_dead = fl;
            break;
          }
          if (lane() == 0) {
            L->la_m[j] = m;
            L->la_fl[j] = fl;
            L->la_st[j] = st_used;
          }
          Deff++;
          prev = sel;
          nprev = m;
        }
      }
      if (Deff == 0) {  // no starting observation survives its walks: the following ends here
        c.flags |= fl_dead;
        return added;
      }
      __syncthreads();  // la_m / la_fl
      // ---- stage 2: the Deff initial DLTs, list j on lane j
      const uint64_t tq1 = EG3D_TICK();
      EG3D_SEC_ADD(c.tsec, 1, tq1 - tq0);
      double X0[3] = {0, 0, 0};
      uint32_t dfl = 0;
      // list j on the 8 lanes of group j (every lane of the group selects the two observations; the decomposition is
      // spread over the group: dlt2_grp8); the start point and the flag then move to lane j, where request j lives
      // (against one lane per list with its matrices in LDS: C3' 43.9 -> 43.5 ms, the DLTs' share 19.5 -> 18.0 %, round 6)
      {
        const int gj = lane() >> 3;
        const bool on = gj < Deff;
        const float* P1 = s.cam_P;
        const float* P2 = s.cam_P;
        float gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f;
        if (on) {
          const Obs* a = L->tmp_a + gj * n_end;
          const int n = L->la_m[gj];
          int mi = 0;
          int32_t mv = a[0].view;
          for (int i = 0; i < n; i++)
            if (a[i].view < mv) {
              mv = a[i].view;
              mi = i;
            }
          const int la = n - 1;
          if (a[mi].view == a[la].view) dfl = 16u;
          P1 = s.cam_P + (size_t)a[mi].view * 16;
          gx1 = a[mi].x;
          gy1 = a[mi].y;
          P2 = s.cam_P + (size_t)a[la].view * 16;
          gx2 = a[la].x;
          gy2 = a[la].y;
        }
        double Xg[3] = {0, 0, 0};
        dlt2_grp8(L->dltg, on, P1, gx1, gy1, P2, gx2, gy2, Xg);
        const int src = (lane() & 7) * 8;  // lane j < 8 takes group j's result
        X0[0] = (double)__shfl((float)Xg[0], src);  // DLT results are float-valued
        X0[1] = (double)__shfl((float)Xg[1], src);
        X0[2] = (double)__shfl((float)Xg[2], src);
        dfl = (uint32_t)__shfl((int)dfl, src);
        if (lane() >= Deff) dfl = 0;
      }
      // ---- stage 3: the Deff Gauss-Newton solves as one batch (request j on lane j)
      const uint64_t tq2 = EG3D_TICK();
      EG3D_SEC_ADD(c.tsec, 5, tq2 - tq1);
      {
        const bool want = lane() < Deff;
        const float X0f[3] = {(float)X0[0], (float)X0[1], (float)X0[2]};  // DLT results are float-valued
        float Xr[3];
        const bool ok = coop_gn_groups<GN_KEEP, LONG_GN, kPreIt>(s.cam_P, *L, want, L->tmp_a + (want ? lane() : 0) * n_end,
                                       want ? L->la_m[lane()] : 0, false, 0, 0.f, 0.f, X0f, Xr);
        // results stay in the request table: L->res_ok[j], L->x0[j]
        (void)ok;
        (void)Xr;
      }
      // ---- stage 4: accept in order
      EG3D_SEC_ADD(c.tsec, 6, EG3D_TICK() - tq2);
      bool redo = false, stop = false;
      int redo_j = 0;
      for (int j = 0; j < Deff; j++) {
        const uint32_t dflj = lane_bcast(dfl, j);
        if (L->res_ok[j]) {
          const float X[3] = {L->x0[j][0], L->x0[j][1], L->x0[j][2]};
          c.flags |= L->la_fl[j] | dflj;
          if (!follow_append(c, front, L->tmp_a + j * n_end, L->la_m[j], X)) {
            stop = true;
            break;
          }
          added++;
#if defined(EG3D_SECTION_TIMING) && !defined(EG3D_ONE_SECTION)
          EG3D_SEC_ADD(c.tsec, 11, 1ull << 16);  // diagnostic: steps accepted from a look-ahead round
#endif
        } else {
#if defined(EG3D_SECTION_TIMING) && !defined(EG3D_ONE_SECTION)
          EG3D_SEC_ADD(c.tsec, 11, 1ull << 32);  // diagnostic: look-ahead rounds that ended in a redo
#endif
          redo = true;  // the rest of the sequential N-view step from the chain's current end (below)
          redo_j = j;
          break;
        }
      }
      // The step that failed is candidate la_st[j] of the sequential N-view step from the chain's current end (the
      // steps before it were appended, so that end IS the list it was walked from): its walks, its DLT and its
      // all-observation solve would be repeated with the same operands and fail the same way. Go on where the
      // sequential order goes on after that failure: the 3-subset fallback on the list, then the later candidates.
      // (Against the whole sequential N-view step again, round 6: C3' 42.3 -> 40.7 ms, C2 4.97 -> 4.26 ms.)
      if (redo && !stop) {
        const int mj = L->la_m[redo_j], stj = L->la_st[redo_j];
        const uint32_t flj = L->la_fl[redo_j] | lane_bcast(dfl, redo_j);
        Obs keep;
        keep.view = 0;
        keep.pl = keep.seg = 0;
        keep.x = keep.y = 0.f;
        if (lane() < mj) keep = L->tmp_a[redo_j * n_end + lane()];
        __syncthreads();
        if (lane() < mj) L->tmp_a[lane()] = keep;
        __syncthreads();
        c.flags |= flj;
        const ChainPt& e2 = front ? chain_at(c, 0) : chain_at(c, c.len - 1);
        float X[3];
        const uint64_t tsq0 = EG3D_TICK();
        int m = stepn_fallback(*this, s, c.tmp_a, mj, c.tmp_b, c.tmp_mask, X, c.flags);
        if (m == 0) m = stepn_chain(*this, s, c, e2, dirs, X, stj + 1);
        EG3D_SEC_ADD(c.tsec, 15, EG3D_TICK() - tsq0);
        if (m == 0) return added;
        if (!follow_append(c, front, c.tmp_a, m, X)) return added;
        added++;
        look_ahead = EG3D_LA_RESUME >= 2;
        d_cap = EG3D_LA_RESUME;
        continue;
      }
      __syncthreads();  // the lists / results are rewritten next
      if (stop) return added;
      if (!redo) {
        if (Deff < D) {  // step Deff died in its walks after Deff accepted steps: the following ends
          c.flags |= fl_dead;
          return added;
        }
        if (d_cap < EG3D_LOOKAHEAD) d_cap *= 2;
        continue;
      }
      // NOT REACHED: a round ends accepted whole, in `stop` (returned above) or in `redo` (continued above). The compiler
      // does not see it — the kernels are 24-296 bytes shorter without these three lines — so they stay until a change
      // that is timed against its parent takes them out.
      seq = true;
      look_ahead = EG3D_LA_RESUME >= 2;
      d_cap = EG3D_LA_RESUME;
      }
      if (seq) {
        const ChainPt& e2 = front ? chain_at(c, 0) : chain_at(c, c.len - 1);
        float X[3];
        const uint64_t tsq0 = EG3D_TICK();
        const int m = stepn_chain(*this, s, c, e2, dirs, X);
        EG3D_SEC_ADD(c.tsec, 15, EG3D_TICK() - tsq0);
#if defined(EG3D_SECTION_TIMING) && !defined(EG3D_ONE_SECTION)
        EG3D_SEC_ADD(c.tsec, 11, 1ull);  // diagnostic: sequential N-view steps
#endif
        if (m == 0) return added;
        if (!follow_append(c, front, c.tmp_a, m, X)) return added;
        added++;
      }
    }
  }
  // uniform section: all lanes hold the same (a, n, X0) and receive the same answer
  __device__ __forceinline__ bool gn_array(const DevScene& s, const Obs* a, int n, const double X0[3],
                                           float Xout[3]) const {
    // one request (lane 0), the whole wave on its rows
    const float X0f[3] = {(float)X0[0], (float)X0[1], (float)X0[2]};  // callers pass float-valued starts
    float Xr[3];
    const bool ok = coop_gn_groups<GN_KEEP, LONG_GN, kPreIt>(s.cam_P, *L, lane() == 0, a, n, false, 0, 0.f, 0.f, X0f, Xr);
    Xout[0] = lane_bcast(Xr[0], 0);
    Xout[1] = lane_bcast(Xr[1], 0);
    Xout[2] = lane_bcast(Xr[2], 0);
    return lane_bcast(ok ? 1 : 0, 0) != 0;
  }
  __device__ __forceinline__ bool add_array(const DevScene& s, const Obs* a, int n, const Obs& extra, const float X0[3],
                                            float Xout[3]) const {
    float Xr[3];
    const bool ok = coop_gn_groups<GN_KEEP, LONG_GN, kPreIt>(s.cam_P, *L, lane() == 0, a, n, true, extra.view, extra.x, extra.y, X0, Xr);
    Xout[0] = lane_bcast(Xr[0], 0);
    Xout[1] = lane_bcast(Xr[1], 0);
    Xout[2] = lane_bcast(Xr[2], 0);
    return lane_bcast(ok ? 1 : 0, 0) != 0;
  }
  __device__ __forceinline__ bool add_one(const DevScene& s, const Chain& c, const ChainPt& p, const Obs& extra,
                                          float Xout[3]) const {
    const float X0f[3] = {p.X[0], p.X[1], p.X[2]};
    float Xr[3];
    const bool ok = coop_gn_groups<GN_KEEP, LONG_GN, kPreIt>(s.cam_P, *L, lane() == 0, c.pool + p.off, (int)p.nobs, true, extra.view, extra.x,
                                   extra.y, X0f, Xr);
    Xout[0] = lane_bcast(Xr[0], 0);
    Xout[1] = lane_bcast(Xr[1], 0);
    Xout[2] = lane_bcast(Xr[2], 0);
    return lane_bcast(ok ? 1 : 0, 0) != 0;
  }
  // B independent ADD solves, 64 per window, request j on lane j. A window goes cooperative
  // (rows = observations) when that needs fewer row-passes than the longest single solve;
  // otherwise each lane runs its own solve. Both produce the same bits.
  template <class Get, class Put>
  __device__ __forceinline__ void add_solves(const DevScene& s, Chain& c, int B, Get get, Put put) const {
    int take = EG3D_COOP_REQ;
    for (int w0 = 0; w0 < B; w0 += take) {
      const int j = w0 + lane();
      const ChainPt* pt = nullptr;
      Obs o;
      o.view = 0;
      o.pl = o.seg = 0;
      o.x = o.y = 0.f;
      bool want = lane() < EG3D_COOP_REQ && j < B && get(j, pt, o);
      take = EG3D_COOP_REQ;
      float X[3] = {0.f, 0.f, 0.f};
      float X0[3] = {0.f, 0.f, 0.f};
      if (want) {
        X0[0] = pt->X[0];
        X0[1] = pt->X[1];
        X0[2] = pt->X[2];
      }
      const bool ok = coop_gn_groups<GN_KEEP, LONG_GN, kPreIt>(s.cam_P, *L, want, want ? c.pool + pt->off : nullptr, want ? (int)pt->nobs : 0, true,
                                     o.view, o.x, o.y, X0, X);
      if (want) put(j, ok, X);
    }
  }
};
using TeamWave = TeamWaveT<0, 1>;

// Waves per SIMD the expand kernel is built for. Round 4: 4 (128 VGPRs) — CoopLds was cut to 8 LDS allocation units
// (eg3d_dev_coopgn.h) so that four single-wave workgroups really fit a SIMD: rounds 2-3 compared "2 / 3 / 4" with an LDS
// footprint that capped the residency at 3 whatever the registers, i.e. they never measured 4. At 4 the compiler
// spills 261 vector registers (352 B of scratch per lane; almost all of them around the inlined solver calls, not
// inside its loops) against 24 at 3, and the kernel moves 48.9 instead of 29.4 GB per C3' launch — and is faster on
// every workload: C3' K3b 50.3 vs 52.1 ms (47.3 vs 49.6 ms per step in flight), C2 6.85 vs 7.26 ms, the 8192-seed C4
// step 2070 vs 2233 ms, one pass over all of C4 22.7 vs 24.7 s. (2 waves with nothing spilled: 68.2 ms / 2687 ms.)
// What the extra wave hides — the dependent trips of the walks and of a solve's steps — outweighs the spill traffic:
// occupancy is the lever on this kernel. -DEG3D_K3B_WAVES=3 (tools/build_variant.sh) rebuilds the other one.
#ifndef EG3D_K3B_WAVES
#define EG3D_K3B_WAVES 4
#endif
// ---- working slices: a slot-indexed arena ---------------------------------------------------------
// A chain's working state (point headers, observation pool, candidate / pending arrays) lives in a
// SLICE of ChainLayout::total bytes. Slices belong to SLOTS, not to chains: the arena holds as many
// slices as wavefronts can be resident (a few thousand), a chain borrows one for its lifetime and the
// next chain on that slot reuses the same addresses — the arena is a few hundred MB that stays in
// L2 / Infinity Cache and in the TLB, where a slice per chain was 4 GB (C3') to tens of GB (C4) of
// first-touch traffic per launch. Slots are XCD-AFFINE: the per-XCD L2s are not coherent with each
// other, so a slice is only ever touched through ONE XCD's L2 — a wave reads its XCC id and takes a
// slot from that XCD's pool. Hand-over needs no cache maintenance then: the releasing wave waits for
// its stores to be acknowledged by that L2 (s_waitcnt vmcnt(0)) before it returns the slot, and a chain
// never reads a byte of its slice that it has not written itself (so a stale line in a CU's L1 from
// an earlier tenant is never observed). The pool of an XCD is a ring of slot ids with ticket counters:
// pop = take a ticket, then swap the cell at that position to 0 until a slot id comes out; push = take a
// ticket, then CAS the cell from 0 to the id. A pool holds at least as many slots as blocks can be
// resident on its XCD, so a pop only ever waits for a push that is already under way.
__global__ void k_pool_init(SlotPools P) {
  uint32_t* b = P.base + (size_t)blockIdx.x * P.stride;
  for (uint32_t i = threadIdx.x; i < P.ring_n; i += blockDim.x) b[32 + i] = i < P.slots_per_xcd ? i + 1u : 0u;
  if (threadIdx.x == 0) {
    b[0] = 0;
    b[16] = P.slots_per_xcd;
  }
}
__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 7u;
}
#define EG3D_SLOT_NONE 0xffffffffu
__device__ __forceinline__ uint32_t pool_pop(const SlotPools& P, uint32_t xcc) {
  uint32_t* b = P.base + (size_t)xcc * P.stride;
  const uint32_t h = atomicAdd(&b[0], 1u);
  uint32_t* cell = &b[32 + (h & (P.ring_n - 1u))];
  for (uint32_t spin = 0; spin < (1u << 22); spin++) {  // bounded: a pool smaller than the residency is a host bug
    const uint32_t v = atomicExch(cell, 0u);
    if (v) return v - 1u;
    __builtin_amdgcn_s_sleep(16);
  }
  return EG3D_SLOT_NONE;
}
// false = the cell never emptied within the bound (cannot happen while the ring has more cells than slots; reported as
// CTR_SLOT_STARVED by the caller rather than silently losing the slot)
__device__ __forceinline__ bool pool_push(const SlotPools& P, uint32_t xcc, uint32_t slot) {
  uint32_t* b = P.base + (size_t)xcc * P.stride;
  const uint32_t t = atomicAdd(&b[16], 1u);
  uint32_t* cell = &b[32 + (t & (P.ring_n - 1u))];
  for (uint32_t spin = 0; spin < (1u << 22); spin++) {
    if (atomicCAS(cell, 0u, slot + 1u) == 0u) return true;
    __builtin_amdgcn_s_sleep(4);
  }
  return false;
}

// One wavefront per chain, launched longest-first. The finished chain is PACKED into the launch's
// staging area (point headers + its observations back to back, bump-allocated in order of completion)
// before the slot is returned: what leaves the kernel is the chain's result, 16 B per point and per
// observation written once with coalesced stores — not the working slice.
// <WAVES per SIMD the register allocation aims at, GN_KEEP>: the product instantiates <EG3D_K3B_WAVES, 0>. Round 4 measured a
// "wide" instantiation <2, 4> (256 registers: nothing spills, the Gauss-Newton rows of up to four chunks stay in registers
// between the passes of an iteration, so long solves do not recompute them): bit-exact, and SLOWER on every workload
// (C3' K3b 53.2 -> 68.2 ms, the 8192-seed C4 step 2230 -> 2687 ms): what the third wave per SIMD hides in the walks, the
// candidate search and the dependent steps of a solve outweighs the row arithmetic saved.
template <int WAVES, int GN_KEEP, int SCENE>
__global__ void __launch_bounds__(64, WAVES) k3b_expand_t(DevScene s, StageAView a, const TaskDesc* tasks,
                                                 const ChainSeed* chains, uint32_t n_chains, const uint32_t* hyp_off,
                                                 const HypResult* res, const HPoint* arena, const int32_t* map_view,
                                                 const uint32_t* map_entry, const uint32_t* map_n, ChainLayout L,
                                                 unsigned char* slices, SlotPools pools, StageBuf stage, ChainOut* outs,
                                                 uint32_t* out_points, uint32_t* out_obs, Counters* ctr,
                                                 const uint32_t* order) {
  if (blockIdx.x >= n_chains) return;
  __shared__ CoopLds lds;
  const uint32_t lane = threadIdx.x;
  const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[blockIdx.x]);  // longest-first schedule; results stay indexed by chain
  const uint32_t xcc = xcc_id();
  uint32_t slot = 0;
  if (lane == 0) slot = pool_pop(pools, xcc);
  slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
  ChainOut co;
  if (slot == EG3D_SLOT_NONE) {
    if (lane == 0) {
      memset(&co, 0, sizeof(co));
      outs[j] = co;
      out_points[j] = 0;
      out_obs[j] = 0;
      atomicOr(&ctr->flags, CTR_SLOT_STARVED);
    }
    return;
  }
  TeamWaveT<GN_KEEP, SCENE> tm;
  tm.L = &lds;
  if (lane == 0) {
    lds.cams_mid_range = s.cams_mid_range ? 1 : 0;
    lds.long_refused = 0;
    lds.t_start = (uint32_t)wall_clock64();
  }
  __syncthreads();
  // wave-uniform descriptors: kept in scalar registers for the chain's whole life (as vector registers they would be
  // 17 of the 168 the kernel may use, and spilled)
  const ChainSeed cs = tm.uni(chains[j]);
  const TaskDesc d = tm.uni(tasks[cs.task]);
  unsigned char* slice = slices + L.total * ((size_t)xcc * pools.slots_per_xcd + slot);
  expand_chain(tm, s, a, d, cs, tm.uni(hyp_off[cs.task]), res, arena, map_view, map_entry, map_n, L, slice, co);
  // ---- pack the result: 64 points at a time, their observations as one flat range
  unsigned long long pb = 0, ob = 0;
  if (lane == 0) {
    pb = atomicAdd(&stage.used[0], (unsigned long long)co.n_points);
    ob = atomicAdd(&stage.used[1], (unsigned long long)co.n_obs);
  }
  pb = lane_bcast(pb, 0);
  ob = lane_bcast(ob, 0);
  co.spt = pb;
  co.sobs = ob;
  if (pb + co.n_points <= stage.cap_pts && ob + co.n_obs <= stage.cap_obs) {
    __syncthreads();
    uint32_t* s_excl = (uint32_t*)&lds.prod[0][0];  // [65] first flat observation of each of the 64 points in flight
    uint32_t* s_blk = s_excl + 65;                  // [64] where each point's block starts in the pool
    const ChainPt* pts = (const ChainPt*)(slice + L.off_pts) + co.head;
    const Obs* pool = (const Obs*)(slice + L.off_pool);
    StagePt* spt = stage.pts + pb;
    Obs* sob = stage.obs + ob;
    for (uint32_t i0 = 0; i0 < co.n_points; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool act = i < co.n_points;
      ChainPt p;
      p.nobs = 0;
      p.off = 0;
      p.X[0] = p.X[1] = p.X[2] = 0.f;
      if (act) p = pts[i];
      const uint32_t incl = (uint32_t)wave_incl_scan((int)p.nobs);
      const uint32_t total = lane_bcast(incl, 63);
      s_excl[lane] = incl - p.nobs;
      s_blk[lane] = p.off;
      if (lane == 63) s_excl[64] = total;
      if (act) {
        StagePt sp;
        sp.X[0] = p.X[0];
        sp.X[1] = p.X[1];
        sp.X[2] = p.X[2];
        sp.nobs = p.nobs;
        spt[i] = sp;
      }
      __syncthreads();
      for (uint32_t f = lane; f < total; f += 64) {
        uint32_t lo = 0;  // the point whose range holds f: largest q with s_excl[q] <= f (empty points skipped)
#pragma unroll
        for (uint32_t step = 32; step; step >>= 1)
          if (s_excl[lo + step] <= f) lo += step;
        sob[f] = pool[s_blk[lo] + (f - s_excl[lo])];
      }
      __syncthreads();
      sob += total;
    }
  }
  // every store to the slice has been acknowledged by this XCD's L2 before the slot changes hands
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (lane == 0) {
    if (!pool_push(pools, xcc, slot)) atomicOr(&ctr->flags, CTR_SLOT_STARVED);
    outs[j] = co;
    out_points[j] = co.n_points;
    out_obs[j] = co.n_obs;
    if (co.flags) atomicOr(&ctr->flags, co.flags);
    if (SCENE == 0 && lds.long_refused) atomicOr(&ctr->flags, CTR_LONG_REFUSED);
    if (co.bytes) atomicAdd(&ctr->bytes, (unsigned long long)co.bytes);
    // how long this chain held its wavefront (a launch cannot be shorter than its slowest chain: reported per call)
    atomicMax(&ctr->max_chain_ticks, (uint32_t)wall_clock64() - lds.t_start);
  }
}

// After an expand launch in which chains outgrew their working slices: the chains of THAT launch (order[0..n)) whose result
// carries a capacity flag are listed for a relaunch with larger slices — the others keep their packed results — and what
// the listed chains added to the launch's byte counter is taken back (they will add it again).
__global__ void k_collect_overflow(const ChainOut* outs, const uint32_t* order, uint32_t n, uint32_t* redo, uint32_t* n_redo,
                                   Counters* ctr) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint32_t j = order[b];
  const ChainOut co = outs[j];
  if (co.flags & 3u) {  // EG3D_FLAG_CHAIN_OVERFLOW | EG3D_FLAG_OBS_OVERFLOW (include/eg3d.h)
    redo[atomicAdd(n_redo, 1u)] = j;
    if (co.bytes) atomicAdd(&ctr->bytes, 0ull - (unsigned long long)co.bytes);
  }
}

// Cost estimate of a chain for the longest-processing-time-first launch order of K3b:
// initial length x track size of its seed (every track view may attach to every point).
__global__ void k_chain_cost(StageAView a, const TaskDesc* tasks, const ChainSeed* chains, uint32_t n_chains,
                             uint32_t* cost, uint32_t* idx) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_chains) return;
  const ChainSeed cs = chains[j];
  const uint32_t seed = tasks[cs.task].seed;
  const uint32_t k = track_len(a, seed);
  cost[j] = (cs.n1 + 1 + cs.n2) * k;
  idx[j] = j;
}

}  // namespace eg3d
