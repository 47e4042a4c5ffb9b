// Host-visible declarations of K11 (eg3d_k11_louvain.hip): pipeline 1's community detection (eg3d_detect_communities), a
// deterministic Louvain on exact fixed-point weights. The definition is tests/louvain_ref.py; DESIGN.md 4, K11.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eg3d {

#define K11_BLOCK 256
#define K11_WAVES (K11_BLOCK / 64)
#define K11_NONE 0xFFFFFFFFu      /* table: a free slot; member: a node without a row; best: no candidate */
#define K11_MIN_SLOTS 16u
#define K11_MAX_SLOTS 1024u       /* 4 waves x 1024 slots x 12 B = 48 KB of LDS per block */
#define K11_DEFAULT_SLOTS 512u    /* a choice, not a measured result */

// what k11_validate ORs into its flag word, one bit per rule
enum : uint32_t { K11_BAD_OFFSETS = 1u, K11_BAD_NEIGHBOUR = 2u, K11_BAD_ORDER = 4u, K11_SELF_LOOP = 8u, K11_BAD_WEIGHT = 16u,
                  K11_ASYMMETRIC = 32u, K11_WEIGHT_MISMATCH = 64u };

// 64-bit counters of a call (one array, zeroed in ranges between the passes)
enum { K11_C_INSIDE = 0, K11_C_LIMB0 = 1 /* .. 4 */, K11_C_CHANGED = 5, K11_C_OVF_ROWS = 6, K11_C_OVF_ENTRIES = 7, K11_C_TOTAL = 8,
       K11_C_FLAGS = 9, K11_C_NOT_IDENTITY = 10, K11_C_UNIQUE = 11, K11_N_CTR = 12 };

// The graph of a phase: a CSR with a self-loop entry allowed (a coarse vertex's internal weight, counted once in its degree),
// rows ascending, the row of every entry, integer weights.
struct K11Csr {
  uint32_t n, nnz;
  const uint32_t* off;
  const uint32_t* nbr;
  const uint32_t* erow;
  const unsigned long long* q;
};
// What a sweep reads: the partition, degrees, community totals and sizes, M.
struct K11Part {
  const uint32_t* C;
  const unsigned long long* k;
  const unsigned long long* a;
  const uint32_t* size;
  unsigned long long M;
};

// (1) one lane per offset and per directed entry of the caller's CSR: the rules of eg3d_detect_communities ORed into
//     *flags; erow and q of every entry
void launch_k11_validate(hipStream_t st, uint32_t n, uint32_t nnz, const uint32_t* off, const uint32_t* nbr, const float* w,
                         uint32_t* erow, unsigned long long* q, unsigned long long* flags);
// (2) member[i] = i for a node with a row, K11_NONE without
void launch_k11_members(hipStream_t st, uint32_t n, const uint32_t* off, uint32_t* member);
// (3) k[i] = sum of row i; *total (zeroed before) += all of them; C[i] = i
void launch_k11_degrees(hipStream_t st, K11Csr g, unsigned long long* k, uint32_t* C, unsigned long long* total);
// (4) a[C[i]] += k[i], size[C[i]] += 1 (both zeroed before)
void launch_k11_totals(hipStream_t st, uint32_t n, const uint32_t* C, const unsigned long long* k, unsigned long long* a,
                       uint32_t* size);
// (5) THE SWEEP: one wavefront per vertex, e[y] in a per-wave LDS table of `1 << log2_slots` slots; T[i] = target(i). A row
//     whose communities do not fit is appended to ovf (ctr[K11_C_OVF_ROWS], ctr[K11_C_OVF_ENTRIES] += its length) and gets
//     its T from (6)-(8). ctr[K11_C_CHANGED] += 1 per vertex whose target is not its community.
void launch_k11_targets(hipStream_t st, K11Csr g, K11Part p, uint32_t log2_slots, uint32_t* T, uint32_t* ovf,
                        unsigned long long* ctr);
// (6) cnt[r] = length of overflow row r, cnt[n_ovf] = 0; (7) after the scan: key = r << 32 | C[j], value q (0 for the
//     self-loop entry) of every entry of the overflow rows, one wavefront per row
void launch_k11_ovf_counts(hipStream_t st, K11Csr g, const uint32_t* ovf, uint32_t n_ovf, uint32_t* cnt);
void launch_k11_ovf_expand(hipStream_t st, K11Csr g, const uint32_t* C, const uint32_t* ovf, uint32_t n_ovf, const uint32_t* ooff,
                           unsigned long long* key, unsigned long long* val);
// (8) over the sorted and reduced (key, e) pairs, *n_pairs of them: one wavefront per overflow row finds its segment and its
//     target as (5) does
void launch_k11_ovf_targets(hipStream_t st, K11Part p, const uint32_t* ovf, uint32_t n_ovf, const unsigned long long* key,
                            const unsigned long long* e, const unsigned long long* n_pairs, uint32_t* T, unsigned long long* ctr);
// (9) the numerator's two sums of the partition T with totals a: ctr[K11_C_INSIDE] += q of the entries inside a community
//     (one lane per entry, one atomic per block); ctr[K11_C_LIMB0 + l] += limb l (32 bits) of every a[c]^2
void launch_k11_inside(hipStream_t st, K11Csr g, const uint32_t* T, unsigned long long* ctr);
void launch_k11_squares(hipStream_t st, uint32_t n, const unsigned long long* a, unsigned long long* ctr);
// (10) renumbering by first appearance: minm[C[i]] = min i (minm filled with ~0 before) and ctr[K11_C_NOT_IDENTITY] += (C[i]
//      != i); flag[i] = i is the first member of its community and has a row, flag[n] = 0; after the scan of the flags:
//      Cn[i] = rank[minm[C[i]]]; member[v] = Cn[member[v]]
void launch_k11_min_member(hipStream_t st, uint32_t n, const uint32_t* C, uint32_t* minm, unsigned long long* ctr);
void launch_k11_first_flags(hipStream_t st, uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* off, uint32_t* flag);
void launch_k11_relabel(hipStream_t st, uint32_t n, const uint32_t* C, const uint32_t* minm, const uint32_t* rank, uint32_t* Cn);
void launch_k11_compose(hipStream_t st, uint32_t n_nodes, const uint32_t* Cn, uint32_t* member);
// (11) coarsening: key = Cn[i] << 32 | Cn[j] of every entry (value q); after sort and reduce_by_key: erow / nbr = the words
void launch_k11_coarse_keys(hipStream_t st, K11Csr g, const uint32_t* Cn, unsigned long long* key);
void launch_k11_split_keys(hipStream_t st, const unsigned long long* key, uint32_t n, uint32_t* erow, uint32_t* nbr);
// (12) ids[v] = member[v], -1 for K11_NONE
void launch_k11_ids(hipStream_t st, uint32_t n_nodes, const uint32_t* member, int64_t* ids);

// rocPRIM behind plain signatures. tmp == nullptr: the size query.
hipError_t k11_sort_pairs(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in, unsigned long long* key_out,
                          const unsigned long long* val_in, unsigned long long* val_out, size_t n);
// (key_out, sum_out) = the distinct keys of the ascending key_in with the integer sums of their values; *n_out their number
hipError_t k11_reduce_by_key(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* key_in,
                             const unsigned long long* val_in, unsigned long long* key_out, unsigned long long* sum_out,
                             unsigned long long* n_out, size_t n);

}  // namespace eg3d
