// gk_support.h — the paired-end support table (gk_support: pathsMap + badPairs) as the translation units that are not
// gk_pairs.hip see it.  The kernels stay in gk_pairs.hip; what the N-rank reduce (gk_dist_reduce_support, gk_dist.hip)
// needs of them is exposed here as host calls that work on the context's stream.
#pragma once

#include <unordered_map>

#include "gk_internal.h"

struct gk_graph;

static constexpr gk::u64 SUP_EMPTY = ~0ull;
// ctr: [0] distinct pairs [1] bad pairs [2] orientations walked [3] table full [4] a count passed 2^32-1 (checked inserts only)
struct SupView { gk::u64 *keys; gk::u32 *cnt; gk::u64 mask; unsigned long long *ctr; };
struct gk_support {
    gk_ctx *ctx = nullptr;
    gk::u64 *d_keys = nullptr;                 // (e1 << 32 | e2), open addressing, power-of-two capacity
    gk::u32 *d_cnt = nullptr;
    gk::u64 cap = 0;
    unsigned long long *d_ctr = nullptr;       // 8 words (SupView::ctr)
    std::unordered_map<gk::u64, gk::u32> paths;   // host copy for the split (support_to_host), valid while host_valid
    bool host_valid = false;
    float last_ms[5] = {0, 0, 0, 0, 0};        // last gk_graph_walk_pairs: keys from the stream, getAll batch, in-edge lists + checks, walks, overflow walks on the host
    gk::u64 last_overflow = 0;                 // orientations of the last call that went to the host walker
    gk::u64 last_orientations = 0;             // orientations the last call handed to the walk stage (device kernel or, under "pairs_host", the host walker)
};

namespace gk {
// ---- the table's two inserts, for the kernels that count into a support (gk_pairs.hip, gk_thread.hip)
__device__ __forceinline__ void sup_add(const SupView &s, u64 key, u32 c) {
    u64 i = mix64(key) & s.mask;
    for (u64 n = 0; n <= s.mask; n++) {
        u64 cur = s.keys[i];
        if (cur == SUP_EMPTY) {
            cur = atomicCAS(reinterpret_cast<unsigned long long *>(&s.keys[i]), (unsigned long long)SUP_EMPTY, (unsigned long long)key);
            if (cur == SUP_EMPTY) { atomicAdd(&s.ctr[0], 1ull); cur = key; }
        }
        if (cur == key) { atomicAdd(&s.cnt[i], c); return; }
        i = (i + 1) & s.mask;
    }
    s.ctr[3] = 1;
}
// sup_add with a check the walks do not need (one count per pair orientation cannot wrap): a u32 count that wraps raises ctr[4]
__device__ __forceinline__ void sup_add_checked(const SupView &s, u64 key, u32 c) {
    u64 i = mix64(key) & s.mask;
    for (u64 n = 0; n <= s.mask; n++) {
        u64 cur = s.keys[i];
        if (cur == SUP_EMPTY) {
            cur = atomicCAS(reinterpret_cast<unsigned long long *>(&s.keys[i]), (unsigned long long)SUP_EMPTY, (unsigned long long)key);
            if (cur == SUP_EMPTY) { atomicAdd(&s.ctr[0], 1ull); cur = key; }
        }
        if (cur == key) {
            const u32 old = atomicAdd(&s.cnt[i], c);
            if (old + c < old) s.ctr[4] = 1;
            return;
        }
        i = (i + 1) & s.mask;
    }
    s.ctr[3] = 1;
}

// room for `want` distinct pairs at load <= 0.5 (a power of two of slots); contents are kept
int support_reserve(gk_support *s, u64 want);
// the first four counters (distinct, bad, walked, full) to the host
int support_counters(const gk_support *s, unsigned long long *h4);
// The live (key, count) records of s, grouped by owner rank: region p = [region[p], region[p+1]) of d_keys / d_cnt, the
// owner a hash of the key mod P (P <= 64, gk_dist_create's world limit; P = 1 compacts the table).  `room` records must fit
// (GK_E_STATE otherwise: the distinct counter disagrees with the table).  region: P + 1 host words.  Three launches:
// per-workgroup LDS histograms, a scan, the scatter.  canon (nmap entries, or nullptr): the keys leave in the canonical edge
// numbering of graph_edge_canon (GK_E_STATE if a key names an edge that is not live there).
int support_bucket(gk_support *s, int P, u64 *d_keys, u32 *d_cnt, u64 room, u64 *region, const u32 *canon = nullptr, u64 nmap = 0);
// The canonical edge numbering of a replica: live edges ordered by (a 64-bit hash of) their content key, (start k-mer, first
// base) — the same on every replica that holds the same edges, whatever ids its build gave them.  *d_canon [n_edges]: local id ->
// canonical (0xffffffff dead), *d_inv [*nlive]: canonical -> local id; both belong to `keep`, the caller's owner.
// *content_fp: equal on two replicas iff they hold the same live edges (start and end k-mer, first base, length).  GK_E_STATE if
// two live edges share a content key (a node split made copies that share a k-mer).  The sort is rocPRIM's radix sort.
int graph_edge_canon(gk_graph *g, DevScratch &keep, u32 **d_canon, u32 **d_inv, u64 *nlive, u64 *content_fp);
// canonical pair keys back to the local numbering, in place
int support_keys_uncanon(gk_ctx *ctx, u64 *d_keys, u64 n, const u32 *d_inv, u64 nlive);
// insert n records into s (reserved here for distinct + n).  checked: a count that passes 2^32-1 sets *overflow (the table
// then holds a wrapped count: throw it away) — the walk's own insert has no such check.
int support_insert(gk_support *s, const u64 *d_keys, const u32 *d_cnt, u64 n, bool checked, bool *overflow);
// s takes t's table with the counters {distinct (as counted by t's inserts), bad, walked}; t gets s's old table
int support_adopt(gk_support *s, gk_support *t, u64 bad, u64 walked);
}  // namespace gk
