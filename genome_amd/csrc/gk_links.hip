// gk_links.hip — scaffold links: the pair orientations whose mates lie on two DIFFERENT edges, which gk_graph_pair_distances counts
// as `apart` and drops, kept as a table (e, f) -> (count, sum_u); the joins read from it and the chains the joins form.  The rules
// are this project's own and stated in include/genome_amd.h ("scaffold links"); tests/links_ref.py restates them.
//
// Reference: none.  GraphSimplifier.scala ends at the split and the contigs; nothing there orders two edges the graph does not
// connect.
//
// The front end (keys cut from the stream, the four getAll as one batch in HBM, the position check) is gk_graph_walk_pairs' own:
// pairs_front (gk_pairs.hip).  k_pair_links is k_pair_distances' shape (gk_insert.hip): one lane per orientation over the batch's
// CSR, two offsets and, for a placed orientation, two values and two edge lengths; class counts by ballot.  What it adds is one
// insert per `linked` lane into an open-addressed table, gk_support's idiom (gk_support.h: sup_add) with a second plane.
// LDS: the eight class counters only, so the eight 256-thread workgroups a CU holds are bounded by waves, not by LDS (the note at
// PD_LDS_BINS in gk_insert.hip).
// Contention: a library's fragments land on few (e, f) compared with the orientations of a batch, so many lanes add to one slot.
// Every linked lane adds for itself: two atomics on the slot it found.  Combining the equal keys of a wave first (a match loop:
// the leader's key by __shfl, a ballot on equality, the leader adds the popcount and the summed u) was built and measured, and
// does not win: 1.045 ms against 1.042 ms a call on a 4 Mbp genome (profiles/r11/pair_links_4Mbp_400k_pairs_combine_LOSES.txt);
// a wave's neighbours in the stream are unrelated fragments.  It is gone.
//
// The second half of the file is what the N-rank reduce of the table needs (gk_links.h): the canonical edge numbering by path
// content (graph_edge_pathkeys) and the table's records as planes (rec_bucket / rec_insert / rec_uncanon).
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <memory>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "gk_graph.h"
#include "gk_records.h"
#include "gk_scan.h"
#include "gk_support.h"

// ctr: [0] distinct links [3] table full [4] a count passed 2^32-1 (SupView::ctr's numbering)
struct LinkView { u64 *keys; u32 *cnt; unsigned long long *sum; u64 mask; unsigned long long *ctr; };
struct gk_links {
    gk_ctx *ctx = nullptr;
    u64 *d_keys = nullptr;                     // (e << 32 | f), SUP_EMPTY = free; open addressing, power-of-two capacity
    u32 *d_cnt = nullptr;
    unsigned long long *d_sum = nullptr;       // sum of u over the slot's observations, mod 2^64
    u64 cap = 0;
    unsigned long long *d_ctr = nullptr;       // 8 words (LinkView::ctr)
    u64 id_bound = 0;                          // every edge id in the table is below this (the arrays of gk_links_joins)
};

namespace {

enum { LK_UNPLACED = 1, LK_REPETITIVE, LK_AT_NODE, LK_SAME_EDGE, LK_SHORT_EDGE, LK_TOO_FAR, LK_LINKED, LK_NCLASS };

// sup_add_checked with the second plane: claim the slot, then the two adds
__device__ __forceinline__ void link_add(const LinkView &t, u64 key, u32 c, u64 su) {
    u64 i = mix64(key) & t.mask;
    for (u64 n = 0; n <= t.mask; n++) {
        u64 cur = t.keys[i];
        if (cur == SUP_EMPTY) {
            cur = atomicCAS(reinterpret_cast<unsigned long long *>(&t.keys[i]), (unsigned long long)SUP_EMPTY, (unsigned long long)key);
            if (cur == SUP_EMPTY) { atomicAdd(&t.ctr[0], 1ull); cur = key; }
        }
        if (cur == key) {
            const u32 old = atomicAdd(&t.cnt[i], c);
            if (old + c < old) t.ctr[4] = 1;
            atomicAdd(&t.sum[i], (unsigned long long)su);
            return;
        }
        i = (i + 1) & t.mask;
    }
    t.ctr[3] = 1;
}
__device__ __forceinline__ u64 link_find(const LinkView &t, u64 key) {      // the slot, or ~0
    u64 i = mix64(key) & t.mask;
    for (u64 n = 0; n <= t.mask; n++) {
        const u64 cur = t.keys[i];
        if (cur == key) return i;
        if (cur == SUP_EMPTY) return ~0ull;
        i = (i + 1) & t.mask;
    }
    return ~0ull;
}

// One lane per pair orientation o: P1 = vals[off[2o] .. off[2o+1]), P2 = vals[off[2o+1] .. off[2o+2]) (PairFront).
__global__ __launch_bounds__(BLOCK) void k_pair_links(GraphView g, const unsigned long long *__restrict__ off, const u64 *__restrict__ vals, u64 norient, u64 k,
                                                      u64 min_len, u64 max_span, LinkView t, unsigned long long *classes) {
    __shared__ u32 lc[LK_NCLASS];
    if (threadIdx.x < LK_NCLASS) lc[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    u32 wc[LK_NCLASS] = {};                  // this wave's class counts (the same in every lane: sums of ballots)
    // (the trip count is uniform over a wave: the ballots below see all 64 lanes)
    for (u64 base = (u64)blockIdx.x * BLOCK; base < norient; base += (u64)gridDim.x * BLOCK) {
        const u64 o = base + threadIdx.x;
        u32 cls = 0;                         // 0: a lane past the end
        u64 key = 0, u = 0;
        if (o < norient) {
            const u64 a0 = off[2 * o], a1 = off[2 * o + 1], a2 = off[2 * o + 2];
            const u64 n1 = a1 - a0, n2 = a2 - a1;
            if (n1 == 0 || n2 == 0) cls = LK_UNPLACED;
            else if (n1 >= 2 || n2 >= 2) cls = LK_REPETITIVE;
            else {
                const u64 va = vals[a0], vb = vals[a1];
                if (!GK_POS_IS_EDGE(va) || !GK_POS_IS_EDGE(vb)) cls = LK_AT_NODE;
                else if (GK_POS_ID(va) == GK_POS_ID(vb)) cls = LK_SAME_EDGE;
                else {
                    const u32 e = GK_POS_ID(va), f = GK_POS_ID(vb);                  // (k_check_positions: live edges, dist < len)
                    const u64 le = g.e_len[e], lf = g.e_len[f];
                    u = (le + k - GK_POS_DIST(va)) + ((u64)GK_POS_DIST(vb) + k);
                    if (k + le < min_len || k + lf < min_len) cls = LK_SHORT_EDGE;
                    else if (u > max_span) cls = LK_TOO_FAR;
                    else { cls = LK_LINKED; key = ((u64)e << 32) | f; }
                }
            }
        }
#pragma unroll
        for (u32 c = 1; c < LK_NCLASS; c++) wc[c] += (u32)__popcll(__ballot(cls == c));
        if (cls == LK_LINKED) link_add(t, key, 1u, u);
    }
    if (lane == 0) {
#pragma unroll
        for (u32 c = 1; c < LK_NCLASS; c++) if (wc[c]) atomicAdd(&lc[c], wc[c]);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < LK_NCLASS && lc[threadIdx.x]) {
        atomicAdd(&classes[threadIdx.x], (unsigned long long)lc[threadIdx.x]);
        atomicAdd(&classes[0], (unsigned long long)lc[threadIdx.x]);
    }
}

// growth and merge: the old table's (or the source's) live slots through the same insert
__global__ __launch_bounds__(BLOCK) void k_link_rehash(const u64 *okeys, const u32 *ocnt, const unsigned long long *osum, u64 ocap, LinkView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ocap; i += (u64)gridDim.x * BLOCK)
        if (okeys[i] != SUP_EMPTY) link_add(t, okeys[i], ocnt[i], osum[i]);
}
__global__ __launch_bounds__(BLOCK) void k_link_add_list(const u32 *e1, const u32 *e2, const u32 *cnt, const u64 *sum, u64 n, LinkView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) link_add(t, ((u64)e1[i] << 32) | e2[i], cnt[i], sum[i]);
}
// would dst += src wrap a count?  src's keys are distinct, so one read-only lookup per key decides it before anything is written
__global__ __launch_bounds__(BLOCK) void k_link_check_merge(const u64 *skeys, const u32 *scnt, u64 scap, LinkView d, u32 *wraps) {
    bool w = false;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < scap; i += (u64)gridDim.x * BLOCK) {
        const u64 key = skeys[i];
        if (key == SUP_EMPTY) continue;
        const u64 at = link_find(d, key);
        const u32 a = at == ~0ull ? 0u : d.cnt[at], c = scnt[i];
        if (a + c < a) w = true;
    }
    if (w) *wraps = 1u;
}
__global__ __launch_bounds__(BLOCK) void k_link_total(const u64 *keys, const u32 *cnt, u64 cap, unsigned long long *total) {
    u64 s = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < cap; i += (u64)gridDim.x * BLOCK) if (keys[i] != SUP_EMPTY) s += cnt[i];
    for (int d = 32; d; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, (unsigned long long)s);
}

// ---- joins ---------------------------------------------------------------------------------------------------------------------
// pass 1, over the slots: a supported link counts at both its ends and leaves its slot at its first edge.  st: [0] links
// [1] supported.  Ids are below nid (gk_links::id_bound).
__global__ __launch_bounds__(BLOCK) void k_join_count(const u64 *__restrict__ keys, const u32 *__restrict__ cnt, u64 cap, u32 min_support, u32 *nsucc, u32 *npred,
                                                      u64 *succ_slot, unsigned long long *st) {
    u32 nl = 0, ns = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < cap; base += (u64)gridDim.x * BLOCK) {
        const u64 i = base + threadIdx.x;
        const u64 key = i < cap ? keys[i] : SUP_EMPTY;
        const bool live = key != SUP_EMPTY, sup = live && cnt[i] >= min_support;
        nl += (u32)__popcll(__ballot(live));
        ns += (u32)__popcll(__ballot(sup));
        if (sup) {
            const u32 e = (u32)(key >> 32), f = (u32)key;
            atomicAdd(&nsucc[e], 1u);
            atomicAdd(&npred[f], 1u);
            succ_slot[e] = i;                // (read only where nsucc[e] == 1: then this is the one store)
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(&st[0], (unsigned long long)nl);
        if (ns) atomicAdd(&st[1], (unsigned long long)ns);
    }
}
// pass 2, one lane per edge id: flag[e] = e's one supported link is the only one into its target.  st: [3] forks [4] merges.
__global__ __launch_bounds__(BLOCK) void k_join_flag(const u64 *__restrict__ keys, u64 nid, const u32 *__restrict__ nsucc, const u32 *__restrict__ npred,
                                                     const u64 *__restrict__ succ_slot, u32 *flag, unsigned long long *st) {
    u32 nf = 0, nm = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < nid; base += (u64)gridDim.x * BLOCK) {
        const u64 e = base + threadIdx.x;
        bool fork = false, merge = false;
        if (e < nid) {
            const u32 s = nsucc[e];
            fork = s >= 2;
            merge = npred[e] >= 2;
            flag[e] = s == 1 && npred[(u32)keys[succ_slot[e]]] == 1 ? 1u : 0u;
        }
        nf += (u32)__popcll(__ballot(fork));
        nm += (u32)__popcll(__ballot(merge));
    }
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(&st[3], (unsigned long long)nf);
        if (nm) atomicAdd(&st[4], (unsigned long long)nm);
    }
}
// the compaction in id order: join number at[e] of the scan is e's
__global__ __launch_bounds__(BLOCK) void k_join_emit(const u64 *__restrict__ keys, const u32 *__restrict__ cnt, const unsigned long long *__restrict__ sum, u64 nid,
                                                     const u32 *__restrict__ flag, const unsigned long long *__restrict__ at, const u64 *__restrict__ succ_slot,
                                                     u32 *e1, u32 *e2, u32 *count, u64 *sum_u) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < nid; e += (u64)gridDim.x * BLOCK) {
        if (!flag[e]) continue;
        const u64 s = succ_slot[e], j = at[e];
        e1[j] = (u32)e; e2[j] = (u32)keys[s]; count[j] = cnt[s]; sum_u[j] = sum[s];
    }
}

LinkView link_view(const gk_links *l) { return LinkView{l->d_keys, l->d_cnt, l->d_sum, l->cap - 1, l->d_ctr}; }

// room for `want` distinct links at load <= 0.5 (a power of two of slots); contents are kept
int links_reserve(gk_links *l, u64 want) {
    gk_ctx *ctx = l->ctx;
    const u64 need = pow2ceil(std::max<u64>(2 * want + 1024, 4096));
    if (l->cap >= need) return GK_OK;
    u64 *nk = nullptr;
    u32 *nc = nullptr;
    unsigned long long *ns = nullptr;
    hipError_t e = pool_malloc(ctx, &nk, need * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &nc, need * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &ns, need * 8);
    if (e == hipSuccess) e = hipMemsetAsync(nk, 0xff, need * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nc, 0, need * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ns, 0, need * 8, ctx->stream);
    if (e == hipSuccess && l->cap) {
        e = hipMemsetAsync(l->d_ctr, 0, 8, ctx->stream);                      // (the rehash counts the distinct links again)
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_link_rehash, dim3(ggrid(ctx, l->cap)), dim3(BLOCK), 0, ctx->stream, l->d_keys, l->d_cnt, l->d_sum, l->cap,
                               LinkView{nk, nc, ns, need - 1, l->d_ctr});
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) { (void)pool_free(ctx, nk); (void)pool_free(ctx, nc); (void)pool_free(ctx, ns); return hip_fail(ctx, e, "gk_links: table"); }
    (void)pool_free(ctx, l->d_keys); (void)pool_free(ctx, l->d_cnt); (void)pool_free(ctx, l->d_sum);
    l->d_keys = nk; l->d_cnt = nc; l->d_sum = ns; l->cap = need;
    return GK_OK;
}

// dst += src, refused before dst is written if a count would wrap; both on one context
int links_merge(gk_links *dst, const gk_links *src, const char *who) {
    gk_ctx *ctx = dst->ctx;
    const std::string w(who);
    unsigned long long hs = 0, hd = 0;
    GK_HIP(ctx, read_back(ctx, {{&hs, src->d_ctr, 8}, {&hd, dst->d_ctr, 8}}));
    if (!src->cap || !hs) return GK_OK;
    if (dst->cap && hd) {
        DevScratch tmp(ctx);
        u32 *d_wrap = nullptr, h_wrap = 0;
        GK_HIP(ctx, tmp.zeroed(&d_wrap, 1));
        hipLaunchKernelGGL(k_link_check_merge, dim3(ggrid(ctx, src->cap)), dim3(BLOCK), 0, ctx->stream, src->d_keys, src->d_cnt, src->cap, link_view(dst), d_wrap);
        GK_HIP(ctx, read_back(ctx, &h_wrap, d_wrap));
        if (h_wrap) return fail(ctx, GK_E_CAPACITY, w + ": a count would pass 2^32-1; nothing was added");
    }
    if (int rc = links_reserve(dst, hd + hs)) return rc;
    hipLaunchKernelGGL(k_link_rehash, dim3(ggrid(ctx, src->cap)), dim3(BLOCK), 0, ctx->stream, src->d_keys, src->d_cnt, src->d_sum, src->cap, link_view(dst));
    unsigned long long full = 0;
    GK_HIP(ctx, read_back(ctx, &full, dst->d_ctr + 3));
    if (full) return fail(ctx, GK_E_CAPACITY, w + ": the link table filled up (internal sizing error)");
    dst->id_bound = std::max(dst->id_bound, src->id_bound);
    return GK_OK;
}

// a call's own table (what it counts into before the merge), destroyed with the scope
using LocalLinks = std::unique_ptr<gk_links, void (*)(gk_links *)>;

// ---- the path key: a canonical edge numbering by content, for graphs whose edits made copies (gk_links.h) ------------------------
// The work is the pool's live WORDS, not its edges: word j of edge e (the 32 bases seq[32j .. 32j + 31], read from the edge's own
// first byte, so that where the pool put the edge does not matter) has the number woff[e] + j, woff the scan of the live edges'
// word counts.  That number space is cut into chunks of PK_CHUNK_WORDS = 64 words, one wave step each, whatever edge they fall in:
// an edge of a megabase is spread over the whole grid and 64 edges of one word share a step.  A step's lanes load 512 contiguous
// bytes (8 per lane), add their two terms per word, and the wave reduces them before anything leaves it: one 64-bit atomic add
// per sum and (edge, chunk).  Where all PK_STEPS chunks of a wave's trip lie in one edge — all but the trips at an edge's ends —
// they are summed in registers first and the trip costs one add, by __shfl_down; a trip that crosses edges finds every lane's
// edge by a search between the trip's first and last edge and reduces by SEGMENT (a Hillis-Steele scan that adds only across
// lanes of one edge; edges ascend with the lane), and the last lane of each segment adds.  No LDS: the sums live in registers and
// the only cross-lane traffic is the shuffles.  Cost: the pool's live bytes read once (8 B per word against three mix64, six
// 64-bit multiplies); the atomics are 16 B per 512 B read at worst; and, before a trip's first pool byte, one binary search of
// woff for the trip's first edge — about log2(n_edges) dependent loads, 20 on a graph of 10^6 edges, whose upper levels every wave
// shares in L2 — which is why a trip is PK_STEPS = 8 chunks (4 KiB) and not one.  The trip's last edge is searched FROM the first
// (doubling steps, then bisection): one load where the trip lies in one edge.  A wave's next trip lies a whole grid further on, so
// nothing carries over.  None of this has been timed yet (scripts/time_links_reduce.py reports the pass against a copy of the
// same bytes).
constexpr u32 PK_STEPS = 8;
// the largest e in [lo, hi] with woff[e] <= w: the edge that holds word w (dead edges hold none: woff[e] == woff[e + 1])
__device__ __forceinline__ u32 pk_edge_of(const unsigned long long *__restrict__ woff, u32 lo, u32 hi, u64 w) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (woff[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the same, searched upwards from lo (woff[lo] <= w): doubling steps, then bisection — O(log(answer - lo)) loads, one when the answer is lo
__device__ __forceinline__ u32 pk_edge_from(const unsigned long long *__restrict__ woff, u32 lo, u32 top, u64 w) {
    for (u32 step = 1; lo < top; step <<= 1) {
        const u32 nx = top - lo < step ? top : lo + step;
        if (woff[nx] > w) return pk_edge_of(woff, lo, nx - 1, w);
        lo = nx;
    }
    return lo;
}
// word j of an edge whose sequence starts at byte p: a whole word is one (unaligned) 8-byte load; the ragged last word is read byte
// by byte, only the bytes the edge owns, and the bases past its end are masked off
__device__ __forceinline__ u64 pk_load_word(const uint8_t *__restrict__ p, u64 j, u64 len) {
    const u64 rem = len - 32 * j;
    u64 w = 0;
    if (rem >= 32) { __builtin_memcpy(&w, p + 8 * j, 8); return w; }
    const u32 nb = (u32)(rem + 3) / 4;
    for (u32 b = 0; b < nb; b++) w |= (u64)p[8 * j + b] << (8 * b);
    return w & low_mask((int)(2 * rem));
}
__global__ __launch_bounds__(BLOCK) void k_pk_words(GraphView g, u32 *nw) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) nw[e] = g.e_alive[e] ? (u32)((g.e_len[e] + 31) / 32) : 0u;
}
__global__ __launch_bounds__(BLOCK) void k_pk_hash(GraphView g, const unsigned long long *__restrict__ woff, u64 nwords, unsigned long long *sums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u64 TRIP = (u64)PK_CHUNK_WORDS * PK_STEPS;
    const u64 stride = (u64)gridDim.x * (BLOCK / 64) * TRIP;
    const u32 ne = (u32)g.n_edges;
    for (u64 base = ((u64)blockIdx.x * (BLOCK / 64) + wave) * TRIP; base < nwords; base += stride) {      // (uniform over the wave)
        const u64 last = min(base + TRIP, nwords) - 1;
        const u32 e_lo = pk_edge_of(woff, 0, ne - 1, base), e_hi = pk_edge_from(woff, e_lo, ne - 1, last);
        if (e_lo == e_hi) {
            const u64 w0 = woff[e_lo], len = g.e_len[e_lo];
            const uint8_t *p = g.pool + g.e_off[e_lo];
            u64 a1 = 0, a2 = 0;
#pragma unroll
            for (u32 s = 0; s < PK_STEPS; s++) {
                const u64 w = base + s * PK_CHUNK_WORDS + lane;
                if (w > last) continue;
                u64 t1, t2;
                pk_word_terms(pk_load_word(p, w - w0, len), w - w0, &t1, &t2);
                a1 += t1; a2 += t2;
            }
            for (int d = 32; d; d >>= 1) { a1 += __shfl_down(a1, d); a2 += __shfl_down(a2, d); }
            if (lane == 0) { atomicAdd(&sums[2 * (u64)e_lo], (unsigned long long)a1); atomicAdd(&sums[2 * (u64)e_lo + 1], (unsigned long long)a2); }
            continue;
        }
        for (u32 s = 0; s < PK_STEPS; s++) {
            const u64 w = base + s * PK_CHUNK_WORDS + lane;
            const bool in = w <= last;
            u32 e = NONE;
            u64 t1 = 0, t2 = 0;
            if (in) {
                e = pk_edge_of(woff, e_lo, e_hi, w);
                const u64 j = w - woff[e];
                pk_word_terms(pk_load_word(g.pool + g.e_off[e], j, g.e_len[e]), j, &t1, &t2);
            }
            for (int d = 1; d < 64; d <<= 1) {
                const u64 u1 = __shfl_up(t1, d), u2 = __shfl_up(t2, d);
                const u32 ue = __shfl_up(e, d);
                if (lane >= d && ue == e) { t1 += u1; t2 += u2; }
            }
            const u32 next = __shfl_down(e, 1);
            if (in && (lane == 63 || next != e)) { atomicAdd(&sums[2 * (u64)e], (unsigned long long)t1); atomicAdd(&sums[2 * (u64)e + 1], (unsigned long long)t2); }
        }
    }
}
// h1[e], h2[e] = the key (~0, ~0 dead), ids[e] = e; out[0] += live edges, out[1] += the fingerprint's term of every live edge
__global__ __launch_bounds__(BLOCK) void k_pk_keys(GraphView g, const unsigned long long *__restrict__ sums, u64 *h1, u64 *h2, u32 *ids, unsigned long long *out) {
    u64 live = 0, fp = 0;
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        ids[e] = (u32)e;
        if (!g.e_alive[e]) { h1[e] = h2[e] = ~0ull; continue; }
        const u32 s = g.e_start[e];
        u64 a, b;
        pk_finish(sums[2 * e], sums[2 * e + 1], g.node_lo[s], g.node_hi[s], g.e_len[e], &a, &b);
        h1[e] = a; h2[e] = b;
        live++;
        fp += mix64(a ^ mix64(b + PK_FP));
    }
    for (int d = 32; d; d >>= 1) { live += __shfl_down(live, d); fp += __shfl_down(fp, d); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], (unsigned long long)live); atomicAdd(&out[1], (unsigned long long)fp); }
}
__global__ __launch_bounds__(BLOCK) void k_pk_gather(const u64 *__restrict__ h1, const u32 *__restrict__ ids, u64 n, u64 *out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) out[i] = h1[ids[i]];
}
// after the sorts (by h2, then stably by h1): canon[local id] = rank, inv[rank] = local id; an edge whose neighbour in the order
// has its key is a duplicate
__global__ __launch_bounds__(BLOCK) void k_pk_canon(const u64 *__restrict__ sk1, const u32 *__restrict__ sid, const u64 *__restrict__ h2, u64 nlive, u32 *canon,
                                                    u32 *inv, uint8_t *dup) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nlive; i += (u64)gridDim.x * BLOCK) {
        const u32 id = sid[i];
        canon[id] = (u32)i;
        inv[i] = id;
        const bool before = i && sk1[i - 1] == sk1[i] && h2[sid[i - 1]] == h2[id], after = i + 1 < nlive && sk1[i + 1] == sk1[i] && h2[sid[i + 1]] == h2[id];
        dup[id] = before || after ? 1 : 0;
    }
}

// ---- the link table's records as planes (gk_links.h) -----------------------------------------------------------------------------
struct LinkSrc {
    const u64 *keys; const u32 *cnt; const unsigned long long *sum; u64 cap;
    __device__ __forceinline__ bool get(u64 i, const RecCanon &c, u64 *key, u32 *n, u64 *x) const {
        const u64 k = keys[i];
        if (k == SUP_EMPTY) return false;
        const u32 a = rec_canon_id(c, (u32)(k >> 32)), b = rec_canon_id(c, (u32)k);
        if (a == NONE || b == NONE) return false;
        *key = ((u64)a << 32) | b; *n = cnt[i]; *x = sum[i];
        return true;
    }
};
__global__ __launch_bounds__(BLOCK) void k_link_add_planes(RecPlanes p, u64 n, LinkView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) link_add(t, p.key[i], p.cnt[i], p.x[i]);
}

}  // namespace

namespace gk {
int graph_edge_pathkeys(gk_graph *g, DevScratch &keep, u32 **d_canon, u32 **d_inv, uint8_t **d_dup, u64 *nlive, u64 *content_fp, u64 **d_h1, u64 **d_h2) {
    gk_ctx *ctx = g->ctx;
    *d_canon = *d_inv = nullptr; *d_dup = nullptr;
    *nlive = 0; *content_fp = 0;
    const u64 ne = g->v.n_edges;
    if (ne >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "graph_edge_pathkeys: more than 2^32 - 1 edge ids");
    DevScratch tmp(ctx);
    u32 *d_nw = nullptr, *d_id = nullptr, *d_id2 = nullptr, *d_id3 = nullptr;
    u64 *h1 = nullptr, *h2 = nullptr, *d_k = nullptr, *d_k2 = nullptr;
    unsigned long long *d_woff = nullptr, *d_sums = nullptr, *d_out = nullptr, h_out[2] = {0, 0}, h_words = 0;
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
    u32 *canon = nullptr, *inv = nullptr;
    uint8_t *dup = nullptr;
    keep.get(&h1, ne);
    keep.get(&h2, ne);
    keep.get(&canon, ne);
    keep.zeroed(&dup, ne);
    if (canon) keep.note(hipMemsetAsync(canon, 0xff, std::max<u64>(ne, 1) * 4, ctx->stream));
    if (keep.error() != hipSuccess) return hip_fail(ctx, keep.error(), "graph_edge_pathkeys: maps");
    tmp.get(&d_nw, ne);
    tmp.get(&d_woff, ne + 1);
    tmp.zeroed(&d_sums, 2 * ne);
    tmp.get(&d_id, ne); tmp.get(&d_id2, ne); tmp.get(&d_id3, ne);
    tmp.get(&d_k, ne); tmp.get(&d_k2, ne);
    tmp.zeroed(&d_out, 2);
    if (ne) tmp.note(rocprim::radix_sort_pairs(nullptr, temp_bytes, d_k, d_k2, d_id, d_id2, (size_t)ne, 0, 64, ctx->stream));   // (the size query)
    tmp.get((uint8_t **)&d_temp, temp_bytes);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "graph_edge_pathkeys: scratch");
    if (ne) {
        hipLaunchKernelGGL(k_pk_words, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, g->v, d_nw);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, tmp, d_nw, ne, d_woff));
        GK_HIP(ctx, read_back(ctx, &h_words, d_woff + ne));
        if (h_words) {
            constexpr u64 per_wg = (u64)PK_CHUNK_WORDS * PK_STEPS * (BLOCK / 64);
            const u64 grid = std::min<u64>((h_words + per_wg - 1) / per_wg, grid_cap(ctx));
            hipLaunchKernelGGL(k_pk_hash, dim3((unsigned)grid), dim3(BLOCK), 0, ctx->stream, g->v, d_woff, (u64)h_words, d_sums);
        }
        hipLaunchKernelGGL(k_pk_keys, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, g->v, d_sums, h1, h2, d_id, d_out);
        GK_HIP(ctx, hipGetLastError());
        // by (h1, h2): the radix sort is stable, so the minor key goes first
        GK_HIP(ctx, hipMemcpyAsync(d_k, h2, ne * 8, hipMemcpyDeviceToDevice, ctx->stream));
        GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, temp_bytes, d_k, d_k2, d_id, d_id2, (size_t)ne, 0, 64, ctx->stream));
        hipLaunchKernelGGL(k_pk_gather, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, h1, d_id2, ne, d_k);
        GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, temp_bytes, d_k, d_k2, d_id2, d_id3, (size_t)ne, 0, 64, ctx->stream));
    }
    GK_HIP(ctx, read_back(ctx, h_out, d_out, 2));
    keep.get(&inv, h_out[0]);
    if (keep.error() != hipSuccess) return hip_fail(ctx, keep.error(), "graph_edge_pathkeys: maps");
    if (h_out[0]) hipLaunchKernelGGL(k_pk_canon, dim3(ggrid(ctx, h_out[0])), dim3(BLOCK), 0, ctx->stream, d_k2, d_id3, h2, (u64)h_out[0], canon, inv, dup);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // (the scratch goes with this scope)
    *d_canon = canon; *d_inv = inv; *d_dup = dup;
    if (d_h1) *d_h1 = h1;
    if (d_h2) *d_h2 = h2;
    *nlive = h_out[0];
    *content_fp = h_out[1] + mix64(h_out[0] ^ PK_LIVE);
    return GK_OK;
}

template <> gk_ctx *rec_ctx<gk_links>(const gk_links *l) { return l->ctx; }
template <> int rec_distinct<gk_links>(const gk_links *l, u64 *n) {
    unsigned long long h = 0;
    GK_HIP(l->ctx, read_back(l->ctx, &h, l->d_ctr));
    *n = h;
    return GK_OK;
}
template <> int rec_bucket<gk_links>(gk_links *l, int P, const RecPlanes &out, u64 room, u64 *region, const u32 *canon, const uint8_t *dup, u64 nmap) {
    return records_bucket(l->ctx, LinkSrc{l->d_keys, l->d_cnt, l->d_sum, l->cap}, P, out, room, region, canon, dup, nmap, "the links");
}
template <> int rec_insert<gk_links>(gk_links *l, const RecPlanes &in, u64 n, bool *overflow) {
    gk_ctx *ctx = l->ctx;
    *overflow = false;
    if (n == 0) return GK_OK;
    u64 have = 0;
    if (int rc = rec_distinct(l, &have)) return rc;
    if (int rc = links_reserve(l, have + n)) return rc;
    hipLaunchKernelGGL(k_link_add_planes, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, in, n, link_view(l));
    unsigned long long f[2] = {0, 0};                          // [3] table full, [4] a count wrapped
    GK_HIP(ctx, read_back(ctx, f, l->d_ctr + 3, 2));
    if (f[0]) return fail(ctx, GK_E_CAPACITY, "the link table filled up (internal sizing error)");
    *overflow = f[1] != 0;
    return GK_OK;
}
template <> int rec_uncanon<gk_links>(gk_ctx *ctx, const RecPlanes &p, u64 n, const u32 *d_inv, u64 nlive) { return records_uncanon(ctx, p, n, false, d_inv, nlive); }
template <> int rec_new<gk_links>(gk_ctx *ctx, u64 want, u64 id_bound, gk_links **out) {
    if (int rc = gk_links_create(ctx, out)) return rc;
    (*out)->id_bound = id_bound;
    return links_reserve(*out, want);
}
template <> void rec_free<gk_links>(gk_links *l) { gk_links_destroy(l); }
template <> int rec_adopt<gk_links>(gk_links *s, gk_links *t) {
    GK_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));
    std::swap(s->d_keys, t->d_keys); std::swap(s->d_cnt, t->d_cnt); std::swap(s->d_sum, t->d_sum); std::swap(s->cap, t->cap); std::swap(s->d_ctr, t->d_ctr);
    s->id_bound = std::max(s->id_bound, t->id_bound);
    return GK_OK;
}
}  // namespace gk

extern "C" {

int gk_links_create(gk_ctx *ctx, gk_links **out) {
    if (!ctx || !out) return fail(ctx, GK_E_INVALID, "gk_links_create: null argument");
    *out = nullptr;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    gk_links *l = new gk_links();
    l->ctx = ctx;
    hipError_t e = pool_malloc(ctx, &l->d_ctr, 64);
    if (e == hipSuccess) e = hipMemsetAsync(l->d_ctr, 0, 64, ctx->stream);
    if (e != hipSuccess) { (void)pool_free(ctx, l->d_ctr); delete l; return hip_fail(ctx, e, "gk_links_create"); }
    *out = l;
    return GK_OK;
}

void gk_links_destroy(gk_links *l) {
    if (!l) return;
    gk_ctx *ctx = l->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)pool_free(ctx, l->d_keys);
    (void)pool_free(ctx, l->d_cnt);
    (void)pool_free(ctx, l->d_sum);
    (void)pool_free(ctx, l->d_ctr);
    delete l;
}

int gk_graph_pair_links(gk_graph *g, gk_vmap *positions, gk_links *links, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint64_t min_len,
                        uint64_t max_span, uint64_t *classes8) {
    if (classes8) for (int c = 0; c < 8; c++) classes8[c] = 0;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    const char *who = "gk_graph_pair_links";
    if (!positions || !links || !classes8 || (!bin && nbytes)) return fail(ctx, GK_E_INVALID, std::string(who) + ": null argument");
    if (vmap_ctx(positions) != ctx || links->ctx != ctx) return fail(ctx, GK_E_INVALID, std::string(who) + ": the position map and the links must live on the graph's context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, std::string(who) + ": the position map has another k");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    DevScratch tmp(ctx);
    PairFront F;
    if (int rc = pairs_front(g, positions, bin, nbytes, npairs, who, tmp, F)) return rc;
    if (F.nq == 0) return GK_OK;
    if (int rc = pairs_front_checked(ctx, F, who)) return rc;         // the kernel reads e_len by the positions' edge ids
    const u64 norient = F.nq / 2;
    // The call's own table: an orientation inserts at most one key, so `norient` distinct links at load <= 0.5 always hold the
    // batch.  That is 40 bytes per orientation beside the 80 and more the front end's keys and CSR already took, so a batch the
    // front end could hold is never too much for it: no sub-batches.
    gk_links *local = nullptr;
    if (int rc = gk_links_create(ctx, &local)) return rc;
    LocalLinks own(local, gk_links_destroy);
    if (int rc = links_reserve(local, norient)) return rc;
    local->id_bound = g->v.n_edges;
    unsigned long long *d_cls = nullptr, h_cls[8] = {}, h_ctr[5] = {};
    GK_HIP(ctx, tmp.zeroed(&d_cls, 8));
    hipLaunchKernelGGL(k_pair_links, dim3(ggrid(ctx, norient)), dim3(BLOCK), 0, ctx->stream, g->v, F.d_off, F.d_vals, norient, (u64)g->k, (u64)min_len,
                       (u64)max_span, link_view(local), d_cls);
    GK_HIP(ctx, read_back(ctx, {{h_cls, d_cls, sizeof(h_cls)}, {h_ctr, local->d_ctr, sizeof(h_ctr)}}));
    if (h_ctr[3]) return fail(ctx, GK_E_CAPACITY, std::string(who) + ": the link table filled up (internal sizing error)");
    if (h_ctr[4]) return fail(ctx, GK_E_CAPACITY, std::string(who) + ": a count would pass 2^32-1; nothing was added");
    if (int rc = links_merge(links, local, who)) return rc;
    for (int c = 0; c < 8; c++) classes8[c] = h_cls[c];
    return GK_OK;
}

int gk_links_size(const gk_links *l, uint64_t *links, uint64_t *observations) {
    if (!l) return fail(nullptr, GK_E_INVALID, "null links handle");
    gk_ctx *ctx = l->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    DevScratch tmp(ctx);
    unsigned long long *d_total = nullptr, h_total = 0, h_links = 0;
    GK_HIP(ctx, tmp.zeroed(&d_total, 1));
    if (l->cap) hipLaunchKernelGGL(k_link_total, dim3(ggrid(ctx, l->cap)), dim3(BLOCK), 0, ctx->stream, l->d_keys, l->d_cnt, l->cap, d_total);
    GK_HIP(ctx, read_back(ctx, {{&h_total, d_total, 8}, {&h_links, l->d_ctr, 8}}));
    if (links) *links = h_links;
    if (observations) *observations = h_total;
    return GK_OK;
}

int gk_links_export(const gk_links *l, uint32_t *e1, uint32_t *e2, uint32_t *count, uint64_t *sum_u, uint64_t cap, uint64_t *n) {
    if (!l) return fail(nullptr, GK_E_INVALID, "null links handle");
    gk_ctx *ctx = l->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<u64> k(l->cap);
    std::vector<u32> c(l->cap);
    std::vector<unsigned long long> s(l->cap);
    if (l->cap) GK_HIP(ctx, read_back(ctx, {{k.data(), l->d_keys, l->cap * 8}, {c.data(), l->d_cnt, l->cap * 4}, {s.data(), l->d_sum, l->cap * 8}}));
    u64 live = 0;
    for (u64 i = 0; i < l->cap; i++) live += k[i] != SUP_EMPTY;
    if (n) *n = live;
    if (live > cap) return fail(ctx, GK_E_CAPACITY, "gk_links_export: need room for " + std::to_string(live) + " links");
    if (live && (!e1 || !e2 || !count || !sum_u)) return fail(ctx, GK_E_INVALID, "gk_links_export: null argument");
    u64 j = 0;
    for (u64 i = 0; i < l->cap; i++)
        if (k[i] != SUP_EMPTY) { e1[j] = (u32)(k[i] >> 32); e2[j] = (u32)k[i]; count[j] = c[i]; sum_u[j] = s[i]; j++; }
    return GK_OK;
}

int gk_links_add(gk_links *l, const uint32_t *e1, const uint32_t *e2, const uint32_t *count, const uint64_t *sum_u, uint64_t n) {
    if (!l) return fail(nullptr, GK_E_INVALID, "null links handle");
    gk_ctx *ctx = l->ctx;
    if (n == 0) return GK_OK;
    if (!e1 || !e2 || !count || !sum_u) return fail(ctx, GK_E_INVALID, "gk_links_add: null argument");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    // the list goes into a table of its own (duplicates add up there, checked), which is then merged: l is only written once
    // nothing can wrap
    gk_links *t = nullptr;
    if (int rc = gk_links_create(ctx, &t)) return rc;
    LocalLinks own(t, gk_links_destroy);
    if (int rc = links_reserve(t, n)) return rc;
    for (u64 i = 0; i < n; i++) {
        if (e1[i] == NONE || e2[i] == NONE) return fail(ctx, GK_E_INVALID, "gk_links_add: 0xffffffff is not an edge id");
        t->id_bound = std::max<u64>(t->id_bound, (u64)std::max(e1[i], e2[i]) + 1);
    }
    DevScratch tmp(ctx);
    u32 *d_e1 = nullptr, *d_e2 = nullptr, *d_c = nullptr;
    u64 *d_s = nullptr;
    tmp.upload(&d_e1, e1, n);
    tmp.upload(&d_e2, e2, n);
    tmp.upload(&d_c, count, n);
    tmp.upload(&d_s, sum_u, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_links_add: upload");
    hipLaunchKernelGGL(k_link_add_list, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, d_e1, d_e2, d_c, d_s, (u64)n, link_view(t));
    unsigned long long f[2] = {0, 0};                          // [3] table full, [4] a count wrapped
    GK_HIP(ctx, read_back(ctx, f, t->d_ctr + 3, 2));
    if (f[0]) return fail(ctx, GK_E_CAPACITY, "gk_links_add: the link table filled up (internal sizing error)");
    if (f[1]) return fail(ctx, GK_E_CAPACITY, "gk_links_add: a count of the list would pass 2^32-1; nothing was added");
    return links_merge(l, t, "gk_links_add");
}

int gk_links_joins(const gk_links *l, uint32_t min_support, uint32_t *e1, uint32_t *e2, uint32_t *count, uint64_t *sum_u, uint64_t cap, uint64_t *n,
                   uint64_t *stats5) {
    if (n) *n = 0;
    if (stats5) for (int i = 0; i < 5; i++) stats5[i] = 0;
    if (!l) return fail(nullptr, GK_E_INVALID, "null links handle");
    gk_ctx *ctx = l->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nid = l->id_bound;
    if (!l->cap || !nid) return GK_OK;
    DevScratch tmp(ctx);
    u32 *d_nsucc = nullptr, *d_npred = nullptr, *d_flag = nullptr;
    u64 *d_slot = nullptr;
    unsigned long long *d_at = nullptr, *d_st = nullptr, h_st[5] = {}, h_joins = 0;
    tmp.zeroed(&d_nsucc, nid);
    tmp.zeroed(&d_npred, nid);
    tmp.get(&d_slot, nid);
    tmp.get(&d_flag, nid);
    tmp.get(&d_at, nid + 1);
    tmp.zeroed(&d_st, 5);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_links_joins: scratch");
    hipLaunchKernelGGL(k_join_count, dim3(ggrid(ctx, l->cap)), dim3(BLOCK), 0, ctx->stream, l->d_keys, l->d_cnt, l->cap, min_support, d_nsucc, d_npred, d_slot, d_st);
    hipLaunchKernelGGL(k_join_flag, dim3(ggrid(ctx, nid)), dim3(BLOCK), 0, ctx->stream, l->d_keys, nid, d_nsucc, d_npred, d_slot, d_flag, d_st);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_flag, nid, d_at));
    GK_HIP(ctx, read_back(ctx, {{h_st, d_st, sizeof(h_st)}, {&h_joins, d_at + nid, 8}}));
    h_st[2] = h_joins;
    if (stats5) for (int i = 0; i < 5; i++) stats5[i] = h_st[i];
    if (n) *n = h_joins;
    if (h_joins > cap) return fail(ctx, GK_E_CAPACITY, "gk_links_joins: need room for " + std::to_string(h_joins) + " joins");
    if (h_joins == 0) return GK_OK;
    if (!e1 || !e2 || !count || !sum_u) return fail(ctx, GK_E_INVALID, "gk_links_joins: null argument");
    u32 *d_e1 = nullptr, *d_e2 = nullptr, *d_c = nullptr;
    u64 *d_s = nullptr;
    tmp.get(&d_e1, h_joins);
    tmp.get(&d_e2, h_joins);
    tmp.get(&d_c, h_joins);
    tmp.get(&d_s, h_joins);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_links_joins: output");
    hipLaunchKernelGGL(k_join_emit, dim3(ggrid(ctx, nid)), dim3(BLOCK), 0, ctx->stream, l->d_keys, l->d_cnt, l->d_sum, nid, d_flag, d_at, d_slot, d_e1, d_e2, d_c, d_s);
    GK_HIP(ctx, read_back(ctx, {{e1, d_e1, (size_t)h_joins * 4}, {e2, d_e2, (size_t)h_joins * 4}, {count, d_c, (size_t)h_joins * 4}, {sum_u, d_s, (size_t)h_joins * 8}}));
    return GK_OK;
}

// Pure host code: no context, no device.
int gk_scaffold_chains(const uint32_t *e1, const uint32_t *e2, uint64_t n, uint32_t *members, uint64_t members_cap, uint64_t *chain_off, uint64_t chains_cap,
                       uint64_t *nchains, uint64_t *ncycles) {
    if (nchains) *nchains = 0;
    if (ncycles) *ncycles = 0;
    if (n && (!e1 || !e2)) return fail(nullptr, GK_E_INVALID, "gk_scaffold_chains: null argument");
    std::unordered_map<u32, u32> succ;
    std::unordered_set<u32> has_pred;
    succ.reserve(n); has_pred.reserve(n);
    for (u64 i = 0; i < n; i++)
        if (!succ.emplace(e1[i], e2[i]).second || !has_pred.insert(e2[i]).second)
            return fail(nullptr, GK_E_INVALID, "gk_scaffold_chains: an edge id occurs twice as e1 or twice as e2 (not a join list)");
    std::vector<u32> order(e1, e1 + n);
    std::sort(order.begin(), order.end());
    std::vector<std::vector<u32>> chains;
    std::unordered_set<u32> seen;
    seen.reserve(2 * n);
    u64 cycles = 0, total = 0;
    for (int pass = 0; pass < 2; pass++)                      // the paths from their heads; what is left lies on cycles, each from its smallest id
        for (const u32 head : order) {
            if (pass == 0 ? has_pred.count(head) != 0 : seen.count(head) != 0) continue;
            std::vector<u32> c{head};
            for (auto it = succ.find(head); it != succ.end() && it->second != head; it = succ.find(it->second)) c.push_back(it->second);
            seen.insert(c.begin(), c.end());
            total += c.size();
            cycles += pass;
            chains.push_back(std::move(c));
        }
    std::sort(chains.begin(), chains.end(), [](const std::vector<u32> &a, const std::vector<u32> &b) { return a[0] < b[0]; });
    if (nchains) *nchains = chains.size();
    if (ncycles) *ncycles = cycles;
    if (chains.size() > chains_cap || total > members_cap)
        return fail(nullptr, GK_E_CAPACITY, "gk_scaffold_chains: need room for " + std::to_string(chains.size()) + " chains of " + std::to_string(total) + " members");
    if (!chain_off || (total && !members)) return fail(nullptr, GK_E_INVALID, "gk_scaffold_chains: null argument");
    u64 at = 0;
    for (size_t i = 0; i < chains.size(); i++) {
        chain_off[i] = at;
        for (const u32 e : chains[i]) members[at++] = e;
    }
    chain_off[chains.size()] = at;
    return GK_OK;
}

}  // extern "C"
