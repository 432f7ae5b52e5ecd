// gk_cycles.hip — perfect cycles kept (include/genome_amd.h, "perfect cycles"): what the reference drops at Graph.scala:375 and
// :220-221.  Nothing here knows what a table slot is: gk_graph.hip finds the members of the k-mer table's all-(1,1) cycles and
// hands them over dense (CycleMembers); gk_graph_ops.hip calls cycles_keep_classes between k_node_class and k_chain.
//
//   cycles_min            the minimum over each cycle of a functional graph, by pointer doubling (k_cy_round)
//   graph_append_cycles   k-mer level: anchors -> nodes, one arc per anchor -> edges, appended to a built graph
//   cycles_keep_classes   node level: self-loop nodes stay, the anchors of all-interior cycles become kept nodes
//
// All kernels are integer, grid-stride, latency bound (one random 8-byte read per element and round, two key reads when both
// candidates are alive); no LDS beyond block_reserve's, no MFMA.
#include <algorithm>
#include <string>

#include "gk_graph.h"
#include "gk_scan.h"

// ---- the minimum over each cycle ------------------------------------------------------------------------------------------------
// One 64-bit word per element: pointer | argmin << 32.  The invariant of a word of u that is neither CY_UNREG nor a fixed point:
// its pointer is succ^c(u) for some c >= 1 and its argmin is the first smallest key among succ^0(u) .. succ^(c-1)(u) — or
// CY_LEAVES when one of those has its successor outside the set.  A round reads the word of the pointer's target and writes its
// own: (target's pointer, min of the two argmins).  The pair travels in ONE word, read and written by single 8-byte accesses, so
// whichever version of the target's word a lane meets — this round's or the last one's — satisfies the invariant, and the two
// ranges are adjacent: the new word satisfies it too.  That is why the round is in place.  (Two words, pointer and minimum, read
// one after the other could pair a new pointer with an old minimum and skip the elements between them.)  A word's range never
// shrinks, so after round r it spans at least 2^r elements or has met the end of its chain; ceil(log2 n) rounds cover every
// cycle of a set of n.  Nothing stops moving on a cycle: the round count comes from n, not from a flag.
__device__ __forceinline__ bool cy_less(const u64 *__restrict__ klo, const u64 *__restrict__ khi, u32 a, u32 b) {
    if (khi) { const u64 ha = khi[a], hb = khi[b]; if (ha != hb) return ha < hb; }
    return klo[a] < klo[b];
}
__device__ __forceinline__ bool cy_same(const u64 *__restrict__ klo, const u64 *__restrict__ khi, u32 a, u32 b) {
    return klo[a] == klo[b] && (!khi || khi[a] == khi[b]);
}
// the single 8-byte accesses the argument above rests on, said in the source
__device__ __forceinline__ u64 cy_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cy_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ __launch_bounds__(BLOCK) void k_cy_round(u64 *st, u64 n, const u64 *__restrict__ klo, const u64 *__restrict__ khi, u32 *err) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < n; u += (u64)gridDim.x * BLOCK) {
        const u64 su = cy_load(&st[u]);
        if (su == CY_UNREG) continue;
        const u32 v = (u32)su, amu = (u32)(su >> 32);
        if ((u64)v == u || amu == CY_LEAVES) continue;      // a fixed point (the end of a chain, a cycle of one), or known to leave
        if ((u64)v >= n) { *err = 1; continue; }
        const u64 sv = cy_load(&st[v]);
        if (sv == CY_UNREG) { *err = 2; continue; }         // a candidate's successor is a candidate or a fixed point
        const u32 amv = (u32)(sv >> 32);
        u32 am = CY_LEAVES;
        if (amv != CY_LEAVES) {
            if (amv >= n) { *err = 1; continue; }
            am = cy_less(klo, khi, amv, amu) ? amv : amu;
        }
        cy_store(&st[u], ((u64)am << 32) | (u64)(u32)sv);
    }
}
int cycles_min(gk_ctx *ctx, DevScratch &tmp, u64 *st, u64 n, const u64 *klo, const u64 *khi, u64 *rounds) {
    u32 *d_err = nullptr, h_err = 0;
    tmp.zeroed(&d_err, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "perfect cycles: alloc");
    u64 R = 0;
    while ((1ull << R) < n) R++;
    for (u64 r = 0; r < R; r++) hipLaunchKernelGGL(k_cy_round, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, st, n, klo, khi, d_err);
    const hipError_t e = read_back(ctx, &h_err, d_err);
    if (e != hipSuccess) return hip_fail(ctx, e, "perfect cycles: doubling rounds");
    if (h_err) return fail(ctx, GK_E_STATE, "perfect cycles: the successor map is not closed (code " + std::to_string(h_err) + ")");
    if (rounds) *rounds = R;
    return GK_OK;
}

// ---- k-mer level: anchors and arcs appended to a built graph ----------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_cya_init(u64 *st, const u32 *__restrict__ succ, u32 *pred, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        st[i] = (u64)succ[i] | (i << 32);
        pred[succ[i]] = (u32)i;                             // (succ is a permutation of 0..n-1: checked where it was made)
    }
}
// af: the member is an anchor (its own key is its cycle's minimum); pf: ... and the k-mer IS its anchor key, so it names a node pair
__global__ __launch_bounds__(BLOCK) void k_cya_flags(const u64 *__restrict__ st, const u64 *__restrict__ klo, const u64 *__restrict__ khi,
                                                     const uint8_t *__restrict__ meta, u32 *af, u32 *pf, u64 *dist, const u32 *__restrict__ pred, u64 n, u32 *err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 am = (u32)(st[i] >> 32);
        bool a = false;
        if (am == CY_LEAVES || am >= n) *err = 3;           // every member lies on a cycle
        else a = cy_same(klo, khi, (u32)i, am);
        af[i] = a ? 1u : 0u;
        pf[i] = a && !(meta[i] & 4u) ? 1u : 0u;
        dist[i] = (u64)pred[i] | (1ull << 32);              // the way BACK: pointer | steps << 32
    }
}
// distance to the previous anchor, absorbing: a pointer that stands on an anchor stays.  One word per member, in place, by the
// argument above ("my pointer is d steps behind me" holds for the old word and the new one).  d <= the cycle's length < 2^31.
__global__ __launch_bounds__(BLOCK) void k_cya_dist_round(u64 *dist, const u32 *__restrict__ af, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 su = cy_load(&dist[i]);
        const u32 t = (u32)su;
        if (af[t]) continue;
        const u64 sv = cy_load(&dist[t]);
        cy_store(&dist[i], (u64)(u32)sv | (((su >> 32) + (sv >> 32)) << 32));
    }
}
// every anchor: its node (and the dead partner of a palindrome), its out-edge's stub, and — as the END of the arc that comes in —
// the previous anchor's edge length and end.  cnt: [0] anchors whose previous anchor is another one, [1] palindromic anchors,
// [2] the longest cycle
template <int W>
__global__ __launch_bounds__(BLOCK) void k_cya_nodes(GraphView g, int k, CycleMembers cm, const u32 *__restrict__ af, const unsigned long long *__restrict__ aoff,
                                                     const unsigned long long *__restrict__ poff, const u64 *__restrict__ dist, u64 N0, u64 E0,
                                                     unsigned long long *cnt, u32 *err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < cm.n; i += (u64)gridDim.x * BLOCK) {
        if (!af[i]) continue;
        const u32 meta = cm.meta[i];
        const bool isrc = meta & 4u, pal = meta & 8u;
        const int nb = (int)(meta & 3u);
        Kmer<W> x;
        if constexpr (W == 1) x = Kmer<1>{cm.klo[i]}; else x = Kmer<2>{cm.klo[i], cm.khi[i]};
        if (isrc) x = revcomp(x, k);
        const u32 tw = cm.twin[i];
        if (isrc && (tw >= cm.n || !af[tw] || (cm.meta[tw] & 4u))) { *err = 4; continue; }      // the twin of an anchor is an anchor
        const u64 nd = isrc ? N0 + 2 * poff[tw] + 1 : N0 + 2 * poff[i];
        const u64 e = E0 + aoff[i];
        if (nd >= g.n_nodes || e >= g.n_edges) { *err = 5; continue; }
        g.node_lo[nd] = x.lo;
        if constexpr (W == 2) g.node_hi[nd] = x.hi; else g.node_hi[nd] = 0;
        g.node_alive[nd] = 1;
        for (int b = 0; b < 4; b++) g.out_edge[nd * 4 + b] = b == nb ? (u32)e : NONE;
        g.out_order[nd] = order_append(0u, nb);
        g.in_deg[nd] = 1;
        if (pal) {                                          // one node, not two: the odd id of the pair stays dead (as k_make_nodes)
            g.node_lo[nd + 1] = x.lo;
            if constexpr (W == 2) g.node_hi[nd + 1] = x.hi; else g.node_hi[nd + 1] = 0;
            g.node_alive[nd + 1] = 0;
            for (int b = 0; b < 4; b++) g.out_edge[(nd + 1) * 4 + b] = NONE;
            g.out_order[nd + 1] = 0;
            g.in_deg[nd + 1] = 0;
            atomicAdd(&cnt[1], 1ull);
        }
        g.e_start[e] = (u32)nd;
        g.e_first[e] = (uint8_t)nb;
        g.e_alive[e] = 1;
        const u32 pa = (u32)dist[i];
        const u64 d = dist[i] >> 32;
        if (pa >= cm.n || !af[pa]) { *err = 6; continue; }
        const u64 ep = E0 + aoff[pa];
        g.e_len[ep] = d;
        g.e_end[ep] = (u32)nd;
        u64 L = d;
        if (pa != (u32)i) { L += dist[pa] >> 32; atomicAdd(&cnt[0], 1ull); }
        atomicMax(&cnt[2], (unsigned long long)L);
    }
}
// every member places the base that follows it: position 0 of its own arc for an anchor, position d of the previous anchor's arc
// for a member d steps behind it — no lane walks
__global__ __launch_bounds__(BLOCK) void k_cya_emit(GraphView g, const uint8_t *__restrict__ meta, const u32 *__restrict__ af,
                                                    const unsigned long long *__restrict__ aoff, const u64 *__restrict__ dist, u64 E0, u64 n, u64 pool_cap, u32 *err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 a = af[i] ? (u32)i : (u32)dist[i];
        const u64 pos = af[i] ? 0ull : dist[i] >> 32;
        if (a >= n || !af[a]) { *err = 7; continue; }
        const u64 e = E0 + aoff[a];
        if (e >= g.n_edges || pos >= g.e_len[e]) { *err = 8; continue; }
        const u64 byte = g.e_off[e] + (pos >> 2);
        if ((byte | 3ull) >= pool_cap) { *err = 9; continue; }
        atomicOr(reinterpret_cast<u32 *>(g.pool) + (byte >> 2), (u32)(meta[i] & 3u) << (((byte & 3) * 8) + (pos & 3) * 2));
    }
}

int graph_append_cycles(gk_graph *g, DevScratch &tmp, const CycleMembers &cm, uint64_t *stats6) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    const u64 M = cm.n;
    u64 *st = nullptr, *dist = nullptr;
    u32 *pred = nullptr, *af = nullptr, *pf = nullptr, *d_err = nullptr, h_err = 0;
    unsigned long long *aoff = nullptr, *poff = nullptr, *d_cnt = nullptr, h_cnt[4] = {0, 0, 0, 0}, A = 0, P = 0;
    tmp.get(&st, M); tmp.get(&dist, M); tmp.get(&pred, M); tmp.get(&af, M); tmp.get(&pf, M);
    tmp.get(&aoff, M + 1); tmp.get(&poff, M + 1);
    tmp.zeroed(&d_cnt, 4); tmp.zeroed(&d_err, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_build_cycles: alloc");
    const int gm = ggrid(ctx, M);
    hipLaunchKernelGGL(k_cya_init, dim3(gm), dim3(BLOCK), 0, ctx->stream, st, cm.succ, pred, M);
    u64 R = 0;
    if (int rc = cycles_min(ctx, tmp, st, M, cm.klo, cm.khi, &R)) return rc;
    hipLaunchKernelGGL(k_cya_flags, dim3(gm), dim3(BLOCK), 0, ctx->stream, st, cm.klo, cm.khi, cm.meta, af, pf, dist, pred, M, d_err);
    tmp.note(scan_counts(ctx, tmp, af, M, aoff));
    tmp.note(scan_counts(ctx, tmp, pf, M, poff));
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_build_cycles: scan");
    for (u64 r = 0; r < R; r++) hipLaunchKernelGGL(k_cya_dist_round, dim3(gm), dim3(BLOCK), 0, ctx->stream, dist, af, M);
    hipError_t e = read_back(ctx, {{&A, aoff + M, 8}, {&P, poff + M, 8}, {&h_err, d_err, 4}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: anchors");
    if (h_err || !A || !P) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: a member lies on no cycle (code " + std::to_string(h_err) + ")");
    // ids: the anchors' nodes follow the plain build's in pairs (even: the k-mer that is its own anchor key, odd: its reverse
    // complement), in table slot order; the arcs follow the plain build's edges in the same order, one per anchor
    const u64 N0 = (v.n_nodes + 1) & ~1ull, E0 = v.n_edges;
    if (N0 + 2 * P >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph nodes");
    if (E0 + A >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph edges");
    if (int rc = graph_grow_nodes(g, N0 + 2 * P)) return rc;
    if (int rc = graph_grow_edges(g, E0 + A)) return rc;
    v.n_nodes = N0 + 2 * P;
    v.n_edges = E0 + A;
    GK_BY_W(g->W, hipLaunchKernelGGL(k_cya_nodes<W>, dim3(gm), dim3(BLOCK), 0, ctx->stream, v, g->k, cm, af, aoff, poff, dist, N0, E0, d_cnt, d_err));
    const u64 used0 = g->pool_used;                          // the arcs' bytes follow the plain build's: d_cnt[3] counts from 0
    hipLaunchKernelGGL(k_reserve_pool, dim3(ggrid(ctx, A)), dim3(BLOCK), 0, ctx->stream, v, E0, used0, &d_cnt[3]);
    e = read_back(ctx, {{h_cnt, d_cnt, 32}, {&h_err, d_err, 4}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: nodes");
    if (h_err) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: anchors and arcs disagree (code " + std::to_string(h_err) + ")");
    h_cnt[3] += used0;
    if (2 * P - h_cnt[1] != A || (h_cnt[0] & 1)) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: the anchors are not closed under reverse complement");
    // the pool grows by the arcs' bytes (whole 32-bit words: k_cya_emit ORs words), the plain build's bytes stay where they are
    const u64 new_cap = (std::max<u64>(h_cnt[3], 1) + 7) / 4 * 4;
    uint8_t *np = nullptr;
    e = pool_malloc(ctx, &np, new_cap);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: pool");
    if (used0) e = hipMemcpyAsync(np, v.pool, used0, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(np + used0, 0, new_cap - used0, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)pool_free(ctx, np); return hip_fail(ctx, e, "gk_graph_build_cycles: pool"); }
    (void)pool_free(ctx, v.pool);
    v.pool = np;
    g->pool_cap = new_cap;
    g->pool_used = h_cnt[3];
    hipLaunchKernelGGL(k_cya_emit, dim3(gm), dim3(BLOCK), 0, ctx->stream, v, cm.meta, af, aoff, dist, E0, M, new_cap, d_err);
    e = read_back(ctx, &h_err, d_err);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: emit");
    if (h_err) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: arc emission failed (code " + std::to_string(h_err) + ")");
    const u64 two = h_cnt[0] / 2;                            // cycles with two anchors
    stats6[0] = M; stats6[1] = A - two; stats6[2] = A; stats6[3] = h_cnt[1] + two; stats6[4] = h_cnt[2]; stats6[5] = R;
    return GK_OK;
}

// ---- node level: gk_graph_simplify_keep_cycles ----------------------------------------------------------------------------------
// class-1 nodes (one way in, one way out, different edges) with the successor "end of the single out-edge"; a class-1 node
// whose successor is of another class ends its chain
template <int W>
__global__ __launch_bounds__(BLOCK) void k_cyn_init(GraphView g, int k, const uint8_t *__restrict__ cls, u64 *st, u64 *klo, u64 *khi) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        u64 s = CY_UNREG;
        if (cls[n] == 1) {
            const u32 e = g.out_edge[n * 4 + order_base(g.out_order[n], 0)];
            const u32 w = e != NONE ? g.e_end[e] : NONE;
            s = (w != NONE && (u64)w < g.n_nodes && cls[w] == 1) ? ((u64)w | (n << 32)) : (n | ((u64)CY_LEAVES << 32));
        }
        st[n] = s;
        const Kmer<W> x = node_kmer<W>(g, n), rc = revcomp(x, k);
        const Kmer<W> key = kmer_less(rc, x) ? rc : x;      // the anchor key: min(x, rc x)
        klo[n] = key.lo;
        if constexpr (W == 2) khi[n] = key.hi;
    }
}
// cnt: [0] self-loop nodes kept, [1] cycles merged, [2] anchors kept
__global__ __launch_bounds__(BLOCK) void k_cyn_mark(GraphView g, uint8_t *cls, const u64 *__restrict__ st, const u64 *__restrict__ klo,
                                                    const u64 *__restrict__ khi, unsigned long long *cnt) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        const uint8_t c = cls[n];
        if (c == 2) { cls[n] = 0; atomicAdd(&cnt[0], 1ull); continue; }
        if (c != 1) continue;
        const u32 am = (u32)(st[n] >> 32);
        if (am == CY_LEAVES || !cy_same(klo, khi, (u32)n, am)) continue;
        // an anchor.  (Its class is written while other lanes still read classes — but only their OWN and, below, an anchor's
        // successor's argmin from st, never cls of another node.)
        cls[n] = 0;
        atomicAdd(&cnt[2], 1ull);
        // A cycle counts as merged when one of its arcs has an interior node; the anchor with the smallest id counts it.  The
        // hop below goes from anchor to anchor (the next anchor of a is the first minimum from a's successor on), never over
        // the nodes between them: one or two hops, more only where node copies (gk_graph_split_edges_by_spans) share the key.
        bool merged = false, mine = true;
        u32 a = (u32)n;
        for (u64 hops = 0; hops < g.n_nodes; hops++) {      // (the bound is never met: the next-anchor map permutes a cycle's anchors)
            const u32 w = g.e_end[g.out_edge[(u64)a * 4 + order_base(g.out_order[a], 0)]];
            const u32 o = (u32)(st[w] >> 32);
            if ((u64)o >= g.n_nodes) { mine = false; break; }
            merged |= w != o;
            a = o;
            if (a < (u32)n) mine = false;
            if (!mine || a == (u32)n) break;
        }
        if (mine && merged) atomicAdd(&cnt[1], 1ull);
    }
}
int cycles_keep_classes(gk_graph *g, DevScratch &tmp, uint8_t *cls, uint64_t *stats4) {
    gk_ctx *ctx = g->ctx;
    const GraphView &v = g->v;
    u64 *st = nullptr, *klo = nullptr, *khi = nullptr;
    unsigned long long *d_cnt = nullptr, h_cnt[3] = {0, 0, 0};
    tmp.get(&st, v.n_nodes); tmp.get(&klo, v.n_nodes);
    if (g->W == 2) tmp.get(&khi, v.n_nodes);
    tmp.zeroed(&d_cnt, 3);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_simplify_keep_cycles: alloc");
    const int gn = ggrid(ctx, v.n_nodes);
    GK_BY_W(g->W, hipLaunchKernelGGL(k_cyn_init<W>, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, g->k, cls, st, klo, khi));
    if (int rc = cycles_min(ctx, tmp, st, v.n_nodes, klo, khi, nullptr)) return rc;
    hipLaunchKernelGGL(k_cyn_mark, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, cls, st, klo, khi, d_cnt);
    const hipError_t e = read_back(ctx, h_cnt, d_cnt, 3);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_simplify_keep_cycles: anchors");
    stats4[0] = h_cnt[0]; stats4[1] = h_cnt[1]; stats4[2] = h_cnt[2];
    tmp.release(st); tmp.release(klo);                      // (before k_chain's output is allocated)
    if (khi) tmp.release(khi);
    return GK_OK;
}
