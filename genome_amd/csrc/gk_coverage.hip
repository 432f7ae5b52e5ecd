// gk_coverage.hip — how often the k-mers of an edge were seen (the count table's multiplicities carried up to the graph), and
// the removal of dead-end tips decided from those numbers.
//
// Reference: none.  Graph.buildGraph (S/data/graph/Graph.scala:269-382) drops the counts once `contains` has been answered, and
// the reference has no tip removal.  The rules of the two entry points are this project's own and
// stated in include/genome_amd.h; tests/tips_ref.py restates them.  So are the two that remove bubbles by the same numbers
// (gk_graph_edge_distance: a thresholded, banded edit distance of two edges, one wave per pair; gk_graph_pop_bubbles: the weaker of
// two similar parallel edges goes; restated in tests/bubbles_ref.py) — gk_graph_remove_bubbles, the reference's own unfinished
// rule (Graph.scala:121-149), stays in gk_graph.hip as it is.  And the one that removes weak connections (gk_graph_remove_weak_edges:
// an edge with a way on at both ends and a competitor `ratio` times stronger at each, or a mean below a floor; restated in
// tests/weak_ref.py).
//
// Roofline: one independent random table probe per k-mer of every live edge (total edge length + live edges of them) and
// nothing else of size: the random-load rate of HBM, as the unitig walk — whose probes depend on each other, these do not.
#include <algorithm>

#include "gk_graph.h"
#include "gk_scan.h"

// ---------------------------------------------------------------------------------------------
// windows of start.seq ++ edge.seq without a per-base loop per window: pool_bits / path_bits / window_at (gk_graph.h)
// ---------------------------------------------------------------------------------------------
// sum / min / max / missing over a run of windows, rolled: the forward window takes the next base at its end, the reverse
// complement its complement at the front; the bases come out of the pool one byte per four steps
struct CovAcc {
    u64 sum = 0;
    u32 mn = ~0u, mx = 0, miss = 0;
    __device__ __forceinline__ void add(u32 c) { sum += c; mn = min(mn, c); mx = max(mx, c); miss += c == 0u; }
    __device__ __forceinline__ void merge(u64 s, u32 a, u32 b, u32 m) { sum += s; mn = min(mn, a); mx = max(mx, b); miss += m; }
};
template <int W, class S>
__device__ __forceinline__ void cover_run(const Table<W, S> &t, Kmer<2> node, const uint8_t *__restrict__ seq, int k, u64 d0, u64 d1, CovAcc &acc) {
    Kmer<W> x = window_at<W>(node, seq, k, k, d0), rc = revcomp(x, k);
    acc.add(window_count(t, x, rc));
    u32 byte = (d0 & 3) ? seq[d0 >> 2] : 0u;                 // the window at distance d + 1 ends with base d of the edge
    for (u64 d = d0; d + 1 < d1; d++) {
        if ((d & 3) == 0) byte = seq[d >> 2];
        const int b = (int)(byte >> ((d & 3) * 2)) & 3;
        x = append_base(x, b, k);
        rc = prepend_base(3 - b, rc, k);
        acc.add(window_count(t, x, rc));
    }
}

// Per-edge results (EdgeCov, gk_graph.h), indexed by edge id; written for the live edges (`want` == nullptr) or the live edges
// marked in `want`.
static constexpr u64 COV_SHORT = 64;      // windows one lane walks alone
static constexpr u64 COV_RUN = 16;        // consecutive windows per lane and pass of the long form

// short edges (<= COV_SHORT windows): one lane per edge, no atomics
template <int W, class S>
__global__ __launch_bounds__(BLOCK) void k_cov_short(GraphView g, Table<W, S> t, const uint8_t *__restrict__ want, EdgeCov out) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        if (!g.e_alive[e] || (want && !want[e])) continue;
        const u64 nwin = g.e_len[e] + 1;
        if (nwin > COV_SHORT) continue;
        const u32 s = g.e_start[e];
        CovAcc acc;
        cover_run<W, S>(t, Kmer<2>{g.node_lo[s], W == 2 ? g.node_hi[s] : 0ull}, g.pool + g.e_off[e], g.k, 0, nwin, acc);
        out.sum[e] = acc.sum; out.mn[e] = acc.mn; out.mx[e] = acc.mx; out.miss[e] = acc.miss;
    }
}
// long edges: one workgroup per edge at a time; a pass is BLOCK runs of COV_RUN consecutive windows, lane t the t-th.  The partial
// results meet by wave shuffle, then through one LDS step; lane 0 writes.
template <int W, class S>
__global__ __launch_bounds__(BLOCK) void k_cov_long(GraphView g, Table<W, S> t, const uint8_t *__restrict__ want, EdgeCov out) {
    __shared__ u64 s_sum[BLOCK / 64];
    __shared__ u32 s_mn[BLOCK / 64], s_mx[BLOCK / 64], s_miss[BLOCK / 64];
    for (u64 e = blockIdx.x; e < g.n_edges; e += gridDim.x) {            // (uniform over the workgroup: the barriers below are safe)
        if (!g.e_alive[e] || (want && !want[e])) continue;
        const u64 nwin = g.e_len[e] + 1;
        if (nwin <= COV_SHORT) continue;
        const u32 s = g.e_start[e];
        const Kmer<2> node{g.node_lo[s], W == 2 ? g.node_hi[s] : 0ull};
        const uint8_t *seq = g.pool + g.e_off[e];
        CovAcc acc;
        for (u64 d0 = (u64)threadIdx.x * COV_RUN; d0 < nwin; d0 += (u64)BLOCK * COV_RUN)
            cover_run<W, S>(t, node, seq, g.k, d0, min(d0 + COV_RUN, nwin), acc);
        for (int d = 32; d; d >>= 1)
            acc.merge(__shfl_down(acc.sum, d), __shfl_down(acc.mn, d), __shfl_down(acc.mx, d), __shfl_down(acc.miss, d));
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { s_sum[wave] = acc.sum; s_mn[wave] = acc.mn; s_mx[wave] = acc.mx; s_miss[wave] = acc.miss; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < BLOCK / 64; w++) acc.merge(s_sum[w], s_mn[w], s_mx[w], s_miss[w]);
            out.sum[e] = acc.sum; out.mn[e] = acc.mn; out.mx[e] = acc.mx; out.miss[e] = acc.miss;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BLOCK) void k_cov_want(const u32 *__restrict__ ids, u64 n, u64 n_edges, uint8_t *want) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK)
        if (ids[i] < n_edges) want[ids[i]] = 1;
}
// the answers in the order asked; a dead or out-of-range id reads zeros.  missing[0] += the windows not held, once per wave.
__global__ __launch_bounds__(BLOCK) void k_cov_gather(GraphView g, EdgeCov cov, const u32 *__restrict__ ids, u64 n, u64 *kmers, u64 *sum, u32 *mn, u32 *mx,
                                                      unsigned long long *missing) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 i0 = (u64)blockIdx.x * BLOCK; i0 < n; i0 += stride) {       // (uniform over the wave: every lane takes the shuffles)
        const u64 i = i0 + threadIdx.x;
        unsigned long long m = 0;
        if (i < n) {
            const u32 e = ids[i];
            const bool ok = e < g.n_edges && g.e_alive[e];
            kmers[i] = ok ? g.e_len[e] + 1 : 0;
            sum[i] = ok ? cov.sum[e] : 0;
            mn[i] = ok ? cov.mn[e] : 0;
            mx[i] = ok ? cov.mx[e] : 0;
            m = ok ? cov.miss[e] : 0;
        }
        for (int d = 32; d; d >>= 1) m += __shfl_down(m, d);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(missing, m);
    }
}

// ---------------------------------------------------------------------------------------------
// tips (the rule: include/genome_amd.h, gk_graph_clip_tips)
// ---------------------------------------------------------------------------------------------
// mean coverage of a strictly below that of b: sum_a * kmers_b < sum_b * kmers_a as 128-bit integers
__device__ __forceinline__ bool cov_weaker(u64 sum_a, u64 kmers_a, u64 sum_b, u64 kmers_b) {
    const u64 lh = __umul64hi(sum_a, kmers_b), ll = sum_a * kmers_b, rh = __umul64hi(sum_b, kmers_a), rl = sum_b * kmers_a;
    return lh != rh ? lh < rh : ll < rl;
}
// one lane per edge, from the graph as it is (nothing is written but `mark`): flags[0] = a live edge has a window the table
// does not hold
__global__ __launch_bounds__(BLOCK) void k_tip_mark(GraphView g, EdgeCov cov, const unsigned long long *__restrict__ in_off, const u32 *__restrict__ in_list,
                                                    u64 max_len, uint8_t *mark, u32 *flags) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        mark[e] = 0;
        if (!g.e_alive[e]) continue;
        if (cov.miss[e]) flags[0] = 1u;
        const u64 len = g.e_len[e];
        if (len > max_len) continue;
        const u32 u = g.e_start[e], v = g.e_end[e];
        const u32 out_u = (u32)order_count(g.out_order[u]), out_v = (u32)order_count(g.out_order[v]);
        const u64 in_u = in_off[u + 1] - in_off[u], in_v = in_off[v + 1] - in_off[v];
        const u64 sum_e = cov.sum[e], kmers_e = len + 1;
        bool weaker = false;
        if (out_v == 0 && in_v == 1 && out_u >= 2) {                     // out-tip: against the other out-edges of u
            for (int b = 0; b < 4; b++) {
                const u32 f = g.out_edge[(u64)u * 4 + b];
                if (f != NONE && f != (u32)e && g.e_alive[f]) weaker |= cov_weaker(sum_e, kmers_e, cov.sum[f], g.e_len[f] + 1);
            }
        } else if (in_u == 0 && out_u == 1 && in_v >= 2) {               // in-tip: against the other in-edges of v
            for (u64 j = in_off[v]; j < in_off[v + 1]; j++) {
                const u32 f = in_list[j];
                if (f != (u32)e) weaker |= cov_weaker(sum_e, kmers_e, cov.sum[f], g.e_len[f] + 1);
            }
        }
        if (weaker) mark[e] = 1;
    }
}
// ... applied at once — unless the marking found the map wanting: then the graph stays as it was
__global__ __launch_bounds__(BLOCK) void k_tip_apply(GraphView g, const uint8_t *__restrict__ mark, const u32 *__restrict__ flags, unsigned long long *removed) {
    if (flags[0]) return;
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 e0 = (u64)blockIdx.x * BLOCK; e0 < g.n_edges; e0 += stride) {
        const u64 e = e0 + threadIdx.x;
        const bool rm = e < g.n_edges && mark[e];
        if (rm) graph_remove_edge(g, (u32)e);
        const unsigned long long votes = __ballot(rm);
        if ((threadIdx.x & 63) == 0 && votes) atomicAdd(removed, (unsigned long long)__popcll(votes));
    }
}

// ---------------------------------------------------------------------------------------------
// weak connections (the rule: include/genome_amd.h, gk_graph_remove_weak_edges)
// ---------------------------------------------------------------------------------------------
static constexpr u32 WEAK_MAX_RATIO = 65535;             // ratio * kmers stays inside 64 bits
// one lane per edge, from the graph as it is (nothing is written but `mark`, flags[0] and the counters): (A) a competitor `ratio`
// times stronger among the other out-edges of the start node AND among the other in-edges of the end node, (B) a mean below `floor`.
// stats[0] += candidates, stats[1] += marked under (A), stats[2] += marked under (B) alone, once per wave (stats[3] is the apply's).
__global__ __launch_bounds__(BLOCK) void k_weak_mark(GraphView g, EdgeCov cov, const unsigned long long *__restrict__ in_off, const u32 *__restrict__ in_list,
                                                     u64 max_len, u64 ratio, u64 floor, uint8_t *mark, u32 *flags, unsigned long long *stats) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 e0 = (u64)blockIdx.x * BLOCK; e0 < g.n_edges; e0 += stride) {  // (uniform over the wave: every lane takes the ballots)
        const u64 e = e0 + threadIdx.x;
        bool cand = false, by_ratio = false, by_floor = false;
        if (e < g.n_edges) {
            const bool live = g.e_alive[e];
            if (live && cov.miss[e]) flags[0] = 1u;
            const u64 len = live ? g.e_len[e] : 0;
            if (live && len <= max_len) {
                const u32 u = g.e_start[e], v = g.e_end[e];
                const u64 sum_e = cov.sum[e], kmers_e = len + 1;
                cand = order_count(g.out_order[u]) >= 2 && in_off[v + 1] - in_off[v] >= 2;
                if (cand && ratio) {
                    bool out_stronger = false, in_stronger = false;
                    for (int b = 0; b < 4; b++) {
                        const u32 f = g.out_edge[(u64)u * 4 + b];
                        if (f != NONE && f != (u32)e && g.e_alive[f]) out_stronger |= cov_weaker(sum_e, kmers_e, cov.sum[f], ratio * (g.e_len[f] + 1));
                    }
                    if (out_stronger)
                        for (u64 j = in_off[v]; j < in_off[v + 1]; j++) {
                            const u32 f = in_list[j];
                            if (f != (u32)e) in_stronger |= cov_weaker(sum_e, kmers_e, cov.sum[f], ratio * (g.e_len[f] + 1));
                        }
                    by_ratio = in_stronger;
                }
                by_floor = floor && !by_ratio && cov_weaker(sum_e, kmers_e, floor, 1);
            }
            mark[e] = by_ratio || by_floor;
        }
        const unsigned long long c = __ballot(cand), a = __ballot(by_ratio), b = __ballot(by_floor);
        if ((threadIdx.x & 63) == 0) {
            if (c) atomicAdd(stats + 0, (unsigned long long)__popcll(c));
            if (a) atomicAdd(stats + 1, (unsigned long long)__popcll(a));
            if (b) atomicAdd(stats + 2, (unsigned long long)__popcll(b));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// bubbles (the rules: include/genome_amd.h, gk_graph_edge_distance and gk_graph_pop_bubbles)
// ---------------------------------------------------------------------------------------------
static constexpr u32 DIST_MAX_DIFF = 31;                // a band of 2 * 31 + 1 = 63 diagonals: one wave, lane 63 the wall beside it
static constexpr u32 DIST_INVALID = 0xffffffffu;

// bases s .. s + 31 of a sequence of n bases as 32 2-bit codes; s may be negative and s + 32 may pass n: those read as 0, and no
// byte outside the sequence is touched
__device__ __forceinline__ u64 seq_chunk(const uint8_t *__restrict__ seq, i64 s, u64 n) {
    const i64 lo = s > 0 ? s : 0, hi = s + 32 < (i64)n ? s + 32 : (i64)n;
    return hi > lo ? pool_bits(seq, (u64)lo, (int)(hi - lo)) << (2 * (int)(lo - s)) : 0ull;
}

// min(Levenshtein(a, b), D + 1) by one wave, for |m - n| <= D <= 31; every lane of the wave must call it (the shuffles take all
// 64) and every lane gets the answer.  Lane d owns diagonal o = d - D of the matrix: in row i the cell (i, i + o).  The rows
// advance in lock-step:
//   the diagonal neighbour (i-1, j-1) is the lane's own last value, the upper one (i-1, j) lane d + 1's last value, and the
//   left one (i, j-1) lane d - 1's value of THIS row: cur[d] = min over e <= d of (t[e] + d - e), t = min(diagonal, upper) —
//   a prefix minimum in log2(band) shuffle steps.
// Every value is capped at D + 1, which is also what a cell outside the matrix or the band holds: an alignment of cost <= D
// never leaves |i - j| <= D, so the cap changes no value <= D.  Row i reads base i - 1 of a (the same for every lane) and base
// i - 1 + o of b; both come 32 at a time, at the same rows and the same bit position, so a substitution is one XOR.
// The wave leaves as soon as a whole row is over D (the minimum of a row never falls).
__device__ __forceinline__ u32 wave_banded_distance(const uint8_t *__restrict__ a, u64 m, const uint8_t *__restrict__ b, u64 n, u32 D) {
    const u32 lane = threadIdx.x & 63u, cap = D + 1;
    const i64 o = (i64)lane - (i64)D;
    const bool band = lane <= 2 * D;
    u32 cur = band && o >= 0 && (u64)o <= n ? (u32)o : cap;              // row 0 (o <= D < cap)
    u64 abits = 0, bbits = 0;
    for (u64 i = 1; i <= m; i++) {                                       // (uniform over the wave)
        const u64 r = i - 1;
        if ((r & 31) == 0) {
            abits = pool_bits(a, r, (int)(m - r < 32 ? m - r : 32));
            bbits = band ? seq_chunk(b, (i64)r + o, n) : 0ull;
        }
        const u32 sub = ((abits ^ bbits) >> (2 * (int)(r & 31)) & 3) != 0;
        const u32 up = __shfl_down(cur, 1);                              // (lane 63 reads itself: it is never in the band)
        const i64 j = (i64)i + o;
        const bool cell = band && j >= 0 && (u64)j <= n;
        u32 t = cell ? min(min(cur + sub, up + 1), cap) : cap;
        for (u32 s = 1; s <= 2 * D; s <<= 1) {
            const u32 left = __shfl_up(t, s);
            if (lane >= s) t = min(t, left + s);
        }
        cur = cell ? t : cap;
        if (!__any(cur <= D)) return cap;
    }
    return __shfl(cur, (int)((i64)D + (i64)n - (i64)m));
}

// one wave per pair of edge ids
__global__ __launch_bounds__(BLOCK) void k_edge_distance(GraphView g, const u32 *__restrict__ e1, const u32 *__restrict__ e2, u64 n, u32 D, u32 *__restrict__ dist) {
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 p = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); p < n; p += waves) {      // (uniform over the wave)
        const u32 e = __builtin_amdgcn_readfirstlane(e1[p]), f = __builtin_amdgcn_readfirstlane(e2[p]);
        u32 d;
        if (e >= g.n_edges || f >= g.n_edges || !g.e_alive[e] || !g.e_alive[f]) d = DIST_INVALID;
        else if (e == f) d = 0;
        else {
            const u64 m = g.e_len[e], l = g.e_len[f];
            d = (m > l ? m - l : l - m) > D ? D + 1 : wave_banded_distance(g.pool + g.e_off[e], m, g.pool + g.e_off[f], l, D);
        }
        if ((threadIdx.x & 63) == 0) dist[p] = d;
    }
}

// the unordered pairs among the live out-edges of node u that share their end node, both of at most max_len bases: 6 at most
template <class F> __device__ __forceinline__ u32 parallel_pairs(const GraphView &g, u64 u, u64 max_len, F &&emit) {
    u32 ids[4];
    for (int b = 0; b < 4; b++) {
        const u32 f = g.out_edge[u * 4 + b];
        ids[b] = f != NONE && g.e_alive[f] && g.e_len[f] <= max_len ? f : NONE;
    }
    u32 cnt = 0;
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 4; b++)
            if (ids[a] != NONE && ids[b] != NONE && g.e_end[ids[a]] == g.e_end[ids[b]]) emit(cnt++, ids[a], ids[b]);
    return cnt;
}
// one lane per node: the number of its candidate pairs, then (with `off` the exclusive scan of those) the pairs themselves and
// want[e] = 1 for their edges (an edge leaves one node: one lane writes its byte)
__global__ __launch_bounds__(BLOCK) void k_bubble_count(GraphView g, u64 max_len, u32 *__restrict__ cnt) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < g.n_nodes; u += (u64)gridDim.x * BLOCK)
        cnt[u] = g.node_alive[u] && order_count(g.out_order[u]) >= 2 ? parallel_pairs(g, u, max_len, [](u32, u32, u32) {}) : 0u;
}
__global__ __launch_bounds__(BLOCK) void k_bubble_pairs(GraphView g, u64 max_len, const u32 *__restrict__ cnt, const unsigned long long *__restrict__ off,
                                                        u32 *__restrict__ pe, u32 *__restrict__ pf, uint8_t *__restrict__ want) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < g.n_nodes; u += (u64)gridDim.x * BLOCK) {
        if (!cnt[u]) continue;
        const u64 at = off[u];
        parallel_pairs(g, u, max_len, [&](u32 i, u32 e, u32 f) { pe[at + i] = e; pf[at + i] = f; want[e] = 1; want[f] = 1; });
    }
}
// one lane per candidate pair, from the graph as it is (nothing is written but `mark`, zeroed before): the weaker edge of a pair
// within D goes.  flags[0] = a candidate edge has a window the table does not hold; *compared += the pairs whose lengths let the
// distance be computed.
__global__ __launch_bounds__(BLOCK) void k_bubble_mark(GraphView g, EdgeCov cov, const u32 *__restrict__ pe, const u32 *__restrict__ pf, const u32 *__restrict__ dist,
                                                       u64 npairs, u32 D, uint8_t *mark, u32 *flags, unsigned long long *compared) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 p0 = (u64)blockIdx.x * BLOCK; p0 < npairs; p0 += stride) {  // (uniform over the wave: every lane takes the ballot)
        const u64 p = p0 + threadIdx.x;
        bool within = false;
        if (p < npairs) {
            const u32 e = pe[p], f = pf[p];
            if (cov.miss[e] | cov.miss[f]) flags[0] = 1u;
            const u64 le = g.e_len[e], lf = g.e_len[f];
            within = (le > lf ? le - lf : lf - le) <= D;
            if (dist[p] <= D) {
                if (cov_weaker(cov.sum[e], le + 1, cov.sum[f], lf + 1)) mark[e] = 1;
                else if (cov_weaker(cov.sum[f], lf + 1, cov.sum[e], le + 1)) mark[f] = 1;
            }
        }
        const unsigned long long votes = __ballot(within);
        if ((threadIdx.x & 63) == 0 && votes) atomicAdd(compared, (unsigned long long)__popcll(votes));
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int check_counts(const gk_graph *g, gk_map *counts, const char *who) {
    if (!counts || !counts->ctx) return fail(g->ctx, GK_E_INVALID, std::string(who) + ": null map handle");
    if (counts->ctx != g->ctx) return fail(g->ctx, GK_E_INVALID, std::string(who) + ": the map belongs to another context");
    if (counts->k != g->k) return fail(g->ctx, GK_E_INVALID, std::string(who) + ": the map's k is not the graph's");
    return map_materialize(counts);                          // (a new or cleared map: empty slots, not void bytes)
}

// the coverage of every live edge (`want` == nullptr) or of the marked ones into arrays owned by `tmp`; stream-ordered, no sync
int coverage_pass(gk_graph *g, gk_map *counts, DevScratch &tmp, const uint8_t *want, EdgeCov *cov) {
    gk_ctx *ctx = g->ctx;
    const GraphView &v = g->v;
    tmp.get(&cov->sum, v.n_edges);
    tmp.get(&cov->mn, v.n_edges);
    tmp.get(&cov->mx, v.n_edges);
    tmp.get(&cov->miss, v.n_edges);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "edge coverage: per-edge results");
    if (v.n_edges == 0) return GK_OK;
    const int long_grid = (int)std::min<u64>(v.n_edges, grid_cap(ctx));
    GK_BY_SLOT(counts, {
        const Table<W, S> t{reinterpret_cast<S *>(counts->slots), counts->nb2, counts->lnb1, counts->k == 64 ? 1u : 0u, counts->dirty ? 1u : 0u};
        hipLaunchKernelGGL((k_cov_short<W, S>), dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, t, want, *cov);
        hipLaunchKernelGGL((k_cov_long<W, S>), dim3(long_grid), dim3(BLOCK), 0, ctx->stream, v, t, want, *cov);
    });
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}

extern "C" {

int gk_graph_edge_coverage(gk_graph *g, gk_map *counts, const uint32_t *edge_ids, uint64_t n, uint64_t *kmers, uint64_t *sum,
                           uint32_t *min_count, uint32_t *max_count, uint64_t *missing) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (int rc = check_counts(g, counts, "gk_graph_edge_coverage")) return rc;
    if (missing) *missing = 0;
    if (n == 0) return GK_OK;
    if (!edge_ids) return fail(ctx, GK_E_INVALID, "gk_graph_edge_coverage: edge_ids is NULL");
    const GraphView &v = g->v;
    DevScratch tmp(ctx);
    u32 *d_ids = nullptr, *d_mn = nullptr, *d_mx = nullptr;
    u64 *d_kmers = nullptr, *d_sum = nullptr;
    uint8_t *d_want = nullptr;
    unsigned long long *d_missing = nullptr, h_missing = 0;
    tmp.upload(&d_ids, edge_ids, n);
    tmp.get(&d_kmers, n);
    tmp.get(&d_sum, n);
    tmp.get(&d_mn, n);
    tmp.get(&d_mx, n);
    tmp.zeroed(&d_want, v.n_edges);
    tmp.zeroed(&d_missing, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_edge_coverage");
    hipLaunchKernelGGL(k_cov_want, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, d_ids, (u64)n, v.n_edges, d_want);
    EdgeCov cov{};
    if (int rc = coverage_pass(g, counts, tmp, d_want, &cov)) return rc;
    hipLaunchKernelGGL(k_cov_gather, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, v, cov, d_ids, (u64)n, d_kmers, d_sum, d_mn, d_mx, d_missing);
    const hipError_t e = read_back(ctx, {{kmers, d_kmers, (size_t)n * 8}, {sum, d_sum, (size_t)n * 8}, {min_count, d_mn, (size_t)n * 4},
                                         {max_count, d_mx, (size_t)n * 4}, {&h_missing, d_missing, 8}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_edge_coverage");
    if (missing) *missing = h_missing;
    return GK_OK;
}

int gk_graph_clip_tips(gk_graph *g, gk_map *counts, uint64_t max_len, uint64_t *removed_edges) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (int rc = check_counts(g, counts, "gk_graph_clip_tips")) return rc;
    if (removed_edges) *removed_edges = 0;
    const GraphView &v = g->v;
    if (max_len == 0 || v.n_edges == 0) return GK_OK;
    DevScratch tmp(ctx);
    EdgeCov cov{};
    if (int rc = coverage_pass(g, counts, tmp, nullptr, &cov)) return rc;
    // the in-edge lists of the graph as it is
    unsigned long long *d_in_off = nullptr, *d_removed = nullptr, h_removed = 0;
    u32 *d_in_list = nullptr, *d_flags = nullptr, h_flags = 0;
    uint8_t *d_mark = nullptr;
    tmp.get(&d_mark, v.n_edges);
    tmp.zeroed(&d_flags, 1);
    tmp.zeroed(&d_removed, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_clip_tips: marks");
    if (int rc = graph_in_lists(g, tmp, "gk_graph_clip_tips", &d_in_off, &d_in_list)) return rc;
    const int grid = ggrid(ctx, v.n_edges);
    hipLaunchKernelGGL(k_tip_mark, dim3(grid), dim3(BLOCK), 0, ctx->stream, v, cov, d_in_off, d_in_list, (u64)max_len, d_mark, d_flags);
    // the decision is complete before anything is applied, and a map that is not this graph's leaves the graph as it was
    hipLaunchKernelGGL(k_tip_apply, dim3(grid), dim3(BLOCK), 0, ctx->stream, v, d_mark, d_flags, d_removed);
    GK_HIP(ctx, read_back(ctx, {{&h_flags, d_flags, 4}, {&h_removed, d_removed, 8}}));
    if (h_flags) return fail(ctx, GK_E_STATE, "gk_graph_clip_tips: the map does not hold every k-mer of the graph (not the table it was built from?)");
    if (removed_edges) *removed_edges = h_removed;
    return graph_refresh_counts(g);
}

int gk_graph_remove_weak_edges(gk_graph *g, gk_map *counts, uint64_t max_len, uint32_t ratio, uint32_t floor, uint64_t *stats4) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (int rc = check_counts(g, counts, "gk_graph_remove_weak_edges")) return rc;
    if (ratio > WEAK_MAX_RATIO) return fail(ctx, GK_E_INVALID, "gk_graph_remove_weak_edges: ratio is at most 65535 (ratio * kmers stays inside 64 bits)");
    if (stats4) std::fill(stats4, stats4 + 4, (uint64_t)0);
    const GraphView &v = g->v;
    if (max_len == 0 || v.n_edges == 0) return GK_OK;
    DevScratch tmp(ctx);
    EdgeCov cov{};
    if (int rc = coverage_pass(g, counts, tmp, nullptr, &cov)) return rc;
    // the in-edge lists of the graph as it is
    unsigned long long *d_in_off = nullptr, *d_stats = nullptr, h_stats[4] = {0, 0, 0, 0};
    u32 *d_in_list = nullptr, *d_flags = nullptr, h_flags = 0;
    uint8_t *d_mark = nullptr;
    tmp.get(&d_mark, v.n_edges);
    tmp.zeroed(&d_flags, 1);
    tmp.zeroed(&d_stats, 4);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_remove_weak_edges: marks");
    if (int rc = graph_in_lists(g, tmp, "gk_graph_remove_weak_edges", &d_in_off, &d_in_list)) return rc;
    const int grid = ggrid(ctx, v.n_edges);
    hipLaunchKernelGGL(k_weak_mark, dim3(grid), dim3(BLOCK), 0, ctx->stream, v, cov, d_in_off, d_in_list, (u64)max_len, (u64)ratio, (u64)floor, d_mark, d_flags, d_stats);
    // the decision is complete before anything is applied, and a map that is not this graph's leaves the graph as it was
    hipLaunchKernelGGL(k_tip_apply, dim3(grid), dim3(BLOCK), 0, ctx->stream, v, d_mark, d_flags, d_stats + 3);
    GK_HIP(ctx, read_back(ctx, {{&h_flags, d_flags, 4}, {h_stats, d_stats, 32}}));
    if (h_flags) return fail(ctx, GK_E_STATE, "gk_graph_remove_weak_edges: the map does not hold every k-mer of the graph (not the table it was built from?)");
    if (stats4) std::copy(h_stats, h_stats + 4, stats4);
    return graph_refresh_counts(g);
}

int gk_graph_edge_distance(gk_graph *g, const uint32_t *e1, const uint32_t *e2, uint64_t n, uint32_t max_diff, uint32_t *dist) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (max_diff > DIST_MAX_DIFF) return fail(ctx, GK_E_INVALID, "gk_graph_edge_distance: max_diff is at most 31 (a band of 63 diagonals, one wave)");
    if (n == 0) return GK_OK;
    if (!e1 || !e2) return fail(ctx, GK_E_INVALID, "gk_graph_edge_distance: an id array is NULL");
    DevScratch tmp(ctx);
    u32 *d_e1 = nullptr, *d_e2 = nullptr, *d_dist = nullptr;
    tmp.upload(&d_e1, e1, n);
    tmp.upload(&d_e2, e2, n);
    tmp.get(&d_dist, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_edge_distance");
    hipLaunchKernelGGL(k_edge_distance, dim3(ggrid(ctx, n * 64)), dim3(BLOCK), 0, ctx->stream, g->v, d_e1, d_e2, (u64)n, (u32)max_diff, d_dist);
    GK_HIP(ctx, read_back(ctx, {{dist, d_dist, (size_t)n * 4}}));
    return GK_OK;
}

int gk_graph_pop_bubbles(gk_graph *g, gk_map *counts, uint64_t max_len, uint32_t max_diff, uint64_t *removed_edges, uint64_t *pairs_compared) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (int rc = check_counts(g, counts, "gk_graph_pop_bubbles")) return rc;
    if (max_diff > DIST_MAX_DIFF) return fail(ctx, GK_E_INVALID, "gk_graph_pop_bubbles: max_diff is at most 31 (a band of 63 diagonals, one wave)");
    if (removed_edges) *removed_edges = 0;
    if (pairs_compared) *pairs_compared = 0;
    const GraphView &v = g->v;
    if (max_len == 0 || v.n_edges == 0 || v.n_nodes == 0) return GK_OK;
    DevScratch tmp(ctx);
    // the candidate pairs: counted per node, scanned, written
    unsigned long long *d_off = nullptr, *d_removed = nullptr, *d_compared = nullptr, h_pairs = 0, h_removed = 0, h_compared = 0;
    u32 *d_cnt = nullptr, *d_pe = nullptr, *d_pf = nullptr, *d_dist = nullptr, *d_flags = nullptr, h_flags = 0;
    uint8_t *d_want = nullptr, *d_mark = nullptr;
    tmp.get(&d_cnt, v.n_nodes);
    tmp.get(&d_off, v.n_nodes + 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_pop_bubbles: candidate counts");
    const int ngrid = ggrid(ctx, v.n_nodes);
    hipLaunchKernelGGL(k_bubble_count, dim3(ngrid), dim3(BLOCK), 0, ctx->stream, v, (u64)max_len, d_cnt);
    GK_HIP(ctx, scan_counts(ctx, tmp, d_cnt, v.n_nodes, d_off));
    GK_HIP(ctx, read_back(ctx, &h_pairs, d_off + v.n_nodes));
    if (h_pairs == 0) return GK_OK;
    tmp.get(&d_pe, h_pairs);
    tmp.get(&d_pf, h_pairs);
    tmp.get(&d_dist, h_pairs);
    tmp.zeroed(&d_want, v.n_edges);
    tmp.zeroed(&d_mark, v.n_edges);
    tmp.zeroed(&d_flags, 1);
    tmp.zeroed(&d_removed, 1);
    tmp.zeroed(&d_compared, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_pop_bubbles: candidate pairs");
    hipLaunchKernelGGL(k_bubble_pairs, dim3(ngrid), dim3(BLOCK), 0, ctx->stream, v, (u64)max_len, d_cnt, d_off, d_pe, d_pf, d_want);
    // coverage of the edges in some bubble only, and the distance of every pair
    EdgeCov cov{};
    if (int rc = coverage_pass(g, counts, tmp, d_want, &cov)) return rc;
    hipLaunchKernelGGL(k_edge_distance, dim3(ggrid(ctx, h_pairs * 64)), dim3(BLOCK), 0, ctx->stream, v, d_pe, d_pf, (u64)h_pairs, (u32)max_diff, d_dist);
    // the decision is complete before anything is applied, and a map that is not this graph's leaves the graph as it was
    hipLaunchKernelGGL(k_bubble_mark, dim3(ggrid(ctx, h_pairs)), dim3(BLOCK), 0, ctx->stream, v, cov, d_pe, d_pf, d_dist, (u64)h_pairs, (u32)max_diff, d_mark, d_flags,
                       d_compared);
    hipLaunchKernelGGL(k_tip_apply, dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, d_mark, d_flags, d_removed);
    GK_HIP(ctx, read_back(ctx, {{&h_flags, d_flags, 4}, {&h_removed, d_removed, 8}, {&h_compared, d_compared, 8}}));
    if (h_flags) return fail(ctx, GK_E_STATE, "gk_graph_pop_bubbles: the map does not hold every k-mer of the candidate edges (not the table the graph was built from?)");
    if (removed_edges) *removed_edges = h_removed;
    if (pairs_compared) *pairs_compared = h_compared;
    return graph_refresh_counts(g);
}

}  // extern "C"
