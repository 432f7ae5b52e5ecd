// gk_graph.h — the device-side view of a MapGraph (S/data/graph/Graph.scala:153-209), the host handle and the block-wide device
// helpers, shared by gk_graph.hip (the build from a k-mer table), gk_graph_ops.hip (everything on a built graph: the arrays,
// structural edits, in-edge lists), gk_pairs.hip (the paired-end stage), gk_graphio.hip (the graph file) and the readers of a
// count table (gk_coverage.hip, gk_correct.hip: window_count).
#pragma once

#include <memory>
#include <unordered_map>
#include <vector>

#include "gk_internal.h"
#include "gk_tile.h"

using namespace gk;

struct gk_vmap;
namespace gk {
int vmap_put_new_dev(gk_vmap *m, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_val, uint64_t n);
int vmap_k(const gk_vmap *m);
gk_ctx *vmap_ctx(const gk_vmap *m);
}

static constexpr u32 NONE = 0xFFFFFFFFu;
static constexpr u32 AUX_TERMINAL = 1u << 8;
static constexpr u32 AUX_SECONDARY = 1u << 9;
// Once k_make_nodes has numbered the terminal k-mers, a terminal slot's annotation IS its node: AUX_NODE | j, where the stored
// orientation is node 2j and its reverse complement node 2j + 1.  (Until round 3 a separate u32 per table SLOT held that
// number: 4 bytes x capacity — 19 GB at C5 — and one more random read at every edge's end.)  Its degree masks are not
// needed any more at that point: a walk stops at a terminal k-mer, it never leaves one through the table.
static constexpr u32 AUX_NODE = 1u << 31;
__device__ __forceinline__ u32 aux_node(u32 aux, bool fwd) { return 2u * (aux & 0x7fffffffu) + (fwd ? 0u : 1u); }

// ---------------------------------------------------------------------------------------------
// device-side view of a graph
// ---------------------------------------------------------------------------------------------
struct GraphView {
    int k;
    u64 n_nodes, n_edges;
    u64 *node_lo, *node_hi;
    uint8_t *node_alive;
    u32 *out_edge;      // [n_nodes*4], by first base
    u32 *out_order;     // count in bits 0..2, i-th base in bits 4+2i..5+2i
    u32 *in_deg;
    u32 *e_start, *e_end;
    u64 *e_len, *e_off;
    uint8_t *e_alive, *e_first;
    uint8_t *pool;
    u32 *nidx;          // open-addressed k-mer -> node id index
    u64 nidx_mask;
};

struct gk_graph {
    gk_ctx *ctx = nullptr;
    int k = 0, W = 1;
    GraphView v{};
    void *node_blob = nullptr, *edge_blob = nullptr;      // the node / edge arrays of `v` are carved out of these two allocations
    u64 node_cap = 0, edge_cap = 0, pool_cap = 0, pool_used = 0;
    u64 live_nodes = 0, live_edges = 0, live_len = 0;
    // wall time of the phases of gk_graph_build (every phase ends in a stream sync): classify, terminals -> nodes + edge
    // stubs, unitig measure (k_walk pass 0 / pointer jumping), pool reservation, unitig emit, node index + counts
    float build_ms[6] = {0, 0, 0, 0, 0, 0};
    u64 walked_bases = 0;        // bases emitted by the unitig construction (= total edge length at build time)
    int used_pj = 0;
    bool index_ready = false;    // the k-mer -> node id index (nidx) exists: it is built on the first point query / by-k-mer edit, not by the build
    int used_masks = 0;          // the classify came with the table (masks computed by the keys' owners, gk_dist_gather_map): no k_classify ran
    float mbt_ms = 0;            // building the minimizer-bucketed copy of the table, when the build used one ("graph_mbt")
    u64 mbt_slots = 0;
    bool keep_cycles = false;    // gk_graph_build_cycles: the build ends by appending the perfect cycles' anchors and arcs
    u64 cycle_stats[6] = {0, 0, 0, 0, 0, 0};
    // host snapshot of the edge arrays for the paired-end walks, valid while `epoch` (bumped by every edit) has not moved:
    // a stream of gk_graph_walk_pairs batches downloads the graph once
    u64 epoch = 0, snap_epoch = ~0ull;
    std::shared_ptr<void> snap;
};

__device__ __forceinline__ int order_count(u32 o) { return (int)(o & 7u); }
__device__ __forceinline__ int order_base(u32 o, int i) { return (int)((o >> (4 + 2 * i)) & 3u); }
__device__ __forceinline__ u32 order_append(u32 o, int b) {
    int c = order_count(o);
    return ((o & ~7u) | (u32)(c + 1)) | ((u32)b << (4 + 2 * c));
}
__device__ __forceinline__ u32 order_remove(u32 o, int b) {
    u32 r = 0;
    for (int i = 0; i < order_count(o); i++) if (order_base(o, i) != b) r = order_append(r, order_base(o, i));
    return r;
}
__device__ __forceinline__ u32 rev4(u32 m) { return ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3); }
__device__ __forceinline__ int pool_get(const uint8_t *pool, u64 off, u64 i) { return (pool[off + (i >> 2)] >> ((i & 3) * 2)) & 3; }
// Windows of the path start.seq ++ edge.seq without a per-base loop per window (gk_coverage.hip: windows of the graph's own k;
// gk_multik.hip: windows of a larger k).
// n <= 32 bases from base i0 of a 2-bit sequence (4 bases per byte, LSB first).  Touches only bytes that hold a base asked for.
__device__ __forceinline__ u64 pool_bits(const uint8_t *__restrict__ p, u64 i0, int n) {
    if (n <= 0) return 0;
    const u64 b0 = i0 >> 2;
    const int sh = (int)(i0 & 3) * 2, nb = (int)(((i0 + (u64)n + 3) >> 2) - b0);      // 1 .. 9 bytes
    u64 lo = 0, hi = 0;
    for (int j = 0; j < nb && j < 8; j++) lo |= (u64)p[b0 + j] << (8 * j);
    if (nb > 8) hi = p[b0 + 8];
    const u64 r = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return r & low_mask(2 * n);
}
// n <= 32 bases from base i0 of the path (the start node's k bases, then the edge's)
__device__ __forceinline__ u64 path_bits(Kmer<2> node, const uint8_t *__restrict__ seq, int k, u64 i0, int n) {
    if (i0 >= (u64)k) return pool_bits(seq, i0 - (u64)k, n);
    const int m = min(n, k - (int)i0);                       // of them from the node
    const u64 a = window_bits(node, 2 * (int)i0) & low_mask(2 * m);
    return m == n ? a : a | (pool_bits(seq, 0, n - m) << (2 * m));
}
// the window of kw bases at base d of the path of a node of k bases (kw = k: a k-mer of the graph; W = the words of kw)
template <int W> __device__ __forceinline__ Kmer<W> window_at(Kmer<2> node, const uint8_t *__restrict__ seq, int k, int kw, u64 d) {
    if constexpr (W == 1) return Kmer<1>{path_bits(node, seq, k, d, kw)};
    else return Kmer<2>{path_bits(node, seq, k, d, 32), path_bits(node, seq, k, d + 32, kw - 32)};
}
template <int W> __device__ __forceinline__ Kmer<W> node_kmer(const GraphView &g, u64 n);
template <> __device__ __forceinline__ Kmer<1> node_kmer<1>(const GraphView &g, u64 n) { return Kmer<1>{g.node_lo[n]}; }
template <> __device__ __forceinline__ Kmer<2> node_kmer<2>(const GraphView &g, u64 n) { return Kmer<2>{g.node_lo[n], g.node_hi[n]}; }
__device__ __forceinline__ u32 wave_incl_scan(u32 v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        u32 t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
// block-wide exclusive scan of small per-thread counts; *total = block sum
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32 *total, u32 *lds4) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
    for (int w = 0; w < BLOCK / 64; ++w) {
        u32 c = lds4[w];
        if (w < wave) base += c;
        tot += c;
    }
    *total = tot;
    return base + inc - v;
}
// reserve `v` units per thread from a global cursor with ONE atomic per block; returns this
// thread's first unit
__device__ __forceinline__ u64 block_reserve(u32 v, unsigned long long *cursor, u32 *lds4, unsigned long long *s_base) {
    u32 tot;
    u32 pre = block_excl_scan(v, &tot, lds4);
    if (threadIdx.x == 0) *s_base = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull;
    __syncthreads();
    u64 r = *s_base + pre;
    __syncthreads();
    return r;
}

// byte offsets of the sequences of the edges first_edge .. n_edges-1 in the pool (each edge starts on a byte boundary): base +
// what the cursor, which counts from 0, hands out.  The pointer-jumping build (all edges) and the perfect cycles' arcs.
static __global__ __launch_bounds__(BLOCK) void k_reserve_pool(GraphView g, u64 first_edge, u64 base, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 n = g.n_edges - first_edge;
    const u64 ngroups = (n + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 e = first_edge + grp * BLOCK + threadIdx.x;
        // per-block totals stay < 2^32 for edges up to 16M bases each; longer ones reserve alone
        u64 bytes = e < g.n_edges ? (g.e_len[e] + 3) / 4 : 0;
        u32 small = bytes < (1u << 22) ? (u32)bytes : 0u;
        u64 o = block_reserve(small, cursor, lds4, &s_base);
        if (e < g.n_edges) g.e_off[e] = base + (small == bytes ? o : atomicAdd(cursor, (unsigned long long)bytes));
    }
}

// MapGraph.removeEdge (Graph.scala:191-195) of a live edge, safe beside other lanes removing other edges: the start node's
// out-edge slot and insertion order, the edge itself, the end node's in-degree (k_remove_edges_by_id, k_tip_apply)
__device__ __forceinline__ void graph_remove_edge(const GraphView &g, u32 e) {
    const u32 v = g.e_start[e];
    const int b = g.e_first[e];
    if (atomicCAS(&g.out_edge[(u64)v * 4 + b], e, NONE) == e) {
        u32 seen = g.out_order[v], prev;
        do { prev = seen; seen = atomicCAS(&g.out_order[v], prev, order_remove(prev, b)); } while (seen != prev);
    }
    g.e_alive[e] = 0;
    atomicSub(&g.in_deg[g.e_end[e]], 1u);
}

// The count of one window.  Its hash-rule orientation (canonical, gk_device.h) is where a table filled by the rule holds it.
// Where the rule cannot tell the strands apart (equal hashes), and in a table that took verbatim keys (Table::both, as
// k_classify), the other orientation may be stored too: the two counts add up.  A palindrome is one key.
template <int W, class S>
__device__ __forceinline__ u32 window_count(const Table<W, S> &t, Kmer<W> x, Kmer<W> rc) {
    const i32 hx = ref_hash(x), hr = ref_hash(rc);
    const bool fwd = hx < hr;
    i64 s = table_find(t, fwd ? x : rc);
    u32 c = s >= 0 ? slot_count(&t.slots[s]) : 0u;
    if ((t.both || hx == hr) && !(x == rc)) {
        s = table_find(t, fwd ? rc : x);
        if (s >= 0) c += slot_count(&t.slots[s]);
    }
    return c;
}

// host-side helpers of gk_graph_ops.hip that the build, the paired-end stage, the tip rule and the graph file use
int check_graph(const gk_graph *g);
int ggrid(const gk_ctx *ctx, u64 items);                  // grid of BLOCK-thread workgroups for `items` work items
int graph_refresh_counts(gk_graph *g);                    // live nodes / edges / bases; bumps the graph's epoch
int graph_build_index(gk_graph *g);                       // k-mer -> node id index
inline int graph_ensure_index(gk_graph *g) { return g->index_ready ? 0 : graph_build_index(g); }   // before any kernel that calls node_find / reads nidx
int graph_grow_nodes(gk_graph *g, u64 new_cap);
int graph_grow_edges(gk_graph *g, u64 new_n);               // contents kept; n_edges is the caller's to raise
// the node / edge arrays of a graph without any (ids 0..n-1, none alive, out_edge NONE, out_order / in_deg 0): the build and gk_graph_load
int graph_alloc_nodes(gk_graph *g, u64 n);
int graph_alloc_edges(gk_graph *g, u64 n);
// gk_graph.hip: the pointer-jumping build's slot -> rank structure of a map's table, copied to the host (gk_test_slot_ranks)
int graph_slot_ranks(gk_map *m, uint64_t *masks, uint64_t *bases, uint64_t cap_blocks, uint64_t *nblk, uint64_t *total);
// Node.inEdgeIds as CSR by end node of the graph as it is now: (*off)[v] .. (*off)[v+1] index *list; both live in `tmp`.
// Stream-ordered, no synchronisation; `who` names the entry point in the error text.  (Not exported, like DevScratch.)
__attribute__((visibility("hidden"))) int graph_in_lists(gk_graph *g, DevScratch &tmp, const char *who, unsigned long long **off, u32 **list);

// Perfect cycles (gk_cycles.hip; the rule is in include/genome_amd.h, "perfect cycles").  The hot step at both levels is the minimum
// over each cycle of a functional graph, by pointer doubling on ONE packed word per element: bits 0..31 the pointer, bits 32..63
// the index of the smallest key met so far (CY_LEAVES: the chain ends outside the set), CY_UNREG: not in the set.
static constexpr u64 CY_UNREG = ~0ull;
static constexpr u32 CY_LEAVES = 0xFFFFFFFFu;
// st[0..n) as the caller initialised it — a cycle candidate u: succ(u) | u << 32; an element whose successor is outside the set:
// u | CY_LEAVES << 32 (a fixed point); anything else CY_UNREG.  On return every element of a cycle holds the index of its cycle's
// smallest key (the first one met going forward on a tie), every other candidate CY_LEAVES.  *rounds = ceil(log2 n).  No sync.
__attribute__((visibility("hidden"))) int cycles_min(gk_ctx *ctx, DevScratch &tmp, u64 *st, u64 n, const u64 *klo, const u64 *khi, u64 *rounds);
// the members of the k-mer table's perfect cycles, dense (gk_graph.hip fills it): successor, anchor key, the base that follows
// (bits 0..1) | the k-mer is not its own anchor key << 2 | palindrome << 3, and the member that is the reverse complement
struct CycleMembers { u64 n; u32 *succ; u64 *klo, *khi; uint8_t *meta; u32 *twin; };
__attribute__((visibility("hidden"))) int graph_append_cycles(gk_graph *g, DevScratch &tmp, const CycleMembers &cm, uint64_t *stats6);
// the keeping simplify's part between k_node_class and k_chain: class 2 -> 0, the anchors of all-interior cycles -> 0
__attribute__((visibility("hidden"))) int cycles_keep_classes(gk_graph *g, DevScratch &tmp, uint8_t *cls, uint64_t *stats4);

// Edge coverage from a count table (gk_coverage.hip), for the callers that decide something from it (tips, bubbles) or print it
// (gk_contigs.hip).  Per-edge results are indexed by edge id and live in the caller's `tmp`; coverage_pass writes them for every
// live edge (`want` == nullptr) or for the live edges marked in `want`, stream-ordered, without a sync.  check_counts: the table
// is of this graph's k and context (GK_E_INVALID otherwise) and its slots are materialised.
struct EdgeCov { u64 *sum; u32 *mn, *mx, *miss; };
int check_counts(const gk_graph *g, gk_map *counts, const char *who);
__attribute__((visibility("hidden"))) int coverage_pass(gk_graph *g, gk_map *counts, DevScratch &tmp, const uint8_t *want, EdgeCov *cov);

// The rows of a scaffold plan (gk_scaffolds.hip) as the judge reads them (gk_place.hip): the plan's own device arrays.  Segment i of
// record r (rec_seg[r] <= i < rec_seg[r + 1]) is an N run (seg_edge == NONE) or a piece of P(seg_edge[i]) that starts at base
// seg_start[i] of the record and leaves out the first seg_skip[i] bases of the path.  rows = the edge segments.
struct ScafRows {
    gk_ctx *ctx;
    gk_graph *g;
    u64 epoch, records, chain_recs, segs, rows;
    const unsigned long long *rec_seg;
    const u32 *seg_edge, *seg_start;
    const uint8_t *seg_skip;
};
__attribute__((visibility("hidden"))) void scaffolds_rows(const gk_scaffolds *s, ScafRows *out);

// The front end every paired-end entry point shares (gk_pairs.hip; GraphSimplifier.scala:213-217): the pairs whose mates both
// hold k bases are cut from the `.bin` stream (a fixed-stride stream on the device by k_pair_keys, a ragged one on the host),
// their four getAll run as ONE batch whose results stay in HBM as CSR, and k_check_positions is queued behind it.  Key 4p + q
// of cut pair p: q = 0 p1.take(k), 1 p2.take(k).revComplement, 2 p2.take(k), 3 p1.take(k).revComplement — orientation o of
// the batch reads the runs 2o (P1) and 2o + 1 (P2).  Everything lives in `tmp`.  pairs_front returns with the lookups done
// (t_keys / t_lookup: monotonic ms at the end of the cut and of the batch) and the check still in flight, so that a caller can
// queue more work before pairs_front_checked waits for it: GK_E_STATE if a position names nothing live in this graph.
struct PairFront {
    u64 nq = 0;                                  // keys cut: 4 per pair that was not skipped (0: nothing else is set)
    unsigned long long *d_off = nullptr;         // [nq + 1]
    u64 *d_vals = nullptr;                       // [total]
    unsigned long long total = 0;
    u32 *d_flag = nullptr;                       // [0] raised by k_check_positions, [1] zero, the caller's
    double t_keys = 0, t_lookup = 0;
};
double pairs_now();
__attribute__((visibility("hidden"))) int pairs_front(gk_graph *g, gk_vmap *positions, const uint8_t *bin, size_t nbytes, uint64_t npairs, const char *who,
                                                      DevScratch &tmp, PairFront &F);
__attribute__((visibility("hidden"))) int pairs_front_checked(gk_ctx *ctx, const PairFront &F, const char *who);
