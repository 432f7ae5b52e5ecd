// gk_thread_common.h — what the two kernels that thread single reads through the graph share: k_thread_reads (gk_thread.hip: the
// crossings of one node) and k_thread_spans (gk_spans.hip: the crossings at both ends of one edge).  The lookup of a window in
// the position map with its untrusted-position check, a strand's bases and the window classes of gk_graph_thread_reads' rule
// (include/genome_amd.h).  Device code only.
#pragma once

#include "gk_graph.h"
#include "gk_vmap_probe.h"

namespace gk {
void vmap_table(const gk_vmap *m, void **slots, uint32_t *nb2, uint32_t *lnb1);
}

constexpr int TH_MAXW = 256;                   // windows of a record: at most 255 - k + 1 <= 254
// what a window's lookup left, beside a position: no valid GraphPosition has these bit patterns (an edge id of 2^31 - 1)
constexpr u64 PV_NONE = ~0ull, PV_MANY = ~0ull - 1;
enum { TC_OFF = 0, TC_REPEATED = 1, TC_ON_EDGE = 2, TC_BROKEN = 3, TC_CROSSING = 4 };

// the position Edge(e, d) as the position map holds it
__device__ __forceinline__ u64 thread_edge_pos(u32 e, u64 d) { return (1ull << 63) | ((u64)e << 32) | d; }

// getAll(w) reduced to {none, many, the position}.  The one position is untrusted (k_check_positions' test, gk_pairs.hip): one
// that names nothing live in this graph raises *bad and counts as none, so that nothing below indexes the graph with it.
template <int W>
__device__ __forceinline__ u64 thread_lookup(const Table<W> &pm, const GraphView &g, Kmer<W> x, u32 *bad) {
    u64 v = 0;
    const u32 n = vmap_count_one(pm, x, &v);
    if (n == 0) return PV_NONE;
    if (n > 1) return PV_MANY;
    const u32 id = GK_POS_ID(v);
    const bool ok = GK_POS_IS_EDGE(v) ? (id < g.n_edges && g.e_alive[id] && (u64)GK_POS_DIST(v) < g.e_len[id])
                                      : ((v >> 32) == 0 && id < g.n_nodes && g.node_alive[id]);
    if (!ok) { *bad = 1u; return PV_NONE; }
    return v;
}

// base p of strand s of the record at tile byte `ro` (s = 1: the reverse complement; complement is ^ 3)
__device__ __forceinline__ int strand_base(const uint8_t *tb, u32 ro, int len, int s, int p) {
    const int q = s ? len - 1 - p : p;
    const int b = (tb[ro + 1 + (q >> 2)] >> ((q & 3) * 2)) & 3;
    return s ? b ^ 3 : b;
}

// The class of inner window i of strand s (gk_graph_thread_reads' table, rows 1..5), from the positions pos[0 .. n) of the strand's
// windows; a crossing leaves its (in-edge << 32 | out-edge) in *key.
__device__ __forceinline__ int thread_window_class(const GraphView &g, const uint8_t *tb, u32 ro, int len, int k, int s, int i, const u64 *pos, u64 *key) {
    const u64 P = pos[i];
    if (P == PV_NONE) return TC_OFF;
    if (P == PV_MANY) return TC_REPEATED;
    if (GK_POS_IS_EDGE(P)) return TC_ON_EDGE;
    const u32 v = (u32)P;
    const u64 nx = pos[i + 1], pv = pos[i - 1];
    // exit: the out-edge of v by the base behind the window, and the next window one step along it
    const u32 f = g.out_edge[(u64)v * 4 + strand_base(tb, ro, len, s, i + k)];
    bool ok = f != NONE && g.e_alive[f] != 0 && nx < PV_MANY;
    if (ok) ok = nx == (g.e_len[f] > 1 ? thread_edge_pos(f, 1) : (u64)g.e_end[f]);
    // entry: the previous window one step before the end of an in-edge of v, or the start node of one of length 1
    u32 e = NONE;
    if (ok && pv < PV_MANY) {
        if (GK_POS_IS_EDGE(pv)) {
            const u32 pe = GK_POS_ID(pv);
            if ((u64)GK_POS_DIST(pv) + 1 == g.e_len[pe] && g.e_end[pe] == v) e = pe;
        } else {
            const u32 pe = g.out_edge[(u64)(u32)pv * 4 + strand_base(tb, ro, len, s, i + k - 1)];
            if (pe != NONE && g.e_alive[pe] != 0 && g.e_len[pe] == 1 && g.e_end[pe] == v) e = pe;
        }
    }
    if (e == NONE) return TC_BROKEN;
    *key = ((u64)e << 32) | f;
    return TC_CROSSING;
}
