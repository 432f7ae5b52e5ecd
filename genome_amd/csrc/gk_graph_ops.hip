// gk_graph_ops.hip — everything that works on a built de Bruijn graph, as HIP kernels (gfx950): structural simplification,
// components, checksum, exports, the position map, point queries and edits, contig statistics, and the node / edge arrays
// themselves.  Nothing here touches a k-mer table (the build from one is gk_graph.hip); the layout is described there.
//
// Reference path replaced (S/ = the reference's src/main/scala/ru/ifmo/genome/):
//   MapGraph.addNode/addEdge/removeEdge  S/data/graph/Graph.scala:172-195   node/edge arrays below
//   MapGraph.simplifyGraph               :211-230            k_node_class, k_chain_*, k_simplify_finish
//   Graph.removeBubbles                  :125-149            k_bubbles
//   Graph.components + retain            :54-72, :161-165    k_cc_*, k_retain
//   Graph.getGraphMap                    :90-119             k_pos_*
//
// Where the reference's result depends on node iteration order (out-edge insertion order after
// simplifyGraph), this file reproduces "ascending k-mer order", the oracle's deterministic choice.
#include <algorithm>
#include <string>

#include "gk_graph.h"
#include "gk_scan.h"

__device__ __forceinline__ bool node_less(const GraphView &g, u32 a, u32 b) {   // unsigned (hi, lo) order
    u64 ah = g.node_hi[a], bh = g.node_hi[b];
    return ah != bh ? ah < bh : g.node_lo[a] < g.node_lo[b];
}

// k-mer -> node id index (open addressing over node ids), for point queries on the graph
template <int W> __global__ __launch_bounds__(BLOCK) void k_build_nidx(GraphView g) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        if (!g.node_alive[n]) continue;
        u64 i = slot_hash(node_kmer<W>(g, n)) & g.nidx_mask;
        while (atomicCAS(&g.nidx[i], NONE, (u32)n) != NONE) i = (i + 1) & g.nidx_mask;
    }
}
// The live node with this k-mer.  After a node split several nodes share a sequence, and dead ones stay in the index: the live
// one with the smallest id is the node a k-mer names (gk_graph_node_lookup's rule), whatever order the index took them in —
// k_build_nidx inserts in the order its lanes arrive, k_nidx_insert behind what is there.
template <int W> __device__ __forceinline__ u32 node_find(const GraphView &g, Kmer<W> x) {
    u32 best = NONE;
    u64 i = slot_hash(x) & g.nidx_mask;
    for (u64 p = 0; p <= g.nidx_mask; p++) {
        const u32 n = g.nidx[i];
        if (n == NONE) break;
        if (g.node_alive[n] && node_kmer<W>(g, n) == x && n < best) best = n;
        i = (i + 1) & g.nidx_mask;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------
// simplifyGraph (Graph.scala:211-230)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_in_single(GraphView g, u32 *in_single) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK)
        if (g.e_alive[e] && g.in_deg[g.e_end[e]] == 1) in_single[g.e_end[e]] = (u32)e;
}
// 0 keep; 1 interior (1 in, 1 out, e1 != e2 : merged away, :222-226); 2 self-loop (e1 == e2, :220-221);
// 3 isolated (:215-216)
__global__ __launch_bounds__(BLOCK) void k_node_class(GraphView g, const u32 *in_single, uint8_t *cls) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        uint8_t c = 0;
        if (g.node_alive[n]) {
            const u32 o = g.out_order[n];
            const int nout = order_count(o), nin = (int)g.in_deg[n];
            if (nin == 0 && nout == 0) c = 3;
            else if (nin == 1 && nout == 1) c = in_single[n] == g.out_edge[n * 4 + order_base(o, 0)] ? 2 : 1;
        }
        cls[n] = c;
    }
}
// A chain = a live edge that leaves a kept node and enters an interior node, followed through
// every interior node to the first non-interior end.  Sequential simplifyGraph produces exactly
// one merged edge per chain (e1.seq ++ e2.seq, repeatedly) whatever the node order; chains of
// interior nodes only (perfect cycles) vanish.  pass 0 counts, pass 1 writes.
// A piece of LONG_PIECE bases and more is not copied base by base by the chain's lane (a contig graph has edges of hundreds of
// kilobases: 4 Mbp of merges took 109 ms that way) but listed for k_copy_long, which copies it 16 bases per thread and ORs it
// into the zeroed output; the lane ORs the bytes it shares with such a piece instead of storing them.
static constexpr u64 LONG_PIECE = 1024;
struct LongPiece { u64 src_off, dst_off, dst_base, len; };     // source byte offset, chain's byte offset, base position inside the chain, bases
__device__ __forceinline__ void pool_or(uint8_t *pool, u64 byte, u32 val) {
    atomicOr(reinterpret_cast<u32 *>(pool + (byte & ~3ull)), val << (8u * (u32)(byte & 3ull)));
}
__global__ __launch_bounds__(BLOCK) void k_copy_long(GraphView g, const LongPiece *pieces) {
    const LongPiece p = pieces[blockIdx.x];
    for (u64 c = threadIdx.x; c * 16 < p.len; c += BLOCK) {
        const u64 first = c * 16;
        const u32 n = (u32)min((u64)16, p.len - first);
        // 16 bases = 32 bits of the source starting at base `first` (any 2-bit alignment): five bytes cover them
        const u64 sb = p.src_off + (first >> 2);
        u64 five = 0;
        for (u32 q = 0; q < 5 && (first >> 2) + q < (p.len + 3) / 4; q++) five |= (u64)g.pool[sb + q] << (8 * q);
        u32 bits = (u32)(five >> ((first & 3) * 2));
        if (n < 16) bits &= (1u << (2 * n)) - 1u;
        const u64 bitpos = p.dst_off * 8 + (p.dst_base + first) * 2;            // in the pool
        u32 *w = reinterpret_cast<u32 *>(g.pool) + (bitpos >> 5);
        const u32 sh = (u32)(bitpos & 31);
        atomicOr(w, bits << sh);
        if (sh && (bits >> (32 - sh))) atomicOr(w + 1, bits >> (32 - sh));
    }
}
__global__ __launch_bounds__(BLOCK) void k_chain(GraphView g, const uint8_t *cls, int pass, u64 old_edges, u64 old_pool,
                                                 unsigned long long *counters /* [0]=chains [1]=bytes [2]=long pieces */, u32 *merged_key,
                                                 LongPiece *long_pieces) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < old_edges; e += (u64)gridDim.x * BLOCK) {
        if (!g.e_alive[e]) continue;
        const u32 s = g.e_start[e];
        if (cls[s] != 0 || cls[g.e_end[e]] != 1) continue;
        u64 total = 0;
        u32 cur = (u32)e, maxn = NONE, nlong = 0;
        for (u64 guard = 0; guard <= old_edges; guard++) {
            total += g.e_len[cur];
            if (g.e_len[cur] >= LONG_PIECE) nlong++;
            const u32 v = g.e_end[cur];
            if (cls[v] != 1) break;
            if (maxn == NONE || node_less(g, maxn, v)) maxn = v;
            cur = g.out_edge[(u64)v * 4 + order_base(g.out_order[v], 0)];
        }
        const u64 bytes = (total + 3) / 4;
        if (pass == 0) {
            atomicAdd(&counters[0], 1ull);
            atomicAdd(&counters[1], (unsigned long long)bytes);
            if (nlong) atomicAdd(&counters[2], (unsigned long long)nlong);
            continue;
        }
        const u64 id = old_edges + atomicAdd(&counters[0], 1ull);
        const u64 off = old_pool + atomicAdd(&counters[1], (unsigned long long)bytes);
        // e1.seq ++ e2.seq ++ ...  (Graph.scala:225)
        u64 w = 0;
        u32 acc = 0;
        bool shared = false;                           // the byte being assembled also holds bases of a long piece
        cur = (u32)e;
        for (u64 guard = 0; guard <= old_edges; guard++) {
            const u64 so = g.e_off[cur], sl = g.e_len[cur];
            if (sl >= LONG_PIECE) {
                if (w & 3) { pool_or(g.pool, off + (w >> 2), acc); acc = 0; }      // the piece starts inside this byte
                long_pieces[atomicAdd(&counters[2], 1ull)] = LongPiece{so, off, w, sl};
                w += sl;
                shared = (w & 3) != 0;                                              // ... and ends inside that one
            } else {
                for (u64 i = 0; i < sl; i++) {
                    acc |= (u32)pool_get(g.pool, so, i) << ((w & 3) * 2);
                    if ((w & 3) == 3) {
                        if (shared) pool_or(g.pool, off + (w >> 2), acc); else g.pool[off + (w >> 2)] = (uint8_t)acc;
                        acc = 0; shared = false;
                    }
                    w++;
                }
            }
            g.e_alive[cur] = 0;                        // removeEdge(e1); removeEdge(e2)  :223-224
            const u32 v = g.e_end[cur];
            if (cls[v] != 1) break;
            cur = g.out_edge[(u64)v * 4 + order_base(g.out_order[v], 0)];
        }
        if (w & 3) { if (shared) pool_or(g.pool, off + (w >> 2), acc); else g.pool[off + (w >> 2)] = (uint8_t)acc; }
        g.e_start[id] = s;                             // addEdge(e1.start, e2.end, ...)   :225
        g.e_end[id] = g.e_end[cur];
        g.e_len[id] = total;
        g.e_off[id] = off;
        g.e_first[id] = g.e_first[e];
        g.e_alive[id] = 1;
        g.out_edge[(u64)s * 4 + g.e_first[e]] = (u32)id;
        merged_key[(u64)s * 4 + g.e_first[e]] = maxn;
    }
}
// Remove interior / self-loop / isolated nodes and whatever edges still hang off them (self-loops,
// perfect cycles), and replay the out-edge insertion order at kept nodes: every merge step is
// `outEdgeIds -= b` then `+= b` (removeEdge :192, addEdge :180), i.e. b moves to the end, and the
// last step of a chain happens when its largest interior node (ascending k-mer order) is visited.
__global__ __launch_bounds__(BLOCK) void k_simplify_finish(GraphView g, const uint8_t *cls, const u32 *merged_key) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        if (!g.node_alive[n]) continue;
        const u32 o = g.out_order[n];
        if (cls[n] != 0) {
            for (int i = 0; i < order_count(o); i++) {
                const int b = order_base(o, i);
                const u32 e = g.out_edge[n * 4 + b];
                if (e != NONE) g.e_alive[e] = 0;
                g.out_edge[n * 4 + b] = NONE;
            }
            g.out_order[n] = 0;
            g.in_deg[n] = 0;
            g.node_alive[n] = 0;                       // removeNode :216,:227
            continue;
        }
        u32 r = 0;
        int mb[4], nm = 0;
        for (int i = 0; i < order_count(o); i++) {
            const int b = order_base(o, i);
            if (merged_key[n * 4 + b] == NONE) r = order_append(r, b);
            else mb[nm++] = b;
        }
        for (int i = 1; i < nm; i++)                   // insertion sort of <= 4 entries by chain key
            for (int j = i; j > 0 && node_less(g, merged_key[n * 4 + mb[j]], merged_key[n * 4 + mb[j - 1]]); j--) {
                int tmp = mb[j]; mb[j] = mb[j - 1]; mb[j - 1] = tmp;
            }
        for (int i = 0; i < nm; i++) r = order_append(r, mb[i]);
        g.out_order[n] = r;
    }
}

// Graph.removeBubbles (Graph.scala:125-149) — per node, on the out-edges in insertion order
__global__ __launch_bounds__(BLOCK) void k_bubbles(GraphView g) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        if (!g.node_alive[n]) continue;
        const u32 o = g.out_order[n];
        const int cnt = order_count(o);
        if (cnt < 2) continue;
        u32 out[4];
        bool rem[4] = {false, false, false, false};
        for (int i = 0; i < cnt; i++) out[i] = g.out_edge[n * 4 + order_base(o, i)];
        for (int i = 0; i < cnt; i++) {
            if (rem[i]) continue;                                      // `if !toRemove(out(i))`  :142
            for (int j = i + 1; j < cnt; j++) {
                const u64 la = g.e_len[out[i]], lb = g.e_len[out[j]];
                const u64 d = la > lb ? la - lb : lb - la, mx = la > lb ? la : lb;
                if (g.e_end[out[i]] == g.e_end[out[j]] && d * 5 < mx) rem[j] = true;   // similar :121-123
            }
        }
        u32 r = 0;
        for (int i = 0; i < cnt; i++) {
            const int b = order_base(o, i);
            if (rem[i]) {                                              // removeEdge :191-195
                g.e_alive[out[i]] = 0;
                atomicSub(&g.in_deg[g.e_end[out[i]]], 1u);
                g.out_edge[n * 4 + b] = NONE;
            } else {
                r = order_append(r, b);
            }
        }
        g.out_order[n] = r;
    }
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_remove_edges(GraphView g, const u64 *lo, const u64 *hi, const uint8_t *base, u64 n,
                                                        unsigned long long *removed) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Kmer<W> x;
        if constexpr (W == 1) x = Kmer<1>{lo[i]};
        else x = Kmer<2>{lo[i], hi[i]};
        const u32 v = node_find<W>(g, x);
        const int b = base[i] & 3;
        if (v == NONE || !g.node_alive[v]) continue;
        const u32 e = atomicExch(&g.out_edge[(u64)v * 4 + b], NONE);
        if (e == NONE) continue;
        g.e_alive[e] = 0;
        atomicSub(&g.in_deg[g.e_end[e]], 1u);
        u32 old = g.out_order[v], seen;
        do {
            seen = old;
            old = atomicCAS(&g.out_order[v], seen, order_remove(seen, b));
        } while (old != seen);
        atomicAdd(removed, 1ull);
    }
}

__global__ __launch_bounds__(BLOCK) void k_count_live(GraphView g, unsigned long long *out /* nodes, edges, len */) {
    __shared__ unsigned long long s[3];
    if (threadIdx.x < 3) s[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a = 0, b = 0, c = 0;
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    for (u64 n = tid; n < g.n_nodes; n += stride) a += g.node_alive[n];
    for (u64 e = tid; e < g.n_edges; e += stride) if (g.e_alive[e]) { b++; c += g.e_len[e]; }
    if (a) atomicAdd(&s[0], a);
    if (b) atomicAdd(&s[1], b);
    if (c) atomicAdd(&s[2], c);
    __syncthreads();
    if (threadIdx.x < 3 && s[threadIdx.x]) atomicAdd(&out[threadIdx.x], s[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// components (Graph.scala:54-72) by min-label hooking + pointer jumping; retain (:161-165)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 cc_root(const u32 *parent, u32 v) {
    u32 p = parent[v];
    while (p != v) { v = p; p = parent[v]; }
    return v;
}
__global__ __launch_bounds__(BLOCK) void k_cc_init(GraphView g, u32 *parent) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) parent[n] = (u32)n;
}
// One pass over the edges: a lock-free union (the larger root is hooked under the smaller by a CAS on the root's own word; a
// failed CAS hands back the word's true value and the walk continues from there) with path halving on the way up.  Pointers
// only ever go to smaller ids, so there are no cycles, a stale read is an older ancestor (a longer walk, never a wrong one),
// and the root a component ends with is its smallest node id — the label the round-2 form (min-label hooking + full
// compression, repeated until nothing moved: 5-7 rounds of two kernels and a host round trip each, 7 ms at C3) converged to.
// What bounds the pass is not its reads (12.8e9 requests/s by PMC, a quarter of the random-read ceiling) but same-address
// atomics: when two large trees meet, thousands of edges want the same root's word at once, and a CAS that fails costs what one
// that succeeds does (~88 per microsecond on one address, chip-wide).  So a device-scope LOAD looks first and the CAS is only
// sent when the word still names a root: k_cc_link 5.6 -> ~2 ms, retainLargest at C3 8.4 -> 4.7 ms
// (profiles/r03/ab_components_find_variants.txt).
// V (A/B, "cc_find"): 3 = path halving, every hop writes, and the link looks before its CAS (the default); 0 = the same without
// the look; 1 = nothing is written on the way; 2 = only the node the find started from is pointed at the root it found
template <int V> __device__ __forceinline__ u32 cc_find(u32 *parent, u32 v) {
    const u32 v0 = v;
    u32 p = parent[v];
    while (p != v) {
        const u32 gp = parent[p];
        if (gp == p) { v = p; break; }
        if (V == 0 || V == 3) parent[v] = gp;     // (v is not a root and never becomes one again: no CAS targets this word)
        v = gp; p = parent[v];
    }
    if (V == 2 && v != v0 && parent[v0] != v) parent[v0] = v;
    return v;
}
template <int V> __global__ __launch_bounds__(BLOCK) void k_cc_link(GraphView g, u32 *parent) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        if (!g.e_alive[e]) continue;
        u32 ru = cc_find<V>(parent, g.e_start[e]), rv = cc_find<V>(parent, g.e_end[e]);
        while (ru != rv) {
            if (ru < rv) { const u32 x = ru; ru = rv; rv = x; }
            if (V == 3) {
                // look before the CAS (a device-scope load: another XCD's hook is visible): when two large trees meet, thousands of
                // edges want the same root's word, and a failed same-address CAS costs what a successful one does
                const u32 cur = __hip_atomic_load(&parent[ru], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur != ru) { ru = cc_find<V>(parent, cur); rv = cc_find<V>(parent, rv); continue; }
            }
            const u32 old = atomicCAS(&parent[ru], ru, rv);
            if (old == ru) break;
            ru = cc_find<V>(parent, old);
            rv = cc_find<V>(parent, rv);
        }
    }
}
// Component sizes and summed edge lengths.  A giant component means millions of increments of ONE counter, and same-address
// atomics retire at ~88 per microsecond chip-wide (143 ms of the 169 ms retain step at C3 in round 1; 7.7-10 ms in round 2
// with a per-wave carry: still 4.4e5 atomics on the giant root).  Now every WORKGROUP keeps a (root -> partial sum) table in
// LDS for its whole share of the nodes / edges: lanes of a wave that share a root are combined first (ballot), the wave adds
// its partial to the LDS table, and the table goes out once, at the end — one global atomic per (workgroup, root): 2048 on the
// giant root.  A root that finds the LDS table full goes straight to memory (distinct small components: no contention there).
static constexpr u32 CC_TAB = 1024;
template <class T> struct CcTable {
    u32 root[CC_TAB];
    T sum[CC_TAB];
    __device__ __forceinline__ void clear() { for (u32 i = threadIdx.x; i < CC_TAB; i += BLOCK) { root[i] = NONE; sum[i] = 0; } }
    // one lane per call and root
    __device__ __forceinline__ void add(u32 r, T v, T *global) {
        u32 h = hash32(r) & (CC_TAB - 1);
        for (u32 n = 0; n < 16; n++) {
            u32 cur = root[h];
            if (cur == NONE) cur = atomicCAS(&root[h], NONE, r);
            if (cur == NONE || cur == r) { atomicAdd(&sum[h], v); return; }
            h = (h + 1) & (CC_TAB - 1);
        }
        atomicAdd(&global[r], v);
    }
    __device__ __forceinline__ void flush(T *global) {
        for (u32 i = threadIdx.x; i < CC_TAB; i += BLOCK) if (root[i] != NONE && sum[i]) atomicAdd(&global[root[i]], sum[i]);
    }
};
// (also the one compression pass after k_cc_link: every live node's word becomes its root — a walker that passes through a
// word already compressed lands on the same root)
__global__ __launch_bounds__(BLOCK) void k_cc_sizes(GraphView g, u32 *parent, u32 *size, unsigned long long *ncomp) {
    __shared__ CcTable<u32> tab;
    __shared__ u32 s_roots;
    if (threadIdx.x == 0) s_roots = 0;
    tab.clear();
    __syncthreads();
    const int lane = threadIdx.x & 63;
    u32 nroots = 0;
    for (u64 n0 = (u64)blockIdx.x * BLOCK + (threadIdx.x & ~63u); n0 < g.n_nodes; n0 += (u64)gridDim.x * BLOCK) {   // wave-uniform trip count
        const u64 n = n0 + lane;
        const bool active = n < g.n_nodes && g.node_alive[n];
        u32 root = 0xffffffffu;
        if (active) { root = cc_root(parent, (u32)n); parent[n] = root; }
        unsigned long long todo = __ballot(active);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const u32 lr = __shfl(root, leader);
            const unsigned long long same = __ballot(active && root == lr);
            if (lane == leader) tab.add(lr, (u32)__popcll(same), size);
            todo &= ~same;
        }
        nroots += (u32)__popcll(__ballot(active && root == (u32)n));
    }
    if (lane == 0 && nroots) atomicAdd(&s_roots, nroots);
    __syncthreads();
    tab.flush(size);
    if (threadIdx.x == 0 && s_roots) atomicAdd(ncomp, (unsigned long long)s_roots);
}
// summed out-edge length per component (GraphBuilder.scala:44-46: comp.flatMap(_.outEdges.values).map(_.seq.size).sum): every
// live edge adds its length to the root of its start node
__global__ __launch_bounds__(BLOCK) void k_cc_edge_len(GraphView g, const u32 *parent, unsigned long long *len) {
    __shared__ CcTable<unsigned long long> tab;
    tab.clear();
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (u64 e0 = (u64)blockIdx.x * BLOCK + (threadIdx.x & ~63u); e0 < g.n_edges; e0 += (u64)gridDim.x * BLOCK) {
        const u64 e = e0 + lane;
        const bool active = e < g.n_edges && g.e_alive[e];
        const u32 root = active ? parent[g.e_start[e]] : 0xffffffffu;
        const unsigned long long mylen = active ? g.e_len[e] : 0ull;
        unsigned long long todo = __ballot(active);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const u32 lr = __shfl(root, leader);
            const bool mine = active && root == lr;
            const unsigned long long same = __ballot(mine);
            unsigned long long part = mine ? mylen : 0ull;
            for (int d = 32; d; d >>= 1) part += __shfl_down(part, d);
            const unsigned long long tot = __shfl(part, 0);           // (lane 0 holds the wave's sum of this root's lengths)
            if (lane == leader) tab.add(lr, tot, len);
            todo &= ~same;
        }
    }
    __syncthreads();
    tab.flush(len);
}
// one (node count, summed out-edge length) pair per component, in root order
__global__ __launch_bounds__(BLOCK) void k_cc_collect(GraphView g, const u32 *parent, const u32 *size, const unsigned long long *len,
                                                      u32 *out_nodes, unsigned long long *out_len, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_nodes + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 n = grp * BLOCK + threadIdx.x;
        const bool root = n < g.n_nodes && g.node_alive[n] && parent[n] == (u32)n;
        const u64 o = block_reserve(root ? 1u : 0u, cursor, lds4, &s_base);
        if (root) { out_nodes[o] = size[n]; out_len[o] = len[n]; }
    }
}
// order-independent checksums of the canonical serialisation: nodes = k-mers; edges = (start k-mer,
// end k-mer, length, every base) — ids, array order and pool offsets do not enter
__global__ __launch_bounds__(BLOCK) void k_graph_checksum(GraphView g, unsigned long long *out /* nodes, edges */) {
    u64 cn = 0, ce = 0;
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    for (u64 n = tid; n < g.n_nodes; n += stride)
        if (g.node_alive[n]) cn += mix64(g.node_lo[n] ^ mix64(g.node_hi[n] ^ 0x13198a2e03707344ULL));
    for (u64 e = tid; e < g.n_edges; e += stride) {
        if (!g.e_alive[e]) continue;
        const u32 s = g.e_start[e], t = g.e_end[e];
        u64 h = mix64(g.node_lo[s] ^ mix64(g.node_hi[s] ^ 1)) + 3 * mix64(g.node_lo[t] ^ mix64(g.node_hi[t] ^ 2)) + 5 * mix64(g.e_len[e]);
        const u64 off = g.e_off[e], len = g.e_len[e], nbytes = (len + 3) / 4;
        for (u64 i = 0; i < nbytes; i++) {
            u32 b = g.pool[off + i];
            if (i == nbytes - 1 && (len & 3)) b &= (1u << ((len & 3) * 2)) - 1u;      // bits after the last base are not content
            h = mix64(h ^ (b + 0x9e3779b97f4a7c15ULL * (i + 1)));
        }
        ce += h;
    }
    for (int d = 32; d; d >>= 1) { cn += __shfl_down(cn, d); ce += __shfl_down(ce, d); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], cn); atomicAdd(&out[1], ce); }
}
__global__ __launch_bounds__(BLOCK) void k_cc_max(GraphView g, const u32 *size, u32 *best) {
    u32 m = 0;
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK)
        if (g.node_alive[n]) m = max(m, size[n]);
    for (int d = 32; d; d >>= 1) m = max(m, (u32)__shfl_down(m, d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(best, m);
}
// among the components of maximal size pick the one holding the smallest k-mer: stage 0 min hi,
// stage 1 min lo among those, stage 2 record its root (one atomic per wave, see k_cc_sizes)
__global__ __launch_bounds__(BLOCK) void k_cc_pick(GraphView g, const u32 *parent, const u32 *size, const u32 *best_p, int stage,
                                                   unsigned long long *mins /* hi, lo */, u32 *winner) {
    unsigned long long m = ~0ull;
    const u32 best = *best_p;                       // (k_cc_max's result: stays on the device)
    const unsigned long long min_hi = stage >= 1 ? mins[0] : 0ull, min_lo = stage == 2 ? mins[1] : 0ull;
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        if (!g.node_alive[n] || size[parent[n]] != best) continue;
        if (stage == 0) m = min(m, (unsigned long long)g.node_hi[n]);
        else if (stage == 1) { if (g.node_hi[n] == min_hi) m = min(m, (unsigned long long)g.node_lo[n]); }
        else if (g.node_hi[n] == min_hi && g.node_lo[n] == min_lo) *winner = parent[n];
    }
    if (stage < 2) {
        for (int d = 32; d; d >>= 1) m = min(m, (unsigned long long)__shfl_down(m, d));
        if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(&mins[stage], m);
    }
}
__global__ __launch_bounds__(BLOCK) void k_retain(GraphView g, const u32 *parent, const u32 *winner_p) {
    const u32 winner = *winner_p;
    if (winner == NONE) return;                     // (nothing selected: the host reports it, the graph stays as it was)
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    for (u64 e = tid; e < g.n_edges; e += stride)
        if (g.e_alive[e] && !(parent[g.e_start[e]] == winner && parent[g.e_end[e]] == winner)) g.e_alive[e] = 0;
    for (u64 n = tid; n < g.n_nodes; n += stride)
        if (g.node_alive[n] && parent[n] != winner) {
            g.node_alive[n] = 0;
            g.out_order[n] = 0;
            g.in_deg[n] = 0;
            for (int b = 0; b < 4; b++) g.out_edge[n * 4 + b] = NONE;
        }
}

// ---------------------------------------------------------------------------------------------
// export
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_export_nodes(GraphView g, u64 *lo, u64 *hi, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_nodes + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 n = grp * BLOCK + threadIdx.x;
        const bool live = n < g.n_nodes && g.node_alive[n];
        u64 o = block_reserve(live ? 1u : 0u, cursor, lds4, &s_base);
        if (live) { lo[o] = g.node_lo[n]; hi[o] = g.node_hi[n]; }
    }
}
__global__ __launch_bounds__(BLOCK) void k_export_edges(GraphView g, u64 *slo, u64 *shi, u64 *elo, u64 *ehi, i64 *len, i64 *off,
                                                        uint8_t *seq, unsigned long long *cursors /* [0] edges [1] bytes */) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_edges + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 e = grp * BLOCK + threadIdx.x;
        const bool live = e < g.n_edges && g.e_alive[e];
        u64 o = block_reserve(live ? 1u : 0u, &cursors[0], lds4, &s_base);
        if (!live) continue;
        const u64 bytes = (g.e_len[e] + 3) / 4;
        const u64 so = atomicAdd(&cursors[1], (unsigned long long)bytes);
        const u32 s = g.e_start[e], t = g.e_end[e];
        slo[o] = g.node_lo[s]; shi[o] = g.node_hi[s];
        elo[o] = g.node_lo[t]; ehi[o] = g.node_hi[t];
        len[o] = (i64)g.e_len[e];
        off[o] = (i64)so;
        const u64 src = g.e_off[e];
        for (u64 i = 0; i < bytes; i++) seq[so + i] = g.pool[src + i];
    }
}
template <int W> __global__ void k_out_order(GraphView g, u64 lo, u64 hi, int *out5) {
    Kmer<W> x;
    if constexpr (W == 1) x = Kmer<1>{lo};
    else x = Kmer<2>{lo, hi};
    const u32 v = node_find<W>(g, x);
    if (v == NONE || !g.node_alive[v]) { out5[0] = -1; return; }
    const u32 o = g.out_order[v];
    out5[0] = order_count(o);
    for (int i = 0; i < order_count(o); i++) out5[1 + i] = order_base(o, i);
}

// ---------------------------------------------------------------------------------------------
// Graph.getGraphMap (Graph.scala:90-119): every k-mer of the graph -> where it sits.  A node's k-mer -> NodeGraphPosition(id);
// for an edge, the k-mers at distance 1 .. len-1 from its start node — windows of (start.seq ++ edge.seq) — ->
// EdgeGraphPosition(id, dist); the window at distance len is the end node's own k-mer and is not added (:108-113).
// One lane per (edge, distance): the window is cut out of the start k-mer and the 2-bit pool directly, no rolling.
// ---------------------------------------------------------------------------------------------
static constexpr u64 POS_EDGE = 1ull << 63;
__device__ __forceinline__ int path_base(const GraphView &g, u32 s, u64 off, int k, u64 i) {      // base i of start.seq ++ edge.seq
    if (i < (u64)k) return (int)(((i < 32 ? g.node_lo[s] : g.node_hi[s]) >> (2 * (i & 31))) & 3);
    return pool_get(g.pool, off, i - (u64)k);
}
template <int W> __device__ __forceinline__ Kmer<W> path_window(const GraphView &g, u32 s, u64 off, int k, u64 dist) {
    Kmer<W> x{};
    for (int i = 0; i < k; i++) {
        const u64 b = (u64)path_base(g, s, off, k, dist + (u64)i);
        if (i < 32) x.lo |= b << (2 * i);
        else if constexpr (W == 2) x.hi |= b << (2 * (i - 32));
    }
    return x;
}
// pass 0: entries per live edge (len - 1) -> its first entry through a block-aggregated cursor; pass 1 (flat): fill
__global__ __launch_bounds__(BLOCK) void k_pos_reserve(GraphView g, unsigned long long *first_entry, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_edges + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 e = grp * BLOCK + threadIdx.x;
        const u64 cnt = e < g.n_edges && g.e_alive[e] ? g.e_len[e] - 1 : 0;
        const u32 small = cnt < (1u << 22) ? (u32)cnt : 0u;
        u64 o = block_reserve(small, cursor, lds4, &s_base);
        if (e < g.n_edges) first_entry[e] = small == cnt ? o : atomicAdd(cursor, (unsigned long long)cnt);
    }
}
template <int W>
__global__ __launch_bounds__(BLOCK) void k_pos_fill(GraphView g, int k, const unsigned long long *__restrict__ first_entry, u64 node_entries,
                                                    u64 *lo, u64 *hi, u64 *val) {
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    // short edges: one lane walks the edge; long ones (> 64 entries): the whole grid strides over their distances below
    for (u64 e = tid; e < g.n_edges; e += stride) {
        if (!g.e_alive[e]) continue;
        const u64 cnt = g.e_len[e] - 1;
        if (cnt > 64) continue;
        const u32 s = g.e_start[e];
        const u64 off = g.e_off[e], at = node_entries + first_entry[e];
        for (u64 d = 1; d <= cnt; d++) {
            const Kmer<W> x = path_window<W>(g, s, off, k, d);
            lo[at + d - 1] = x.lo;
            if constexpr (W == 2) hi[at + d - 1] = x.hi;
            val[at + d - 1] = POS_EDGE | ((u64)e << 32) | d;
        }
    }
}
template <int W>
__global__ __launch_bounds__(BLOCK) void k_pos_fill_long(GraphView g, int k, const unsigned long long *__restrict__ first_entry, u64 node_entries,
                                                         u64 *lo, u64 *hi, u64 *val) {
    // one WORKGROUP per long edge at a time (grid-stride over edges), its lanes over the distances
    for (u64 e = blockIdx.x; e < g.n_edges; e += gridDim.x) {
        if (!g.e_alive[e]) continue;
        const u64 cnt = g.e_len[e] - 1;
        if (cnt <= 64) continue;
        const u32 s = g.e_start[e];
        const u64 off = g.e_off[e], at = node_entries + first_entry[e];
        for (u64 d = 1 + threadIdx.x; d <= cnt; d += BLOCK) {
            const Kmer<W> x = path_window<W>(g, s, off, k, d);
            lo[at + d - 1] = x.lo;
            if constexpr (W == 2) hi[at + d - 1] = x.hi;
            val[at + d - 1] = POS_EDGE | ((u64)e << 32) | d;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_pos_nodes(GraphView g, u64 *lo, u64 *hi, u64 *val, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_nodes + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 n = grp * BLOCK + threadIdx.x;
        const bool live = n < g.n_nodes && g.node_alive[n];
        const u64 o = block_reserve(live ? 1u : 0u, cursor, lds4, &s_base);
        if (live) { lo[o] = g.node_lo[n]; if (hi) hi[o] = g.node_hi[n]; val[o] = (u64)n; }
    }
}

// ---------------------------------------------------------------------------------------------
// point edits by id (the simplifier's node split: addNode, replaceStart, replaceEnd — Graph.scala:172-176, 197-209)
// ---------------------------------------------------------------------------------------------
__global__ void k_replace_start(GraphView g, u32 e, u32 ns, int *status) {
    if (e >= g.n_edges || !g.e_alive[e] || ns >= g.n_nodes || !g.node_alive[ns]) { *status = 1; return; }
    const u32 old = g.e_start[e];
    const int b = g.e_first[e];
    // edge.start.outEdgeIds -= edge.seq(0)            :200
    if (g.out_edge[(u64)old * 4 + b] == e) { g.out_edge[(u64)old * 4 + b] = NONE; g.out_order[old] = order_remove(g.out_order[old], b); }
    // newStart.outEdgeIds += edge.seq(0) -> edge.id   :201  (an immutable Map: an existing key keeps its place, its value is replaced)
    const u32 prev = g.out_edge[(u64)ns * 4 + b];
    g.out_edge[(u64)ns * 4 + b] = e;
    if (prev == NONE) g.out_order[ns] = order_append(g.out_order[ns], b);
    g.e_start[e] = ns;                                  // edges(edge.id) = new Edge(edge.id, newStart.id, ...)  :199
    *status = 0;
}
__global__ void k_replace_end(GraphView g, u32 e, u32 ne, int *status) {
    if (e >= g.n_edges || !g.e_alive[e] || ne >= g.n_nodes || !g.node_alive[ne]) { *status = 1; return; }
    const u32 old = g.e_end[e];
    if (g.in_deg[old]) g.in_deg[old]--;                 // edge.end.inEdgeIds -= edge.id   :207
    g.in_deg[ne]++;                                     // newEnd.inEdgeIds += edge.id     :208
    g.e_end[e] = ne;
    *status = 0;
}
__global__ void k_add_node(GraphView g, u32 n, u64 lo, u64 hi) {
    g.node_lo[n] = lo; g.node_hi[n] = hi;
    g.node_alive[n] = 1;
    g.out_order[n] = 0; g.in_deg[n] = 0;
    for (int b = 0; b < 4; b++) g.out_edge[(u64)n * 4 + b] = NONE;
}
__global__ __launch_bounds__(BLOCK) void k_nodes_by_id(GraphView g, const u32 *ids, u64 n, u64 *lo, u64 *hi, uint8_t *alive, u32 *in_deg, u32 *out_deg) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 v = ids[i];
        const bool ok = v < g.n_nodes;
        lo[i] = ok ? g.node_lo[v] : 0; hi[i] = ok ? g.node_hi[v] : 0;
        alive[i] = ok ? g.node_alive[v] : 0;
        in_deg[i] = ok ? g.in_deg[v] : 0;
        out_deg[i] = ok ? (u32)order_count(g.out_order[v]) : 0;
    }
}
__global__ __launch_bounds__(BLOCK) void k_edges_by_id(GraphView g, const u32 *ids, u64 n, u32 *start, u32 *end, u64 *len, uint8_t *first, uint8_t *alive) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 e = ids[i];
        const bool ok = e < g.n_edges;
        start[i] = ok ? g.e_start[e] : NONE; end[i] = ok ? g.e_end[e] : NONE;
        len[i] = ok ? g.e_len[e] : 0; first[i] = ok ? g.e_first[e] : 0; alive[i] = ok ? g.e_alive[e] : 0;
    }
}
template <int W> __global__ void k_node_lookup(GraphView g, u64 lo, u64 hi, int base, u32 *out2) {
    Kmer<W> x;
    if constexpr (W == 1) x = Kmer<1>{lo};
    else x = Kmer<2>{lo, hi};
    const u32 best = node_find<W>(g, x);
    out2[0] = best;
    out2[1] = best != NONE && base >= 0 && base < 4 ? g.out_edge[(u64)best * 4 + base] : NONE;
}
__global__ void k_nidx_insert(GraphView g, u32 n, u64 h) {
    u64 i = h & g.nidx_mask;
    while (atomicCAS(&g.nidx[i], NONE, n) != NONE) i = (i + 1) & g.nidx_mask;
}

// in-edge lists (Node.inEdgeIds) as CSR by end node (graph_in_lists below): cnt[v] += 1 per live edge ending at v; then, with `off`
// the exclusive scan of those counts and `cursor` zeroed, list[off[v] ..] = the ids of those edges (order unspecified)
__global__ __launch_bounds__(BLOCK) void k_in_count(GraphView g, u32 *cnt) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK)
        if (g.e_alive[e]) atomicAdd(&cnt[g.e_end[e]], 1u);
}
__global__ __launch_bounds__(BLOCK) void k_in_fill(GraphView g, const unsigned long long *off, u32 *cursor, u32 *list) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK)
        if (g.e_alive[e]) { const u32 v = g.e_end[e]; list[off[v] + atomicAdd(&cursor[v], 1u)] = (u32)e; }
}

// =============================================================================================
// host side
// =============================================================================================
// ---- contig statistics (CheckGraph.scala:37-41): one reduction, then a radix select over the 64-bit lengths by histogram passes ----
// out: [0] count, [1] sum, [2] max over the live edges longer than `longer_than`
__global__ __launch_bounds__(BLOCK) void k_contig_reduce(GraphView g, u64 longer_than, unsigned long long *out) {
    unsigned long long c = 0, s = 0, m = 0;
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        const u64 len = g.e_len[e];
        if (g.e_alive[e] && len > longer_than) { c++; s += len; m = len > m ? len : m; }
    }
    for (int d = 32; d; d >>= 1) {
        c += __shfl_down(c, d); s += __shfl_down(s, d);
        const unsigned long long o = __shfl_down(m, d);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && c) { atomicAdd(&out[0], c); atomicAdd(&out[1], s); atomicMax(&out[2], m); }
}
// one level of both selects: the byte at `shift` of the lengths whose higher bits equal a prefix.  hist[0..255] counts the lengths
// under the median's prefix (a plain rank), hist[256..511] sums the lengths under the N50's prefix (a length-weighted rank).
__global__ __launch_bounds__(BLOCK) void k_contig_hist(GraphView g, u64 longer_than, int shift, u64 prefix_med, u64 prefix_n50, unsigned long long *hist) {
    __shared__ unsigned long long s_h[512];
    for (int i = threadIdx.x; i < 512; i += BLOCK) s_h[i] = 0;
    __syncthreads();
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        const u64 len = g.e_len[e];
        if (!g.e_alive[e] || len <= longer_than) continue;
        const u64 above = shift >= 56 ? 0 : len >> (shift + 8);
        const u32 b = (u32)(len >> shift) & 255u;
        if (above == prefix_med) atomicAdd(&s_h[b], 1ull);
        if (above == prefix_n50) atomicAdd(&s_h[256 + b], (unsigned long long)len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += BLOCK) if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

int ggrid(const gk_ctx *ctx, u64 items) {
    u64 blocks = (items + BLOCK - 1) / BLOCK;
    if (blocks < 1) blocks = 1;
    return (int)std::min<u64>(blocks, grid_cap(ctx));
}

template <class T> static hipError_t dev_grow(gk_ctx *ctx, T **p, u64 old_n, u64 new_n, hipStream_t st) {
    T *np_ = nullptr;
    hipError_t e = pool_malloc(ctx, &np_, std::max<u64>(new_n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (*p && old_n) e = hipMemcpyAsync(np_, *p, old_n * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)pool_free(ctx, *p);
    *p = np_;
    return e;
}

// Node and edge arrays live in ONE allocation each (a device allocation costs ~1 ms at these sizes: twelve of them were 10 % of
// gk_graph_build at C3); the view's pointers are carved out of the blobs, 256-byte aligned.
static size_t al256g(size_t v) { return (v + 255) & ~(size_t)255; }
struct NodeCarve { size_t lo, hi, alive, out_edge, out_order, in_deg, total; };
struct EdgeCarve { size_t start, end, len, off, alive, first, total; };
static NodeCarve node_carve(u64 c) {
    NodeCarve k{};
    size_t o = 0;
    k.lo = o; o += al256g(c * 8);
    k.hi = o; o += al256g(c * 8);
    k.out_edge = o; o += al256g(c * 16);
    k.out_order = o; o += al256g(c * 4);
    k.in_deg = o; o += al256g(c * 4);
    k.alive = o; o += al256g(c);
    k.total = o;
    return k;
}
static EdgeCarve edge_carve(u64 c) {
    EdgeCarve k{};
    size_t o = 0;
    k.len = o; o += al256g(c * 8);
    k.off = o; o += al256g(c * 8);
    k.start = o; o += al256g(c * 4);
    k.end = o; o += al256g(c * 4);
    k.alive = o; o += al256g(c);
    k.first = o; o += al256g(c);
    k.total = o;
    return k;
}
static void node_view(GraphView &v, char *blob, const NodeCarve &k) {
    v.node_lo = (u64 *)(blob + k.lo); v.node_hi = (u64 *)(blob + k.hi); v.node_alive = (uint8_t *)(blob + k.alive);
    v.out_edge = (u32 *)(blob + k.out_edge); v.out_order = (u32 *)(blob + k.out_order); v.in_deg = (u32 *)(blob + k.in_deg);
}
static void edge_view(GraphView &v, char *blob, const EdgeCarve &k) {
    v.e_start = (u32 *)(blob + k.start); v.e_end = (u32 *)(blob + k.end); v.e_len = (u64 *)(blob + k.len); v.e_off = (u64 *)(blob + k.off);
    v.e_alive = (uint8_t *)(blob + k.alive); v.e_first = (uint8_t *)(blob + k.first);
}

int graph_alloc_nodes(gk_graph *g, u64 n) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    const u64 c = std::max<u64>(n, 1);
    const NodeCarve k = node_carve(c);
    GK_HIP(ctx, pool_malloc(ctx, &g->node_blob, k.total));
    node_view(v, (char *)g->node_blob, k);
    // out_edge <- NONE (0xff..), out_order / in_deg / alive <- 0: two memsets over the two contiguous stretches
    GK_HIP(ctx, hipMemsetAsync(v.out_edge, 0xff, c * 16, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync((char *)g->node_blob + k.out_order, 0, k.total - k.out_order, ctx->stream));
    v.n_nodes = n;
    g->node_cap = c;
    return GK_OK;
}
int graph_alloc_edges(gk_graph *g, u64 n) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    const u64 c = std::max<u64>(n, 1);
    const EdgeCarve k = edge_carve(c);
    GK_HIP(ctx, pool_malloc(ctx, &g->edge_blob, k.total));
    edge_view(v, (char *)g->edge_blob, k);
    GK_HIP(ctx, hipMemsetAsync(v.e_alive, 0, c, ctx->stream));
    v.n_edges = n;
    g->edge_cap = c;
    return GK_OK;
}
int graph_grow_edges(gk_graph *g, u64 new_n) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (new_n <= g->edge_cap) { return GK_OK; }
    const u64 old = v.n_edges;
    const EdgeCarve k = edge_carve(new_n);
    void *blob = nullptr;
    GK_HIP(ctx, pool_malloc(ctx, &blob, k.total));
    GraphView nv = v;
    edge_view(nv, (char *)blob, k);
    hipError_t e = hipMemsetAsync(nv.e_alive, 0, new_n, ctx->stream);
    if (e == hipSuccess && old) {
        e = hipMemcpyAsync(nv.e_start, v.e_start, old * 4, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.e_end, v.e_end, old * 4, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.e_len, v.e_len, old * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.e_off, v.e_off, old * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.e_alive, v.e_alive, old, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.e_first, v.e_first, old, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)pool_free(ctx, blob); return hip_fail(ctx, e, "graph: growing the edge arrays"); }
    (void)pool_free(ctx, g->edge_blob);
    g->edge_blob = blob;
    v = nv;
    g->edge_cap = new_n;
    return GK_OK;
}

int graph_refresh_counts(gk_graph *g) {
    gk_ctx *ctx = g->ctx;
    g->epoch++;                  // (every edit of the graph ends here or in a point edit)
    unsigned long long *d = nullptr, h[3] = {0, 0, 0};
    DevScratch tmp(ctx);
    GK_HIP(ctx, tmp.get(&d, 3));
    hipError_t e = hipMemsetAsync(d, 0, 24, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_count_live, dim3(ggrid(ctx, std::max(g->v.n_nodes, g->v.n_edges))), dim3(BLOCK), 0, ctx->stream, g->v, d);
        e = read_back(ctx, h, d, 3);
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "graph_refresh_counts");
    g->live_nodes = h[0]; g->live_edges = h[1]; g->live_len = h[2];
    return GK_OK;
}

int graph_build_index(gk_graph *g) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (v.nidx) { GK_HIP(ctx, pool_free(ctx, v.nidx)); v.nidx = nullptr; }
    const u64 cap = pow2ceil(std::max<u64>(16, 2 * v.n_nodes + 2));
    GK_HIP(ctx, pool_malloc(ctx, &v.nidx, cap * 4));
    GK_HIP(ctx, hipMemsetAsync(v.nidx, 0xff, cap * 4, ctx->stream));
    v.nidx_mask = cap - 1;
    if (v.n_nodes) {
        GK_BY_W(g->W, hipLaunchKernelGGL(k_build_nidx<W>, dim3(ggrid(ctx, v.n_nodes)), dim3(BLOCK), 0, ctx->stream, v));
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    g->index_ready = true;
    return GK_OK;
}

int check_graph(const gk_graph *g) {
    if (!g || !g->ctx) return fail(nullptr, GK_E_INVALID, "null graph handle");
    hipError_t e = hipSetDevice(g->ctx->device);
    if (e != hipSuccess) return hip_fail(g->ctx, e, "hipSetDevice");
    return GK_OK;
}

int graph_in_lists(gk_graph *g, DevScratch &tmp, const char *who, unsigned long long **off, u32 **list) {
    gk_ctx *ctx = g->ctx;
    const GraphView &v = g->v;
    u32 *cnt = nullptr;                       // the counts, then (zeroed again) the fill's cursors
    const std::string what = std::string(who) + ": in-edge lists";
    tmp.get(off, v.n_nodes + 1);
    tmp.zeroed(&cnt, v.n_nodes);
    tmp.get(list, v.n_edges);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), what.c_str());
    if (v.n_edges) hipLaunchKernelGGL(k_in_count, dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, cnt);
    tmp.note(scan_counts(ctx, tmp, cnt, v.n_nodes, *off));
    tmp.note(hipMemsetAsync(cnt, 0, std::max<u64>(v.n_nodes, 1) * 4, ctx->stream));
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), what.c_str());
    if (v.n_edges) hipLaunchKernelGGL(k_in_fill, dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, *off, cnt, *list);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(ctx, e, what.c_str());
    return GK_OK;
}

extern "C" {

int gk_graph_counts(gk_graph *g, uint64_t *nodes, uint64_t *edges, uint64_t *total_edge_len) {
    if (int rc = check_graph(g)) return rc;
    if (nodes) *nodes = g->live_nodes;
    if (edges) *edges = g->live_edges;
    if (total_edge_len) *total_edge_len = g->live_len;
    return GK_OK;
}

int gk_graph_contig_stats(gk_graph *g, uint64_t longer_than, uint64_t *count, uint64_t *sum, uint64_t *median, uint64_t *n50, uint64_t *max) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    uint64_t *outs[5] = {count, sum, median, n50, max};
    for (uint64_t *o : outs) if (o) *o = 0;
    if (g->v.n_edges == 0) return GK_OK;
    DevScratch tmp(ctx);
    unsigned long long *d = nullptr, h[512];                 // d: [0..2] the reduction, [8..519] one level's histograms
    GK_HIP(ctx, tmp.get(&d, 8 + 512));
    GK_HIP(ctx, hipMemsetAsync(d, 0, 64, ctx->stream));
    const int grid = ggrid(ctx, g->v.n_edges);
    hipLaunchKernelGGL(k_contig_reduce, dim3(grid), dim3(BLOCK), 0, ctx->stream, g->v, (u64)longer_than, d);
    GK_HIP(ctx, read_back(ctx, h, d, 3));
    const u64 cnt = h[0], total = h[1], mx = h[2];
    if (cnt == 0) return GK_OK;
    // sorted[count / 2] ascending; and, lengths descending, the first at which the running sum reaches half the total (rounded up)
    u64 rank = cnt / 2, acc = 0, pm = 0, pn = 0;
    const u64 half = total / 2 + (total & 1);
    int shift = 56;
    while (shift > 0 && (mx >> shift) == 0) shift -= 8;      // (the bytes above the maximum's top byte are zero in every length)
    for (; shift >= 0; shift -= 8) {
        GK_HIP(ctx, hipMemsetAsync(d + 8, 0, 512 * 8, ctx->stream));
        hipLaunchKernelGGL(k_contig_hist, dim3(grid), dim3(BLOCK), 0, ctx->stream, g->v, (u64)longer_than, shift, pm, pn, d + 8);
        GK_HIP(ctx, read_back(ctx, h, d + 8, 512));
        int bm = -1, bn = -1;
        for (int b = 0; b < 256 && bm < 0; b++) { if (rank < h[b]) bm = b; else rank -= h[b]; }
        for (int b = 255; b >= 0 && bn < 0; b--) { if (acc + h[256 + b] >= half) bn = b; else acc += h[256 + b]; }
        if (bm < 0 || bn < 0) return fail(ctx, GK_E_STATE, "gk_graph_contig_stats: the select lost its rank (the graph changed under the call?)");
        pm = (pm << 8) | (u64)bm;
        pn = (pn << 8) | (u64)bn;
    }
    if (count) *count = cnt;
    if (sum) *sum = total;
    if (median) *median = pm;
    if (n50) *n50 = pn;
    if (max) *max = mx;
    return GK_OK;
}

}  // extern "C"

// keep_stats4 == nullptr: MapGraph.simplifyGraph as it is; otherwise the keeping form (gk_graph_simplify_keep_cycles)
static int graph_simplify(gk_graph *g, uint64_t *keep_stats4) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (v.n_nodes == 0) return GK_OK;
    u32 *in_single = nullptr, *merged_key = nullptr;
    uint8_t *cls = nullptr;
    unsigned long long *d_cnt = nullptr, h_cnt[3] = {0, 0, 0};
    LongPiece *long_pieces = nullptr;
    DevScratch tmp(ctx);
    tmp.get(&in_single, v.n_nodes);
    tmp.get(&merged_key, v.n_nodes * 4);
    tmp.get(&cls, v.n_nodes);
    tmp.zeroed(&d_cnt, 3);
    if (tmp.error() == hipSuccess) {                             // (NONE everywhere: a fill, not a zeroing)
        tmp.note(hipMemsetAsync(in_single, 0xff, v.n_nodes * 4, ctx->stream));
        tmp.note(hipMemsetAsync(merged_key, 0xff, v.n_nodes * 16, ctx->stream));
    }
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_simplify: alloc");
    const int gn = ggrid(ctx, v.n_nodes), ge = ggrid(ctx, std::max<u64>(v.n_edges, 1));
    hipLaunchKernelGGL(k_in_single, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, in_single);
    hipLaunchKernelGGL(k_node_class, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, in_single, cls);
    const u64 nodes_before = g->live_nodes;
    if (keep_stats4) {
        if (int rc = cycles_keep_classes(g, tmp, cls, keep_stats4)) return rc;
    }
    const u64 old_edges = v.n_edges, old_pool = g->pool_used;
    hipLaunchKernelGGL(k_chain, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, cls, 0, old_edges, old_pool, d_cnt, merged_key, (LongPiece *)nullptr);
    hipError_t e = read_back(ctx, h_cnt, d_cnt, 3);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_simplify: count");
    if (h_cnt[0]) {
        if (old_edges + h_cnt[0] >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph edges");
        if (int rc = graph_grow_edges(g, old_edges + h_cnt[0])) return rc;
        if (old_pool + h_cnt[1] + 8 > g->pool_cap) {             // (+8: k_copy_long ORs whole 32-bit words, the last one may reach past the last byte)
            e = dev_grow(ctx, &v.pool, old_pool, old_pool + h_cnt[1] + 8, ctx->stream);
            if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_simplify: pool");
            g->pool_cap = old_pool + h_cnt[1] + 8;
        }
        tmp.note(hipMemsetAsync(d_cnt, 0, 24, ctx->stream));
        if (h_cnt[2]) {                                          // long pieces are ORed into their place: it starts as zeroes
            tmp.get(&long_pieces, h_cnt[2]);
            tmp.note(hipMemsetAsync(v.pool + old_pool, 0, h_cnt[1], ctx->stream));
        }
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_simplify");
        hipLaunchKernelGGL(k_chain, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, cls, 1, old_edges, old_pool, d_cnt, merged_key, long_pieces);
        if (h_cnt[2]) hipLaunchKernelGGL(k_copy_long, dim3((unsigned)h_cnt[2]), dim3(BLOCK), 0, ctx->stream, v, long_pieces);
        v.n_edges = old_edges + h_cnt[0];
        g->pool_used = old_pool + h_cnt[1];
    }
    hipLaunchKernelGGL(k_simplify_finish, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, cls, merged_key);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_simplify: finish");
    const int rc = graph_refresh_counts(g);
    if (keep_stats4) keep_stats4[3] = nodes_before - g->live_nodes;
    return rc;
}

extern "C" {

int gk_graph_simplify(gk_graph *g) { return graph_simplify(g, nullptr); }

int gk_graph_simplify_keep_cycles(gk_graph *g, uint64_t *stats4) {
    uint64_t st[4] = {0, 0, 0, 0};
    const int rc = graph_simplify(g, st);
    if (stats4) for (int i = 0; i < 4; i++) stats4[i] = st[i];
    return rc;
}

int gk_graph_remove_bubbles(gk_graph *g) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (g->v.n_nodes == 0) return GK_OK;
    hipLaunchKernelGGL(k_bubbles, dim3(ggrid(ctx, g->v.n_nodes)), dim3(BLOCK), 0, ctx->stream, g->v);
    GK_HIP(ctx, hipGetLastError());
    return graph_refresh_counts(g);
}

int gk_graph_remove_edges(gk_graph *g, const uint64_t *start_lo, const uint64_t *start_hi, const uint8_t *base, uint64_t n,
                          uint64_t *removed) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (removed) *removed = 0;
    if (n == 0) return GK_OK;
    if (int rc = graph_ensure_index(g)) return rc;             // (edges are named by their start k-mer here)
    if (!start_lo || !base || (g->W == 2 && !start_hi)) return fail(ctx, GK_E_INVALID, "null argument");
    u64 *d_lo = nullptr, *d_hi = nullptr;
    uint8_t *d_b = nullptr;
    unsigned long long *d_rm = nullptr, h_rm = 0;
    DevScratch tmp(ctx);
    tmp.upload(&d_lo, start_lo, n);
    if (start_hi) tmp.upload(&d_hi, start_hi, n);
    else tmp.zeroed(&d_hi, n);
    tmp.upload(&d_b, base, n);
    tmp.zeroed(&d_rm, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_remove_edges");
    GK_BY_W(g->W, hipLaunchKernelGGL(k_remove_edges<W>, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, g->v, d_lo, d_hi, d_b, n, d_rm));
    if (const hipError_t e = read_back(ctx, &h_rm, d_rm); e != hipSuccess) return hip_fail(ctx, e, "gk_graph_remove_edges");
    if (removed) *removed = h_rm;
    return graph_refresh_counts(g);
}

}  // extern "C"

// Graph.components (Graph.scala:54-72): label every live node with its component's root (min-label hooking + pointer
// jumping) and count nodes per root.  *parent / *size ([n_nodes] each) come from the caller's `tmp` and live as long as it does.
static int graph_components(gk_graph *g, DevScratch &tmp, u32 **parent_out, u32 **size_out, u64 *ncomp) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    u32 *parent = nullptr, *size = nullptr;
    unsigned long long *d_ncomp = nullptr;
    tmp.get(&parent, v.n_nodes);
    tmp.zeroed(&size, v.n_nodes);
    tmp.zeroed(&d_ncomp, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "graph components: alloc");
    const int gn = ggrid(ctx, std::max<u64>(v.n_nodes, 1)), ge = ggrid(ctx, std::max<u64>(v.n_edges, 1));
    hipLaunchKernelGGL(k_cc_init, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, parent);
    if (ctx->hook_cc_find == 1) hipLaunchKernelGGL(k_cc_link<1>, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, parent);
    else if (ctx->hook_cc_find == 3) hipLaunchKernelGGL(k_cc_link<3>, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, parent);
    else if (ctx->hook_cc_find == 2) hipLaunchKernelGGL(k_cc_link<2>, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, parent);
    else hipLaunchKernelGGL(k_cc_link<0>, dim3(ge), dim3(BLOCK), 0, ctx->stream, v, parent);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "graph components: hooking");
    unsigned long long h = 0;
    hipLaunchKernelGGL(k_cc_sizes, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, parent, size, d_ncomp);
    if ((e = read_back(ctx, &h, d_ncomp)) != hipSuccess) return hip_fail(ctx, e, "graph components: sizes");
    tmp.release(d_ncomp);
    *parent_out = parent; *size_out = size; *ncomp = h;
    return GK_OK;
}

extern "C" {

int gk_graph_retain_largest(gk_graph *g, uint64_t *kept_nodes, uint64_t *components) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (kept_nodes) *kept_nodes = 0;
    if (components) *components = 0;
    if (g->live_nodes == 0) return GK_OK;
    u32 *parent = nullptr, *size = nullptr, *d_u32 = nullptr;       // d_u32: [0] unused [1] best [2] winner
    unsigned long long *d_u64 = nullptr;                            // [0] unused [1] min hi [2] min lo
    u64 ncomp = 0;
    DevScratch tmp(ctx);
    if (int rc = graph_components(g, tmp, &parent, &size, &ncomp)) return rc;
    const int gn = ggrid(ctx, v.n_nodes);
    const unsigned long long h64[3] = {0, ~0ull, ~0ull};
    u32 h32[3] = {0, 0, NONE};
    tmp.upload(&d_u64, h64, 3);
    tmp.upload(&d_u32, h32, 3);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_retain_largest: alloc");
    // max size -> smallest k-mer among the components of that size -> its root -> retain: four dependent steps, no host in between
    hipLaunchKernelGGL(k_cc_max, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, size, &d_u32[1]);
    for (int stage = 0; stage < 3; stage++)
        hipLaunchKernelGGL(k_cc_pick, dim3(gn), dim3(BLOCK), 0, ctx->stream, v, parent, size, &d_u32[1], stage, &d_u64[1], &d_u32[2]);
    hipLaunchKernelGGL(k_retain, dim3(ggrid(ctx, std::max(v.n_nodes, v.n_edges))), dim3(BLOCK), 0, ctx->stream, v, parent, &d_u32[2]);
    if (const hipError_t e = read_back(ctx, h32, d_u32, 3); e != hipSuccess) return hip_fail(ctx, e, "gk_graph_retain_largest: retain");
    if (h32[2] == NONE) return fail(ctx, GK_E_STATE, "no component selected");
    if (components) *components = ncomp;
    int rc = graph_refresh_counts(g);
    if (rc == GK_OK && kept_nodes) *kept_nodes = g->live_nodes;
    return rc;
}

int gk_graph_component_stats(gk_graph *g, uint32_t *nodes_per_component, uint64_t *edge_len_per_component, uint64_t cap, uint64_t *n) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (n) *n = 0;
    if (g->live_nodes == 0) return GK_OK;
    u32 *parent = nullptr, *size = nullptr, *d_nodes = nullptr;
    unsigned long long *len = nullptr, *d_len = nullptr, *d_cur = nullptr;
    u64 ncomp = 0;
    DevScratch tmp(ctx);
    if (int rc = graph_components(g, tmp, &parent, &size, &ncomp)) return rc;
    if (n) *n = ncomp;
    if (ncomp > cap) return fail(ctx, GK_E_CAPACITY, "component buffer too small: need " + std::to_string(ncomp));
    if (!nodes_per_component || !edge_len_per_component) return fail(ctx, GK_E_INVALID, "null component buffer");
    tmp.zeroed(&len, v.n_nodes);
    tmp.get(&d_nodes, ncomp);
    tmp.get(&d_len, ncomp);
    tmp.zeroed(&d_cur, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_component_stats: alloc");
    hipLaunchKernelGGL(k_cc_edge_len, dim3(ggrid(ctx, std::max<u64>(v.n_edges, 1))), dim3(BLOCK), 0, ctx->stream, v, parent, len);
    hipLaunchKernelGGL(k_cc_collect, dim3(ggrid(ctx, v.n_nodes)), dim3(BLOCK), 0, ctx->stream, v, parent, size, len, d_nodes, d_len, d_cur);
    const hipError_t e = read_back(ctx, {{nodes_per_component, d_nodes, ncomp * 4}, {edge_len_per_component, d_len, ncomp * 8}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_component_stats");
    return GK_OK;
}

int gk_graph_checksum(gk_graph *g, uint64_t *nodes_checksum, uint64_t *edges_checksum) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    unsigned long long *d = nullptr, h[2] = {0, 0};
    DevScratch tmp(ctx);
    GK_HIP(ctx, tmp.get(&d, 2));
    hipError_t e = hipMemsetAsync(d, 0, 16, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_graph_checksum, dim3(ggrid(ctx, std::max<u64>(std::max(g->v.n_nodes, g->v.n_edges), 1))), dim3(BLOCK), 0, ctx->stream, g->v, d);
        e = read_back(ctx, h, d, 2);
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_checksum");
    if (nodes_checksum) *nodes_checksum = h[0];
    if (edges_checksum) *edges_checksum = h[1];
    return GK_OK;
}

int gk_graph_export_nodes(gk_graph *g, uint64_t *lo, uint64_t *hi, uint64_t cap, uint64_t *n) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (n) *n = g->live_nodes;
    if (g->live_nodes > cap) return fail(ctx, GK_E_CAPACITY, "node export buffer too small: need " + std::to_string(g->live_nodes));
    if (g->live_nodes == 0) return GK_OK;
    if (!lo) return fail(ctx, GK_E_INVALID, "null export buffer");
    const u64 cnt = g->live_nodes;
    u64 *d_lo = nullptr, *d_hi = nullptr;
    unsigned long long *d_cur = nullptr;
    DevScratch tmp(ctx);
    tmp.get(&d_lo, cnt);
    tmp.get(&d_hi, cnt);
    tmp.zeroed(&d_cur, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_export_nodes");
    hipLaunchKernelGGL(k_export_nodes, dim3(ggrid(ctx, g->v.n_nodes)), dim3(BLOCK), 0, ctx->stream, g->v, d_lo, d_hi, d_cur);
    if (const hipError_t e = read_back(ctx, {{lo, d_lo, cnt * 8}, {hi, d_hi, cnt * 8}}); e != hipSuccess) return hip_fail(ctx, e, "gk_graph_export_nodes");
    return GK_OK;
}

int gk_graph_export_edges(gk_graph *g, uint64_t *start_lo, uint64_t *start_hi, uint64_t *end_lo, uint64_t *end_hi,
                          int64_t *len, int64_t *seq_off, uint64_t cap, uint64_t *n,
                          uint8_t *seq2bit, uint64_t seq_cap, uint64_t *seq_bytes) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (n) *n = g->live_edges;
    // upper bound on packed bytes: every live edge rounds up to a byte
    const u64 max_bytes = (g->live_len + 3 * g->live_edges) / 4 + 1;
    if (seq_bytes) *seq_bytes = max_bytes;
    if (g->live_edges > cap) return fail(ctx, GK_E_CAPACITY, "edge export buffer too small: need " + std::to_string(g->live_edges));
    if (g->live_edges == 0) { if (seq_bytes) *seq_bytes = 0; return GK_OK; }
    if (seq_cap < max_bytes) return fail(ctx, GK_E_CAPACITY, "sequence buffer too small: need " + std::to_string(max_bytes));
    if (!start_lo || !end_lo || !len || !seq_off || !seq2bit) return fail(ctx, GK_E_INVALID, "null export buffer");
    const u64 cnt = g->live_edges;
    u64 *d_k[4] = {nullptr, nullptr, nullptr, nullptr};
    i64 *d_len = nullptr, *d_off = nullptr;
    uint8_t *d_seq = nullptr;
    unsigned long long *d_cur = nullptr, h_cur[2] = {0, 0};
    DevScratch tmp(ctx);
    for (int i = 0; i < 4; i++) tmp.get(&d_k[i], cnt);
    tmp.get(&d_len, cnt);
    tmp.get(&d_off, cnt);
    tmp.get(&d_seq, max_bytes);
    tmp.zeroed(&d_cur, 2);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_export_edges");
    hipLaunchKernelGGL(k_export_edges, dim3(ggrid(ctx, g->v.n_edges)), dim3(BLOCK), 0, ctx->stream, g->v, d_k[0], d_k[1], d_k[2], d_k[3], d_len, d_off, d_seq, d_cur);
    hipError_t e = read_back(ctx, {{h_cur, d_cur, 16}, {start_lo, d_k[0], cnt * 8}, {start_hi, d_k[1], cnt * 8}, {end_lo, d_k[2], cnt * 8},
                                   {end_hi, d_k[3], cnt * 8}, {len, d_len, cnt * 8}, {seq_off, d_off, cnt * 8}});
    if (e == hipSuccess && h_cur[1]) e = hipMemcpy(seq2bit, d_seq, h_cur[1], hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_export_edges");
    if (h_cur[0] != cnt) return fail(ctx, GK_E_STATE, "edge export count mismatch");
    if (seq_bytes) *seq_bytes = h_cur[1];
    return GK_OK;
}

int gk_graph_out_order(gk_graph *g, uint64_t lo, uint64_t hi, int *bases4, int *count) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (!bases4 || !count) return fail(ctx, GK_E_INVALID, "null argument");
    if (int rc = graph_ensure_index(g)) return rc;
    int *d = nullptr, h[5] = {-1, 0, 0, 0, 0};
    DevScratch tmp(ctx);
    GK_HIP(ctx, tmp.get(&d, 5));
    GK_BY_W(g->W, hipLaunchKernelGGL(k_out_order<W>, dim3(1), dim3(1), 0, ctx->stream, g->v, lo, hi, d));
    const hipError_t e = read_back(ctx, h, d, 5);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_out_order");
    *count = h[0];
    for (int i = 0; i < 4; i++) bases4[i] = i < h[0] ? h[1 + i] : 0;
    return GK_OK;
}

}  // extern "C"
int graph_grow_nodes(gk_graph *g, u64 new_cap) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (new_cap <= g->node_cap) return GK_OK;
    const u64 old = v.n_nodes;
    const NodeCarve k = node_carve(new_cap);
    void *blob = nullptr;
    GK_HIP(ctx, pool_malloc(ctx, &blob, k.total));
    GraphView nv = v;
    node_view(nv, (char *)blob, k);
    hipError_t e = hipMemsetAsync(nv.node_alive, 0, new_cap, ctx->stream);
    if (e == hipSuccess && old) {
        e = hipMemcpyAsync(nv.node_lo, v.node_lo, old * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.node_hi, v.node_hi, old * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.node_alive, v.node_alive, old, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.out_edge, v.out_edge, old * 16, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.out_order, v.out_order, old * 4, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nv.in_deg, v.in_deg, old * 4, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)pool_free(ctx, blob); return hip_fail(ctx, e, "graph: growing the node arrays"); }
    (void)pool_free(ctx, g->node_blob);
    g->node_blob = blob;
    v = nv;
    g->node_cap = new_cap;
    return GK_OK;
}

extern "C" {

// Graph.getGraphMap (Graph.scala:90-119): putNew of every node k-mer and of every interior k-mer of every edge into `vm`
int gk_graph_position_map(gk_graph *g, gk_vmap *vm, uint64_t *entries) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (entries) *entries = 0;
    if (!vm || vmap_ctx(vm) != ctx) return fail(ctx, GK_E_INVALID, "gk_graph_position_map: the value map must live on the graph's context");
    if (vmap_k(vm) != g->k) return fail(ctx, GK_E_KLEN, "gk_graph_position_map: the map's k differs from the graph's");     // key.length == k
    GraphView &v = g->v;
    unsigned long long *first = nullptr, *d_cur = nullptr, h_cur[2] = {0, 0};
    u64 *lo = nullptr, *hi = nullptr, *val = nullptr;
    DevScratch tmp(ctx);
    tmp.get(&first, v.n_edges);
    tmp.zeroed(&d_cur, 2);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_position_map: alloc");
    if (v.n_edges) hipLaunchKernelGGL(k_pos_reserve, dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, first, &d_cur[0]);
    hipError_t e = read_back(ctx, h_cur, d_cur, 1);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_position_map: reserve");
    // the reference's own check, printed side by side at :117: size == sum of edge lengths + nodes - edges
    const u64 total = g->live_nodes + h_cur[0];
    if (h_cur[0] != g->live_len - g->live_edges) return fail(ctx, GK_E_STATE, "gk_graph_position_map: interior k-mer count does not match the graph's counters");
    if (total == 0) return GK_OK;
    tmp.get(&lo, total);
    if (g->W == 1) tmp.zeroed(&hi, total);
    else tmp.get(&hi, total);
    tmp.get(&val, total);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_position_map: entries");
    hipLaunchKernelGGL(k_pos_nodes, dim3(ggrid(ctx, std::max<u64>(v.n_nodes, 1))), dim3(BLOCK), 0, ctx->stream, v, lo, hi, val, &d_cur[1]);
    if (v.n_edges) {
        GK_BY_W(g->W,
            hipLaunchKernelGGL(k_pos_fill<W>, dim3(ggrid(ctx, v.n_edges)), dim3(BLOCK), 0, ctx->stream, v, g->k, first, g->live_nodes, lo, hi, val);
            hipLaunchKernelGGL(k_pos_fill_long<W>, dim3((int)std::min<u64>(v.n_edges, grid_cap(ctx))), dim3(BLOCK), 0, ctx->stream, v, g->k, first, g->live_nodes, lo, hi, val));
    }
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_position_map: fill");
    if (int rc = vmap_put_new_dev(vm, lo, hi, val, total)) return rc;
    if (entries) *entries = total;
    return GK_OK;
}

// first live node holding this k-mer (NONE = 0xffffffff if there is none) and, if base is 0..3, its out-edge for that first base
int gk_graph_node_lookup(gk_graph *g, uint64_t lo, uint64_t hi, int base, uint32_t *node_id, uint32_t *edge_id) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (int rc = graph_ensure_index(g)) return rc;
    u32 *d = nullptr, h[2] = {NONE, NONE};
    DevScratch tmp(ctx);
    GK_HIP(ctx, tmp.get(&d, 2));
    GK_BY_W(g->W, hipLaunchKernelGGL(k_node_lookup<W>, dim3(1), dim3(1), 0, ctx->stream, g->v, lo, hi, base, d));
    const hipError_t e = read_back(ctx, h, d, 2);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_node_lookup");
    if (node_id) *node_id = h[0];
    if (edge_id) *edge_id = h[1];
    return GK_OK;
}

// MapGraph.addNode(seq) (Graph.scala:172-176): a fresh node without edges; several nodes may carry the same sequence
int gk_graph_add_node(gk_graph *g, uint64_t lo, uint64_t hi, uint32_t *node_id) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    if (g->W == 1 ? ((lo >> (2 * g->k)) != 0 || hi != 0) : (g->k < 64 && (hi >> (2 * (g->k - 32))) != 0))
        return fail(ctx, GK_E_KLEN, "gk_graph_add_node: not a " + std::to_string(g->k) + "-mer");
    if (v.n_nodes + 1 >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph nodes");
    if (v.n_nodes + 1 > g->node_cap) { if (int rc = graph_grow_nodes(g, std::max<u64>(g->node_cap * 2, 16))) return rc; }
    const u32 n = (u32)v.n_nodes;
    g->epoch++;
    hipLaunchKernelGGL(k_add_node, dim3(1), dim3(1), 0, ctx->stream, v, n, lo, hi);
    v.n_nodes++;
    g->live_nodes++;
    if (!g->index_ready) {
        // (no index yet: the first query builds it, this node included)
    } else if (2 * v.n_nodes > v.nidx_mask) {
        if (int rc = graph_build_index(g)) return rc;          // the index outgrew its table: rebuild (power of two >= 2 n)
    } else {
        const u64 h = g->W == 1 ? slot_hash(Kmer<1>{lo}) : slot_hash(Kmer<2>{lo, hi});
        hipLaunchKernelGGL(k_nidx_insert, dim3(1), dim3(1), 0, ctx->stream, v, n, h);
    }
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (node_id) *node_id = n;
    return GK_OK;
}

static int graph_point_edit(gk_graph *g, bool start, uint32_t edge_id, uint32_t node_id) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    g->epoch++;
    int *d = nullptr, h = 1;
    DevScratch tmp(ctx);
    GK_HIP(ctx, tmp.get(&d, 1));
    if (start) hipLaunchKernelGGL(k_replace_start, dim3(1), dim3(1), 0, ctx->stream, g->v, edge_id, node_id, d);
    else hipLaunchKernelGGL(k_replace_end, dim3(1), dim3(1), 0, ctx->stream, g->v, edge_id, node_id, d);
    const hipError_t e = read_back(ctx, &h, d);
    if (e != hipSuccess) return hip_fail(ctx, e, "graph edit");
    if (h) return fail(ctx, GK_E_INVALID, std::string(start ? "gk_graph_replace_start" : "gk_graph_replace_end") + ": no such live edge / node");
    return GK_OK;
}
int gk_graph_replace_start(gk_graph *g, uint32_t edge_id, uint32_t new_start_node) { return graph_point_edit(g, true, edge_id, new_start_node); }   // :197-202
int gk_graph_replace_end(gk_graph *g, uint32_t edge_id, uint32_t new_end_node) { return graph_point_edit(g, false, edge_id, new_end_node); }       // :204-209

int gk_graph_nodes_by_id(gk_graph *g, const uint32_t *ids, uint64_t n, uint64_t *lo, uint64_t *hi, uint8_t *alive, uint32_t *in_deg, uint32_t *out_deg) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (n == 0) return GK_OK;
    if (!ids || !lo || !hi || !alive || !in_deg || !out_deg) return fail(ctx, GK_E_INVALID, "gk_graph_nodes_by_id: null argument");
    u32 *d_ids = nullptr, *d_in = nullptr, *d_out = nullptr;
    u64 *d_lo = nullptr, *d_hi = nullptr;
    uint8_t *d_al = nullptr;
    DevScratch tmp(ctx);
    tmp.upload(&d_ids, ids, n);
    tmp.get(&d_in, n);
    tmp.get(&d_out, n);
    tmp.get(&d_lo, n);
    tmp.get(&d_hi, n);
    tmp.get(&d_al, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_nodes_by_id");
    hipLaunchKernelGGL(k_nodes_by_id, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, g->v, d_ids, n, d_lo, d_hi, d_al, d_in, d_out);
    const hipError_t e = read_back(ctx, {{lo, d_lo, n * 8}, {hi, d_hi, n * 8}, {alive, d_al, n}, {in_deg, d_in, n * 4}, {out_deg, d_out, n * 4}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_nodes_by_id");
    return GK_OK;
}

int gk_graph_edges_by_id(gk_graph *g, const uint32_t *ids, uint64_t n, uint32_t *start_node, uint32_t *end_node, uint64_t *len, uint8_t *first_base, uint8_t *alive) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (n == 0) return GK_OK;
    if (!ids || !start_node || !end_node || !len || !first_base || !alive) return fail(ctx, GK_E_INVALID, "gk_graph_edges_by_id: null argument");
    u32 *d_ids = nullptr, *d_s = nullptr, *d_e = nullptr;
    u64 *d_len = nullptr;
    uint8_t *d_f = nullptr, *d_al = nullptr;
    DevScratch tmp(ctx);
    tmp.upload(&d_ids, ids, n);
    tmp.get(&d_s, n);
    tmp.get(&d_e, n);
    tmp.get(&d_len, n);
    tmp.get(&d_f, n);
    tmp.get(&d_al, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_edges_by_id");
    hipLaunchKernelGGL(k_edges_by_id, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, g->v, d_ids, n, d_s, d_e, d_len, d_f, d_al);
    const hipError_t e = read_back(ctx, {{start_node, d_s, n * 4}, {end_node, d_e, n * 4}, {len, d_len, n * 8}, {first_base, d_f, n}, {alive, d_al, n}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_edges_by_id");
    return GK_OK;
}

}  // extern "C"
