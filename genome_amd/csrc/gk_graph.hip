// gk_graph.hip — de Bruijn graph build from a k-mer table as HIP kernels (gfx950).  The only graph file that knows what a table
// slot is; everything that works on a built graph (simplification, components, exports, edits) is gk_graph_ops.hip.
//
// Reference path replaced (S/ = the reference's src/main/scala/ru/ifmo/genome/):
//   Graph.buildGraph      S/data/graph/Graph.scala:269-382   k_classify, k_collect_bits,
//                                                            k_make_nodes, k_walk
//   contains/incoming/outcoming          :270-282            gk::table_find_either (gk_device.h)
//   MapGraph.addNode/addEdge             :172-190            node/edge arrays (gk_graph.h, gk_graph_ops.hip graph_alloc_*)
//
// Layout in HBM: the k-mer table (array of 16/32-B slots) carries the degree annotation in its
// `aux` word (in-mask, out-mask, TERMINAL, SECONDARY) so one probe during a walk touches one
// sector.  The graph itself is structure-of-arrays: node k-mers, a 4-entry out-edge table per node
// (indexed by first base) plus its insertion order (the reference's immutable Map1..Map4 order),
// in-degree; edges as (start, end, length, byte offset) into one 2-bit-packed sequence pool.
// All kernels are integer, HBM/latency bound; no MFMA.
//
// Ids: node/edge ids are array indices in compaction order — arbitrary, like the reference's
// AtomicLong ids under `.par`; results are compared on canonical serialisations.
#include <algorithm>
#include <chrono>
#include <string>

#include "gk_graph.h"
#include "gk_scan.h"

// ---------------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------------
template <class T> struct is_mb { static constexpr bool value = false; };
template <int W> struct is_mb<MbTable<W>> { static constexpr bool value = true; };
// score of one m-mer as minimizer_score has it: hash of its canonical form (gk_device.h)
__device__ __forceinline__ u32 mmer_score(u32 w, int m) {
    const u32 r = (u32)revcomp(Kmer<1>{(u64)w}, m).lo;
    return hash32(w < r ? w : r);
}

// incoming | outcoming << 4 of the stored k-mer y (Graph.scala:270-282): the eight neighbour lookups of the classify; a neighbour
// whose bit is set in `skip` is not looked up here and counts as absent (the distributed classify asks its owner instead)
template <int W, class TT>
__device__ __forceinline__ u32 neighbour_masks(const TT &t, int k, Kmer<W> y, u32 skip) {
    u32 in = 0, out = 0;
    // The 8 lookups are independent, but each is a dependent chain that starts with a cold random
    // sector; done one after the other a lane has ONE miss in flight (168 ms for 1.5e8 16-byte keys).
    // So: prepare all 8 (canonical orientation, segment, start slot), touch the 8 first sectors
    // back to back, then resolve — the later probes of a lookup mostly stay in the sector it opened.
    // The first probed slot's key word is KEPT (eight registers): with 16 waves x 64 lanes x 8 lookups in flight per
    // CU the touched lines (0.5 MB) do not survive in the 32 KiB L1 — nor, 32 CUs to an XCD, in its 4 MiB L2 — until the
    // resolve loop comes back to them, and re-reading them there fetched most sectors from memory TWICE.
    Kmer<W> q[8];
    ProbeAt<W> pa[8];
    u64 w0v[8];
    u32 ties = 0;
    // (minimizer-bucketed table: the candidates' buckets from ONE pass over this k-mer's m-mers — a candidate shares k - 1
    //  bases with it, so its minimizer is the minimum of the shared windows' scores and of its one new window)
    u32 base_succ = 0xffffffffu, base_pred = 0xffffffffu;
    const int mm_ = k < 11 ? k : 11;
    if constexpr (is_mb<TT>::value) {
        const int nwin = k - mm_ + 1;
        u32 mid = 0xffffffffu, s_first = 0xffffffffu, s_last = 0xffffffffu;
        for (int wdw = 0; wdw < nwin; wdw++) {
            const u32 sc = mmer_score((u32)window_bits(y, 2 * wdw) & (u32)low_mask(2 * mm_), mm_);
            if (wdw == 0) s_first = sc;
            if (wdw == nwin - 1) s_last = sc;
            if (wdw != 0 && wdw != nwin - 1) mid = min(mid, sc);
        }
        base_succ = nwin > 1 ? min(mid, s_last) : 0xffffffffu;          // windows 1 .. nwin-1 of y = windows 0 .. nwin-2 of a successor
        base_pred = nwin > 1 ? min(mid, s_first) : 0xffffffffu;         // windows 0 .. nwin-2 of y = windows 1 .. nwin-1 of a predecessor
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (skip >> j & 1u) { w0v[j] = KEY_EMPTY; continue; }            // (asked elsewhere: reads as "not here")
        const Kmer<W> x = (j & 1) ? append_base(y, j >> 1, k) : prepend_base(j >> 1, y, k);
        const Kmer<W> rc = revcomp(x, k);
        const i32 hx = ref_hash(x), hr = ref_hash(rc);
        if ((hx == hr || t.both) && !(x == rc)) ties |= 1u << j;   // both strands may be stored: slow path below
        q[j] = hx < hr ? x : rc;
        if constexpr (is_mb<TT>::value) {
            const u32 neww = (u32)window_bits(x, (j & 1) ? 2 * (k - mm_) : 0) & (u32)low_mask(2 * mm_);
            const u32 score = min((j & 1) ? base_succ : base_pred, mmer_score(neww, mm_));
            pa[j] = probe_at_bucket(t, q[j], (u32)(((u64)hash32(score ^ 0x5bd1e995u) * (u64)t.nb) >> 32));
        } else {
            pa[j] = probe_at(t, q[j], k);
        }
        w0v[j] = pa[j].reg[pa[j].pos].w0;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        bool hit;
        if (ties >> j & 1u) {
            bool f;
            const Kmer<W> x = (j & 1) ? append_base(y, j >> 1, k) : prepend_base(j >> 1, y, k);
            hit = table_find_either(t, x, k, &f) >= 0;
        } else {
            // first slot from the register; only a slot that is occupied by ANOTHER key sends the probe on (to memory)
            if (w0v[j] == KEY_EMPTY) hit = false;
            else {
                bool first_is_it;
                if constexpr (W == 1) first_is_it = w0v[j] == q[j].lo;
                else { const Stored<2> sk = to_stored(q[j]); first_is_it = w0v[j] == sk.w0 && pa[j].reg[pa[j].pos].w1 == sk.w1; }
                hit = first_is_it || probe_find(pa[j], q[j], true) >= 0;
            }
        }
        if (hit) { if (j & 1) out |= 1u << (j >> 1); else in |= 1u << (j >> 1); }
    }
    return in | (out << 4);
}

// op1 of Graph.buildGraph (Graph.scala:320-329) for every live stored key: incoming/outcoming
// through `contains` on both strands (:270-282), 8 lookups per key; result kept in the slot.
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_classify(TT t, int k, unsigned long long *n_term /* [0] terminal k-mers, [2] their out-edges */,
                                                    unsigned long long *termbits /* bit i of word i / 64: slot i is a terminal k-mer (and not SECONDARY) */) {
    // The table this runs on is 40 % full (map_compact): walking the slots directly leaves 60 % of every wave idle through
    // the eight lookups.  A workgroup therefore takes CLASSIFY_SPT slots per thread at a time, compacts the live ones'
    // indices into LDS (ballot + one LDS atomic per wave) and classifies from that dense list: every lane has work, and a
    // wave keeps 64 x 8 independent sectors in flight instead of ~26 x 8.
    constexpr int SPT = 8;
    __shared__ u32 s_cnt, s_n, s_edges;
    __shared__ uint16_t s_idx[BLOCK * SPT];
    // The terminal slots of this round's window as a bitmap, written out once per round: what k_collect_bits turns into the
    // terminal list WITHOUT reading the table again (the separate pass over all slots was 2.5 ms of C3's buildGraph).
    __shared__ u32 s_tb[BLOCK * SPT / 32];
    if (threadIdx.x == 0) { s_cnt = 0; s_edges = 0; }
    u32 cnt = 0, edges = 0;
    const u64 ncap = t.capacity();
    const int lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * (BLOCK * SPT); base < ncap; base += (u64)gridDim.x * (BLOCK * SPT)) {
        __syncthreads();                                    // the previous round's list has been consumed (and its bitmap written)
        if (threadIdx.x == 0) s_n = 0;
        if (threadIdx.x < BLOCK * SPT / 32) s_tb[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SPT; q++) {
            const u64 i = base + (u64)q * BLOCK + threadIdx.x;
            const bool live = i < ncap && slot_live(&t.slots[i]);
            const unsigned long long mask = __ballot(live);
            u32 wbase = 0;
            if (lane == 0 && mask) wbase = atomicAdd(&s_n, (u32)__popcll(mask));
            wbase = __shfl(wbase, 0);
            if (live) s_idx[wbase + (u32)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)(q * BLOCK + threadIdx.x);
        }
        __syncthreads();
        const u32 nlive = s_n;
    for (u32 li = threadIdx.x; li < nlive; li += BLOCK) {
        const u64 i = base + s_idx[li];
        Slot<W> *s = &t.slots[i];
        Kmer<W> y = slot_key(t, i);
        const u32 io = neighbour_masks<W>(t, k, y, 0u);
        const u32 in = io & 15u, out = io >> 4;
        const int ni = __popc(in), no = __popc(out);
        u32 aux = in | (out << 4);
        const bool term = (ni != 1 || no != 1) && (ni != 0 || no != 0);     // Graph.scala:323
        if (term) aux |= AUX_TERMINAL;
        // hash-rule tie (FreqFilter.scala:31-32): x and rc(x) may both be stored; the larger one
        // is marked SECONDARY so the pair yields one pair of nodes
        Kmer<W> rc = revcomp(y, k);
        bool secondary = false;
        if ((t.both || ref_hash(y) == ref_hash(rc)) && !(y == rc) && kmer_less(rc, y) && table_find(t, rc, k) >= 0) secondary = true;
        if (secondary) aux |= AUX_SECONDARY;
        s->aux = aux;
        if (term && !secondary) {
            cnt++;
            // out(y) + out(rc y) = popc(out) + popc(in); a palindrome (y == rc y, even k) is ONE node
            edges += (y == rc) ? (u32)no : (u32)(ni + no);
            const u32 w = s_idx[li];
            atomicOr(&s_tb[w >> 5], 1u << (w & 31u));
        }
    }
        __syncthreads();
        if (threadIdx.x < BLOCK * SPT / 64) {
            const u64 word = (base >> 6) + threadIdx.x;
            if (word * 64 < ncap) termbits[word] = (unsigned long long)s_tb[2 * threadIdx.x] | ((unsigned long long)s_tb[2 * threadIdx.x + 1] << 32);
        }
    }
    __syncthreads();
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (edges) atomicAdd(&s_edges, edges);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) { atomicAdd(&n_term[0], (unsigned long long)s_cnt); atomicAdd(&n_term[2], (unsigned long long)s_edges); }
}

// ---------------------------------------------------------------------------------------------
// The classify over a PartitionedDNAMap (SURVEY.md 8(e) "beyond counting"; the reference ships the classify closure to every
// partition, Graph.scala:320-329 through PartitionedDNAMap.mapReduce :55-58).  Every rank classifies ITS keys: a neighbour
// whose owner (gk::owner_of: the strand-symmetric minimizer, so x and rc(x) agree) is this rank is looked up here, the others
// are asked of their owners — one query all-to-all of canonical keys, one answer all-to-all of bytes (gk_dist.hip) — and the
// 8-bit (incoming, outcoming) mask of every key ends in its slot's annotation word, to travel with the key in the gather.
//   k_dc_scan<W, false>: slots [s0, s1): local lookups -> aux = mask of the local hits; remote neighbours counted per owner
//   k_dc_scan<W, true> : the same enumeration; every remote neighbour's canonical key goes to its owner's region of `qkeys`
//                        and (slot << 3 | j) to the same position of `qref`
//   k_dc_answer        : `contains` for every received key
//   k_dc_apply         : answers back in query order: aux |= bit
// A neighbour shares k - 1 bases with the k-mer, so its minimizer is the minimum over the shared m-mers and its one new m-mer
// (the same trick as the minimizer-bucketed table's classify above).
// ---------------------------------------------------------------------------------------------
template <int W, bool FILL>
__global__ __launch_bounds__(BLOCK) void k_dc_scan(Table<W> t, int k, int rank, int P, u64 s0, u64 s1, unsigned long long *cnt /* [P]: totals (count) / cursors (fill) */,
                                                   const unsigned long long *off /* [P] first query of each owner's region */, u64 *qkeys, u64 *qref) {
    __shared__ u32 s_cnt[64];
    __shared__ unsigned long long s_base[64];
    const int mm_ = k < 11 ? k : 11;
    const int nwin = k - mm_ + 1;
    const u64 per_round = (u64)gridDim.x * BLOCK;
    const u64 nrounds = (s1 - s0 + per_round - 1) / per_round;          // the same for every workgroup: the barriers below are uniform
    for (u64 r = 0; r < nrounds; r++) {
        const u64 i = s0 + r * per_round + (u64)blockIdx.x * BLOCK + threadIdx.x;
        __syncthreads();
        if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        bool live = i < s1 && slot_live(&t.slots[i]);
        // (the counting pass leaves "which neighbours are remote" in bits 8..15 of the annotation word: the filling pass skips the
        //  keys that have none — most of them — without going over their m-mers again)
        if (FILL && live && ((t.slots[i].aux >> 8) & 0xffu) == 0u) live = false;
        u32 remote = 0;                 // bit j: neighbour j lives on another rank
        u64 owners = 0;                 // 6 bits per neighbour
        Kmer<W> y{};
        if (live) {
            y = slot_key(t, i);
            u32 mid = 0xffffffffu, s_first = 0xffffffffu, s_last = 0xffffffffu;
            for (int wdw = 0; wdw < nwin; wdw++) {
                const u32 sc = mmer_score((u32)window_bits(y, 2 * wdw) & (u32)low_mask(2 * mm_), mm_);
                if (wdw == 0) s_first = sc;
                if (wdw == nwin - 1) s_last = sc;
                if (wdw != 0 && wdw != nwin - 1) mid = min(mid, sc);
            }
            const u32 base_succ = nwin > 1 ? min(mid, s_last) : 0xffffffffu, base_pred = nwin > 1 ? min(mid, s_first) : 0xffffffffu;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const Kmer<W> x = (j & 1) ? append_base(y, j >> 1, k) : prepend_base(j >> 1, y, k);
                const u32 neww = (u32)window_bits(x, (j & 1) ? 2 * (k - mm_) : 0) & (u32)low_mask(2 * mm_);
                const u32 score = min((j & 1) ? base_succ : base_pred, mmer_score(neww, mm_));
                const u32 o = (u32)(((u64)hash32(score ^ 0x5bd1e995u) * (u64)P) >> 32);          // == gk::owner_of(x, k, P)
                if ((int)o != rank) { remote |= 1u << j; owners |= (u64)o << (6 * j); }
            }
        }
        u32 posv[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            posv[j] = 0;
            if (remote >> j & 1u) posv[j] = atomicAdd(&s_cnt[(owners >> (6 * j)) & 63u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < P && s_cnt[threadIdx.x]) {
            const unsigned long long b = atomicAdd(&cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
            if (FILL) s_base[threadIdx.x] = b;
        }
        if constexpr (!FILL) {
            if (live) t.slots[i].aux = neighbour_masks<W>(t, k, y, remote) | (remote << 8);
        } else {
            __syncthreads();
            if (live) {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    if (!(remote >> j & 1u)) continue;
                    const u32 o = (u32)(owners >> (6 * j)) & 63u;
                    const Kmer<W> x = (j & 1) ? append_base(y, j >> 1, k) : prepend_base(j >> 1, y, k);
                    const Kmer<W> rc = revcomp(x, k);
                    const Kmer<W> q = ref_hash(x) < ref_hash(rc) ? x : rc;          // the orientation a counting table stores
                    const u64 at = off[o] + s_base[o] + posv[j];
                    if constexpr (W == 1) qkeys[at] = q.lo;
                    else { qkeys[2 * at] = q.lo; qkeys[2 * at + 1] = q.hi; }
                    qref[at] = (i << 3) | (u64)j;
                }
            }
        }
    }
}
// `contains` (Graph.scala:270-272) of canonical keys another rank asks about
template <int W>
__global__ __launch_bounds__(BLOCK) void k_dc_answer(Table<W> t, int k, const u64 *__restrict__ keys, u64 n, uint8_t *ans) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        Kmer<W> x;
        if constexpr (W == 1) x = Kmer<1>{keys[i]};
        else x = Kmer<2>{keys[2 * i], keys[2 * i + 1]};
        bool f;
        ans[i] = table_find_either(t, x, k, &f) >= 0 ? 1 : 0;
    }
}
template <int W>
__global__ __launch_bounds__(BLOCK) void k_dc_apply(Table<W> t, const u64 *__restrict__ qref, const uint8_t *__restrict__ ans, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        if (!ans[i]) continue;
        const u64 ref = qref[i];
        const int j = (int)(ref & 7u);
        atomicOr(&t.slots[ref >> 3].aux, (j & 1) ? 16u << (j >> 1) : 1u << (j >> 1));
    }
}
// what k_classify derives from the masks that came with a gathered table (terminal, the SECONDARY mark of a hash-rule tie, the count of terminal k-mers)
template <int W>
__global__ __launch_bounds__(BLOCK) void k_finish_masks(Table<W> t, int k, unsigned long long *n_term, unsigned long long *termbits) {
    __shared__ u32 s_cnt, s_edges;
    if (threadIdx.x == 0) { s_cnt = 0; s_edges = 0; }
    __syncthreads();
    u32 cnt = 0, edges = 0;
    const u64 ncap = t.capacity();
    // (wave-uniform trip count: a wave's 64 lanes hold 64 consecutive slots = one word of the terminal bitmap)
    for (u64 i0 = (u64)blockIdx.x * BLOCK + (threadIdx.x & ~63u); i0 < ncap; i0 += (u64)gridDim.x * BLOCK) {
        const u64 i = i0 + (threadIdx.x & 63u);
        bool is_term = false;
        if (i < ncap && slot_live(&t.slots[i])) {
        u32 aux = t.slots[i].aux & 0xffu;
        const int ni = __popc(aux & 15u), no = __popc(aux >> 4);
        const bool term = (ni != 1 || no != 1) && (ni != 0 || no != 0);     // Graph.scala:323
        if (term) aux |= AUX_TERMINAL;
        const Kmer<W> y = slot_key(t, i);
        const Kmer<W> rc = revcomp(y, k);
        bool secondary = false;
        if ((t.both || ref_hash(y) == ref_hash(rc)) && !(y == rc) && kmer_less(rc, y) && table_find(t, rc, k) >= 0) secondary = true;
        if (secondary) aux |= AUX_SECONDARY;
        t.slots[i].aux = aux;
        if (term && !secondary) { cnt++; edges += (y == rc) ? (u32)no : (u32)(ni + no); is_term = true; }
        }
        const unsigned long long word = __ballot(is_term);
        if ((threadIdx.x & 63u) == 0) termbits[i0 >> 6] = word;
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    if (edges) atomicAdd(&s_edges, edges);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) { atomicAdd(&n_term[0], (unsigned long long)s_cnt); atomicAdd(&n_term[2], (unsigned long long)s_edges); }
}

// The terminal slots, compacted — from the bitmap the classify left (one word per 64 slots), not from the table: a thread takes one
// word, a workgroup reserves its output with ONE atomic per 256 words (the cursor is a single address: same-address atomics retire
// at ~88 per microsecond chip-wide).  Slots come out in ascending order inside a workgroup's share.
__global__ __launch_bounds__(BLOCK) void k_collect_bits(const unsigned long long *__restrict__ termbits, u64 nwords, u64 *tslots, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (nwords + BLOCK - 1) / BLOCK;
    for (u64 g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const u64 w = g * BLOCK + threadIdx.x;
        unsigned long long bits = w < nwords ? termbits[w] : 0ull;
        u64 o = block_reserve((u32)__popcll(bits), cursor, lds4, &s_base);
        while (bits) {
            const int b = __ffsll((long long)bits) - 1;
            tslots[o++] = w * 64 + (u64)b;
            bits &= bits - 1;
        }
    }
}

// nodeMap (Graph.scala:343-347): node 2j = the stored terminal k-mer, node 2j+1 = its reverse
// complement (termKmers = set ++ set.map(revComplement), :330-333); plus the (node, base) stubs of
// buildEdges (:351): one edge per outgoing base, in A,G,C,T order.
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_make_nodes(TT t, int k, const u64 *tslots, u64 nT, GraphView g,
                                                      unsigned long long *ecursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (nT + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 j = grp * BLOCK + threadIdx.x;
        u32 m0 = 0, m1 = 0;
        Kmer<W> y{}, rc{};
        bool pal = false;
        if (j < nT) {
            const u64 slot = tslots[j];
            const u32 aux = t.slots[slot].aux;
            y = slot_key(t, slot);
            rc = revcomp(y, k);
            pal = (y == rc);
            m0 = (aux >> 4) & 15u;                  // outcoming(y)
            m1 = pal ? 0u : rev4(aux & 15u);        // outcoming(rc y) = complemented incoming(y)
            t.slots[slot].aux = AUX_NODE | (u32)j;          // (nT < 2^31 is checked by the host)
        }
        u64 e = block_reserve((u32)(__popc(m0) + __popc(m1)), ecursor, lds4, &s_base);
        if (j < nT) {
            const u32 n0 = (u32)(2 * j), n1 = n0 + 1;
            g.node_lo[n0] = y.lo; g.node_lo[n1] = rc.lo;
            if constexpr (W == 2) { g.node_hi[n0] = y.hi; g.node_hi[n1] = rc.hi; }
            else { g.node_hi[n0] = 0; g.node_hi[n1] = 0; }
            g.node_alive[n0] = 1; g.node_alive[n1] = pal ? 0 : 1;
            for (int side = 0; side < 2; side++) {
                const u32 n = side ? n1 : n0, m = side ? m1 : m0;
                u32 ord = 0;
                for (int b = 0; b < 4; b++) {
                    u32 id = NONE;
                    if (m & (1u << b)) {
                        id = (u32)e++;
                        g.e_start[id] = n;
                        g.e_first[id] = (uint8_t)b;
                        g.e_alive[id] = 1;
                        ord = order_append(ord, b);
                    }
                    g.out_edge[(u64)n * 4 + b] = id;
                }
                g.out_order[n] = ord;
            }
        }
    }
}

// buildEdges (Graph.scala:349-365): from a node, follow the unique outgoing base until the next
// terminal k-mer.  One lane per edge; every step is one dependent table probe.
// pass 0: walk once — end node, length, in-degree — keeping the first WALK_BUF bases in registers; the workgroup then
//         reserves the pool bytes of ALL its edges with one atomic and an edge that fits the registers (nearly all of
//         them on a bushy error graph: 7 bases on average at C3) writes its sequence straight away.
// pass 1: only for edges longer than WALK_BUF: walk again and emit the bases 2 bits each at e_off (assigned in pass 0).
static constexpr u32 WALK_BUF = 128;          // bases kept in four 64-bit registers
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_walk(TT t, int k, GraphView g, int pass, u64 max_steps,
                                                unsigned long long *pool_cursor, unsigned long long *n_long, u32 *err) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const u64 ngroups = (g.n_edges + BLOCK - 1) / BLOCK;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 e = grp * BLOCK + threadIdx.x;
        const bool active = e < g.n_edges && (pass == 0 || g.e_len[e] > WALK_BUF);
        u64 len = 0;
        u64 b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (active) {
            const u32 n = g.e_start[e];
            const int first = g.e_first[e];
            Kmer<W> cur = append_base(node_kmer<W>(g, n), first, k);       // read.drop(1) :+ base  :353
            len = 1;
            u32 acc = (u32)first;                                           // builder += base        :352
            b0 = (u64)first;
            const u64 off = pass ? g.e_off[e] : 0;
            u32 end = NONE;
            for (u64 step = 0; step <= max_steps; step++) {
                bool fwd;
                i64 slot = table_find_either(t, cur, k, &fwd);
                if (slot < 0) { *err = 1; break; }
                const u32 aux = t.slots[slot].aux;
                if (aux & AUX_NODE) {                                       // nodeMap.contains(seq)  :355
                    end = aux_node(aux, fwd);
                    break;
                }
                const u32 om = fwd ? ((aux >> 4) & 15u) : rev4(aux & 15u);  // outcoming(seq)         :356
                if (__popc(om) != 1) { *err = 2; break; }                   // assert(out.size == 1)  :357
                const int nb = __ffs(om) - 1;
                if (pass) {
                    acc |= (u32)nb << ((len & 3) * 2);
                    if ((len & 3) == 3) { g.pool[off + (len >> 2)] = (uint8_t)acc; acc = 0; }
                } else if (len < WALK_BUF) {
                    const u64 bits = (u64)nb << ((len & 31) * 2);
                    if (len < 32) b0 |= bits; else if (len < 64) b1 |= bits; else if (len < 96) b2 |= bits; else b3 |= bits;
                }
                len++;
                cur = append_base(cur, nb, k);                              // seq.drop(1) :+ out(0)  :360
            }
            if (pass) {
                if (len & 3) g.pool[off + (len >> 2)] = (uint8_t)acc;
            } else {
                g.e_end[e] = end;
                g.e_len[e] = len;
                if (end != NONE) atomicAdd(&g.in_deg[end], 1u);             // end.inEdgeIds += id    :181
                else *err = 3;
            }
        }
        if (pass) continue;
        // pool bytes of this workgroup's edges: one atomic (per-block totals stay < 2^32 for edges up to 16M bases; longer ones reserve alone)
        const u64 bytes = active ? (len + 3) / 4 : 0;
        const u32 small = bytes < (1u << 22) ? (u32)bytes : 0u;
        u64 o = block_reserve(small, pool_cursor, lds4, &s_base);
        if (!active) continue;
        if (small != bytes) o = atomicAdd(pool_cursor, (unsigned long long)bytes);
        g.e_off[e] = o;
        if (len > WALK_BUF) { atomicAdd(n_long, 1ull); continue; }
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const u64 word = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((u64)(w * 8 + j) < bytes) g.pool[o + w * 8 + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

// The same walk, fed from a queue.  With one edge per lane a wave lasts as long as its LONGEST edge: on an error graph the
// mean edge is 7 bases and the longest of 64 is ten times that, so nine lanes in ten idle (17 of C3's 59 ms).  Here a lane
// that finishes its edge takes the next one: a wave claims 1024 consecutive edges from the global queue with one atomic
// (a claim per edge, or per refill, would be millions of atomics on ONE address at ~88 per microsecond) and hands them to
// its idle lanes by ballot.  Nothing else in the loop is shared: the first WALK_BUF bases of an edge go to a 32-byte staging
// slot per edge, and k_place_edges afterwards assigns the pool offsets (one atomic per 2048 edges) and copies the staged
// bases.  Edges longer than WALK_BUF are emitted by k_walk's pass 1 as before.
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_walk_q(TT t, int k, GraphView g, u64 max_steps,
                                                  unsigned long long *queue, ulonglong2 *stage, unsigned long long *n_long, u32 *err) {
    constexpr u64 CHUNK = 1024;
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    u64 loc_next = 0, loc_end = 0;                 // wave-uniform: claimed edges not yet handed to a lane
    bool drained = false;                          // wave-uniform: the global queue is empty
    bool have = false;
    u64 e = 0, len = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    Kmer<W> cur{};
    u32 longs = 0;
    for (;;) {
        // ---- idle lanes take edges
        for (int attempt = 0; attempt < 2; attempt++) {
            const unsigned long long need = __ballot(!have);
            if (!need) break;
            const u64 avail = loc_end - loc_next;
            const u64 rank = (u64)__popcll(need & lt_mask);
            if (!have && rank < avail) {
                e = loc_next + rank;
                const u32 n = g.e_start[e];
                const int first = g.e_first[e];
                cur = append_base(node_kmer<W>(g, n), first, k);           // read.drop(1) :+ base  :353
                len = 1;
                b0 = (u64)first; b1 = b2 = b3 = 0;                          // builder += base        :352
                have = true;
            }
            loc_next += min((u64)__popcll(need), avail);
            if (loc_next < loc_end || drained) break;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(queue, (unsigned long long)CHUNK);
            base = __shfl(base, 0);
            if (base >= g.n_edges) { drained = true; loc_next = loc_end = 0; break; }
            loc_next = base;
            loc_end = min((u64)base + CHUNK, g.n_edges);
        }
        if (!__ballot(have)) { if (drained) break; else continue; }
        // ---- one step of every lane that holds an edge
        if (have) {
            bool fwd;
            const i64 slot = table_find_either(t, cur, k, &fwd);
            u32 end = NONE;
            bool finished = false;
            if (slot < 0) { *err = 1; finished = true; }
            else {
                const u32 aux = t.slots[slot].aux;
                if (aux & AUX_NODE) {                                       // nodeMap.contains(seq)  :355
                    end = aux_node(aux, fwd);
                    finished = true;
                } else {
                    const u32 om = fwd ? ((aux >> 4) & 15u) : rev4(aux & 15u);  // outcoming(seq)     :356
                    if (__popc(om) != 1) { *err = 2; finished = true; }     // assert(out.size == 1)  :357
                    else if (len > max_steps) { *err = 3; finished = true; }
                    else {
                        const int nb = __ffs(om) - 1;
                        if (len < WALK_BUF) {
                            const u64 bits = (u64)nb << ((len & 31) * 2);
                            if (len < 32) b0 |= bits; else if (len < 64) b1 |= bits; else if (len < 96) b2 |= bits; else b3 |= bits;
                        }
                        len++;
                        cur = append_base(cur, nb, k);                      // seq.drop(1) :+ out(0)  :360
                    }
                }
            }
            if (finished) {
                g.e_end[e] = end;
                g.e_len[e] = len;
                if (end != NONE) atomicAdd(&g.in_deg[end], 1u);             // end.inEdgeIds += id    :181
                else *err = 3;
                if (len > WALK_BUF) longs++;
                else {
                    stage[2 * e] = make_ulonglong2(b0, b1);
                    if (len > 64) stage[2 * e + 1] = make_ulonglong2(b2, b3);
                }
                have = false;
            }
        }
    }
    for (int d = 32; d; d >>= 1) longs += __shfl_down(longs, d);
    if (lane == 0 && longs) atomicAdd(n_long, (unsigned long long)longs);
}

// pool offsets of all edges (each starts on a byte boundary) + the staged bases of the short ones into the pool.
// A workgroup takes 8 consecutive edges per thread and reserves their bytes with ONE atomic.
__global__ __launch_bounds__(BLOCK) void k_place_edges(GraphView g, const ulonglong2 *stage, unsigned long long *cursor) {
    __shared__ u32 lds4[BLOCK / 64];
    __shared__ unsigned long long s_base;
    constexpr int EPT = 8;
    const u64 per_block = (u64)BLOCK * EPT;
    const u64 ngroups = (g.n_edges + per_block - 1) / per_block;
    for (u64 grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const u64 e0 = grp * per_block + (u64)threadIdx.x * EPT;
        u64 bytes[EPT];
        u32 small = 0;
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            bytes[j] = e0 + j < g.n_edges ? (g.e_len[e0 + j] + 3) / 4 : 0;
            if (bytes[j] < (1u << 22)) small += (u32)bytes[j];       // (per-block totals stay < 2^32; a longer edge reserves alone)
        }
        u64 o = block_reserve(small, cursor, lds4, &s_base);
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            const u64 e = e0 + j;
            if (e >= g.n_edges) break;
            const u64 nb = bytes[j];
            u64 at = o;
            if (nb < (1u << 22)) o += nb; else at = atomicAdd(cursor, (unsigned long long)nb);
            g.e_off[e] = at;
            if (nb > WALK_BUF / 4) continue;                          // a long edge: k_walk pass 1 emits it
            const ulonglong2 lo = stage[2 * e];
            ulonglong2 hi = make_ulonglong2(0, 0);
            if (nb > 16) hi = stage[2 * e + 1];
            for (u64 q = 0; q < nb; q++) {
                const u64 word = q < 8 ? lo.x : q < 16 ? lo.y : q < 24 ? hi.x : hi.y;
                g.pool[at + q] = (uint8_t)(word >> (8 * (q & 7)));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Unitigs by POINTER JUMPING (list ranking) instead of one lane walking each edge base by base:
// k_walk is one dependent probe per base, so a single 4.6 Mbp unitig (an error-free bacterial
// genome) costs 2 x 4.6M x ~1 us = 10 s on one lane.  Here every ORIENTED interior k-mer
// (id = 2 * rank of its slot among the live slots + orientation; interior = non-terminal with exactly one successor) starts with a
// pointer to its successor and distance 1, pre-terminals (successor is a terminal k-mer) absorb,
// and log2(longest unitig) rounds of  d[u] += d[next[u]]; next[u] = next[next[u]]  give every
// interior k-mer its pre-terminal and its distance to it.  From that:
//   edge (s, b): u0 = s.drop(1) :+ b;  len = d[u0] + 2;  end = successor of pt[u0]
//   the base appended after interior u (position j+1 of its edge, u = u_j) is placed by u itself:
//   the chain of rc(u) runs rc(u_{j-1}), ..., rc(u_0), rc(s), so j = d[rc u], u0 = rc(pt[rc u]),
//   s = rc(successor of pt[rc u]), b = last base of u0 — no walk anywhere.
// Members of all-(1,1) cycles never absorb and are skipped (Graph.scala:375 "perfect cycles are
// ignored").  Same results as k_walk (tests run both).
// ---------------------------------------------------------------------------------------------
// unique outgoing base of an interior oriented k-mer (from the slot's masks), -1 if not exactly one
__device__ __forceinline__ int single_out_base(u32 aux, int ori) {
    const u32 om = ori ? rev4(aux & 15u) : ((aux >> 4) & 15u);
    return __popc(om) == 1 ? __ffs(om) - 1 : -1;
}

// ---- rank of a live slot --------------------------------------------------------------------------------------------
// The pointer-jumping state is indexed by LIVE KEY, not by slot: one (live mask, live slots before) pair per 64 slots — 0.25
// bytes per slot — turns a slot index into its rank with one 16-byte read.  (Until round 3 two arrays of 2 x capacity x 16
// bytes were indexed by slot: 64 B per SLOT, 305 GB for C5's table.)
struct alignas(16) RankBlk { u64 mask; u64 base; };
static constexpr u32 RANK_CHUNK = 256;              // 64-slot blocks per chunk (16384 slots): one workgroup, one thread per block
__device__ __forceinline__ u64 rank_of(const RankBlk *rb, u64 slot) {
    const RankBlk b = rb[slot >> 6];
    return b.base + (u64)__popcll(b.mask & ((1ull << (slot & 63)) - 1ull));
}
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_rank_masks(TT t, RankBlk *rb, u64 nblk, u32 *chunk_tot, u64 nchunks) {
    __shared__ u32 s_tot;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 ncap = t.capacity();
    for (u64 c = blockIdx.x; c < nchunks; c += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) s_tot = 0;
        __syncthreads();
        u32 tot = 0;
        for (u32 j = wave; j < RANK_CHUNK; j += BLOCK / 64) {
            const u64 blk = c * RANK_CHUNK + j;
            if (blk >= nblk) break;
            const u64 i = blk * 64 + lane;
            const unsigned long long m = __ballot(i < ncap && slot_live(&t.slots[i]));
            if (lane == 0) rb[blk].mask = m;
            tot += (u32)__popcll(m);
        }
        if (lane == 0 && tot) atomicAdd(&s_tot, tot);
        __syncthreads();
        if (threadIdx.x == 0) chunk_tot[c] = s_tot;
    }
}
// exclusive scan of the chunk totals: ONE workgroup, every thread a contiguous share (3e5 chunks at C5: ~300 per thread)
__global__ __launch_bounds__(1024) void k_rank_scan(const u32 *chunk_tot, u64 *chunk_base, u64 nchunks) {
    __shared__ u64 s_sum[1024];
    const u64 per = (nchunks + 1023) / 1024, c0 = threadIdx.x * per, c1 = min(c0 + per, nchunks);
    u64 sum = 0;
    for (u64 c = c0; c < c1; c++) sum += chunk_tot[c];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) { u64 run = 0; for (int i = 0; i < 1024; i++) { const u64 v = s_sum[i]; s_sum[i] = run; run += v; } chunk_base[nchunks] = run; }
    __syncthreads();
    u64 run = s_sum[threadIdx.x];
    for (u64 c = c0; c < c1; c++) { chunk_base[c] = run; run += chunk_tot[c]; }
}
__global__ __launch_bounds__(RANK_CHUNK) void k_rank_fill(RankBlk *rb, u64 nblk, const u64 *chunk_base, u64 nchunks) {
    __shared__ u32 wsum[RANK_CHUNK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const u64 blk = c * RANK_CHUNK + threadIdx.x;
        const u32 v = blk < nblk ? (u32)__popcll(rb[blk].mask) : 0u;
        u32 inc = wave_incl_scan(v);
        __syncthreads();
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 pre = 0;
        for (int w = 0; w < wave; w++) pre += wsum[w];
        if (blk < nblk) rb[blk].base = chunk_base[c] + pre + inc - v;
    }
}
// the slot -> rank structure of table `t`: rb[0..nblk), chunk_base[nchunks] = the live slots.  Stream-ordered, no sync.
template <int W, class TT>
static void rank_build(gk_ctx *ctx, TT t, RankBlk *rb, u64 nblk, u32 *chunk_tot, u64 *chunk_base, u64 nchunks) {
    hipLaunchKernelGGL((k_rank_masks<W, TT>), dim3((int)std::min<u64>(nchunks, grid_cap(ctx))), dim3(BLOCK), 0, ctx->stream, t, rb, nblk, chunk_tot, nchunks);
    hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(1024), 0, ctx->stream, chunk_tot, chunk_base, nchunks);
    hipLaunchKernelGGL(k_rank_fill, dim3((int)std::min<u64>(nchunks, grid_cap(ctx))), dim3(RANK_CHUNK), 0, ctx->stream, rb, nblk, chunk_base, nchunks);
}

// ---- pointer-jumping state: ONE 64-bit word per oriented live k-mer (index 2 x rank + orientation), updated IN PLACE -------
//   absorbed (the successor is a terminal k-mer):  PJ_ABS | first base of this oriented k-mer << 32 | node id of that terminal
//   on its way:                                    successor index << 29 | distance covered so far (saturating)
//   not registered (terminal, secondary, (0,0)):   ~0
// A jump reads the successor's word and writes the own one; a reader that meets a word in mid-round sees either the old or
// the new state of that k-mer — both are true statements "my pointer is d steps ahead of me" — so no second buffer is needed
// (stale lines in another XCD's L2 are old states too, and kernel boundaries bring everybody up to date).
static constexpr u64 PJ_ABS = 1ull << 63, PJ_UNREG = ~0ull;
static constexpr u32 PJ_DBITS = 29;
static constexpr u64 PJ_DMAX = (1ull << PJ_DBITS) - 1ull;          // 5.4e8 bases: longer unitigs are refused (GK_E_CAPACITY)
static constexpr u64 PJ_MAX_STATES = 1ull << (63 - PJ_DBITS);      // 2^34 oriented k-mers
__device__ __forceinline__ u64 pj_pack(u64 nxt, u64 dist) { return (nxt << PJ_DBITS) | min(dist, PJ_DMAX); }
__device__ __forceinline__ u64 pj_nxt(u64 s) { return s >> PJ_DBITS; }
__device__ __forceinline__ u64 pj_dist(u64 s) { return s & PJ_DMAX; }
__device__ __forceinline__ bool pj_absorbed(u64 s) { return (s & PJ_ABS) && s != PJ_UNREG; }
__device__ __forceinline__ u32 pj_node(u64 s) { return (u32)s; }
__device__ __forceinline__ int pj_first(u64 s) { return (int)((s >> 32) & 3u); }

template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_pj_init(TT t, int k, const RankBlk *__restrict__ rb, u64 *st) {
    const u64 ncap = t.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&t.slots[i])) continue;
        const u32 aux = t.slots[i].aux;
        if (aux & (AUX_NODE | AUX_TERMINAL | AUX_SECONDARY)) continue;
        const Kmer<W> y = slot_key(t, i);
        const u64 r = rank_of(rb, i);
        for (int ori = 0; ori < 2; ori++) {
            const int nb = single_out_base(aux, ori);
            if (nb < 0) continue;                              // (0,0) k-mers are in no unitig
            const Kmer<W> u = ori ? revcomp(y, k) : y;
            bool fwd;
            const i64 ws = table_find_either(t, append_base(u, nb, k), k, &fwd);
            if (ws < 0) continue;
            const u32 wa = t.slots[ws].aux;
            if (wa & AUX_NODE) st[2 * r + ori] = PJ_ABS | ((u64)first_base(u) << 32) | (u64)aux_node(wa, fwd);     // pre-terminal: absorbs
            else st[2 * r + ori] = pj_pack(2 * rank_of(rb, (u64)ws) + (fwd ? 0u : 1u), 1);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_pj_round(u64 *st, u64 n, u32 *changed /* [0] a pointer moved, [1] error */) {
    bool ch = false;
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < n; u += (u64)gridDim.x * BLOCK) {
        const u64 su = st[u];
        if (su & PJ_ABS) continue;                          // absorbed, or not registered
        const u64 sv = st[pj_nxt(su)];                      // the one random read of the round
        if (sv == PJ_UNREG) { changed[1] = 8; continue; }   // an interior k-mer's successor is interior or terminal: cannot happen
        if (sv & PJ_ABS) continue;                          // the pointer is at the chain's pre-terminal: done
        st[u] = pj_pack(pj_nxt(sv), pj_dist(su) + pj_dist(sv));
        ch = true;
    }
    if (ch) changed[0] = 1;
}

template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_pj_edges(TT t, int k, GraphView g, const RankBlk *__restrict__ rb, const u64 *__restrict__ st, u32 *err) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        const u32 n = g.e_start[e];
        const Kmer<W> u0 = append_base(node_kmer<W>(g, n), g.e_first[e], k);
        bool fwd;
        const i64 s0 = table_find_either(t, u0, k, &fwd);
        if (s0 < 0) { *err = 1; continue; }
        u32 end = NONE;
        u64 len = 1;
        const u32 a0 = t.slots[s0].aux;
        if (a0 & AUX_NODE) {
            end = aux_node(a0, fwd);
        } else {
            const u64 s = st[2 * rank_of(rb, (u64)s0) + (fwd ? 0u : 1u)];
            u64 sp = s;                                     // the chain's pre-terminal
            if (!(s & PJ_ABS)) { sp = st[pj_nxt(s)]; len = pj_dist(s) + 2; if (pj_dist(s) == PJ_DMAX) { *err = 9; continue; } }
            else len = 2;
            if (!pj_absorbed(sp)) { *err = 4; continue; }   // unregistered / not absorbed: cannot happen on a chain that leaves a node
            end = pj_node(sp);
        }
        g.e_end[e] = end;
        g.e_len[e] = len;
        if (end != NONE) atomicAdd(&g.in_deg[end], 1u);
        else *err = 3;
    }
}

__device__ __forceinline__ void pool_or(uint8_t *pool, u64 off, u64 pos, int base) {
    const u64 byte = off + (pos >> 2);
    u32 *w = reinterpret_cast<u32 *>(pool) + (byte >> 2);
    atomicOr(w, (u32)base << (((byte & 3) * 8) + (pos & 3) * 2));
}

// every interior oriented k-mer u places the base that follows it (see the derivation above): a scan over the table's slots
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_pj_emit(TT t, int k, GraphView g, const RankBlk *__restrict__ rb, const u64 *__restrict__ st, u32 *err) {
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    for (u64 e = tid; e < g.n_edges; e += stride) pool_or(g.pool, g.e_off[e], 0, g.e_first[e]);       // builder += base  :352
    const u64 ncap = t.capacity();
    for (u64 i = tid; i < ncap; i += stride) {
        if (!slot_live(&t.slots[i])) continue;
        const u32 aux = t.slots[i].aux;
        if (aux & (AUX_NODE | AUX_TERMINAL | AUX_SECONDARY)) continue;
        const u64 r = rank_of(rb, i);
        for (int ori = 0; ori < 2; ori++) {
            const u64 su = st[2 * r + ori];
            if (su == PJ_UNREG) continue;
            const u64 sv = st[2 * r + (ori ^ 1)];               // v = rc(u): same slot, other orientation
            if (sv == PJ_UNREG) { *err = 7; continue; }         // the partner orientation must have been registered too
            const u64 pu = (su & PJ_ABS) ? su : st[pj_nxt(su)], pv = (sv & PJ_ABS) ? sv : st[pj_nxt(sv)];
            if (!pj_absorbed(pu) || !pj_absorbed(pv)) continue; // member of an all-(1,1) cycle
            const u64 dv = (sv & PJ_ABS) ? 0ull : pj_dist(sv);
            if (dv == PJ_DMAX) { *err = 9; continue; }
            const int nb = single_out_base(aux, ori);
            const u32 rs_node = pj_node(pv);                    // node of rc(s)
            if (nb < 0 || rs_node == NONE) { *err = 5; continue; }
            const u32 partner = rs_node ^ 1u;
            const u32 s_node = g.node_alive[partner] ? partner : rs_node;      // palindromic node: s == rc(s)
            const int b = 3 - pj_first(pv);                     // last base of u0 = complement of the first base of rc(u0)
            const u32 e = g.out_edge[(u64)s_node * 4 + b];
            if (e == NONE) { *err = 6; continue; }
            pool_or(g.pool, g.e_off[e], dv + 1, nb);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Perfect cycles kept (gk_graph_build_cycles; the rule: include/genome_amd.h "perfect cycles").  The table-reading half: which
// oriented k-mers the plain build left on no node and inside no edge, and — dense, for gk_cycles.hip — their successors, anchor
// keys and next bases.  The plain build has run: a terminal slot's annotation is its node, every other slot still has its masks.
// ---------------------------------------------------------------------------------------------
// oriented k-mers with one way in and one way out (a palindrome is ONE): those inside the plain build's edges, and the members
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_cyc_census(TT t, int k, unsigned long long *out) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    u32 cnt = 0;
    const u64 ncap = t.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&t.slots[i])) continue;
        const u32 aux = t.slots[i].aux;
        if (aux & (AUX_NODE | AUX_TERMINAL | AUX_SECONDARY)) continue;
        if (__popc(aux & 15u) != 1 || __popc((aux >> 4) & 15u) != 1) continue;
        const Kmer<W> y = slot_key(t, i);
        cnt += (y == revcomp(y, k)) ? 1u : 2u;
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(out, (unsigned long long)s_cnt);
}
// after the absorbing rounds (k_pj_init, k_pj_round): a registered state whose pointer has not reached a pre-terminal is on a
// cycle.  Both orientations of a palindrome were registered and nothing points at the second: it is left out.
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_cyc_members(TT t, int k, const RankBlk *__restrict__ rb, const u64 *__restrict__ st, u32 *flag) {
    const u64 ncap = t.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&t.slots[i])) continue;
        const u32 aux = t.slots[i].aux;
        if (aux & (AUX_NODE | AUX_TERMINAL | AUX_SECONDARY)) continue;
        const Kmer<W> y = slot_key(t, i);
        const bool pal = y == revcomp(y, k);
        const u64 r = rank_of(rb, i);
        for (int ori = 0; ori < (pal ? 1 : 2); ori++) {
            const u64 su = st[2 * r + ori];
            if (su == PJ_UNREG) continue;
            const u64 pu = (su & PJ_ABS) ? su : st[pj_nxt(su)];
            if (!pj_absorbed(pu)) flag[2 * r + ori] = 1u;
        }
    }
}
template <int W, class TT>
__global__ __launch_bounds__(BLOCK) void k_cyc_fill(TT t, int k, const RankBlk *__restrict__ rb, const u32 *__restrict__ flag,
                                                    const unsigned long long *__restrict__ off, CycleMembers cm, u32 *err) {
    const u64 ncap = t.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&t.slots[i])) continue;
        const u32 aux = t.slots[i].aux;
        if (aux & (AUX_NODE | AUX_TERMINAL | AUX_SECONDARY)) continue;
        const u64 r = rank_of(rb, i);
        if (!flag[2 * r] && !flag[2 * r + 1]) continue;
        const Kmer<W> y = slot_key(t, i), ry = revcomp(y, k);
        const bool pal = y == ry;
        for (int ori = 0; ori < 2; ori++) {
            const u64 u = 2 * r + ori;
            if (!flag[u]) continue;
            const u64 d = off[u];
            if (d >= cm.n) { *err = 1; continue; }
            const Kmer<W> x = ori ? ry : y, rx = ori ? y : ry;
            const int nb = single_out_base(aux, ori);
            bool fwd = true;
            const i64 ws = nb < 0 ? -1 : table_find_either(t, append_base(x, nb, k), k, &fwd);
            u64 sd = d;
            if (ws < 0) *err = 2;
            else {
                const u64 su = 2 * rank_of(rb, (u64)ws) + (fwd ? 0u : 1u);
                if (!flag[su] || off[su] >= cm.n) *err = 3;             // the successor of a member is a member
                else sd = off[su];
            }
            cm.succ[d] = (u32)sd;
            const bool isrc = kmer_less(rx, x);
            const Kmer<W> key = isrc ? rx : x;                          // the anchor key: min(x, rc x)
            cm.klo[d] = key.lo;
            if constexpr (W == 2) cm.khi[d] = key.hi;
            cm.meta[d] = (uint8_t)((nb & 3) | (isrc ? 4 : 0) | (pal ? 8 : 0));
            u64 tw = d;
            if (!pal) { if (!flag[u ^ 1] || off[u ^ 1] >= cm.n) *err = 4; else tw = off[u ^ 1]; }      // the reverse complement of a cycle is a cycle
            cm.twin[d] = (u32)tw;
        }
    }
}
// succ must be a permutation of the members for the way back (k_cya_init's pred) to be defined: every member is hit once
__global__ __launch_bounds__(BLOCK) void k_cyc_hits(const u32 *__restrict__ succ, u64 n, u32 *hits) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) atomicAdd(&hits[succ[i]], 1u);
}
__global__ __launch_bounds__(BLOCK) void k_cyc_hits_check(const u32 *__restrict__ hits, u64 n, u32 *err) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) if (hits[i] != 1u) *err = 5;
}

template <int W, class TT> static int graph_add_cycles(gk_map *m, gk_graph *g, TT t) {
    gk_ctx *ctx = m->ctx;
    const int k = m->k;
    const u64 tcap = t.capacity();
    DevScratch tmp(ctx);
    unsigned long long *d_cand = nullptr, cand = 0;
    u32 *d_err = nullptr;
    tmp.zeroed(&d_cand, 1);
    tmp.zeroed(&d_err, 4);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_build_cycles: alloc");
    // the cheap exit: every (1,1) oriented k-mer is inside one edge of the plain build (len - 1 of them per edge) or on a cycle
    hipLaunchKernelGGL((k_cyc_census<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, d_cand);
    hipError_t e = read_back(ctx, &cand, d_cand);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: census");
    const u64 inside = g->live_len - g->live_edges;
    if (cand < inside) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: the edges hold more interior k-mers than the table has");
    const u64 members = cand - inside;
    if (!members) return GK_OK;
    if (members >= (1ull << 31)) return fail(ctx, GK_E_CAPACITY, "more than 2^31 k-mers on perfect cycles");
    // which ones: the build's absorbing pointer jumping again (whichever unitig construction the build used, its state is gone)
    const u64 nstates = 2 * m->size, nblk = (tcap + 63) / 64, nchunks = (nblk + RANK_CHUNK - 1) / RANK_CHUNK;
    if (nstates >= PJ_MAX_STATES) return fail(ctx, GK_E_CAPACITY, "more than 2^33 k-mers: beyond the pointer-jumping state's index");
    u64 *st = nullptr;
    RankBlk *rb = nullptr;
    u32 *chunk_tot = nullptr, *flag = nullptr, *hits = nullptr;
    u64 *chunk_base = nullptr;
    unsigned long long *off = nullptr;
    tmp.get(&rb, nblk); tmp.get(&chunk_tot, nchunks); tmp.get(&chunk_base, nchunks + 1); tmp.get(&st, nstates);
    tmp.zeroed(&flag, nstates); tmp.get(&off, nstates + 1);
    if (tmp.error() == hipSuccess) tmp.note(hipMemsetAsync(st, 0xff, nstates * 8, ctx->stream));       // PJ_UNREG
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_build_cycles: pointer-jumping arrays");
    rank_build<W, TT>(ctx, t, rb, nblk, chunk_tot, chunk_base, nchunks);
    hipLaunchKernelGGL((k_pj_init<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, rb, st);
    int max_rounds = 2;
    while ((1ull << (max_rounds - 2)) < std::max<u64>(nstates, 2)) max_rounds++;
    for (int round = 0; round < max_rounds; round++)        // (no early exit: with members something moves in every round)
        hipLaunchKernelGGL(k_pj_round, dim3(ggrid(ctx, nstates)), dim3(BLOCK), 0, ctx->stream, st, nstates, d_err + 1);
    hipLaunchKernelGGL((k_cyc_members<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, rb, st, flag);
    tmp.note(scan_counts(ctx, tmp, flag, nstates, off));
    unsigned long long ranked = 0, M = 0;
    u32 h_err[4] = {0, 0, 0, 0};
    e = tmp.error();
    if (e == hipSuccess) e = read_back(ctx, {{&ranked, chunk_base + nchunks, 8}, {&M, off + nstates, 8}, {h_err, d_err, 16}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: members");
    if (ranked != m->size) return fail(ctx, GK_E_STATE, "live slots (" + std::to_string(ranked) + ") differ from the map's size (" + std::to_string(m->size) + ")");
    if (h_err[2]) return fail(ctx, GK_E_STATE, "pointer jumping met an unregistered successor (code " + std::to_string(h_err[2]) + ")");
    if (M != members) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: " + std::to_string(M) + " k-mers on cycles, the census says " + std::to_string(members));
    tmp.release(st);
    CycleMembers cm{};
    cm.n = M;
    tmp.get(&cm.succ, M); tmp.get(&cm.klo, M); tmp.get(&cm.meta, M); tmp.get(&cm.twin, M);
    if (W == 2) tmp.get(&cm.khi, M);
    tmp.zeroed(&hits, M);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_build_cycles: member arrays");
    hipLaunchKernelGGL((k_cyc_fill<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, rb, flag, off, cm, d_err);
    hipLaunchKernelGGL(k_cyc_hits, dim3(ggrid(ctx, M)), dim3(BLOCK), 0, ctx->stream, cm.succ, (u64)M, hits);
    hipLaunchKernelGGL(k_cyc_hits_check, dim3(ggrid(ctx, M)), dim3(BLOCK), 0, ctx->stream, hits, (u64)M, d_err);
    e = read_back(ctx, h_err, d_err, 1);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build_cycles: fill");
    if (h_err[0]) return fail(ctx, GK_E_STATE, "gk_graph_build_cycles: the cycle members are not closed (code " + std::to_string(h_err[0]) + ")");
    tmp.release(rb); tmp.release(chunk_tot); tmp.release(chunk_base); tmp.release(flag); tmp.release(off); tmp.release(hits);
    if (int rc = graph_append_cycles(g, tmp, cm, g->cycle_stats)) return rc;
    g->index_ready = false;
    const int rc = graph_refresh_counts(g);
    g->walked_bases = g->live_len;
    return rc;
}

static void graph_free_arrays(gk_graph *g) {
    gk_ctx *ctx = g->ctx;
    GraphView &v = g->v;
    for (void *p : {g->node_blob, g->edge_blob, (void *)v.pool, (void *)v.nidx}) (void)pool_free(ctx, p);
    g->node_blob = g->edge_blob = nullptr;
    v = GraphView{};
}

// TT: the table the graph phase reads — the map's own hashed table, or the minimizer-bucketed copy built from it (graph_build_entry)
template <int W, class TT> static int graph_build_impl(gk_map *m, gk_graph *g, TT t, bool masks_valid = false) {
    gk_ctx *ctx = m->ctx;
    const int k = m->k;
    const u64 tcap = t.capacity();
    unsigned long long *d_cnt = nullptr;     // [0] terminals [1] cursor [2] edges [3] ecursor [4] pool cursor
    u32 *d_err = nullptr;
    u64 *tslots = nullptr;
    unsigned long long *termbits = nullptr;  // one bit per slot of the table the build reads: a terminal k-mer lives there (k_classify / k_finish_masks -> k_collect_bits)
    int rc = GK_OK;
    DevScratch tmp(ctx);
    hipError_t e = tmp.get(&d_cnt, 8);
    if (e == hipSuccess) e = tmp.get(&d_err, 4);
    // (a bucketed table's slot count need not be a multiple of 64: k_classify writes every word with word * 64 < tcap, the last
    //  one with zeroes above tcap — one word per STARTED group of 64 slots, here and in k_collect_bits below)
    const u64 nwords = (tcap + 63) / 64;
    if (e == hipSuccess) e = tmp.get(&termbits, nwords);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, 64, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 16, ctx->stream);
    unsigned long long h_cnt[8] = {0};
    u32 h_err = 0;
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: alloc");
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](int i) {
        const auto now = std::chrono::steady_clock::now();
        g->build_ms[i] += std::chrono::duration<float, std::milli>(now - t_prev).count();
        t_prev = now;
    };
    // 1. degree classification of every live key — or, on a table gathered WITH its owners' masks (gk_dist_gather_map in its
    //    classified form), only what follows from the masks: one streaming pass, no neighbour lookups
    bool from_masks = false;
    if constexpr (!is_mb<TT>::value) from_masks = masks_valid;
    if constexpr (!is_mb<TT>::value) {
        if (from_masks) hipLaunchKernelGGL((k_finish_masks<W>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, &d_cnt[0], termbits);
    }
    if (!from_masks) hipLaunchKernelGGL((k_classify<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, &d_cnt[0], termbits);
    g->used_masks = from_masks ? 1 : 0;
    if ((e = read_back(ctx, h_cnt, d_cnt, 1)) != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: classify");
    lap(0);
    const u64 nT = h_cnt[0];
    if (2 * nT >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph nodes");        // (also: j < 2^31 fits AUX_NODE | j)
    // 2. terminal slots -> nodes (both strands) and edge stubs
    e = tmp.get(&tslots, nT);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: alloc nodes");
    hipLaunchKernelGGL(k_collect_bits, dim3(ggrid(ctx, nwords + 1)), dim3(BLOCK), 0, ctx->stream, termbits, nwords, tslots, &d_cnt[1]);
    if ((e = read_back(ctx, h_cnt, d_cnt, 3)) != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: collect");
    if (h_cnt[1] != nT) return fail(ctx, GK_E_STATE, "terminal count mismatch");
    tmp.release(termbits);                 // (an eighth of a byte per slot: gone before the graph arrays exist)
    const u64 nE = h_cnt[2];
    if (nE >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, "more than 2^32 graph edges");
    if ((rc = graph_alloc_nodes(g, 2 * nT)) != GK_OK) return rc;
    if ((rc = graph_alloc_edges(g, nE)) != GK_OK) return rc;
    g->v.k = k;
    if (nT) {
        hipLaunchKernelGGL((k_make_nodes<W, TT>), dim3(ggrid(ctx, nT)), dim3(BLOCK), 0, ctx->stream, t, k, tslots, nT, g->v, &d_cnt[3]);
        if ((e = read_back(ctx, h_cnt, d_cnt, 4)) != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: make_nodes");
        // every edge slot the walk will visit must have been written by k_make_nodes
        if (h_cnt[3] != nE) return fail(ctx, GK_E_STATE, "edge stub count mismatch: " + std::to_string(h_cnt[3]) + " vs " + std::to_string(nE));
    }
    lap(1);
    // 3. unitigs: measure, reserve the sequence pool, emit.  One lane per edge walking base by base
    //    (k_walk) when edges are short; pointer jumping when they are long (see k_pj_* above).
    if (nE) {
        const bool use_pj = ctx->hook_unitigs ? ctx->hook_unitigs == 2 : (m->size / std::max<u64>(nE, 1) >= 16);   // (hook: gk_ctx_set_option "graph_unitigs")
        u64 *st = nullptr;                     // pointer jumping: one word per oriented live k-mer
        RankBlk *rb = nullptr;                 // ... and the slot -> rank structure
        u32 *chunk_tot = nullptr;
        u64 *chunk_base = nullptr;
        ulonglong2 *stage = nullptr;           // queue-fed walk: the first WALK_BUF bases of every edge, 32 bytes each
        if (use_pj) {
            // what is alive here besides the table: 16 B per live key (st) + 0.25 B per slot (rb) — DESIGN.md section 6
            const u64 nstates = 2 * m->size, nblk = (tcap + 63) / 64, nchunks = (nblk + RANK_CHUNK - 1) / RANK_CHUNK;
            if (nstates >= PJ_MAX_STATES) return fail(ctx, GK_E_CAPACITY, "more than 2^33 k-mers: beyond the pointer-jumping state's index");
            e = tmp.get(&rb, nblk);
            if (e == hipSuccess) e = tmp.get(&chunk_tot, nchunks);
            if (e == hipSuccess) e = tmp.get(&chunk_base, nchunks + 1);
            if (e == hipSuccess) e = tmp.get(&st, nstates);
            if (e == hipSuccess) e = hipMemsetAsync(st, 0xff, std::max<u64>(nstates, 1) * 8, ctx->stream);         // PJ_UNREG
            if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: pointer-jumping arrays");
            rank_build<W, TT>(ctx, t, rb, nblk, chunk_tot, chunk_base, nchunks);
            unsigned long long ranked = 0;
            if ((e = read_back(ctx, &ranked, chunk_base + nchunks)) != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: slot ranks");
            if (ranked != m->size) return fail(ctx, GK_E_STATE, "live slots (" + std::to_string(ranked) + ") differ from the map's size (" + std::to_string(m->size) + ")");
            hipLaunchKernelGGL((k_pj_init<W, TT>), dim3(ggrid(ctx, tcap)), dim3(BLOCK), 0, ctx->stream, t, k, rb, st);
            e = hipGetLastError();
            // a chain of n k-mers is resolved after ceil(log2 n) rounds; what still moves then is an all-(1,1) cycle (Graph.scala:375)
            int max_rounds = 2;
            while ((1ull << (max_rounds - 2)) < std::max<u64>(nstates, 2)) max_rounds++;
            for (int round = 0; round < max_rounds && nstates && e == hipSuccess; round++) {
                u32 flags[2] = {0, 0};
                e = hipMemsetAsync(d_err + 1, 0, 8, ctx->stream);      // (d_err has 4 words: [0] the build's error, [1] moved, [2] round error)
                if (e != hipSuccess) break;
                hipLaunchKernelGGL(k_pj_round, dim3(ggrid(ctx, nstates)), dim3(BLOCK), 0, ctx->stream, st, nstates, d_err + 1);
                e = read_back(ctx, flags, d_err + 1, 2);
                if (e == hipSuccess && flags[1]) return fail(ctx, GK_E_STATE, "pointer jumping met an unregistered successor (code " + std::to_string(flags[1]) + ")");
                if (!flags[0]) break;
            }
            if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: pj rounds");
            hipLaunchKernelGGL((k_pj_edges<W, TT>), dim3(ggrid(ctx, nE)), dim3(BLOCK), 0, ctx->stream, t, k, g->v, rb, st, d_err);
        } else {
            // every oriented interior k-mer lies on exactly one edge: sum of lengths <= edges + 2 x live keys, and every edge
            // rounds up to a byte — the pool can be allocated before the walk, so the walk can write as it goes
            g->pool_cap = ((nE + 2 * m->size) / 4 + nE + 16) / 4 * 4;
            e = pool_malloc(ctx, &g->v.pool, g->pool_cap);
            if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: pool");
            if (ctx->hook_walk_queue == 0)        // ("graph_walk_queue": 0 = one edge per lane, the round-1 form; A/B)
                hipLaunchKernelGGL((k_walk<W, TT>), dim3(ggrid(ctx, nE)), dim3(BLOCK), 0, ctx->stream, t, k, g->v, 0, tcap + 1, &d_cnt[4], &d_cnt[6], d_err);
            else {
                e = tmp.get(&stage, 2 * nE);
                if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: edge staging");
                const int gq = (int)std::min<u64>((nE + 4 * BLOCK - 1) / (4 * BLOCK), grid_cap(ctx));
                hipLaunchKernelGGL((k_walk_q<W, TT>), dim3(std::max(gq, 1)), dim3(BLOCK), 0, ctx->stream, t, k, g->v, tcap + 1, &d_cnt[7], stage, &d_cnt[6], d_err);
                hipLaunchKernelGGL(k_place_edges, dim3(ggrid(ctx, nE / 8 + 1)), dim3(BLOCK), 0, ctx->stream, g->v, stage, &d_cnt[4]);
            }
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        lap(2);
        g->used_pj = use_pj ? 1 : 0;
        if (e == hipSuccess && use_pj) hipLaunchKernelGGL(k_reserve_pool, dim3(ggrid(ctx, nE)), dim3(BLOCK), 0, ctx->stream, g->v, (u64)0, (u64)0, &d_cnt[4]);
        if (e == hipSuccess) e = read_back(ctx, {{h_cnt, d_cnt, 56}, {&h_err, d_err, 4}});
        if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: walk");
        if (h_err) return fail(ctx, GK_E_STATE, "unitig construction failed (code " + std::to_string(h_err) +
                               "): the table changed since classification or is inconsistent");
        g->pool_used = h_cnt[4];
        if (use_pj) {
            g->pool_cap = (std::max<u64>(g->pool_used, 1) + 7) / 4 * 4;        // whole 32-bit words (k_pj_emit ORs words)
            e = pool_malloc(ctx, &g->v.pool, g->pool_cap);
            if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: pool");
        } else if (g->pool_used > g->pool_cap) {
            return fail(ctx, GK_E_STATE, "edge sequences need " + std::to_string(g->pool_used) + " bytes, bound was " + std::to_string(g->pool_cap));
        }
        lap(3);
        if (use_pj) {
            e = hipMemsetAsync(g->v.pool, 0, g->pool_cap, ctx->stream);
            if (e == hipSuccess) {
                hipLaunchKernelGGL((k_pj_emit<W, TT>), dim3(ggrid(ctx, std::max<u64>(tcap, nE))), dim3(BLOCK), 0, ctx->stream, t, k, g->v, rb, st, d_err);
                e = read_back(ctx, &h_err, d_err);
            }
        } else {
            if (h_cnt[6]) {          // edges longer than the walk's register buffer: second walk, emitting
                hipLaunchKernelGGL((k_walk<W, TT>), dim3(ggrid(ctx, nE)), dim3(BLOCK), 0, ctx->stream, t, k, g->v, 1, tcap + 1, &d_cnt[4], &d_cnt[6], d_err);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        }
        tmp.release(st); tmp.release(rb); tmp.release(chunk_tot); tmp.release(chunk_base); tmp.release(stage);      // (not at scope exit: graph_refresh_counts follows)
        if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: emit");
        if (h_err) return fail(ctx, GK_E_STATE, "unitig emission failed (code " + std::to_string(h_err) + ")");
        lap(4);
    } else {
        e = pool_malloc(ctx, &g->v.pool, 1);
        if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: pool");
        g->pool_cap = 1;
    }
    // (the k-mer -> node index serves point queries and by-k-mer edits only — GraphBuilder's own flow, components, the export and
    //  the paired-end stage go by ids: it is built by the first call that needs it, graph_ensure_index; 1.5 ms of C3's buildGraph)
    g->index_ready = false;
    rc = graph_refresh_counts(g);
    g->walked_bases = g->live_len;
    lap(5);
    if (rc == GK_OK && g->keep_cycles) rc = graph_add_cycles<W, TT>(m, g, t);      // (gk_graph_build_cycles: after the plain build, which it leaves as it is)
    return rc;
}

template <int W> __global__ __launch_bounds__(BLOCK) void k_mb_clear(Slot<W> *slots, u64 n) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        if constexpr (W == 1) slots[i] = Slot<1>{KEY_EMPTY, 0u, 0u};
        else slots[i] = Slot<2>{KEY_EMPTY, KEY_EMPTY, 0u, 0u};
    }
}

// ---- the minimizer-bucketed copy (MbTable, gk_device.h) ------------------------------------------------------------------------
template <int W> __global__ __launch_bounds__(BLOCK) void k_mb_count(Table<W> src, int k, u32 nb, u32 *cnt, u32 *bucket_of) {
    const u64 ncap = src.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&src.slots[i])) continue;
        const u32 b = (u32)owner_of(slot_key(src, i), k, (int)nb);
        bucket_of[i] = b;
        atomicAdd(&cnt[b], 1u);
    }
}
// keys in a bucket -> slots of its region: the power of two that keeps the load at or under 0.5, 8 at least
__global__ __launch_bounds__(BLOCK) void k_mb_sizes(u32 *cnt, u32 nb) {
    for (u64 b = (u64)blockIdx.x * BLOCK + threadIdx.x; b < nb; b += (u64)gridDim.x * BLOCK) {
        u32 want = max(8u, 2u * cnt[b]), p = 8u;
        while (p < want) p <<= 1;
        cnt[b] = p;
    }
}
template <int W> __global__ __launch_bounds__(BLOCK) void k_mb_fill(Table<W> src, const u32 *bucket_of, MbTable<W> dst, u32 *err) {
    const u64 ncap = src.capacity();
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ncap; i += (u64)gridDim.x * BLOCK) {
        if (!slot_live(&src.slots[i])) continue;
        const Kmer<W> key = slot_key(src, i);
        const Stored<W> kk = to_stored(key);
        const ProbeAt<W> p = probe_at_bucket(dst, key, bucket_of[i]);
        Slot<W> *reg = const_cast<Slot<W> *>(p.reg);
        u32 at = p.pos;
        bool placed = false;
        for (u32 n = 0; n <= p.mask && !placed; n++, at = (at + 1) & p.mask) {
            // (every key of the source is unique: a slot is taken by claiming its first word; with 16-byte keys a slot whose first
            //  word equals ours belongs to ANOTHER key that shares it — see seg_claim_unique)
            const u64 c0 = cas64(&reg[at].w0, KEY_EMPTY, kk.w0);
            if constexpr (W == 1) { if (c0 == KEY_EMPTY) placed = true; }
            else { if ((c0 == KEY_EMPTY || c0 == kk.w0) && cas64(&reg[at].w1, KEY_EMPTY, kk.w1) == KEY_EMPTY) placed = true; }
            if (placed) reg[at].extra = src.slots[i].extra;
        }
        if (!placed) *err = 1u;
    }
}

template <int W> static int graph_build_entry(gk_map *m, gk_graph *g, bool masks_valid) {
    gk_ctx *ctx = m->ctx;
    // (m->dirty: keys were inserted verbatim and at least one was not its k-mer's hash-rule orientation — the reference's
    //  `contains` probes both strands unconditionally, Graph.scala:270; so does every lookup below then)
    Table<W> t{reinterpret_cast<Slot<W> *>(m->slots), m->nb2, m->lnb1, m->k == 64 ? 1u : 0u, m->dirty ? 1u : 0u};
    // "graph_mbt" = 1: classify and walk on a minimizer-bucketed COPY of the table (A/B, profiles/r03); never for k = 64 (tagged slots)
    const bool use_mb = ctx->hook_graph_mbt > 0 && m->k != 64 && m->size >= 4096;
    if (!use_mb) return graph_build_impl<W, Table<W>>(m, g, t, masks_valid);
    const auto t0 = std::chrono::steady_clock::now();
    const u32 nb = (u32)std::min<u64>(std::max<u64>(m->size / (u64)std::max(ctx->hook_graph_mbt_keys, 16), 1), 1u << 30);
    u32 *d_cnt = nullptr, *d_bucket = nullptr, *d_err = nullptr;
    unsigned long long *d_off = nullptr, total = 0;
    Slot<W> *slots = nullptr;
    DevScratch tmp(ctx);
    hipError_t e = tmp.get(&d_cnt, nb);
    if (e == hipSuccess) e = tmp.get(&d_bucket, m->capacity);
    if (e == hipSuccess) e = tmp.get(&d_off, (u64)nb + 1);
    if (e == hipSuccess) e = tmp.get(&d_err, 1);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (u64)nb * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_err, 0, 4, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: bucketed table");
    hipLaunchKernelGGL(k_mb_count<W>, dim3(ggrid(ctx, m->capacity)), dim3(BLOCK), 0, ctx->stream, t, m->k, nb, d_cnt, d_bucket);
    hipLaunchKernelGGL(k_mb_sizes, dim3(ggrid(ctx, nb)), dim3(BLOCK), 0, ctx->stream, d_cnt, nb);
    e = scan_counts(ctx, tmp, d_cnt, nb, d_off);
    if (e == hipSuccess) e = read_back(ctx, &total, d_off + nb);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: bucket regions");
    e = tmp.get(&slots, total);
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: bucketed table");
    hipLaunchKernelGGL(k_mb_clear<W>, dim3(ggrid(ctx, total / 4 + 1)), dim3(BLOCK), 0, ctx->stream, slots, (u64)total);
    MbTable<W> mt{slots, reinterpret_cast<const u64 *>(d_off), nb, m->dirty ? 1u : 0u, (u64)total};
    hipLaunchKernelGGL(k_mb_fill<W>, dim3(ggrid(ctx, m->capacity)), dim3(BLOCK), 0, ctx->stream, t, d_bucket, mt, d_err);
    u32 h_err = 0;
    if ((e = read_back(ctx, &h_err, d_err)) != hipSuccess) return hip_fail(ctx, e, "gk_graph_build: filling the bucketed table");
    if (h_err) return fail(ctx, GK_E_STATE, "gk_graph_build: a bucket region filled up (internal sizing error)");
    tmp.release(d_bucket);
    tmp.release(d_cnt);
    g->mbt_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g->mbt_slots = total;
    return graph_build_impl<W, MbTable<W>>(m, g, mt);
}

// The rank structure of a map's own table on the host (the test build's gk_test_slot_ranks; nothing in the product calls it):
// the table is brought into the graph layout the way gk_graph_build does, rank_build runs on it as in the build, and the
// (mask, base) pairs and chunk_base[nchunks] come back.  *nblk is set before the capacity check.
int graph_slot_ranks(gk_map *m, uint64_t *masks, uint64_t *bases, uint64_t cap_blocks, uint64_t *nblk_out, uint64_t *total) {
    gk_ctx *ctx = m->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = map_materialize(m)) return rc;
    if (int rc = map_to_graph_layout(m)) return rc;
    const u64 nblk = (m->capacity + 63) / 64, nchunks = (nblk + RANK_CHUNK - 1) / RANK_CHUNK;
    *nblk_out = nblk;
    if (nblk > cap_blocks) return fail(ctx, GK_E_CAPACITY, "slot ranks: " + std::to_string(nblk) + " blocks, room for " + std::to_string(cap_blocks));
    DevScratch tmp(ctx);
    RankBlk *rb = nullptr;
    u32 *chunk_tot = nullptr;
    u64 *chunk_base = nullptr;
    tmp.get(&rb, nblk);
    tmp.get(&chunk_tot, nchunks);
    tmp.get(&chunk_base, nchunks + 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "slot ranks: alloc");
    GK_BY_W(m->W, {
        Table<W> t{reinterpret_cast<Slot<W> *>(m->slots), m->nb2, m->lnb1, m->k == 64 ? 1u : 0u, m->dirty ? 1u : 0u};
        rank_build<W, Table<W>>(ctx, t, rb, nblk, chunk_tot, chunk_base, nchunks);
    });
    std::vector<RankBlk> h(nblk);
    unsigned long long ranked = 0;
    const hipError_t e = read_back(ctx, {{h.data(), rb, nblk * sizeof(RankBlk)}, {&ranked, chunk_base + nchunks, 8}});
    if (e != hipSuccess) return hip_fail(ctx, e, "slot ranks");
    for (u64 i = 0; i < nblk; i++) { masks[i] = h[i].mask; bases[i] = h[i].base; }
    *total = ranked;
    return GK_OK;
}

static int graph_build_common(gk_map *m, gk_graph **out, bool keep_cycles, uint64_t *stats6) {
    if (!m || !m->ctx) return fail(nullptr, GK_E_INVALID, "null map handle");
    if (!out) return fail(m->ctx, GK_E_INVALID, "gk_graph_build: out is NULL");
    *out = nullptr;
    GK_HIP(m->ctx, hipSetDevice(m->ctx->device));
    if (int rc = map_materialize(m)) return rc;
    // The graph phase annotates every k-mer in its slot: a COUNT table of 8-byte keys (12-byte slots, no annotation word) is
    // rebuilt into the graph layout first — what deleteAll(v < rounds) does anyway on the reference's path (GraphBuilder.scala:30-36).
    if (int rc = map_to_graph_layout(m)) return rc;
    gk_graph *g = new gk_graph();
    g->ctx = m->ctx;
    g->k = m->k;
    g->W = m->W;
    g->keep_cycles = keep_cycles;
    // (the build re-uses the annotation word — a terminal slot's becomes its node — so owner-computed masks serve ONE build)
    const bool masks_valid = m->masks_valid;
    m->masks_valid = false;
    int rc = m->W == 1 ? graph_build_entry<1>(m, g, masks_valid) : graph_build_entry<2>(m, g, masks_valid);
    if (rc != GK_OK) {
        graph_free_arrays(g);
        delete g;
        return rc;
    }
    if (stats6) for (int i = 0; i < 6; i++) stats6[i] = g->cycle_stats[i];
    *out = g;
    return GK_OK;
}

extern "C" {

int gk_graph_build(gk_map *m, gk_graph **out) { return graph_build_common(m, out, false, nullptr); }

int gk_graph_build_cycles(gk_map *m, gk_graph **out, uint64_t *stats6) {
    if (stats6) for (int i = 0; i < 6; i++) stats6[i] = 0;
    return graph_build_common(m, out, true, stats6);
}

void gk_graph_destroy(gk_graph *g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    graph_free_arrays(g);
    delete g;
}

int gk_graph_build_stats(gk_graph *g, float *phase_ms6, uint64_t *walked_bases, int *pointer_jumping) {
    if (int rc = check_graph(g)) return rc;
    if (phase_ms6) for (int i = 0; i < 6; i++) phase_ms6[i] = g->build_ms[i];
    if (walked_bases) *walked_bases = g->walked_bases;
    if (pointer_jumping) *pointer_jumping = g->used_pj;
    return GK_OK;
}

int gk_graph_classified_by_owners(gk_graph *g, int *flag) {
    if (int rc = check_graph(g)) return rc;
    if (flag) *flag = g->used_masks;
    return GK_OK;
}

int gk_graph_bucketed_table_stats(gk_graph *g, float *build_ms, uint64_t *slots) {
    if (int rc = check_graph(g)) return rc;
    if (build_ms) *build_ms = g->mbt_ms;
    if (slots) *slots = g->mbt_slots;
    return GK_OK;
}

}  // extern "C"

// ---- host side of the classify over a PartitionedDNAMap (kernels k_dc_* above; the exchanges are gk_dist.hip's) ----------------
namespace gk {
template <int W> static Table<W> graph_table_of(gk_map *m) {
    return Table<W>{reinterpret_cast<Slot<W> *>(m->slots), m->nb2, m->lnb1, m->k == 64 ? 1u : 0u, m->dirty ? 1u : 0u};
}
// slots [s0, s1) of a GRAPH-layout table: local neighbour lookups into the annotation word, remote neighbours counted per owner in d_cnt[P] (zeroed here)
int dclass_count(gk_map *m, int rank, int P, u64 s0, u64 s1, unsigned long long *d_cnt) {
    gk_ctx *ctx = m->ctx;
    GK_HIP(ctx, hipMemsetAsync(d_cnt, 0, 64 * 8, ctx->stream));
    if (s1 > m->capacity) s1 = m->capacity;
    if (s0 >= s1) return GK_OK;
    const int grid = ggrid(ctx, s1 - s0);
    GK_BY_W(m->W, hipLaunchKernelGGL((k_dc_scan<W, false>), dim3(grid), dim3(BLOCK), 0, ctx->stream, graph_table_of<W>(m), m->k, rank, P, s0, s1, d_cnt, nullptr, nullptr, nullptr));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}
// the same slots again: the remote neighbours' canonical keys into their owners' regions (d_off[p] = first query for owner p; d_cur[P] zeroed here)
int dclass_fill(gk_map *m, int rank, int P, u64 s0, u64 s1, const unsigned long long *d_off, unsigned long long *d_cur, u64 *d_qkeys, u64 *d_qref) {
    gk_ctx *ctx = m->ctx;
    GK_HIP(ctx, hipMemsetAsync(d_cur, 0, 64 * 8, ctx->stream));
    if (s1 > m->capacity) s1 = m->capacity;
    if (s0 >= s1) return GK_OK;
    const int grid = ggrid(ctx, s1 - s0);
    GK_BY_W(m->W, hipLaunchKernelGGL((k_dc_scan<W, true>), dim3(grid), dim3(BLOCK), 0, ctx->stream, graph_table_of<W>(m), m->k, rank, P, s0, s1, d_cur, d_off, d_qkeys, d_qref));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}
int dclass_answer(gk_map *m, const u64 *d_keys, u64 n, uint8_t *d_ans) {
    gk_ctx *ctx = m->ctx;
    if (!n) return GK_OK;
    GK_BY_W(m->W, hipLaunchKernelGGL((k_dc_answer<W>), dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, graph_table_of<W>(m), m->k, d_keys, n, d_ans));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}
int dclass_apply(gk_map *m, const u64 *d_qref, const uint8_t *d_ans, u64 n) {
    gk_ctx *ctx = m->ctx;
    if (!n) return GK_OK;
    GK_BY_W(m->W, hipLaunchKernelGGL((k_dc_apply<W>), dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, graph_table_of<W>(m), d_qref, d_ans, n));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}
}  // namespace gk
