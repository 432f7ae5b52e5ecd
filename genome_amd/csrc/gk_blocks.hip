// gk_blocks.hip — alignment blocks and breakpoints: every edge of a graph aligned to a reference genome as the exact runs it shares
// with it, and every place where two neighbouring runs of an edge do not continue each other classed.  Both rules are this
// project's own and stated in include/genome_amd.h ("alignment blocks", "breakpoints"); tests/blocks_ref.py restates them.
//
// Reference: none.  CheckGraph.scala asks whether a window of the genome is in the graph; nothing there asks where an edge lies.
//
// k_block_windows is k_place_windows' shape (gk_place.hip, which stays as it is): 4096 window starts per workgroup, 16 per lane,
// the characters staged in LDS.  Where the placement pass folds the hits of a run away, this one keeps the run: a window start is
// an EVENT on a strand iff its hit differs from the hit one start before it, and only events reach HBM.  A lane needs the hit
// before its first start: the first lane of a wave evaluates that window itself (the tile is staged with a halo of k characters
// instead of k - 1), every other lane takes it from its neighbour by a shuffle AFTER its loop, so the event at a lane's first
// start is decided last and written in front of the lane's others.  Two launches per slice: the count launch leaves one word per
// lane (its events per strand, and whether its first start is one) and the events per workgroup; gk_scan.h turns those into
// bases; the emit launch looks every window up again and writes each event with one 16-byte vector store at
// base of the workgroup + events of the lanes before it + events of the lane so far: stream order per strand, no atomics but the
// counters'.  A record's last slice evaluates one start more, P = the record's window count, as a window without a hit, so every
// run is closed by an event of its own record and strand.
// gk_blocks_finish: one lane per event makes the rows, two stable radix sorts order them (the events arrive ordered by strand,
// record and start, the minor half of the key), one lane per row classes its breakpoint, one lane per edge id its edge.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "gk_scan.h"
#include "gk_text.h"
#include "gk_thread_common.h"

namespace {

constexpr u64 BL_SLICE_DEFAULT = 64ull << 20;          // characters per device slice
constexpr u32 BL_RUN = 16;                             // consecutive window starts per lane
constexpr u32 BL_WT = 256 * BL_RUN;                    // per workgroup
constexpr u64 BL_COORD_MASK = (1ull << 40) - 1;
constexpr u64 BL_MAX_RECORDS = 1ull << 24;
constexpr u64 BL_MAX_BASES = 1ull << 39;
constexpr u64 BL_BOTTOM = ~0ull;                       // an event's second word when the hit is none
enum { BC_VALID = 0, BC_WINDOWS = 1, BC_COVERED = 2, BC_BAD = 3, BC_N = 4 };                  // device counters of the window pass
enum { BK_FIRST = 0, BK_OVERLAP = 1, BK_TRANSLOCATION = 2, BK_INVERSION = 3, BK_RELOCATION = 4, BK_INDEL = 5, BK_COLINEAR = 6 };
enum { BE_UNALIGNED = 0, BE_REPEAT = 1, BE_MISASSEMBLED = 2, BE_INDEL = 3, BE_COLINEAR = 4, BE_EXACT = 5 };
enum { EF_OVERLAP = 1, EF_MIS = 2, EF_INDEL = 4, EF_COLINEAR = 8 };                            // the per-edge word of k_blk_class
// device counters of the finish
enum { FC_BRK = 0, FC_EDGE = 6, FC_FULL = 12, FC_KMERS = 13, FC_PIECES = 14, FC_PIECE_BASES = 15, FC_SHIFT_SUM = 16, FC_SHIFT_MAX = 17, FC_N = 18 };
constexpr int BLOCKS_NSTATS = 24;

struct Hit { u32 e, d; u64 c; };                       // e == NONE: no hit; c: the candidate + 2^39
__device__ __forceinline__ bool same_hit(const Hit &a, const Hit &b) { return a.e == b.e && (a.e == NONE || a.c == b.c); }
__device__ __forceinline__ u32 bl_code(u32 c) { return c == 'A' ? 0u : c == 'G' ? 1u : c == 'C' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ ulonglong2 bl_event(u32 rec, u64 x, const Hit &h) {
    return make_ulonglong2(((u64)rec << 40) | x, h.e == NONE ? BL_BOTTOM : (((u64)h.e << 32) | h.d));
}

// one lookup: the hit of an `edge` class, none otherwise.  The position is untrusted exactly as in pl_lookup (gk_place.hip): one
// that names nothing live in this graph raises *bad and is dropped before any edge array is indexed by it.  The raise is a plain
// store, not one of the per-wave counter atomics: any number of lanes may store, all of them the value 1, nothing on the device
// reads the word, and the host reads it after the count launch (the emit launch sees the same positions, so a slice that would
// raise it there has been refused before).  The race is harmless, as pl_flush's saturation flag is.
template <int W>
__device__ __forceinline__ void bl_lookup(const Table<W> &pm, const GraphView &g, Kmer<W> x, u32 *e, u32 *d, unsigned long long *bad) {
    u64 v = 0;
    *e = NONE;
    if (vmap_count_one(pm, x, &v) != 1 || !GK_POS_IS_EDGE(v)) return;
    const u32 id = GK_POS_ID(v);
    if (!(id < g.n_edges && g.e_alive[id] && (u64)GK_POS_DIST(v) < g.e_len[id])) { *bad = 1ull; return; }
    *e = id; *d = GK_POS_DIST(v);
}
template <int W>
__device__ __forceinline__ void bl_hits(const Table<W> &pm, const GraphView &g, int k, Kmer<W> km, Kmer<W> rc, u64 x, Hit *hf, Hit *hr, unsigned long long *bad) {
    hf->d = hr->d = 0;
    bl_lookup(pm, g, km, &hf->e, &hf->d, bad);
    hf->c = (1ull << 39) + x - hf->d;
    bl_lookup(pm, g, rc, &hr->e, &hr->d, bad);
    hr->c = (1ull << 39) + x + hr->d + (u64)k - 1;
}

// T[0 .. L) = the slice with its halo: T[i] is character x0 + i of record `rec`; the characters before `own` were counted by the
// slice before.  Window start q is THIS slice's from `first` on (0, or 1 when the halo is k characters: start 0 is then the last
// start of the slice before, evaluated again only as a predecessor).  sentinel: the record ends with this slice.
// EMIT == false: lane_info[workgroup * 256 + thread] = events fwd | events rev << 8 | first start is one fwd << 16 | rev << 17,
// tile_cnt[workgroup] / tile_cnt[gridDim.x + workgroup] = the workgroup's events, and the counters.
// EMIT == true: the events, at evf[tile_off[workgroup] + ..] and evr[tile_off[gridDim.x + workgroup] - total0 + ..].
template <int W, bool EMIT>
__global__ __launch_bounds__(256) void k_block_windows(Table<W> pm, GraphView g, int k, const uint8_t *__restrict__ T, u64 L, u64 own, u32 first, u32 sentinel, u64 x0,
                                                       u32 rec, u32 *__restrict__ lane_info, u32 *__restrict__ tile_cnt,
                                                       const unsigned long long *__restrict__ tile_off, u64 total0, ulonglong2 *__restrict__ evf,
                                                       ulonglong2 *__restrict__ evr, unsigned long long *ctr) {
    // staged: characters pb - 1 .. pb + BL_WT + k - 2, widened to 16 bytes on both sides: at most 1 + BL_WT + 63 + 15 + 15 bytes at
    // k = 64, rounded up to whole 16-byte vectors
    constexpr u32 TXT_BYTES = BL_WT + 128;
    static_assert(((1 + BL_WT + 63 + 15 + 15 + 15) & ~15u) <= TXT_BYTES, "the LDS tile does not hold a workgroup's characters and the halo of k <= 64");
    __shared__ u32 s_txt[TXT_BYTES / 4];
    __shared__ u32 s_w[4];
    const u64 P = L >= (u64)k ? L - (u64)k + 1 : 0;
    const u64 pb = (u64)blockIdx.x * BL_WT;
    const u64 cend = umin(L, pb + BL_WT + (u64)k - 1);
    const u64 a0 = stage_tile(s_txt, T, pb ? pb - 1 : 0, cend);           // (pb < L: the grid is the tiles of L)
    __syncthreads();
    const uint8_t *sc = reinterpret_cast<const uint8_t *>(s_txt);
    const int lane = threadIdx.x & 63;
    const u64 p = pb + (u64)threadIdx.x * BL_RUN;
    u64 bf = 0, br = 0;                                       // EMIT: where the lane's first event of each strand goes
    u32 sf = 0, sr = 0;                                       // EMIT: 1 iff the lane's first start is an event
    if (EMIT) {
        const u32 info = lane_info[(u64)blockIdx.x * 256 + threadIdx.x];
        u32 tot = 0;
        const u32 ex = block_excl_scan((info & 0xffu) | (((info >> 8) & 0xffu) << 16), &tot, s_w);      // (a tile holds at most 4097 events a strand)
        bf = tile_off[blockIdx.x] + (ex & 0xffffu);
        br = tile_off[(u64)gridDim.x + blockIdx.x] - total0 + (ex >> 16);
        sf = (info >> 16) & 1u; sr = (info >> 17) & 1u;
    }
    Hit pf{NONE, 0u, 0ull}, pr{NONE, 0u, 0ull};               // the hits one start before
    Hit ff = pf, fr = pr;                                     // the hits at the lane's first start, if its event is still open
    bool defer = false;
    u32 nf = 0, nr = 0;                                       // events found inside the loop
    u32 cv = 0, cw = 0, cc = 0;
    if (p < L) {
        Kmer<W> km{}, rc{};
        u32 good = 0;
        const bool pre = lane == 0 && p > 0;                  // no neighbour to ask: one window more
        const u64 st = p - (pre ? 1u : 0u);
        if (st < P)
            for (int j = 0; j < k - 1; j++) {
                const u32 c = bl_code(sc[st + j - a0]);
                km = append_base(km, (int)(c & 3u), k);
                rc = prepend_base((int)(3u - (c & 3u)), rc, k);
                good = c < 4u ? good + 1 : 0;
            }
        if (pre && st < P) {
            const u32 c = bl_code(sc[st + k - 1 - a0]);
            km = append_base(km, (int)(c & 3u), k);
            rc = prepend_base((int)(3u - (c & 3u)), rc, k);
            good = c < 4u ? good + 1 : 0;
            if (good >= (u32)k) bl_hits(pm, g, k, km, rc, x0 + st, &pf, &pr, &ctr[BC_BAD]);
        }
        for (u32 r = 0; r < BL_RUN && p + r < L; r++) {
            const u64 q = p + r;
            if (q >= own && bl_code(sc[q - a0]) < 4u) cv++;
            if (q > P || (q == P && !sentinel)) continue;
            Hit hf{NONE, 0u, 0ull}, hr{NONE, 0u, 0ull};
            bool window = false;
            if (q < P) {
                const u32 c = bl_code(sc[q + k - 1 - a0]);
                km = append_base(km, (int)(c & 3u), k);
                rc = prepend_base((int)(3u - (c & 3u)), rc, k);
                good = c < 4u ? good + 1 : 0;
                window = good >= (u32)k;
                if (window) bl_hits(pm, g, k, km, rc, x0 + q, &hf, &hr, &ctr[BC_BAD]);
            }
            if (q >= first) {
                if (window) { cw++; cc += (hf.e != NONE || hr.e != NONE) ? 1u : 0u; }
                if (r == 0 && lane != 0) { defer = true; ff = hf; fr = hr; }
                else {
                    if (!same_hit(hf, pf)) { if (EMIT) evf[bf + sf + nf] = bl_event(rec, x0 + q, hf); nf++; }
                    if (!same_hit(hr, pr)) { if (EMIT) evr[br + sr + nr] = bl_event(rec, x0 + q, hr); nr++; }
                }
            }
            pf = hf; pr = hr;
        }
    }
    // the neighbour's last hits (every lane of the wave takes part; a lane that ran out of windows has none after it that has any)
    Hit qf, qr;
    qf.e = __shfl_up(pf.e, 1); qf.c = __shfl_up((unsigned long long)pf.c, 1); qf.d = 0;
    qr.e = __shfl_up(pr.e, 1); qr.c = __shfl_up((unsigned long long)pr.c, 1); qr.d = 0;
    u32 df = 0, dr = 0;
    if (defer) {
        if (!same_hit(ff, qf)) { if (EMIT) evf[bf] = bl_event(rec, x0 + p, ff); df = 1; }
        if (!same_hit(fr, qr)) { if (EMIT) evr[br] = bl_event(rec, x0 + p, fr); dr = 1; }
    }
    if (!EMIT) {
        lane_info[(u64)blockIdx.x * 256 + threadIdx.x] = (nf + df) | ((nr + dr) << 8) | (df << 16) | (dr << 17);
        const u64 ev = wave_sum((unsigned long long)(nf + df) | ((unsigned long long)(nr + dr) << 32));
        const u64 cs = wave_sum((unsigned long long)cv | ((unsigned long long)cw << 16) | ((unsigned long long)cc << 32));      // (at most 1024 each)
        if (lane == 0) {
            s_w[threadIdx.x >> 6] = (u32)ev | ((u32)(ev >> 32) << 16);
            if (cs & 0xffffu) atomicAdd(&ctr[BC_VALID], (unsigned long long)(cs & 0xffffu));
            if ((cs >> 16) & 0xffffu) atomicAdd(&ctr[BC_WINDOWS], (unsigned long long)((cs >> 16) & 0xffffu));
            if (cs >> 32) atomicAdd(&ctr[BC_COVERED], (unsigned long long)(cs >> 32));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const u32 t = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            tile_cnt[blockIdx.x] = t & 0xffffu;
            tile_cnt[(u64)gridDim.x + blockIdx.x] = t >> 16;
        }
    }
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
// the events of both strands as one list: forward first
struct EvView { const ulonglong2 *ev[2]; u64 n[2]; };
__device__ __forceinline__ const ulonglong2 *ev_at(const EvView &v, u64 i, u32 *s, u64 *li) {
    *s = i < v.n[0] ? 0u : 1u;
    *li = i - (*s ? v.n[0] : 0);
    return v.ev[*s] + *li;
}
__global__ __launch_bounds__(BLOCK) void k_blk_flags(EvView v, u32 *__restrict__ flag) {
    const u64 n = v.n[0] + v.n[1];
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        u32 s; u64 li;
        flag[i] = ev_at(v, i, &s, &li)->y != BL_BOTTOM;
    }
}
// one lane per event: a hit's event is a row, and the next event of its strand ends it
__global__ __launch_bounds__(BLOCK) void k_blk_rows(EvView v, int k, const u32 *__restrict__ flag, const unsigned long long *__restrict__ rank, u32 *__restrict__ u_edge,
                                                    u32 *__restrict__ u_sr, long long *__restrict__ u_pos, u64 *__restrict__ u_dd, u32 *__restrict__ idx) {
    const u64 n = v.n[0] + v.n[1];
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        if (!flag[i]) continue;
        u32 s; u64 li;
        const ulonglong2 *ev = ev_at(v, i, &s, &li);
        const u64 w0 = ev->x, w1 = ev->y, j = rank[i];
        const u64 xa = w0 & BL_COORD_MASK;
        u64 xb = xa;                                         // (a run is always closed by an event of its record: see the window pass)
        if (li + 1 < v.n[s] && (ev[1].x >> 40) == (w0 >> 40)) xb = (ev[1].x & BL_COORD_MASK) - 1;
        const u32 d = (u32)w1, span = (u32)(xb - xa);
        u_edge[j] = (u32)(w1 >> 32);
        u_sr[j] = (s << 24) | (u32)(w0 >> 40);
        u_pos[j] = s ? (long long)(xa + d + (u64)k - 1) : (long long)xa - (long long)d;
        u_dd[j] = s ? (((u64)(d - span) << 32) | d) : (((u64)d << 32) | (d + span));
        idx[j] = (u32)j;
    }
}
__global__ __launch_bounds__(BLOCK) void k_blk_edge_keys(const u32 *__restrict__ u_edge, const u32 *__restrict__ idx, u64 n, u32 *__restrict__ key) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) key[i] = u_edge[idx[i]];
}
struct RowView { u32 *edge, *record, *dlo, *dhi; uint8_t *strand, *brk; long long *pos, *shift; };
__global__ __launch_bounds__(BLOCK) void k_blk_permute(const u32 *__restrict__ idx, u64 n, const u32 *__restrict__ u_edge, const u32 *__restrict__ u_sr,
                                                       const long long *__restrict__ u_pos, const u64 *__restrict__ u_dd, RowView r) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 j = idx[i];
        const u32 sr = u_sr[j];
        const u64 dd = u_dd[j];
        r.edge[i] = u_edge[j]; r.strand[i] = (uint8_t)(sr >> 24); r.record[i] = sr & 0xffffffu; r.pos[i] = u_pos[j];
        r.dlo[i] = (u32)(dd >> 32); r.dhi[i] = (u32)dd;
    }
}
// one lane per row: its breakpoint against the row before it, the first and last row of its edge, the edge's word
__global__ __launch_bounds__(BLOCK) void k_blk_class(RowView r, u64 n, u64 tol, u32 *__restrict__ e_flags, u32 *__restrict__ e_first, u32 *__restrict__ e_last1,
                                                     unsigned long long *st) {
    u32 wc[7] = {};
    unsigned long long kmers = 0, ssum = 0, smax = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < n; base += (u64)gridDim.x * BLOCK) {          // (uniform over the wave)
        const u64 i = base + threadIdx.x;
        u32 b = 7;                                           // 7: no row
        unsigned long long nk = 0, ash = 0;
        if (i < n) {
            const u32 e = r.edge[i];
            long long shift = 0;
            b = BK_FIRST;
            if (i && r.edge[i - 1] == e) {
                if (r.dlo[i] <= r.dhi[i - 1]) b = BK_OVERLAP;
                else if (r.record[i] != r.record[i - 1]) b = BK_TRANSLOCATION;
                else if (r.strand[i] != r.strand[i - 1]) b = BK_INVERSION;
                else {
                    shift = r.strand[i] ? r.pos[i - 1] - r.pos[i] : r.pos[i] - r.pos[i - 1];
                    const unsigned long long a = shift < 0 ? (unsigned long long)(-shift) : (unsigned long long)shift;
                    b = a > tol ? BK_RELOCATION : a ? BK_INDEL : BK_COLINEAR;
                    if (b == BK_INDEL) ash = a;
                }
                atomicOr(&e_flags[e], b == BK_OVERLAP ? (u32)EF_OVERLAP : b <= BK_RELOCATION ? (u32)EF_MIS : b == BK_INDEL ? (u32)EF_INDEL : (u32)EF_COLINEAR);
            } else e_first[e] = (u32)i;
            if (i + 1 == n || r.edge[i + 1] != e) e_last1[e] = (u32)i + 1u;
            r.brk[i] = (uint8_t)b; r.shift[i] = shift;
            nk = (unsigned long long)(r.dhi[i] - r.dlo[i]) + 1ull;
        }
#pragma unroll
        for (u32 q = 1; q < 7; q++) wc[q] += (u32)__popcll(__ballot(b == q));
        kmers += wave_sum(nk);
        ssum += wave_sum(ash);
        for (int d = 32; d; d >>= 1) ash = max(ash, (unsigned long long)__shfl_xor(ash, d));
        smax = max(smax, ash);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (u32 q = 1; q < 7; q++) if (wc[q]) atomicAdd(&st[FC_BRK + q - 1], (unsigned long long)wc[q]);
        if (kmers) atomicAdd(&st[FC_KMERS], kmers);
        if (ssum) atomicAdd(&st[FC_SHIFT_SUM], ssum);
        if (smax) atomicMax(&st[FC_SHIFT_MAX], smax);
    }
}
// one lane per edge id: the edge class, `full`, its rows
__global__ __launch_bounds__(BLOCK) void k_blk_edges(GraphView g, u64 ne, RowView r, const u32 *__restrict__ e_flags, u32 *__restrict__ e_first,
                                                     const u32 *__restrict__ e_last1, uint8_t *__restrict__ e_cls, uint8_t *__restrict__ e_full, u32 *__restrict__ e_nrows,
                                                     unsigned long long *st) {
    u32 wc[6] = {}, nfull = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < ne; base += (u64)gridDim.x * BLOCK) {         // (uniform over the wave)
        const u64 e = base + threadIdx.x;
        u32 c = 6;                                           // 6: no live edge
        bool full = false;
        if (e < ne) {
            u32 nrows = 0;
            if (g.e_alive[e]) {
                const u32 l1 = e_last1[e], fl = e_flags[e];
                if (!l1) c = BE_UNALIGNED;
                else {
                    const u32 f = e_first[e];
                    nrows = l1 - f;
                    c = fl & EF_OVERLAP ? BE_REPEAT : fl & EF_MIS ? BE_MISASSEMBLED : fl & EF_INDEL ? BE_INDEL : fl & EF_COLINEAR ? BE_COLINEAR : BE_EXACT;
                    full = r.dlo[f] == 1u && (u64)r.dhi[l1 - 1] + 1 == g.e_len[e];
                }
            }
            if (!nrows) e_first[e] = 0u;
            e_cls[e] = c == 6 ? (uint8_t)BE_UNALIGNED : (uint8_t)c; e_full[e] = full ? 1 : 0; e_nrows[e] = nrows;
        }
#pragma unroll
        for (u32 q = 0; q < 6; q++) wc[q] += (u32)__popcll(__ballot(c == q));
        nfull += (u32)__popcll(__ballot(full));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (u32 q = 0; q < 6; q++) if (wc[q]) atomicAdd(&st[FC_EDGE + q], (unsigned long long)wc[q]);
        if (nfull) atomicAdd(&st[FC_FULL], (unsigned long long)nfull);
    }
}
// pieces: a row starts one iff it is the first of its edge or carries a breakpoint of class 2 .. 4, and its edge is no repeat
__global__ __launch_bounds__(BLOCK) void k_blk_piece_flags(RowView r, u64 n, const uint8_t *__restrict__ e_cls, u32 *__restrict__ flag) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 b = r.brk[i];
        flag[i] = e_cls[r.edge[i]] != BE_REPEAT && (b == BK_FIRST || (b >= BK_TRANSLOCATION && b <= BK_RELOCATION));
    }
}
__global__ __launch_bounds__(BLOCK) void k_blk_piece_starts(RowView r, u64 n, const u32 *__restrict__ flag, const unsigned long long *__restrict__ rank, u32 *__restrict__ p_dlo,
                                                            u32 *__restrict__ p_edge) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK)
        if (flag[i]) { p_dlo[rank[i]] = r.dlo[i]; p_edge[rank[i]] = r.edge[i]; }
}
// the last row of a piece: the next row starts one, or is of another edge (a repeat's rows have no piece at all), or there is none
__global__ __launch_bounds__(BLOCK) void k_blk_piece_ends(RowView r, u64 n, int k, const uint8_t *__restrict__ e_cls, const u32 *__restrict__ flag,
                                                          const unsigned long long *__restrict__ rank, const u32 *__restrict__ p_dlo, u64 *__restrict__ p_len,
                                                          unsigned long long *st) {
    unsigned long long np = 0, nb = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < n; base += (u64)gridDim.x * BLOCK) {          // (uniform over the wave)
        const u64 i = base + threadIdx.x;
        unsigned long long len = 0;
        if (i < n && e_cls[r.edge[i]] != BE_REPEAT && (i + 1 == n || flag[i + 1] || r.edge[i + 1] != r.edge[i])) {
            const u64 j = rank[i + 1] - 1;                   // (starts up to and including row i) - 1
            len = (unsigned long long)(r.dhi[i] - p_dlo[j]) + (unsigned long long)k;
            p_len[j] = len;
        }
        np += (unsigned long long)__popcll(__ballot(len != 0));
        nb += wave_sum(len);
    }
    if ((threadIdx.x & 63) == 0) {
        if (np) atomicAdd(&st[FC_PIECES], np);
        if (nb) atomicAdd(&st[FC_PIECE_BASES], nb);
    }
}
__global__ __launch_bounds__(BLOCK) void k_blk_gather(const u32 *__restrict__ ids, u64 n, const uint8_t *__restrict__ cls, const uint8_t *__restrict__ full,
                                                      const u32 *__restrict__ first, const u32 *__restrict__ nrows, uint8_t *o_cls, uint8_t *o_full, u32 *o_first, u32 *o_nrows) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 e = ids[i];                        // (below the bound: checked on the host)
        o_cls[i] = cls[e]; o_full[i] = full[e]; o_first[i] = first[e]; o_nrows[i] = nrows[e];
    }
}

}  // namespace

struct gk_blocks {
    gk_ctx *ctx = nullptr;
    gk_graph *g = nullptr;
    gk_vmap *vm = nullptr;
    int k = 0, W = 1;
    u64 epoch = 0, ne = 0;
    bool failed = false, finished = false, sorted = false;
    u64 records = 0, bases = 0;
    unsigned long long *d_ctr = nullptr;         // BC_N words
    ulonglong2 *d_ev[2] = {nullptr, nullptr};    // the events of each strand, in stream order
    u64 ev_cap[2] = {0, 0}, ev_n[2] = {0, 0};
    // made by the first finish (the rows in the rule's order) and by every finish (brk, shift, the per-edge arrays, the pieces)
    u64 nrows = 0, npieces = 0;
    void *row_blob[8] = {};
    RowView rows{};
    u32 *e_flags = nullptr, *e_first = nullptr, *e_last1 = nullptr, *e_nrows = nullptr;
    uint8_t *e_cls = nullptr, *e_full = nullptr;
    u64 *p_len = nullptr;
    u32 *p_edge = nullptr;
    u64 stats[BLOCKS_NSTATS] = {};
    TextUpload up;
    float ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

u64 bl_slice_max(const gk_ctx *ctx) { return ctx->hook_place_slice > 0 ? (u64)ctx->hook_place_slice : BL_SLICE_DEFAULT; }

int bl_live(const gk_blocks *b, const char *who) {
    if (!b || !b->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null blocks handle");
    const hipError_t e = hipSetDevice(b->ctx->device);
    if (e != hipSuccess) return hip_fail(b->ctx, e, "hipSetDevice");
    if (b->g->epoch != b->epoch) return fail(b->ctx, GK_E_STATE, std::string(who) + ": the graph was edited after the blocks handle was created");
    return GK_OK;
}
int bl_done(const gk_blocks *b, const char *who) {
    if (int rc = bl_live(b, who)) return rc;
    if (!b->finished) return fail(b->ctx, GK_E_STATE, std::string(who) + ": gk_blocks_finish has not run");
    return GK_OK;
}
int bl_fail(gk_blocks *b, int code, const std::string &msg) {
    b->failed = true;
    return fail(b->ctx, code, msg);
}
#define BL_HIP(b, call)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess) { (b)->failed = true; return gk::hip_fail((b)->ctx, e__, #call); } \
    } while (0)

// room for `need` events of strand s: a larger block from the pool, what is there copied over
int bl_reserve(gk_blocks *b, int s, u64 need) {
    if (need <= b->ev_cap[s]) return GK_OK;
    gk_ctx *ctx = b->ctx;
    const u64 cap = std::max<u64>(need + need / 2, 1ull << 16);
    ulonglong2 *nw = nullptr;
    BL_HIP(b, pool_malloc(ctx, &nw, cap * sizeof(ulonglong2)));
    if (b->ev_n[s]) {
        const hipError_t e = hipMemcpyAsync(nw, b->d_ev[s], b->ev_n[s] * sizeof(ulonglong2), hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) { (void)pool_free(ctx, nw); b->failed = true; return hip_fail(ctx, e, "gk_blocks_add_record: growing the event buffer"); }
    }
    if (b->d_ev[s]) (void)pool_free(ctx, b->d_ev[s]);            // (waits for the copy)
    b->d_ev[s] = nw;
    b->ev_cap[s] = cap;
    return GK_OK;
}

// the record of one call, slice by slice.  The feeder is gk_placements_add_record's restated, not shared: a slice here brings k
// characters along, not k - 1, and runs two launches with a read-back between them, so the placements' timings would change
// their meaning if both went through one loop.
int bl_run(gk_blocks *b, const char *bases, u64 n) {
    gk_ctx *ctx = b->ctx;
    const int k = b->k;
    const u64 slice_max = bl_slice_max(ctx), cap = std::min<u64>(n, slice_max) + 64;          // a slice and its halo (k <= 64)
    const int nbuf = n > slice_max ? 2 : 1;
    const bool pinned = TextUpload::is_pinned(bases);
    const u64 max_tiles = (cap + BL_WT - 1) / BL_WT;
    double up_ms = 0, count_ms = 0, emit_ms = 0;
    DevScratch tmp(ctx);
    uint8_t *tb[2] = {nullptr, nullptr};
    u32 *d_info = nullptr, *d_cnt = nullptr;
    unsigned long long *d_off = nullptr;
    for (int i = 0; i < nbuf; i++) tmp.get(&tb[i], std::max<u64>(cap + 64, 1ull << 20));      // (a block of 1 MiB is pooled)
    tmp.get(&d_info, max_tiles * 256);
    tmp.get(&d_cnt, 2 * max_tiles);
    tmp.get(&d_off, 2 * max_tiles + 1);
    u64 *d_sums = nullptr;
    tmp.get(&d_sums, 2 * max_tiles / SCAN_CHUNK + 2);
    if (tmp.error() != hipSuccess) { b->failed = true; return hip_fail(ctx, tmp.error(), "gk_blocks_add_record: slice buffers"); }
    void *slots = nullptr;
    uint32_t nb2 = 1, lnb1 = 0;
    vmap_table(b->vm, &slots, &nb2, &lnb1);
    const TimedSection kt{ctx};
    auto halo_of = [&](u64 s0) { return std::min<u64>((u64)k, s0); };
    int bi = 0, rc = GK_OK;
    u64 s0 = 0;
    if (!pinned && n > slice_max) { if ((rc = b->up.reserve(ctx, slice_max + 64))) { b->failed = true; return rc; } }
    if ((rc = b->up.upload(ctx, 0, tb[0], bases, std::min<u64>(n, slice_max), pinned, &up_ms))) { b->failed = true; return rc; }
    while (s0 < n) {
        const u64 len = std::min<u64>(n - s0, slice_max), halo = halo_of(s0), L = halo + len, s1 = s0 + len;
        const u32 first = halo == (u64)k ? 1u : 0u, sentinel = s1 == n ? 1u : 0u;
        const unsigned grid = (unsigned)((L + BL_WT - 1) / BL_WT);
        BL_HIP(b, hipStreamWaitEvent(ctx->stream, b->up.up1[bi], 0));
        BL_HIP(b, kt.start());
        GK_BY_W(b->W, hipLaunchKernelGGL((k_block_windows<W, false>), dim3(grid), dim3(256), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u},
                                         b->g->v, k, tb[bi], L, halo, first, sentinel, s0 - halo, (u32)b->records, d_info, d_cnt,
                                         (const unsigned long long *)nullptr, (u64)0, (ulonglong2 *)nullptr, (ulonglong2 *)nullptr, b->d_ctr));
        BL_HIP(b, hipGetLastError());
        BL_HIP(b, scan_counts(ctx, d_cnt, 2 * (u64)grid, d_off, d_sums));
        if ((rc = kt.end(&count_ms))) { b->failed = true; return rc; }
        unsigned long long tot0 = 0, tot = 0, bad = 0;
        BL_HIP(b, read_back(ctx, {{&tot0, d_off + grid, 8}, {&tot, d_off + 2 * (u64)grid, 8}, {&bad, b->d_ctr + BC_BAD, 8}}));
        {
            float t = 0;
            BL_HIP(b, hipEventElapsedTime(&t, b->up.up0[bi], b->up.up1[bi]));
            up_ms += t;
        }
        if (bad) return bl_fail(b, GK_E_STATE, "gk_blocks_add_record: the position map names an edge that is not live in this graph (a stale map)");
        // (the stream is idle: the other buffer is free, and the next slice goes up on the copy stream beside this one's emit launch)
        if (s1 < n) {
            const u64 h1 = halo_of(s1), len1 = std::min<u64>(n - s1, slice_max);
            if ((rc = b->up.upload(ctx, 1 - bi, tb[1 - bi], bases + (s1 - h1), h1 + len1, pinned, &up_ms))) { b->failed = true; return rc; }
        }
        const u64 cnt[2] = {tot0, tot - tot0};
        for (int s = 0; s < 2; s++) if ((rc = bl_reserve(b, s, b->ev_n[s] + cnt[s]))) return rc;
        if (tot) {
            BL_HIP(b, kt.start());
            GK_BY_W(b->W, hipLaunchKernelGGL((k_block_windows<W, true>), dim3(grid), dim3(256), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u},
                                             b->g->v, k, tb[bi], L, halo, first, sentinel, s0 - halo, (u32)b->records, d_info, d_cnt, (const unsigned long long *)d_off,
                                             (u64)tot0, b->d_ev[0] + b->ev_n[0], b->d_ev[1] + b->ev_n[1], b->d_ctr));
            BL_HIP(b, hipGetLastError());
            if ((rc = kt.end(&emit_ms))) { b->failed = true; return rc; }
            b->ev_n[0] += cnt[0]; b->ev_n[1] += cnt[1];
        }
        s0 = s1;
        bi = 1 - bi;
    }
    BL_HIP(b, hipStreamSynchronize(ctx->copy_stream));
    b->ms[0] = (float)up_ms; b->ms[1] = (float)count_ms; b->ms[2] = (float)emit_ms;
    return GK_OK;
}

void bl_free_rows(gk_blocks *b) {
    for (void *&q : b->row_blob) { if (q) (void)pool_free(b->ctx, q); q = nullptr; }
    if (b->p_len) (void)pool_free(b->ctx, b->p_len);
    if (b->p_edge) (void)pool_free(b->ctx, b->p_edge);
    b->p_len = nullptr; b->p_edge = nullptr;
    b->rows = RowView{};
}

// events -> rows in the rule's order; once per set of records.  A failure leaves no rows behind: the next finish starts over.
int bl_sort_rows(gk_blocks *b);
int bl_sort(gk_blocks *b) {
    if (b->sorted) return GK_OK;
    bl_free_rows(b);
    const int rc = bl_sort_rows(b);
    if (rc != GK_OK) bl_free_rows(b);
    else b->sorted = true;
    return rc;
}
int bl_sort_rows(gk_blocks *b) {
    gk_ctx *ctx = b->ctx;
    const u64 nev = b->ev_n[0] + b->ev_n[1];
    const EvView ev{{b->d_ev[0], b->d_ev[1]}, {b->ev_n[0], b->ev_n[1]}};
    DevScratch tmp(ctx);
    u32 *d_flag = nullptr;
    unsigned long long *d_rank = nullptr;
    unsigned long long nrows = 0;
    if (nev) {
        tmp.get(&d_flag, nev);
        tmp.get(&d_rank, nev + 1);
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_blocks_finish: scratch");
        hipLaunchKernelGGL(k_blk_flags, dim3(ggrid(ctx, nev)), dim3(BLOCK), 0, ctx->stream, ev, d_flag);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, tmp, d_flag, nev, d_rank));
        GK_HIP(ctx, read_back(ctx, &nrows, d_rank + nev));
    }
    if (nrows > 0xffffffffull) return fail(ctx, GK_E_CAPACITY, "gk_blocks_finish: more than 2^32 - 1 rows");
    b->nrows = nrows;
    if (nrows) {
        const u64 n = nrows;
        u32 *u_edge = nullptr, *u_sr = nullptr, *idx = nullptr, *idx1 = nullptr, *idx2 = nullptr, *key = nullptr, *key2 = nullptr;
        long long *u_pos = nullptr;
        u64 *u_dd = nullptr, *dd2 = nullptr;
        void *d_temp = nullptr;
        size_t t1 = 0, t2 = 0;
        tmp.get(&u_edge, n); tmp.get(&u_sr, n); tmp.get(&u_pos, n); tmp.get(&u_dd, n); tmp.get(&dd2, n);
        tmp.get(&idx, n); tmp.get(&idx1, n); tmp.get(&idx2, n); tmp.get(&key, n); tmp.get(&key2, n);
        tmp.note(rocprim::radix_sort_pairs(nullptr, t1, u_dd, dd2, idx, idx1, (size_t)n, 0, 64, ctx->stream));         // (the size queries)
        tmp.note(rocprim::radix_sort_pairs(nullptr, t2, key, key2, idx1, idx2, (size_t)n, 0, 32, ctx->stream));
        tmp.get((uint8_t **)&d_temp, std::max(t1, t2));
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_blocks_finish: scratch");
        const size_t sizes[8] = {4, 4, 4, 4, 1, 1, 8, 8};
        hipError_t e = hipSuccess;
        for (int i = 0; i < 8 && e == hipSuccess; i++) e = pool_malloc(ctx, &b->row_blob[i], n * sizes[i]);
        if (e == hipSuccess) e = pool_malloc(ctx, &b->p_len, n * 8);
        if (e == hipSuccess) e = pool_malloc(ctx, &b->p_edge, n * 4);
        if (e != hipSuccess) return hip_fail(ctx, e, "gk_blocks_finish: rows");
        b->rows = RowView{(u32 *)b->row_blob[0], (u32 *)b->row_blob[1], (u32 *)b->row_blob[2], (u32 *)b->row_blob[3], (uint8_t *)b->row_blob[4], (uint8_t *)b->row_blob[5],
                          (long long *)b->row_blob[6], (long long *)b->row_blob[7]};
        hipLaunchKernelGGL(k_blk_rows, dim3(ggrid(ctx, nev)), dim3(BLOCK), 0, ctx->stream, ev, b->k, d_flag, d_rank, u_edge, u_sr, u_pos, u_dd, idx);
        GK_HIP(ctx, hipGetLastError());
        // by (edge, dlo, dhi); the rows arrive ordered by (strand, record, start), the rest of the key, and the radix sort is stable:
        // the minor key goes first
        GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, t1, u_dd, dd2, idx, idx1, (size_t)n, 0, 64, ctx->stream));
        hipLaunchKernelGGL(k_blk_edge_keys, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, u_edge, idx1, n, key);
        GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, t2, key, key2, idx1, idx2, (size_t)n, 0, 32, ctx->stream));
        hipLaunchKernelGGL(k_blk_permute, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, idx2, n, u_edge, u_sr, u_pos, u_dd, b->rows);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GK_OK;
}

}  // namespace

extern "C" {

void gk_blocks_destroy(gk_blocks *b) {
    if (!b) return;
    gk_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    bl_free_rows(b);
    for (void *q : {(void *)b->d_ctr, (void *)b->d_ev[0], (void *)b->d_ev[1], (void *)b->e_flags, (void *)b->e_first, (void *)b->e_last1, (void *)b->e_nrows,
                    (void *)b->e_cls, (void *)b->e_full})
        if (q) (void)pool_free(ctx, q);
    b->up.destroy();
    delete b;
}

int gk_blocks_create(gk_graph *g, gk_vmap *positions, gk_blocks **out) {
    if (!out) return fail(g ? g->ctx : nullptr, GK_E_INVALID, "gk_blocks_create: out is NULL");
    *out = nullptr;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (!positions) return fail(ctx, GK_E_INVALID, "gk_blocks_create: null position map");
    if (vmap_ctx(positions) != ctx) return fail(ctx, GK_E_INVALID, "gk_blocks_create: the position map lives on another context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, "gk_blocks_create: the position map has another k");
    gk_blocks *b = new gk_blocks;
    b->ctx = ctx; b->g = g; b->vm = positions; b->k = g->k; b->W = words_for_k(g->k); b->epoch = g->epoch; b->ne = g->v.n_edges;
    const u64 m = std::max<u64>(b->ne, 1);
    hipError_t e = b->up.create();
    if (e == hipSuccess) e = pool_malloc(ctx, &b->d_ctr, BC_N * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_flags, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_first, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_last1, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_nrows, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_cls, m);
    if (e == hipSuccess) e = pool_malloc(ctx, &b->e_full, m);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_ctr, 0, BC_N * 8, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { const int rc = hip_fail(ctx, e, "gk_blocks_create"); gk_blocks_destroy(b); return rc; }
    *out = b;
    return GK_OK;
}

int gk_blocks_add_record(gk_blocks *b, const char *bases, uint64_t n) {
    if (int rc = bl_live(b, "gk_blocks_add_record")) return rc;
    gk_ctx *ctx = b->ctx;
    if (b->failed) return fail(ctx, GK_E_STATE, "gk_blocks_add_record: the handle failed earlier (see the first error); destroy it");
    if (b->finished) return fail(ctx, GK_E_STATE, "gk_blocks_add_record: gk_blocks_finish has run; the handle takes no more records");
    if (!bases && n) return fail(ctx, GK_E_INVALID, "gk_blocks_add_record: null bases");
    if (b->records >= BL_MAX_RECORDS) return bl_fail(b, GK_E_CAPACITY, "gk_blocks_add_record: more than 2^24 records");
    if (n >= BL_MAX_BASES) return bl_fail(b, GK_E_CAPACITY, "gk_blocks_add_record: a record of 2^39 bases or more");
    const auto t_call = clk::now();
    b->ms[0] = b->ms[1] = b->ms[2] = 0;
    if (n) { if (int rc = bl_run(b, bases, n)) return rc; }
    b->records++;
    b->bases += n;
    b->ms[3] = (float)ms_since(t_call);
    return GK_OK;
}

int gk_blocks_finish(gk_blocks *b, uint64_t tol) {
    if (int rc = bl_live(b, "gk_blocks_finish")) return rc;
    gk_ctx *ctx = b->ctx;
    if (b->failed) return fail(ctx, GK_E_STATE, "gk_blocks_finish: the handle failed earlier (see the first error); destroy it");
    const auto t_call = clk::now();
    double k_ms = 0;
    const TimedSection kt{ctx};
    GK_HIP(ctx, kt.start());
    if (int rc = bl_sort(b)) return rc;
    const u64 n = b->nrows, m = std::max<u64>(b->ne, 1);
    DevScratch tmp(ctx);
    unsigned long long *d_st = nullptr, *d_rank = nullptr, h_st[FC_N] = {}, h_ctr[BC_N] = {};
    u32 *d_flag = nullptr, *p_dlo = nullptr;
    tmp.zeroed(&d_st, FC_N);
    tmp.get(&d_flag, n); tmp.get(&d_rank, n + 1); tmp.get(&p_dlo, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_blocks_finish: scratch");
    GK_HIP(ctx, hipMemsetAsync(b->e_flags, 0, m * 4, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(b->e_first, 0, m * 4, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(b->e_last1, 0, m * 4, ctx->stream));
    if (n) hipLaunchKernelGGL(k_blk_class, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, b->rows, n, (u64)tol, b->e_flags, b->e_first, b->e_last1, d_st);
    if (b->ne)
        hipLaunchKernelGGL(k_blk_edges, dim3(ggrid(ctx, b->ne)), dim3(BLOCK), 0, ctx->stream, b->g->v, b->ne, b->rows, b->e_flags, b->e_first, b->e_last1, b->e_cls, b->e_full,
                           b->e_nrows, d_st);
    GK_HIP(ctx, hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(k_blk_piece_flags, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, b->rows, n, b->e_cls, d_flag);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, tmp, d_flag, n, d_rank));
        hipLaunchKernelGGL(k_blk_piece_starts, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, b->rows, n, d_flag, d_rank, p_dlo, b->p_edge);
        hipLaunchKernelGGL(k_blk_piece_ends, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, b->rows, n, b->k, b->e_cls, d_flag, d_rank, p_dlo, b->p_len, d_st);
    }
    GK_HIP(ctx, read_back(ctx, {{h_st, d_st, sizeof(h_st)}, {h_ctr, b->d_ctr, sizeof(h_ctr)}}));
    if (int rc = kt.end(&k_ms)) return rc;
    u64 *st = b->stats;
    st[0] = b->records; st[1] = b->bases; st[2] = h_ctr[BC_VALID]; st[3] = h_ctr[BC_WINDOWS]; st[4] = h_ctr[BC_COVERED]; st[5] = n;
    for (int c = 0; c < 6; c++) { st[6 + c] = h_st[FC_BRK + c]; st[12 + c] = h_st[FC_EDGE + c]; }
    st[18] = h_st[FC_FULL]; st[19] = h_st[FC_KMERS]; st[20] = h_st[FC_PIECES]; st[21] = h_st[FC_PIECE_BASES]; st[22] = h_st[FC_SHIFT_SUM]; st[23] = h_st[FC_SHIFT_MAX];
    b->npieces = h_st[FC_PIECES];
    b->finished = true;
    b->ms[4] = (float)k_ms;
    b->ms[5] = (float)ms_since(t_call);
    return GK_OK;
}

int gk_blocks_stats(const gk_blocks *b, uint64_t *stats) {
    if (int rc = bl_done(b, "gk_blocks_stats")) return rc;
    if (!stats) return fail(b->ctx, GK_E_INVALID, "gk_blocks_stats: stats is NULL");
    for (int i = 0; i < BLOCKS_NSTATS; i++) stats[i] = b->stats[i];
    return GK_OK;
}

int gk_blocks_rows(const gk_blocks *b, uint32_t *edge, uint8_t *strand, uint32_t *record, int64_t *pos, uint32_t *dlo, uint32_t *dhi, uint8_t *brk, int64_t *shift,
                   uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (int rc = bl_done(b, "gk_blocks_rows")) return rc;
    gk_ctx *ctx = b->ctx;
    if (!n) return fail(ctx, GK_E_INVALID, "gk_blocks_rows: n is NULL");
    const u64 m = b->nrows;
    *n = m;
    if (m > cap) return fail(ctx, GK_E_CAPACITY, "gk_blocks_rows: room for " + std::to_string(cap) + " rows, " + std::to_string(m) + " needed");
    if (m == 0) return GK_OK;
    const RowView &r = b->rows;
    GK_HIP(ctx, read_back(ctx, {{edge, r.edge, (size_t)m * 4}, {strand, r.strand, (size_t)m}, {record, r.record, (size_t)m * 4}, {pos, r.pos, (size_t)m * 8},
                                {dlo, r.dlo, (size_t)m * 4}, {dhi, r.dhi, (size_t)m * 4}, {brk, r.brk, (size_t)m}, {shift, r.shift, (size_t)m * 8}}));
    return GK_OK;
}

int gk_blocks_edges(const gk_blocks *b, const uint32_t *edge_ids, uint64_t n, uint8_t *cls, uint8_t *full, uint32_t *first_row, uint32_t *nrows) {
    if (int rc = bl_done(b, "gk_blocks_edges")) return rc;
    gk_ctx *ctx = b->ctx;
    if (n == 0) return GK_OK;
    if (!edge_ids) return fail(ctx, GK_E_INVALID, "gk_blocks_edges: edge_ids is NULL");
    for (u64 i = 0; i < n; i++)
        if (edge_ids[i] >= b->ne) return fail(ctx, GK_E_INVALID, "gk_blocks_edges: edge id " + std::to_string(edge_ids[i]) + " is not below the bound " + std::to_string(b->ne));
    DevScratch tmp(ctx);
    u32 *d_ids = nullptr, *o_first = nullptr, *o_nrows = nullptr;
    uint8_t *o_cls = nullptr, *o_full = nullptr;
    tmp.upload(&d_ids, edge_ids, n);
    tmp.get(&o_cls, n); tmp.get(&o_full, n); tmp.get(&o_first, n); tmp.get(&o_nrows, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_blocks_edges: scratch");
    hipLaunchKernelGGL(k_blk_gather, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, d_ids, (u64)n, b->e_cls, b->e_full, b->e_first, b->e_nrows, o_cls, o_full, o_first, o_nrows);
    GK_HIP(ctx, read_back(ctx, {{cls, o_cls, (size_t)n}, {full, o_full, (size_t)n}, {first_row, o_first, (size_t)n * 4}, {nrows, o_nrows, (size_t)n * 4}}));
    return GK_OK;
}

int gk_blocks_pieces(const gk_blocks *b, uint64_t *len, uint32_t *edge, uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (int rc = bl_done(b, "gk_blocks_pieces")) return rc;
    gk_ctx *ctx = b->ctx;
    if (!n) return fail(ctx, GK_E_INVALID, "gk_blocks_pieces: n is NULL");
    const u64 m = b->npieces;
    *n = m;
    if (m > cap) return fail(ctx, GK_E_CAPACITY, "gk_blocks_pieces: room for " + std::to_string(cap) + " pieces, " + std::to_string(m) + " needed");
    if (m == 0) return GK_OK;
    GK_HIP(ctx, read_back(ctx, {{len, b->p_len, (size_t)m * 8}, {edge, b->p_edge, (size_t)m * 4}}));
    return GK_OK;
}

int gk_blocks_last_ms(const gk_blocks *b, float *ms6) {
    if (!b) return fail(nullptr, GK_E_INVALID, "gk_blocks_last_ms: null handle");
    if (!ms6) return fail(b->ctx, GK_E_INVALID, "gk_blocks_last_ms: null buffer");
    for (int i = 0; i < 6; i++) ms6[i] = b->ms[i];
    return GK_OK;
}

}  // extern "C"
