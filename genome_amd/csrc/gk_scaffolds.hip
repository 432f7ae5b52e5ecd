// gk_scaffolds.hip — scaffolds as FASTA text, written on the device: one record per chain of edges, junctions inside the graph
// joined on the shared node, gaps outside it filled with N, one strand per chain; the edges in no chain follow as contig records.
//
// The rule is this project's own and stated in include/genome_amd.h ("scaffolds: this project's own rule"); tests/scaffolds_ref.py
// restates it.  The chains are gk_scaffold_chains' (gk_links.hip), the text helpers and the chunked stream gk_fastaout.h's.
//
// The plan.  The chain list's front end, the check included, is gk_chains.h's.  k_scaf_segments: one lane per member decides the
// junction before it and fills two slots, an N run and a piece of the edge's path; a scan over the slot lengths
// places every slot in its scaffold.  k_scaf_strand: one wave per chain compares the scaffold with its reverse complement, a lane
// finding its base by a binary search in the chain's slots, and sizes the record.  k_scaf_single: k_contig_classify's comparison
// over the live edges no chain claimed.  Three more scans and two compactions leave the records (name, byte offset, segment range, n)
// and the segments (edge or N, first base, bases skipped) in text order.
// k_scaffold_emit is output-centric like k_contig_emit: a byte range comes in, a lane writes one aligned 8-byte word, the record
// found by one binary search per wave, the segment by one per item and then by stepping.  No LDS, no atomics.
#include <memory>
#include <vector>

#include "gk_chains.h"
#include "gk_fastaout.h"
#include "gk_scan.h"

static constexpr uint8_t SC_SHORT = 1, SC_FORWARD = 2, SC_SELF = 3, SC_REVERSE = 4;
static constexpr uint8_t MC_FIRST = 0, MC_ADJACENT = 1, MC_GAPPED = 2, MC_CLAMPED = 3, MC_OVERLAPPED = 4;
// device counters of a plan
enum { SS_FORWARD = 0, SS_SELF, SS_REVERSE, SS_SINGLE, SS_MEMBERS, SS_ADJACENT, SS_GAPPED, SS_CLAMPED, SS_NBASES, SS_BASES, SS_OVERFLOW, SS_OVERLAPPED, SS_DROPPED, SS_N };
static constexpr int SCAFFOLD_STATS = 13;

// ---------------------------------------------------------------------------------------------
// segments
// ---------------------------------------------------------------------------------------------
// Member j of chain c fills slots 2j (an N run, or nothing) and 2j + 1 (its piece).  Runs only behind a clean check.  `overlap`
// (may be null) is the caller's and is not trusted: an entry that the rule cannot have given raises SF_OVERLAP.
__device__ __forceinline__ bool scaf_overlap_holds(const GraphView &g, u32 p, u32 e, u64 pp, u32 o) {
    const u32 sp = g.e_start[p], se = g.e_start[e];
    const u64 plo = g.node_lo[sp], phi = g.k > 32 ? g.node_hi[sp] : 0ull, elo = g.node_lo[se], ehi = g.k > 32 ? g.node_hi[se] : 0ull;
    const uint8_t *pseq = g.pool + g.e_off[p], *eseq = g.pool + g.e_off[e];
    bool same = true;
    for (u32 i = 0; i < o; i++) same &= path_base(plo, phi, pseq, g.k, pp - o + i) == path_base(elo, ehi, eseq, g.k, i);
    return same;
}
__global__ __launch_bounds__(BLOCK) void k_scaf_segments(GraphView g, const u32 *__restrict__ members, const unsigned long long *__restrict__ chain_off, u64 nchains,
                                                         u64 nm, const long long *__restrict__ gap, const u32 *__restrict__ overlap, long long min_gap, u32 *flags,
                                                         u32 *__restrict__ chain_of,
                                                         uint8_t *__restrict__ mclass, u32 *__restrict__ slot_len, u32 *__restrict__ slot_edge,
                                                         uint8_t *__restrict__ slot_skip) {
    if (chains_unchecked(flags)) return;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nm; j += (u64)gridDim.x * BLOCK) {
        const u64 lo = chain_of_member(chain_off, nchains, j);
        const u32 e = members[j];
        uint8_t cls = MC_FIRST;
        u64 run = 0;
        u32 skip = 0;
        if (j != chain_off[lo]) {
            const u32 p = members[j - 1];
            const u32 o = overlap ? overlap[j - 1] : 0u;
            if (g.e_end[p] == g.e_start[e]) {
                cls = MC_ADJACENT; skip = (u32)g.k;
                if (o) flags[SF_OVERLAP] = 1;
            } else if (o) {                                  // below both path lengths, and the o bases are the same
                const u64 pp = (u64)g.k + g.e_len[p], pe = (u64)g.k + g.e_len[e];
                cls = MC_OVERLAPPED;
                if (o > GK_OVERLAP_MAX || o >= pp || o >= pe || !scaf_overlap_holds(g, p, e, pp, o)) flags[SF_OVERLAP] = 1;
                else skip = o;
            } else {
                const long long gp = gap[j - 1];
                cls = gp < min_gap ? MC_CLAMPED : MC_GAPPED;
                if (gp > 0x7fffffffll) flags[SF_GAP] = 1;
                else run = (u64)max(gp, min_gap);
            }
        }
        u64 piece = (u64)g.k + g.e_len[e] - skip;
        if (piece > 0xffffffffull) { flags[SF_OVERFLOW] = 1; piece = 0; }
        chain_of[j] = (u32)lo;
        mclass[j] = cls;
        slot_len[2 * j] = (u32)run;       slot_edge[2 * j] = NONE;  slot_skip[2 * j] = 0;
        slot_len[2 * j + 1] = (u32)piece; slot_edge[2 * j + 1] = e; slot_skip[2 * j + 1] = (uint8_t)skip;
    }
}

// ---------------------------------------------------------------------------------------------
// strand and size: one wave per chain, one wave per unclaimed edge
// ---------------------------------------------------------------------------------------------
// the code (A0 G1 C2 T3 N4) of the base at scan position `at` of the chain whose slots are [s0, s1): base[s0] <= at < base[s1].
// The last slot whose base is <= at is never an empty one.
__device__ __forceinline__ int scaf_base(const GraphView &g, const unsigned long long *__restrict__ slot_base, const u32 *__restrict__ slot_edge,
                                         const uint8_t *__restrict__ slot_skip, u64 s0, u64 s1, u64 at) {
    u64 lo = s0, hi = s1;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (slot_base[mid] <= at) lo = mid; else hi = mid;
    }
    const u32 e = slot_edge[lo];
    if (e == NONE) return 4;
    const u32 s = g.e_start[e];
    return path_base(g.node_lo[s], g.k > 32 ? g.node_hi[s] : 0ull, g.pool + g.e_off[e], g.k, (u64)slot_skip[lo] + (at - slot_base[lo]));
}
__device__ __forceinline__ int scaf_hdr_len(bool chain, u64 id, u64 n, u64 m, u64 gaps) {
    return 2 + dec_digits(id) + 5 + dec_digits(n) + (chain ? 9 + dec_digits(m) + 6 + dec_digits(gaps) : 0) + 1;
}

// sel[c] = 1 for a record, size[c] = the bytes of its text, chain_n[c] / chain_gaps[c] = its bases / those of them that are N
__global__ __launch_bounds__(BLOCK) void k_scaf_strand(GraphView g, const unsigned long long *__restrict__ chain_off, u64 nchains,
                                                       const unsigned long long *__restrict__ slot_base, const u32 *__restrict__ slot_len,
                                                       const u32 *__restrict__ slot_edge, const uint8_t *__restrict__ slot_skip, const uint8_t *__restrict__ mclass,
                                                       u32 line_width, int strands, u32 *__restrict__ sel, u32 *__restrict__ size, u32 *__restrict__ chain_n,
                                                       u32 *__restrict__ chain_gaps, unsigned long long *stats) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 c = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); c < nchains; c += waves) {      // (uniform over the wave)
        const u64 m0 = chain_off[c], m1 = chain_off[c + 1], s0 = 2 * m0, s1 = 2 * m1;
        const u64 b0 = slot_base[s0], n = slot_base[s1] - b0;
        u64 gaps = 0, adj = 0, gapped = 0, clamped = 0, ovl = 0, dropped = 0;
        for (u64 j = m0 + (u64)lane; j < m1; j += 64) {
            const uint8_t mc = mclass[j];
            gaps += slot_len[2 * j];
            adj += mc == MC_ADJACENT; gapped += mc == MC_GAPPED || mc == MC_CLAMPED; clamped += mc == MC_CLAMPED;
            if (mc == MC_OVERLAPPED) { ovl++; dropped += slot_skip[2 * j + 1]; }
        }
        gaps = wave_sum(gaps); adj = wave_sum(adj); gapped = wave_sum(gapped); clamped = wave_sum(clamped);
        if (__any(ovl != 0)) { ovl = wave_sum(ovl); dropped = wave_sum(dropped); }
        uint8_t cl = SC_SELF;
        const u64 half = (n + 1) / 2;                        // (the complement is an involution: the second half repeats the first)
        for (u64 i0 = 0; i0 < half; i0 += 64) {
            const u64 i = i0 + (u64)lane;
            int a = 0, b = 0;
            if (i < half) {
                a = scaf_base(g, slot_base, slot_edge, slot_skip, s0, s1, b0 + i);
                b = scaf_base(g, slot_base, slot_edge, slot_skip, s0, s1, b0 + (n - 1 - i));
                b = b < 4 ? 3 - b : 4;
            }
            const unsigned long long differ = __ballot(a != b);
            if (differ) {
                cl = __shfl(a < b ? 1 : 0, __ffsll((long long)differ) - 1) ? SC_FORWARD : SC_REVERSE;
                break;
            }
        }
        if (lane == 0) {
            const bool rec = cl != SC_REVERSE || strands == 2;
            const u64 bytes = (u64)scaf_hdr_len(true, c, n, m1 - m0, gaps) + body_bytes(n, line_width);
            const bool over = n > 0xffffffffull || bytes > 0xfffffff0ull;
            sel[c] = rec && !over; size[c] = rec && !over ? (u32)bytes : 0u; chain_n[c] = (u32)n; chain_gaps[c] = (u32)gaps;
            atomicAdd(&stats[SS_FORWARD + (cl - SC_FORWARD)], 1ull);
            if (rec && over) atomicAdd(&stats[SS_OVERFLOW], 1ull);
            if (rec && !over) {
                atomicAdd(&stats[SS_MEMBERS], (unsigned long long)(m1 - m0));
                if (adj) atomicAdd(&stats[SS_ADJACENT], (unsigned long long)adj);
                if (gapped) atomicAdd(&stats[SS_GAPPED], (unsigned long long)gapped);
                if (clamped) atomicAdd(&stats[SS_CLAMPED], (unsigned long long)clamped);
                if (ovl) { atomicAdd(&stats[SS_OVERLAPPED], (unsigned long long)ovl); atomicAdd(&stats[SS_DROPPED], (unsigned long long)dropped); }
                if (gaps) atomicAdd(&stats[SS_NBASES], (unsigned long long)gaps);
                atomicAdd(&stats[SS_BASES], (unsigned long long)n);
            }
        }
    }
}

// the live edges in no chain, as gk_graph_contigs_plan selects and sizes them (k_contig_classify's comparison); sel / size / flag
// point at the edges' part of the record and slot arrays
__global__ __launch_bounds__(BLOCK) void k_scaf_single(GraphView g, const u32 *__restrict__ owner, u64 min_len, u32 line_width, int strands, u32 *__restrict__ sel,
                                                       u32 *__restrict__ size, u32 *__restrict__ flag, unsigned long long *stats) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    unsigned long long recs = 0, bases = 0, over = 0;
    for (u64 e = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e < g.n_edges; e += waves) {      // (uniform over the wave)
        if (!g.e_alive[e] || owner[e]) {
            if (lane == 0) { sel[e] = 0; size[e] = 0; flag[e] = 0; }
            continue;
        }
        const u64 n = (u64)g.k + g.e_len[e];
        uint8_t c = SC_SELF;
        if (n < min_len) c = SC_SHORT;
        else {
            const u32 s = g.e_start[e];
            const u64 nlo = g.node_lo[s], nhi = g.k > 32 ? g.node_hi[s] : 0ull;
            const uint8_t *seq = g.pool + g.e_off[e];
            const u64 half = (n + 1) / 2;
            for (u64 i0 = 0; i0 < half; i0 += 64) {
                const u64 i = i0 + (u64)lane;
                int a = 0, b = 0;
                if (i < half) { a = path_base(nlo, nhi, seq, g.k, i); b = 3 - path_base(nlo, nhi, seq, g.k, n - 1 - i); }
                const unsigned long long differ = __ballot(a != b);
                if (differ) {
                    c = __shfl(a < b ? 1 : 0, __ffsll((long long)differ) - 1) ? SC_FORWARD : SC_REVERSE;
                    break;
                }
            }
        }
        if (lane == 0) {
            const bool rec = c == SC_FORWARD || c == SC_SELF || (c == SC_REVERSE && strands == 2);
            u64 bytes = 0;
            if (rec) {
                bytes = (u64)scaf_hdr_len(false, e, n, 0, 0) + body_bytes(n, line_width);
                if (bytes > 0xfffffff0ull) { over = 1; bytes = 0; }
                else { bases += n; recs++; }
            }
            sel[e] = rec && bytes; size[e] = (u32)bytes; flag[e] = rec && bytes;
        }
    }
    if (lane == 0) {
        if (recs) atomicAdd(&stats[SS_SINGLE], recs);
        if (bases) atomicAdd(&stats[SS_BASES], bases);
        if (over) atomicAdd(&stats[SS_OVERFLOW], over);
    }
}

// a slot becomes a segment of the plan iff it holds bases and its chain is written
__global__ __launch_bounds__(BLOCK) void k_scaf_flags(u64 nm, const u32 *__restrict__ slot_len, const u32 *__restrict__ chain_of, const u32 *__restrict__ sel,
                                                      u32 *__restrict__ flag) {
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < 2 * nm; u += (u64)gridDim.x * BLOCK) flag[u] = slot_len[u] != 0 && sel[chain_of[u >> 1]];
}

// ---------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------
struct ScafPlan {
    const u32 *rec_id;                       // a chain's index in the input (records below chain_recs), or an edge id
    const unsigned long long *rec_off;       // [records + 1] bytes
    const unsigned long long *rec_seg;       // [records + 1] segments
    const u32 *rec_n;                        // bases
    const u32 *rec_m, *rec_gaps;             // [chain_recs] members, N bases
    const u32 *seg_edge;                     // NONE: an N run
    const u32 *seg_start;                    // its first base in the record
    const uint8_t *seg_skip;                 // bases of the edge's path left out before it: 0, k, or an overlap (<= GK_OVERLAP_MAX)
    u64 records, chain_recs;
    u32 line_width;
};
// t < nchains: chain t; t >= nchains: edge t - nchains.  The records in that order: (name, byte offset, first segment, n[, m, gaps])
__global__ __launch_bounds__(BLOCK) void k_scaf_compact_recs(GraphView g, u64 nchains, u64 nm, const unsigned long long *__restrict__ chain_off,
                                                             const u32 *__restrict__ sel, const unsigned long long *__restrict__ rank,
                                                             const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ segrank,
                                                             const u32 *__restrict__ chain_n, const u32 *__restrict__ chain_gaps, u32 *__restrict__ rec_id,
                                                             unsigned long long *__restrict__ rec_off, unsigned long long *__restrict__ rec_seg, u32 *__restrict__ rec_n,
                                                             u32 *__restrict__ rec_m, u32 *__restrict__ rec_gaps) {
    const u64 total = nchains + g.n_edges;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t <= total; t += (u64)gridDim.x * BLOCK) {
        if (t == total) { rec_off[rank[t]] = off[t]; rec_seg[rank[t]] = segrank[2 * nm + g.n_edges]; continue; }
        if (!sel[t]) continue;
        const u64 r = rank[t];
        rec_off[r] = off[t];
        if (t < nchains) {
            rec_id[r] = (u32)t; rec_seg[r] = segrank[2 * chain_off[t]]; rec_n[r] = chain_n[t];
            rec_m[r] = (u32)(chain_off[t + 1] - chain_off[t]); rec_gaps[r] = chain_gaps[t];
        } else {
            const u64 e = t - nchains;
            rec_id[r] = (u32)e; rec_seg[r] = segrank[2 * nm + e]; rec_n[r] = (u32)((u64)g.k + g.e_len[e]);
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_scaf_compact_segs(u64 n_edges, u64 nm, const unsigned long long *__restrict__ chain_off, const u32 *__restrict__ chain_of,
                                                             const u32 *__restrict__ flag, const unsigned long long *__restrict__ segrank,
                                                             const unsigned long long *__restrict__ slot_base, const u32 *__restrict__ slot_edge,
                                                             const uint8_t *__restrict__ slot_skip, u32 *__restrict__ seg_edge, u32 *__restrict__ seg_start,
                                                             uint8_t *__restrict__ seg_skip) {
    const u64 total = 2 * nm + n_edges;
    for (u64 u = (u64)blockIdx.x * BLOCK + threadIdx.x; u < total; u += (u64)gridDim.x * BLOCK) {
        if (!flag[u]) continue;
        const u64 s = segrank[u];
        if (u < 2 * nm) {
            seg_edge[s] = slot_edge[u]; seg_skip[s] = slot_skip[u];
            seg_start[s] = (u32)(slot_base[u] - slot_base[2 * chain_off[chain_of[u >> 1]]]);      // (a written chain has n < 2^32)
        } else { seg_edge[s] = (u32)(u - 2 * nm); seg_skip[s] = 0; seg_start[s] = 0; }
    }
}

// ---------------------------------------------------------------------------------------------
// emission: a byte range of the text
// ---------------------------------------------------------------------------------------------
// ">s<c> len=<n> contigs=<m> gaps=<N bases>\n" of a chain, ">e<id> len=<n>\n" of an edge
struct ScafHdr {
    u64 id, n, m, gaps;
    int di, dn, dm, dg;
    u32 len;
    bool chain;
};
__device__ __forceinline__ ScafHdr scaf_hdr(bool chain, u64 id, u64 n, u64 m, u64 gaps) {
    ScafHdr h;
    h.chain = chain; h.id = id; h.n = n; h.m = m; h.gaps = gaps;
    h.di = dec_digits(id); h.dn = dec_digits(n); h.dm = chain ? dec_digits(m) : 0; h.dg = chain ? dec_digits(gaps) : 0;
    h.len = (u32)(2 + h.di + 5 + h.dn + (chain ? 9 + h.dm + 6 + h.dg : 0) + 1);
    return h;
}
__device__ __forceinline__ char scaf_hdr_byte(const ScafHdr &h, u32 p) {
    if (p < 2) return p ? (h.chain ? 's' : 'e') : '>';
    p -= 2;
    if (p < (u32)h.di) return dec_digit_at(h.id, h.di, (int)p);
    p -= (u32)h.di;
    if (p < 5) return " len="[p];
    p -= 5;
    if (p < (u32)h.dn) return dec_digit_at(h.n, h.dn, (int)p);
    p -= (u32)h.dn;
    if (h.chain) {
        if (p < 9) return " contigs="[p];
        p -= 9;
        if (p < (u32)h.dm) return dec_digit_at(h.m, h.dm, (int)p);
        p -= (u32)h.dm;
        if (p < 6) return " gaps="[p];
        p -= 6;
        if (p < (u32)h.dg) return dec_digit_at(h.gaps, h.dg, (int)p);
    }
    return '\n';
}
// Bytes [t0, t1) of the text, t0 < t1 <= rec_off[records]; `out` and the items as k_contig_emit's (gk_fastaout.h: text_stream).
__global__ __launch_bounds__(BLOCK) void k_scaffold_emit(GraphView g, ScafPlan p, u64 t0, u64 t1, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const u64 base = t0 & ~(u64)7;
    const u64 a0 = min(t1, (t0 + 7) & ~(u64)7), a1 = max(a0, t1 & ~(u64)7);                // whole words: [a0, a1)
    const u64 nhead = a0 - t0, nwords = (a1 - a0) >> 3, items = nhead + nwords + (t1 - a1);
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 tile = ((u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * 64; tile < items; tile += waves * 64) {
        // the record of the wave's first byte: the last r with rec_off[r] <= pos (pos < rec_off[records])
        const u64 wpos = tile < nhead ? t0 + tile : tile < nhead + nwords ? a0 + 8 * (tile - nhead) : a1 + (tile - nhead - nwords);
        u64 lo = 0, hi = p.records;
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            if (p.rec_off[mid] <= wpos) lo = mid; else hi = mid;
        }
        const u64 item = tile + (u64)lane;
        if (item >= items) continue;
        const bool word = item >= nhead && item < nhead + nwords;
        const u64 pos = item < nhead ? t0 + item : word ? a0 + 8 * (item - nhead) : a1 + (item - nhead - nwords);
        const int nb = word ? 8 : 1;
        // walk forward from the wave's record
        u64 r = lo;
        while (p.rec_off[r + 1] <= pos) r++;
        u64 bits = 0, begin = 0, end = 0, nlo = 0, nhi = 0, sg = 0, sg1 = 0;
        u32 col = 0, bi = 0, seg_end = 0, adj = 0, edge = NONE;
        const uint8_t *seq = nullptr;
        ScafHdr h{};
        bool fresh = true, body_init = true, find_seg = true;
        for (int b = 0; b < nb; b++) {
            const u64 at = pos + (u64)b;
            if (!fresh && at >= end) { r++; fresh = true; }
            if (fresh) {
                const bool chain = r < p.chain_recs;
                begin = p.rec_off[r]; end = p.rec_off[r + 1];
                h = scaf_hdr(chain, p.rec_id[r], p.rec_n[r], chain ? p.rec_m[r] : 0, chain ? p.rec_gaps[r] : 0);
                sg1 = p.rec_seg[r + 1];
                fresh = false; body_init = true;
            }
            const u32 rel = (u32)(at - begin);                           // (a record is shorter than 2^32 bytes: the plan refuses others)
            char ch;
            if (rel < h.len) ch = scaf_hdr_byte(h, rel);
            else {
                if (body_init) {                                         // one division per item; the bytes after it step
                    const u32 j = rel - h.len;
                    const u32 line = p.line_width ? j / (p.line_width + 1) : 0u;
                    col = j - line * (p.line_width + 1);
                    bi = j - line;
                    body_init = false; find_seg = true;
                }
                if ((p.line_width && col == p.line_width) || (u64)bi == h.n) { ch = '\n'; col = 0; }
                else {
                    if (find_seg || bi >= seg_end) {
                        if (find_seg) {                                  // the last segment of the record that starts at or before base bi
                            u64 l = p.rec_seg[r], u = sg1;
                            while (u - l > 1) {
                                const u64 mid = l + (u - l) / 2;
                                if (p.seg_start[mid] <= bi) l = mid; else u = mid;
                            }
                            sg = l; find_seg = false;
                        } else sg++;
                        seg_end = sg + 1 < sg1 ? p.seg_start[sg + 1] : (u32)h.n;
                        edge = p.seg_edge[sg];
                        if (edge != NONE) {
                            const u32 s = g.e_start[edge];
                            nlo = g.node_lo[s]; nhi = g.k > 32 ? g.node_hi[s] : 0ull;
                            seq = g.pool + g.e_off[edge];
                            adj = (u32)p.seg_skip[sg] - p.seg_start[sg];          // (mod 2^32: bi + adj is the base of the edge's path)
                        }
                    }
                    ch = edge == NONE ? 'N' : "AGCT"[path_base(nlo, nhi, seq, g.k, (u64)(u32)(bi + adj))];
                    bi++; col++;
                }
            }
            bits |= (u64)(uint8_t)ch << (8 * b);
        }
        if (word) *reinterpret_cast<u64 *>(out + (pos - base)) = bits;
        else out[pos - base] = (uint8_t)bits;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct gk_scaffolds {
    gk_ctx *ctx = nullptr;
    gk_graph *g = nullptr;
    u64 epoch = 0;                       // the graph's when the plan was made: any edit since makes the plan stale
    u32 line_width = 0;
    u64 stats[SCAFFOLD_STATS] = {};
    u64 ovl_stats[2] = {};               // overlapped junctions of the chain records, and the bases they dropped
    u64 records = 0, chain_recs = 0, segs = 0, text_bytes = 0;
    // the plan, on the device: what the text is a pure function of
    u32 *d_rec_id = nullptr, *d_rec_n = nullptr, *d_rec_m = nullptr, *d_rec_gaps = nullptr, *d_seg_edge = nullptr, *d_seg_start = nullptr;
    unsigned long long *d_rec_off = nullptr, *d_rec_seg = nullptr;
    uint8_t *d_seg_skip = nullptr;
    TextStream ts;                       // the chunk buffers, made by the first read / write, and the times of the last one
};

namespace {

int scaffolds_live(const gk_scaffolds *s, const char *who) {
    if (!s || !s->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null scaffolds handle");
    const hipError_t e = hipSetDevice(s->ctx->device);
    if (e != hipSuccess) return hip_fail(s->ctx, e, "hipSetDevice");
    if (s->g->epoch != s->epoch) return fail(s->ctx, GK_E_STATE, std::string(who) + ": the graph was edited after the plan was made");
    return GK_OK;
}

// the launch of k_scaffold_emit for bytes [t, t1) of the text (gk_fastaout.h: text_stream)
auto scaffolds_emit(gk_scaffolds *s) {
    return [s](u64 t, u64 t1, u64 items, uint8_t *out) {
        const ScafPlan plan{s->d_rec_id,  s->d_rec_off,   s->d_rec_seg,  s->d_rec_n, s->d_rec_m,    s->d_rec_gaps,
                            s->d_seg_edge, s->d_seg_start, s->d_seg_skip, s->records, s->chain_recs, s->line_width};
        hipLaunchKernelGGL(k_scaffold_emit, dim3(ggrid(s->ctx, items)), dim3(BLOCK), 0, s->ctx->stream, s->g->v, plan, t, t1, out);
    };
}

void scaffolds_drop_plan(gk_scaffolds *s) {      // the plan's buffers are still the scratch owner's: forget them
    s->d_rec_id = s->d_rec_n = s->d_rec_m = s->d_rec_gaps = s->d_seg_edge = s->d_seg_start = nullptr;
    s->d_rec_off = s->d_rec_seg = nullptr;
    s->d_seg_skip = nullptr;
}

}  // namespace

extern "C" void gk_scaffolds_destroy(gk_scaffolds *s);

void scaffolds_rows(const gk_scaffolds *s, ScafRows *out) {
    *out = ScafRows{s->ctx, s->g, s->epoch, s->records, s->chain_recs, s->segs, s->stats[6] + s->stats[4], s->d_rec_seg, s->d_seg_edge, s->d_seg_start, s->d_seg_skip};
}

// gk_graph_scaffolds_plan is the `overlap` == nullptr case
static int scaffolds_plan(const char *who, gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap,
                          const uint32_t *overlap, int64_t min_gap, uint64_t min_len, uint32_t line_width, int strands, int singletons, gk_scaffolds **out) {
    if (!out) return fail(g ? g->ctx : nullptr, GK_E_INVALID, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (strands != 1 && strands != 2) return fail(ctx, GK_E_INVALID, std::string(who) + ": strands is 1 (one record per scaffold) or 2 (both strands)");
    if (line_width > 0x7fffffffu) return fail(ctx, GK_E_INVALID, std::string(who) + ": line_width beyond 2^31-1");
    if (min_gap < 1 || min_gap > 0x7fffffffll) return fail(ctx, GK_E_INVALID, std::string(who) + ": min_gap outside 1 .. 2^31-1");
    const GraphView &v = g->v;
    const u64 ne = v.n_edges;
    std::unique_ptr<gk_scaffolds, void (*)(gk_scaffolds *)> s(new gk_scaffolds, gk_scaffolds_destroy);
    s->ctx = ctx; s->ts.ctx = ctx; s->g = g; s->epoch = g->epoch; s->line_width = line_width;
    if (ne == 0 && nchains == 0) { *out = s.release(); return GK_OK; }
    DevScratch tmp(ctx);
    ChainList cl;
    if (int rc = chains_begin(who, g, tmp, members, chain_off, nchains, gap, SF_N, &cl)) return rc;
    const u64 nm = cl.nm, T = nchains + ne, U = 2 * nm + ne;
    u32 *d_overlap = nullptr, *d_chain_of = nullptr, *d_slot_len = nullptr, *d_slot_edge = nullptr, *d_sel = nullptr, *d_size = nullptr, *d_chain_n = nullptr,
        *d_chain_gaps = nullptr, *d_flag = nullptr, h_flags[SF_N] = {};
    uint8_t *d_mclass = nullptr, *d_slot_skip = nullptr;
    unsigned long long *d_slot_base = nullptr, *d_rank = nullptr, *d_off = nullptr, *d_segrank = nullptr, *d_stats = nullptr, h_stats[SS_N] = {}, h_records = 0,
                       h_chain_recs = 0, h_bytes = 0, h_segs = 0;
    if (nm && overlap) tmp.upload(&d_overlap, overlap, nm);
    tmp.zeroed(&d_stats, SS_N);
    tmp.get(&d_chain_of, nm);
    tmp.get(&d_mclass, nm);
    tmp.get(&d_slot_len, 2 * nm);
    tmp.get(&d_slot_edge, 2 * nm);
    tmp.get(&d_slot_skip, 2 * nm);
    tmp.get(&d_slot_base, 2 * nm + 1);
    tmp.get(&d_sel, T);
    tmp.get(&d_size, T);
    tmp.get(&d_chain_n, nchains);
    tmp.get(&d_chain_gaps, nchains);
    tmp.get(&d_flag, U);
    tmp.get(&d_rank, T + 1);
    tmp.get(&d_off, T + 1);
    tmp.get(&d_segrank, U + 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), (std::string(who) + ": scratch").c_str());
    // the segments behind the check; one read of the flags
    hipLaunchKernelGGL(k_scaf_segments, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, v, cl.d_members, cl.d_chain_off, (u64)nchains, nm, cl.d_gap, d_overlap,
                       (long long)min_gap, cl.d_flags, d_chain_of, d_mclass, d_slot_len, d_slot_edge, d_slot_skip);
    GK_HIP(ctx, read_back(ctx, h_flags, cl.d_flags, SF_N));
    if (int rc = chains_failed(who, ctx, h_flags, false)) return rc;
    if (h_flags[SF_OVERLAP])
        return fail(ctx, GK_E_INVALID, std::string(who) + ": an overlap at an adjacent junction, above GK_OVERLAP_MAX, not below both path lengths, or whose bases differ");
    if (h_flags[SF_OVERFLOW]) return fail(ctx, GK_E_CAPACITY, std::string(who) + ": a record of 2^32 bytes or more");
    // every slot's place in its scaffold, the strand and size of every chain, the edges no chain claimed
    GK_HIP(ctx, scan_counts(ctx, tmp, d_slot_len, 2 * nm, d_slot_base));
    hipLaunchKernelGGL(k_scaf_strand, dim3(ggrid(ctx, (u64)nchains * 64)), dim3(BLOCK), 0, ctx->stream, v, cl.d_chain_off, (u64)nchains, d_slot_base, d_slot_len, d_slot_edge,
                       d_slot_skip, d_mclass, (u32)line_width, strands, d_sel, d_size, d_chain_n, d_chain_gaps, d_stats);
    GK_HIP(ctx, hipGetLastError());
    if (singletons) {
        hipLaunchKernelGGL(k_scaf_single, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, cl.d_owner, (u64)min_len, (u32)line_width, strands, d_sel + nchains,
                           d_size + nchains, d_flag + 2 * nm, d_stats);
        GK_HIP(ctx, hipGetLastError());
    } else {
        GK_HIP(ctx, hipMemsetAsync(d_sel + nchains, 0, ne * sizeof(u32), ctx->stream));
        GK_HIP(ctx, hipMemsetAsync(d_size + nchains, 0, ne * sizeof(u32), ctx->stream));
        GK_HIP(ctx, hipMemsetAsync(d_flag + 2 * nm, 0, ne * sizeof(u32), ctx->stream));
    }
    hipLaunchKernelGGL(k_scaf_flags, dim3(ggrid(ctx, 2 * nm)), dim3(BLOCK), 0, ctx->stream, nm, d_slot_len, d_chain_of, d_sel, d_flag);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_sel, T, d_rank));
    GK_HIP(ctx, scan_counts(ctx, tmp, d_size, T, d_off));
    GK_HIP(ctx, scan_counts(ctx, tmp, d_flag, U, d_segrank));
    GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}, {&h_records, d_rank + T, 8}, {&h_chain_recs, d_rank + nchains, 8}, {&h_bytes, d_off + T, 8},
                                {&h_segs, d_segrank + U, 8}}));
    if (h_stats[SS_OVERFLOW]) return fail(ctx, GK_E_CAPACITY, std::string(who) + ": a record of 2^32 bytes or more");
    // the plan
    tmp.get(&s->d_rec_id, h_records);
    tmp.get(&s->d_rec_n, h_records);
    tmp.get(&s->d_rec_m, h_chain_recs);
    tmp.get(&s->d_rec_gaps, h_chain_recs);
    tmp.get(&s->d_rec_off, h_records + 1);
    tmp.get(&s->d_rec_seg, h_records + 1);
    tmp.get(&s->d_seg_edge, h_segs);
    tmp.get(&s->d_seg_start, h_segs);
    tmp.get(&s->d_seg_skip, h_segs);
    if (tmp.error() != hipSuccess) { scaffolds_drop_plan(s.get()); return hip_fail(ctx, tmp.error(), (std::string(who) + ": the plan").c_str()); }
    hipLaunchKernelGGL(k_scaf_compact_recs, dim3(ggrid(ctx, T + 1)), dim3(BLOCK), 0, ctx->stream, v, (u64)nchains, nm, cl.d_chain_off, d_sel, d_rank, d_off, d_segrank,
                       d_chain_n, d_chain_gaps, s->d_rec_id, s->d_rec_off, s->d_rec_seg, s->d_rec_n, s->d_rec_m, s->d_rec_gaps);
    hipLaunchKernelGGL(k_scaf_compact_segs, dim3(ggrid(ctx, U)), dim3(BLOCK), 0, ctx->stream, ne, nm, cl.d_chain_off, d_chain_of, d_flag, d_segrank, d_slot_base, d_slot_edge,
                       d_slot_skip, s->d_seg_edge, s->d_seg_start, s->d_seg_skip);
    const hipError_t e = read_back(ctx, {});
    if (e != hipSuccess) { scaffolds_drop_plan(s.get()); return hip_fail(ctx, e, (std::string(who) + ": compaction").c_str()); }
    for (void *p : {(void *)s->d_rec_id, (void *)s->d_rec_n, (void *)s->d_rec_m, (void *)s->d_rec_gaps, (void *)s->d_seg_edge, (void *)s->d_seg_start,
                    (void *)s->d_rec_off, (void *)s->d_rec_seg, (void *)s->d_seg_skip})
        tmp.take(p);
    s->records = h_records; s->chain_recs = h_chain_recs; s->segs = h_segs; s->text_bytes = h_bytes;
    u64 *st = s->stats;
    st[0] = nchains; st[1] = h_stats[SS_FORWARD]; st[2] = h_stats[SS_SELF]; st[3] = h_stats[SS_REVERSE];
    st[4] = h_stats[SS_SINGLE]; st[5] = h_records; st[6] = h_stats[SS_MEMBERS];
    st[7] = h_stats[SS_ADJACENT]; st[8] = h_stats[SS_GAPPED]; st[9] = h_stats[SS_CLAMPED];
    st[10] = h_stats[SS_NBASES]; st[11] = h_stats[SS_BASES]; st[12] = h_bytes;
    s->ovl_stats[0] = h_stats[SS_OVERLAPPED]; s->ovl_stats[1] = h_stats[SS_DROPPED];
    *out = s.release();
    return GK_OK;
}

extern "C" {

void gk_scaffolds_destroy(gk_scaffolds *s) {
    if (!s) return;
    if (s->ctx) {
        (void)hipSetDevice(s->ctx->device);
        text_free_buffers(&s->ts);
        for (void *p : {(void *)s->d_rec_id, (void *)s->d_rec_n, (void *)s->d_rec_m, (void *)s->d_rec_gaps, (void *)s->d_seg_edge, (void *)s->d_seg_start,
                        (void *)s->d_rec_off, (void *)s->d_rec_seg, (void *)s->d_seg_skip})
            (void)pool_free(s->ctx, p);
    }
    delete s;
}

int gk_graph_scaffolds_plan(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, int64_t min_gap,
                            uint64_t min_len, uint32_t line_width, int strands, int singletons, gk_scaffolds **out) {
    return scaffolds_plan("gk_graph_scaffolds_plan", g, members, chain_off, nchains, gap, nullptr, min_gap, min_len, line_width, strands, singletons, out);
}

int gk_graph_scaffolds_plan_overlaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, const uint32_t *overlap,
                                     int64_t min_gap, uint64_t min_len, uint32_t line_width, int strands, int singletons, gk_scaffolds **out) {
    return scaffolds_plan("gk_graph_scaffolds_plan_overlaps", g, members, chain_off, nchains, gap, overlap, min_gap, min_len, line_width, strands, singletons, out);
}

int gk_scaffolds_stats(const gk_scaffolds *s, uint64_t *stats13) {
    if (!s || !s->ctx) return fail(nullptr, GK_E_INVALID, "gk_scaffolds_stats: null scaffolds handle");
    if (!stats13) return fail(s->ctx, GK_E_INVALID, "gk_scaffolds_stats: stats13 is NULL");
    for (int i = 0; i < SCAFFOLD_STATS; i++) stats13[i] = s->stats[i];
    return GK_OK;
}

int gk_scaffolds_overlap_stats(const gk_scaffolds *s, uint64_t *stats2) {
    if (!s || !s->ctx) return fail(nullptr, GK_E_INVALID, "gk_scaffolds_overlap_stats: null scaffolds handle");
    if (!stats2) return fail(s->ctx, GK_E_INVALID, "gk_scaffolds_overlap_stats: stats2 is NULL");
    stats2[0] = s->ovl_stats[0]; stats2[1] = s->ovl_stats[1];
    return GK_OK;
}

int gk_scaffolds_last_ms(const gk_scaffolds *s, float *ms4) {
    if (!s || !s->ctx) return fail(nullptr, GK_E_INVALID, "gk_scaffolds_last_ms: null scaffolds handle");
    if (!ms4) return fail(s->ctx, GK_E_INVALID, "gk_scaffolds_last_ms: ms4 is NULL");
    for (int i = 0; i < 4; i++) ms4[i] = s->ts.last_ms[i];
    return GK_OK;
}

int gk_scaffolds_read(gk_scaffolds *s, uint64_t offset, char *buf, uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (int rc = scaffolds_live(s, "gk_scaffolds_read")) return rc;
    gk_ctx *ctx = s->ctx;
    if (offset > s->text_bytes) return fail(ctx, GK_E_INVALID, "gk_scaffolds_read: the offset lies beyond the text");
    const u64 want = std::min<u64>(cap, s->text_bytes - offset);
    if (want && !buf) return fail(ctx, GK_E_INVALID, "gk_scaffolds_read: buf is NULL");
    u64 done = 0;
    bool sink_failed = false;
    if (int rc = text_stream(&s->ts, s->text_bytes, offset, want, "gk_scaffolds", scaffolds_emit(s),
                             [&](const char *p, u64 m) { std::memcpy(buf + done, p, m); done += m; return true; }, &sink_failed))
        return rc;
    if (n) *n = done;
    return GK_OK;
}

int gk_scaffolds_write(gk_scaffolds *s, const char *path) {
    if (int rc = scaffolds_live(s, "gk_scaffolds_write")) return rc;
    if (!path) return fail(s->ctx, GK_E_INVALID, "gk_scaffolds_write: path is NULL");
    return text_write_file(&s->ts, s->text_bytes, path, "gk_scaffolds", "gk_scaffolds_write", scaffolds_emit(s));
}

int gk_scaffolds_segments(const gk_scaffolds *s, uint64_t *record, uint32_t *edge, uint64_t *first, uint64_t *bases, uint32_t *skipped, uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (!s || !s->ctx) return fail(nullptr, GK_E_INVALID, "gk_scaffolds_segments: null scaffolds handle");
    gk_ctx *ctx = s->ctx;
    if (!n) return fail(ctx, GK_E_INVALID, "gk_scaffolds_segments: n is NULL");
    const u64 rows = s->stats[6] + s->stats[4];              // a piece per member written and per singleton
    *n = rows;
    if (cap < rows) return fail(ctx, GK_E_CAPACITY, "gk_scaffolds_segments: room for " + std::to_string(cap) + " rows, " + std::to_string(rows) + " needed");
    if (rows == 0) return GK_OK;
    if (!record || !edge || !first || !bases || !skipped) return fail(ctx, GK_E_INVALID, "gk_scaffolds_segments: an output array is NULL");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> rec_seg(s->records + 1);
    std::vector<u32> rec_n(s->records), seg_edge(s->segs), seg_start(s->segs);
    std::vector<uint8_t> seg_skip(s->segs);
    GK_HIP(ctx, read_back(ctx, {{rec_seg.data(), s->d_rec_seg, rec_seg.size() * 8}, {rec_n.data(), s->d_rec_n, rec_n.size() * 4},
                                {seg_edge.data(), s->d_seg_edge, seg_edge.size() * 4}, {seg_start.data(), s->d_seg_start, seg_start.size() * 4},
                                {seg_skip.data(), s->d_seg_skip, seg_skip.size()}}));
    u64 row = 0;
    for (u64 r = 0; r < s->records; r++)
        for (u64 i = rec_seg[r]; i < rec_seg[r + 1]; i++) {
            if (seg_edge[i] == NONE) continue;
            record[row] = r; edge[row] = seg_edge[i]; first[row] = seg_start[i]; skipped[row] = seg_skip[i];
            bases[row] = (i + 1 < rec_seg[r + 1] ? seg_start[i + 1] : rec_n[r]) - seg_start[i];
            row++;
        }
    return GK_OK;
}

}  // extern "C"
