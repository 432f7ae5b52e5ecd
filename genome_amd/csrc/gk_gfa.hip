// gk_gfa.hip — the twin of every live edge, by content, and the graph as GFA 1.0 text, written on the device.
//
// Reference: none.  Graph.scala keeps both strands of everything as unrelated edges and GraphSimplifier.scala prints them so; the
// rules here are this project's own and stated in include/genome_amd.h ("edge twins", "the graph as GFA"); tests/gfa_ref.py
// restates them over strings.
//
// Twins, three steps.  k_twin_keys: one wave per live edge folds the path key (gk_links.h: pk_word_terms / pk_finish) of P(e), and
// of R(e) by walking the path's words backwards with reversed, complemented codes — the key R(e) has as the P of another edge.
// The (key of P, id) pairs are sorted by rocPRIM's radix sort, minor word first.  k_twin_match: one wave per live edge finds the
// run of key(P(e)) and the run of key(R(e)) by binary search and CONFIRMS every candidate by comparing the paths 64 bases per step
// (k_contig_classify's loop); a candidate with the key but another content is skipped and counted.  The answer never rests on the
// hash.  No LDS; the only cross-lane traffic is ballots and shuffles.
//
// GFA.  k_gfa_size: one lane per edge decides its segment, the bytes of its S line and of its 0..4 L lines.  Two scans (gk_scan.h)
// give the line offsets by edge id — there is no compaction: an edge without a line has size 0 and the search skips it.  k_gfa_emit
// is k_contig_emit's shape: it is handed a byte range of the text and every lane produces one aligned 8-byte word of it, so chunked
// writes and reads at any offset are the same launch.  An S line spells the segment's own path: nothing is reverse-complemented.
//
// Roofline: the key pass reads the pool's live bytes once (both keys come from the same words); the match reads every path twice
// more (against its own twin and as its twin's candidate); the emit is a streaming write of the text, 2 bits read per 8 written.
#include <rocprim/device/device_radix_sort.hpp>

#include <memory>

#include "gk_fastaout.h"
#include "gk_links.h"
#include "gk_scan.h"

// the classes of gk_graph_edge_twins (0: a dead or out-of-range id); on the device bit 4 of a paired edge's byte says P(e) > R(e)
static constexpr uint8_t TW_DEAD = 0, TW_PAIRED = 1, TW_SELF = 2, TW_MISSING = 3, TW_AMBIGUOUS = 4, TW_REVERSE = 16;
enum { TS_LIVE = 0, TS_PAIRED, TS_SELF, TS_MISSING, TS_AMBIGUOUS, TS_COLLISIONS, TS_N };
// device counters of a GFA plan
enum { GS_LIVE = 0, GS_SEGMENTS, GS_PAIRS, GS_LINKS, GS_BASES, GS_MISSING, GS_OVERFLOW, GS_N };
static constexpr u64 GFA_HEADER_BYTES = 11;                  // "H\tVN:Z:1.0\n"

// ---------------------------------------------------------------------------------------------
// twins: keys
// ---------------------------------------------------------------------------------------------
// bases [a, a + cnt) of a sequence of `len` bases that starts at byte p, base a + t in bits 2t, 2t + 1 (1 <= cnt <= 32, a + cnt <= len);
// only the bytes the sequence owns are read, and bits past the cnt bases are 0
__device__ __forceinline__ u64 seq_bits(const uint8_t *__restrict__ p, u64 len, u64 a, u32 cnt) {
    const u64 b0 = a >> 2, nbytes = (len + 3) >> 2;
    const u32 sh = (u32)(a & 3) * 2;
    u64 w = 0;
    if (b0 + 8 <= nbytes) __builtin_memcpy(&w, p + b0, 8);
    else for (u64 b = b0; b < nbytes; b++) w |= (u64)p[b] << (8 * (b - b0));
    if (sh) {
        w >>= sh;
        if (b0 + 8 < nbytes) w |= (u64)p[b0 + 8] << (64 - sh);
    }
    return w & low_mask((int)(2 * cnt));
}
// bases [a, a + cnt) of the path start k-mer ++ seq, in seq_bits' form: from the k-mer's words, the sequence, or both
__device__ __forceinline__ u64 path_bits(u64 nlo, u64 nhi, const uint8_t *__restrict__ seq, u64 len, int k, u64 a, u32 cnt) {
    if (a >= (u64)k) return seq_bits(seq, len, a - (u64)k, cnt);
    const u32 c1 = (u32)min((u64)cnt, (u64)k - a), sh = (u32)(2 * a);
    u64 w = sh >= 64 ? nhi >> (sh - 64) : sh ? (nlo >> sh) | (nhi << (64 - sh)) : nlo;
    w &= low_mask((int)(2 * c1));
    if (cnt > c1) w |= seq_bits(seq, len, 0, cnt - c1) << (2 * c1);
    return w;
}
// the reverse complement of cnt bases held as seq_bits leaves them
__device__ __forceinline__ u64 rc_bits(u64 w, u32 cnt) {
    u64 r = __brevll(w);                                                     // bit order, then the two bits of every code back
    r = ((r & 0xaaaaaaaaaaaaaaaaull) >> 1) | ((r & 0x5555555555555555ull) << 1);
    return (r >> (64 - 2 * cnt)) ^ low_mask((int)(2 * cnt));
}
// the 128-bit key cut to its low `bits` bits ("twin_key_bits"; the product passes 128).  A live edge's first word never becomes ~0.
__device__ __forceinline__ void key_cut(int bits, u64 *h1, u64 *h2) {
    *h1 &= low_mask(bits);
    *h2 &= bits > 64 ? low_mask(bits - 64) : 0ull;
}
// p1 / p2 [e] = the key of P(e), r1 / r2 [e] = the key of R(e) (~0, ~0 for a dead edge: they sort last), ids[e] = e
template <int W>
__global__ __launch_bounds__(BLOCK) void k_twin_keys(GraphView g, int bits, u64 *__restrict__ p1, u64 *__restrict__ p2, u64 *__restrict__ r1, u64 *__restrict__ r2,
                                                     u32 *__restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 e = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e < g.n_edges; e += waves) {      // (uniform over the wave)
        if (!g.e_alive[e]) {
            if (lane == 0) { ids[e] = (u32)e; p1[e] = p2[e] = r1[e] = r2[e] = ~0ull; }
            continue;
        }
        const u64 len = g.e_len[e], n = (u64)g.k + len, nw = (len + 31) / 32;
        const uint8_t *seq = g.pool + g.e_off[e];
        const u32 s = g.e_start[e];
        const u64 nlo = g.node_lo[s], nhi = W == 2 ? g.node_hi[s] : 0ull;
        u64 a1 = 0, a2 = 0, b1 = 0, b2 = 0;
        for (u64 j0 = 0; j0 < nw; j0 += 64) {
            const u64 j = j0 + (u64)lane;
            if (j < nw) {
                const u32 cnt = (u32)min((u64)32, len - 32 * j);
                u64 t1, t2;
                pk_word_terms(seq_bits(seq, len, 32 * j, cnt), j, &t1, &t2);                                     // word j of P's sequence
                a1 += t1; a2 += t2;
                // word j of R's sequence R[k + 32j ..]: the reverse complement of P[len - 32j - cnt .. len - 32j), which may reach into the start k-mer
                pk_word_terms(rc_bits(path_bits(nlo, nhi, seq, len, g.k, len - 32 * j - cnt, cnt), cnt), j, &t1, &t2);
                b1 += t1; b2 += t2;
            }
        }
        // R's start k-mer: the reverse complement of P's last k bases, one base per lane (k <= 64)
        u64 rlo = 0, rhi = 0;
        if (lane < g.k) {
            const u64 c = (u64)(3 - path_base(nlo, nhi, seq, g.k, n - 1 - (u64)lane));
            if (lane < 32) rlo = c << (2 * lane); else rhi = c << (2 * (lane - 32));
        }
        for (int d = 32; d; d >>= 1) {
            a1 += __shfl_down(a1, d); a2 += __shfl_down(a2, d); b1 += __shfl_down(b1, d); b2 += __shfl_down(b2, d);
            rlo |= __shfl_down(rlo, d); rhi |= __shfl_down(rhi, d);
        }
        if (lane == 0) {
            u64 h1, h2;
            pk_finish(a1, a2, nlo, nhi, len, &h1, &h2);
            key_cut(bits, &h1, &h2);
            p1[e] = h1; p2[e] = h2;
            pk_finish(b1, b2, rlo, rhi, len, &h1, &h2);
            key_cut(bits, &h1, &h2);
            r1[e] = h1; r2[e] = h2;
            ids[e] = (u32)e;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_twin_gather(const u64 *__restrict__ h, const u32 *__restrict__ ids, u64 n, u64 *out) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) out[i] = h[ids[i]];
}

// ---------------------------------------------------------------------------------------------
// twins: runs and confirmation, one wave per live edge
// ---------------------------------------------------------------------------------------------
struct TwinOrder { const u64 *sk1; const u32 *sid; const u64 *p2; u64 n; };      // the edges by (key of P, id): sk1[i] = p1[sid[i]]
// the first i with (sk1[i], p2[sid[i]]) >= (a, b)
__device__ __forceinline__ u64 twin_lower(const TwinOrder &o, u64 a, u64 b) {
    u64 lo = 0, hi = o.n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2, x = o.sk1[mid];
        if (x < a || (x == a && o.p2[o.sid[mid]] < b)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// P(f) against P(e) (rc == false) or against R(e), across the wave, 64 bases per step: 0 equal, else 1 if the first difference has
// P(f)'s base below the other's, 2 if above; paths of different lengths: 3.  Every lane of the wave calls it with the same e, f.
template <int W> __device__ __forceinline__ int twin_compare(const GraphView &g, u32 e, u32 f, bool rc, int lane) {
    const u64 n = (u64)g.k + g.e_len[e];
    if ((u64)g.k + g.e_len[f] != n) return 3;
    const u32 se = g.e_start[e], sf = g.e_start[f];
    const u64 elo = g.node_lo[se], ehi = W == 2 ? g.node_hi[se] : 0ull, flo = g.node_lo[sf], fhi = W == 2 ? g.node_hi[sf] : 0ull;
    const uint8_t *eseq = g.pool + g.e_off[e], *fseq = g.pool + g.e_off[f];
    for (u64 i0 = 0; i0 < n; i0 += 64) {
        const u64 i = i0 + (u64)lane;
        int a = 0, b = 0;
        if (i < n) {
            a = path_base(flo, fhi, fseq, g.k, i);
            b = rc ? 3 - path_base(elo, ehi, eseq, g.k, n - 1 - i) : path_base(elo, ehi, eseq, g.k, i);
        }
        const unsigned long long differ = __ballot(a != b);
        if (differ) return __shfl(a < b ? 1 : 2, __ffsll((long long)differ) - 1);
    }
    return 0;
}
// twin[e], cls[e] for every edge (a dead one: NONE, TW_DEAD); stats[TS_*] += this launch's counts
template <int W>
__global__ __launch_bounds__(BLOCK) void k_twin_match(GraphView g, TwinOrder o, const u64 *__restrict__ p1, const u64 *__restrict__ r1, const u64 *__restrict__ r2,
                                                      u32 *__restrict__ twin, uint8_t *__restrict__ cls, unsigned long long *stats) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    unsigned long long cnt[TS_N] = {};
    for (u64 e64 = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e64 < g.n_edges; e64 += waves) {      // (uniform over the wave)
        const u32 e = (u32)e64;
        if (!g.e_alive[e]) {
            if (lane == 0) { twin[e] = NONE; cls[e] = TW_DEAD; }
            continue;
        }
        // C(e): the confirmed members of key(P(e))'s run, e among them; C'(e): those of key(R(e))'s run.  Both capped at 2.
        u32 nc = 0, nr = 0, first = NONE;
        for (int side = 0; side < 2; side++) {
            const u64 a = side ? r1[e] : p1[e], b = side ? r2[e] : o.p2[e];
            for (u64 i = twin_lower(o, a, b); i < o.n && (side ? nr : nc) < 2; i++) {
                const u32 f = o.sid[i];
                if (o.sk1[i] != a || o.p2[f] != b) break;
                bool same = side == 0 && f == e;
                if (!same) {
                    same = twin_compare<W>(g, e, f, side != 0, lane) == 0;
                    if (!same) cnt[TS_COLLISIONS]++;
                }
                if (!same) continue;
                if (side) { if (nr == 0) first = f; nr++; } else nc++;
            }
        }
        uint8_t c;
        if (nr == 0) c = TW_MISSING;
        else if (nc > 1 || nr > 1) c = TW_AMBIGUOUS;
        else if (first == e) c = TW_SELF;
        else {
            c = TW_PAIRED;
            if (twin_compare<W>(g, first, e, false, lane) == 2) c |= TW_REVERSE;      // P(e) > P(twin) = R(e)
        }
        cnt[TS_LIVE]++;
        cnt[TS_PAIRED + (c & 15) - TW_PAIRED]++;
        if (lane == 0) { twin[e] = (c & 15) == TW_PAIRED || c == TW_SELF ? first : NONE; cls[e] = c; }
    }
    if (lane == 0)
        for (int i = 0; i < TS_N; i++) if (cnt[i]) atomicAdd(&stats[i], cnt[i]);
}
// the answers in the order asked; a dead or out-of-range id: NONE, TW_DEAD
__global__ __launch_bounds__(BLOCK) void k_twin_answer(u64 n_edges, const u32 *__restrict__ twin, const uint8_t *__restrict__ cls, const u32 *__restrict__ ids, u64 n,
                                                       u32 *__restrict__ out_twin, uint8_t *__restrict__ out_cls) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 e = ids[i];
        const bool ok = e < n_edges;
        out_twin[i] = ok ? twin[e] : NONE;
        out_cls[i] = ok ? cls[e] & 15 : TW_DEAD;
    }
}

// ---------------------------------------------------------------------------------------------
// GFA: segments, links, sizes
// ---------------------------------------------------------------------------------------------
struct GfaPlan {
    const u32 *twin;
    const uint8_t *cls;
    const unsigned long long *soff, *loff;      // [n_edges + 1]: the S line of edge e, the L lines of edge e
    const u64 *kc;                              // the KC:i: sums by edge id; nullptr without a count table
};
__device__ __forceinline__ bool tw_closed(uint8_t c) { return (c & 15) == TW_PAIRED || (c & 15) == TW_SELF; }
// seg(e) and its orientation
__device__ __forceinline__ u32 gfa_seg(const u32 *__restrict__ twin, const uint8_t *__restrict__ cls, u32 e, char *o) {
    if (cls[e] == (TW_PAIRED | TW_REVERSE)) { *o = '-'; return twin[e]; }
    *o = '+';
    return e;
}
// the pairs (e, f) that are written, f by its first base 0..3; *pairs = all of e's pairs.  (e, f) is skipped iff its mirror
// (twin f, twin e) exists, is another pair and is the smaller id pair.
__device__ __forceinline__ int gfa_links(const GraphView &g, const u32 *__restrict__ twin, const uint8_t *__restrict__ cls, u32 e, u32 out[4], int *pairs) {
    const u64 v = g.e_end[e];
    const u32 te = tw_closed(cls[e]) ? twin[e] : NONE;
    int n = 0, np = 0;
    for (int b = 0; b < 4; b++) {
        const u32 f = g.out_edge[v * 4 + b];
        if (f == NONE || !g.e_alive[f]) continue;
        np++;
        if (te != NONE && tw_closed(cls[f])) {
            const u32 tf = twin[f];
            if (g.e_end[tf] == g.e_start[te] && (tf != e || te != f) && (tf < e || (tf == e && te < f))) continue;
        }
        out[n++] = f;
    }
    *pairs = np;
    return n;
}
__device__ __forceinline__ u32 gfa_link_bytes(const u32 *__restrict__ twin, const uint8_t *__restrict__ cls, u32 e, u32 f, int dk) {
    char o;
    return (u32)(12 + dec_digits(gfa_seg(twin, cls, e, &o)) + dec_digits(gfa_seg(twin, cls, f, &o)) + dk);
}
// isseg[e], ssize[e] = the bytes of e's S line without a KC field (0: e is no segment), lsize[e] = the bytes of e's L lines
__global__ __launch_bounds__(BLOCK) void k_gfa_size(GraphView g, const u32 *__restrict__ twin, const uint8_t *__restrict__ cls, uint8_t *__restrict__ isseg,
                                                    u32 *__restrict__ ssize, u32 *__restrict__ lsize, unsigned long long *stats) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    const int dk = dec_digits((u64)g.k);
    for (u64 e0 = (u64)blockIdx.x * BLOCK; e0 < g.n_edges; e0 += stride) {      // (uniform over the wave: every lane takes the shuffles)
        const u64 e = e0 + threadIdx.x;
        unsigned long long c[GS_N] = {};
        if (e < g.n_edges) {
            u32 sb = 0, lb = 0;
            bool seg = false;
            if (g.e_alive[e]) {
                char o;
                c[GS_LIVE] = 1;
                seg = gfa_seg(twin, cls, (u32)e, &o) == (u32)e;
                if (seg) {
                    const u64 n = (u64)g.k + g.e_len[e], bytes = 3 + (u64)dec_digits(e) + 1 + n + 6 + (u64)dec_digits(n) + 1;
                    if (bytes > 0xffffffe0ull) { c[GS_OVERFLOW] = 1; seg = false; }      // (room for the KC field below 2^32)
                    else { sb = (u32)bytes; c[GS_SEGMENTS] = 1; c[GS_BASES] = n; }
                }
                u32 f[4];
                int np;
                const int nl = gfa_links(g, twin, cls, (u32)e, f, &np);
                for (int i = 0; i < nl; i++) lb += gfa_link_bytes(twin, cls, (u32)e, f[i], dk);
                c[GS_PAIRS] = (unsigned long long)np; c[GS_LINKS] = (unsigned long long)nl;
            }
            isseg[e] = seg; ssize[e] = sb; lsize[e] = lb;
        }
        for (int i = 0; i < GS_N; i++) {
            if (i == GS_MISSING) continue;
            unsigned long long v = c[i];
            for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[i], v);
        }
    }
}
// with a count table: the KC field's bytes of every segment, and the windows the table does not hold
__global__ __launch_bounds__(BLOCK) void k_gfa_kc(GraphView g, EdgeCov cov, const uint8_t *__restrict__ isseg, u32 *__restrict__ ssize, unsigned long long *stats) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 e0 = (u64)blockIdx.x * BLOCK; e0 < g.n_edges; e0 += stride) {      // (uniform over the wave: every lane takes the shuffles)
        const u64 e = e0 + threadIdx.x;
        unsigned long long miss = 0;
        if (e < g.n_edges && isseg[e]) {
            ssize[e] += (u32)(6 + dec_digits(cov.sum[e]));
            miss = cov.miss[e];
        }
        for (int d = 32; d; d >>= 1) miss += __shfl_down(miss, d);
        if ((threadIdx.x & 63) == 0 && miss) atomicAdd(&stats[GS_MISSING], miss);
    }
}

// ---------------------------------------------------------------------------------------------
// GFA: emission of a byte range of the text
// ---------------------------------------------------------------------------------------------
// the last e in [0, n) with off[e] <= x (x < off[n]): the edge whose line holds byte x of its region; edges without a line are passed over
__device__ __forceinline__ u32 gfa_find(const unsigned long long *__restrict__ off, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return (u32)lo;
}
// one line of the text: the header, the S line of edge a, or the L line (a, oa) -> (b, ob)
struct GfaLine {
    u64 begin, end;                      // its bytes in the text
    int kind;                            // 0 header, 1 S, 2 L
    u32 a, b;
    char oa, ob;
    int da, db;
    u64 n, kc, nlo, nhi;
    int dn, dkc;
    const uint8_t *seq;
};
__device__ __forceinline__ void gfa_line_at(const GraphView &g, const GfaPlan &p, u64 s_bytes, u64 at, GfaLine *L) {
    if (at < GFA_HEADER_BYTES) { L->kind = 0; L->begin = 0; L->end = GFA_HEADER_BYTES; return; }
    if (at < GFA_HEADER_BYTES + s_bytes) {
        const u32 e = gfa_find(p.soff, g.n_edges, at - GFA_HEADER_BYTES), s = g.e_start[e];
        L->kind = 1; L->begin = GFA_HEADER_BYTES + p.soff[e]; L->end = GFA_HEADER_BYTES + p.soff[e + 1];
        L->a = e; L->da = dec_digits(e);
        L->n = (u64)g.k + g.e_len[e]; L->dn = dec_digits(L->n);
        L->kc = p.kc ? p.kc[e] : 0; L->dkc = p.kc ? dec_digits(L->kc) : 0;
        L->nlo = g.node_lo[s]; L->nhi = g.k > 32 ? g.node_hi[s] : 0ull;
        L->seq = g.pool + g.e_off[e];
        return;
    }
    const u64 l0 = GFA_HEADER_BYTES + s_bytes, x = at - l0;
    const u32 e = gfa_find(p.loff, g.n_edges, x);
    const int dk = dec_digits((u64)g.k);
    u32 f[4];
    int np;
    const int nl = gfa_links(g, p.twin, p.cls, e, f, &np);
    u64 lb = p.loff[e];
    int i = 0;
    for (; i + 1 < nl; i++) {                                // (x lies in one of e's lines: the scan summed exactly these)
        const u64 bytes = gfa_link_bytes(p.twin, p.cls, e, f[i], dk);
        if (x < lb + bytes) break;
        lb += bytes;
    }
    L->kind = 2; L->begin = l0 + lb; L->end = L->begin + gfa_link_bytes(p.twin, p.cls, e, f[i], dk);
    L->a = gfa_seg(p.twin, p.cls, e, &L->oa); L->b = gfa_seg(p.twin, p.cls, f[i], &L->ob);
    L->da = dec_digits(L->a); L->db = dec_digits(L->b);
    L->n = (u64)g.k; L->dn = dk;
}
__device__ __forceinline__ char gfa_line_byte(const GraphView &g, const GfaLine &L, u64 rel, bool has_kc) {
    if (L.kind == 0) return "H\tVN:Z:1.0\n"[rel];
    if (L.kind == 1) {
        if (rel < 3) return "S\te"[rel];
        rel -= 3;
        if (rel < (u64)L.da) return dec_digit_at(L.a, L.da, (int)rel);
        rel -= (u64)L.da;
        if (rel == 0) return '\t';
        rel -= 1;
        if (rel < L.n) return "AGCT"[path_base(L.nlo, L.nhi, L.seq, g.k, rel)];
        rel -= L.n;
        if (rel < 6) return "\tLN:i:"[rel];
        rel -= 6;
        if (rel < (u64)L.dn) return dec_digit_at(L.n, L.dn, (int)rel);
        rel -= (u64)L.dn;
        if (has_kc) {
            if (rel < 6) return "\tKC:i:"[rel];
            rel -= 6;
            if (rel < (u64)L.dkc) return dec_digit_at(L.kc, L.dkc, (int)rel);
        }
        return '\n';
    }
    if (rel < 3) return "L\te"[rel];
    rel -= 3;
    if (rel < (u64)L.da) return dec_digit_at(L.a, L.da, (int)rel);
    rel -= (u64)L.da;
    if (rel < 4) return rel == 1 ? L.oa : "\t \te"[rel];
    rel -= 4;
    if (rel < (u64)L.db) return dec_digit_at(L.b, L.db, (int)rel);
    rel -= (u64)L.db;
    if (rel < 3) return rel == 1 ? L.ob : '\t';
    rel -= 3;
    if (rel < (u64)L.dn) return dec_digit_at(L.n, L.dn, (int)rel);
    return rel == (u64)L.dn ? 'M' : '\n';
}
// Bytes [t0, t1) of the text, t0 < t1 <= the text's size; `out` and the items as k_contig_emit has them (gk_fastaout.h:
// text_stream).  A lane finds the line of its first byte by binary search in the offsets and the line after it the same way.
__global__ __launch_bounds__(BLOCK) void k_gfa_emit(GraphView g, GfaPlan p, u64 s_bytes, u64 t0, u64 t1, uint8_t *__restrict__ out) {
    const u64 base = t0 & ~(u64)7;
    const u64 a0 = min(t1, (t0 + 7) & ~(u64)7), a1 = max(a0, t1 & ~(u64)7);                // whole words: [a0, a1)
    const u64 nhead = a0 - t0, nwords = (a1 - a0) >> 3, items = nhead + nwords + (t1 - a1);
    const bool has_kc = p.kc != nullptr;
    for (u64 item = (u64)blockIdx.x * BLOCK + threadIdx.x; item < items; item += (u64)gridDim.x * BLOCK) {
        const bool word = item >= nhead && item < nhead + nwords;
        const u64 pos = item < nhead ? t0 + item : word ? a0 + 8 * (item - nhead) : a1 + (item - nhead - nwords);
        const int nb = word ? 8 : 1;
        GfaLine L;
        L.begin = 1; L.end = 0;                              // (no line yet)
        u64 bits = 0;
        for (int b = 0; b < nb; b++) {
            const u64 at = pos + (u64)b;
            if (at >= L.end) gfa_line_at(g, p, s_bytes, at, &L);
            bits |= (u64)(uint8_t)gfa_line_byte(g, L, at - L.begin, has_kc) << (8 * b);
        }
        if (word) *reinterpret_cast<u64 *>(out + (pos - base)) = bits;
        else out[pos - base] = (uint8_t)bits;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct gk_gfa {
    gk_ctx *ctx = nullptr;
    gk_graph *g = nullptr;
    u64 epoch = 0;                       // the graph's when the plan was made: any edit since makes the plan stale
    u64 stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 s_bytes = 0, text_bytes = GFA_HEADER_BYTES;
    // the plan, on the device: what the text is a pure function of, by edge id
    u32 *d_twin = nullptr;
    uint8_t *d_cls = nullptr;
    unsigned long long *d_soff = nullptr, *d_loff = nullptr;
    u64 *d_kc = nullptr;
    TextStream ts;                       // the chunk buffers, made by the first read / write, and the times of the last one
};

namespace {

// twin / cls by edge id and the six counters, all in `tmp`, stream-ordered: nothing is waited for (n_edges >= 1)
int twins_pass(gk_graph *g, DevScratch &tmp, const char *who, u32 **d_twin, uint8_t **d_cls, unsigned long long **d_stats) {
    gk_ctx *ctx = g->ctx;
    const GraphView &v = g->v;
    const u64 ne = v.n_edges;
    const std::string w(who);
    if (ne >= (u64)NONE) return fail(ctx, GK_E_CAPACITY, w + ": more than 2^32 - 1 edge ids");
    u64 *p1 = nullptr, *p2 = nullptr, *r1 = nullptr, *r2 = nullptr, *d_k = nullptr, *d_k2 = nullptr;
    u32 *d_id = nullptr, *d_id2 = nullptr, *d_id3 = nullptr;
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
    tmp.get(&p1, ne); tmp.get(&p2, ne); tmp.get(&r1, ne); tmp.get(&r2, ne);
    tmp.get(&d_k, ne); tmp.get(&d_k2, ne);
    tmp.get(&d_id, ne); tmp.get(&d_id2, ne); tmp.get(&d_id3, ne);
    tmp.get(d_twin, ne);
    tmp.get(d_cls, ne);
    tmp.zeroed(d_stats, TS_N);
    tmp.note(rocprim::radix_sort_pairs(nullptr, temp_bytes, d_k, d_k2, d_id, d_id2, (size_t)ne, 0, 64, ctx->stream));      // (the size query)
    tmp.get((uint8_t **)&d_temp, temp_bytes);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), (w + ": twin scratch").c_str());
    const int bits = ctx->hook_twin_key_bits;
    GK_BY_W(g->W, hipLaunchKernelGGL(k_twin_keys<W>, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, bits, p1, p2, r1, r2, d_id));
    GK_HIP(ctx, hipGetLastError());
    // by (p1, p2, id): the radix sort is stable, so the minor word goes first and the ids start ascending
    GK_HIP(ctx, hipMemcpyAsync(d_k, p2, ne * 8, hipMemcpyDeviceToDevice, ctx->stream));
    GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, temp_bytes, d_k, d_k2, d_id, d_id2, (size_t)ne, 0, 64, ctx->stream));
    hipLaunchKernelGGL(k_twin_gather, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, p1, d_id2, ne, d_k);
    GK_HIP(ctx, rocprim::radix_sort_pairs(d_temp, temp_bytes, d_k, d_k2, d_id2, d_id3, (size_t)ne, 0, 64, ctx->stream));
    const TwinOrder order{d_k2, d_id3, p2, ne};
    GK_BY_W(g->W, hipLaunchKernelGGL(k_twin_match<W>, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, order, p1, r1, r2, *d_twin, *d_cls, *d_stats));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}

int gfa_live(const gk_gfa *c, const char *who) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null gfa handle");
    const hipError_t e = hipSetDevice(c->ctx->device);
    if (e != hipSuccess) return hip_fail(c->ctx, e, "hipSetDevice");
    if (c->g->epoch != c->epoch) return fail(c->ctx, GK_E_STATE, std::string(who) + ": the graph was edited after the plan was made");
    return GK_OK;
}

// the launch of k_gfa_emit for bytes [t, t1) of the text (gk_fastaout.h: text_stream)
auto gfa_emit(gk_gfa *c) {
    return [c](u64 t, u64 t1, u64 items, uint8_t *out) {
        const GfaPlan plan{c->d_twin, c->d_cls, c->d_soff, c->d_loff, c->d_kc};
        hipLaunchKernelGGL(k_gfa_emit, dim3(ggrid(c->ctx, items)), dim3(BLOCK), 0, c->ctx->stream, c->g->v, plan, c->s_bytes, t, t1, out);
    };
}

}  // namespace

extern "C" {

int gk_graph_edge_twins(gk_graph *g, const uint32_t *edge_ids, uint64_t n, uint32_t *twin, uint8_t *cls, uint64_t *stats6) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (stats6) for (int i = 0; i < TS_N; i++) stats6[i] = 0;
    if (n && !edge_ids) return fail(ctx, GK_E_INVALID, "gk_graph_edge_twins: edge_ids is NULL");
    const u64 ne = g->v.n_edges;
    DevScratch tmp(ctx);
    u32 *d_twin = nullptr, *d_ids = nullptr, *d_out_twin = nullptr;
    uint8_t *d_cls = nullptr, *d_out_cls = nullptr;
    unsigned long long *d_stats = nullptr, h_stats[TS_N] = {};
    if (ne) { if (int rc = twins_pass(g, tmp, "gk_graph_edge_twins", &d_twin, &d_cls, &d_stats)) return rc; }
    if (n) {
        tmp.upload(&d_ids, edge_ids, n);
        tmp.get(&d_out_twin, n);
        tmp.get(&d_out_cls, n);
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_edge_twins: the answers");
        hipLaunchKernelGGL(k_twin_answer, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, ne, d_twin, d_cls, d_ids, (u64)n, d_out_twin, d_out_cls);
    }
    const hipError_t e = read_back(ctx, {{n ? twin : nullptr, d_out_twin, (size_t)n * 4}, {n ? cls : nullptr, d_out_cls, (size_t)n}, {ne ? h_stats : nullptr, d_stats, sizeof(h_stats)}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_graph_edge_twins");
    if (stats6) for (int i = 0; i < TS_N; i++) stats6[i] = h_stats[i];
    return GK_OK;
}

void gk_gfa_destroy(gk_gfa *c) {
    if (!c) return;
    if (c->ctx) {
        (void)hipSetDevice(c->ctx->device);
        text_free_buffers(&c->ts);
        (void)pool_free(c->ctx, c->d_twin);
        (void)pool_free(c->ctx, c->d_cls);
        (void)pool_free(c->ctx, c->d_soff);
        (void)pool_free(c->ctx, c->d_loff);
        (void)pool_free(c->ctx, c->d_kc);
    }
    delete c;
}

int gk_graph_gfa_plan(gk_graph *g, gk_map *counts, gk_gfa **out) {
    if (!out) return fail(g ? g->ctx : nullptr, GK_E_INVALID, "gk_graph_gfa_plan: out is NULL");
    *out = nullptr;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (counts) { if (int rc = check_counts(g, counts, "gk_graph_gfa_plan")) return rc; }
    const GraphView &v = g->v;
    std::unique_ptr<gk_gfa, void (*)(gk_gfa *)> c(new gk_gfa, gk_gfa_destroy);
    c->ctx = ctx; c->ts.ctx = ctx; c->g = g; c->epoch = g->epoch;
    c->stats[7] = GFA_HEADER_BYTES;
    if (v.n_edges == 0) { *out = c.release(); return GK_OK; }
    const u64 ne = v.n_edges;
    DevScratch tmp(ctx);
    u32 *d_twin = nullptr, *d_ssize = nullptr, *d_lsize = nullptr;
    uint8_t *d_cls = nullptr, *d_isseg = nullptr;
    unsigned long long *d_tstats = nullptr, *d_stats = nullptr, *d_soff = nullptr, *d_loff = nullptr, h_stats[GS_N] = {}, h_s = 0, h_l = 0;
    if (int rc = twins_pass(g, tmp, "gk_graph_gfa_plan", &d_twin, &d_cls, &d_tstats)) return rc;
    tmp.get(&d_isseg, ne);
    tmp.get(&d_ssize, ne);
    tmp.get(&d_lsize, ne);
    tmp.get(&d_soff, ne + 1);
    tmp.get(&d_loff, ne + 1);
    tmp.zeroed(&d_stats, GS_N);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_gfa_plan: per-edge scratch");
    hipLaunchKernelGGL(k_gfa_size, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, v, d_twin, d_cls, d_isseg, d_ssize, d_lsize, d_stats);
    GK_HIP(ctx, hipGetLastError());
    EdgeCov cov{};
    if (counts) {
        if (int rc = coverage_pass(g, counts, tmp, d_isseg, &cov)) return rc;
        hipLaunchKernelGGL(k_gfa_kc, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, v, cov, d_isseg, d_ssize, d_stats);
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, scan_counts(ctx, tmp, d_ssize, ne, d_soff));
    GK_HIP(ctx, scan_counts(ctx, tmp, d_lsize, ne, d_loff));
    GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}, {&h_s, d_soff + ne, 8}, {&h_l, d_loff + ne, 8}}));
    if (h_stats[GS_OVERFLOW]) return fail(ctx, GK_E_CAPACITY, "gk_graph_gfa_plan: a line of 2^32 bytes or more");
    c->d_twin = tmp.take(d_twin);
    c->d_cls = tmp.take(d_cls);
    c->d_soff = tmp.take(d_soff);
    c->d_loff = tmp.take(d_loff);
    if (counts) c->d_kc = tmp.take(cov.sum);
    c->s_bytes = h_s; c->text_bytes = GFA_HEADER_BYTES + h_s + h_l;
    u64 *s = c->stats;
    s[0] = h_stats[GS_LIVE]; s[1] = h_stats[GS_SEGMENTS]; s[2] = s[0] - s[1];
    s[3] = h_stats[GS_PAIRS]; s[4] = h_stats[GS_LINKS]; s[5] = s[3] - s[4];
    s[6] = h_stats[GS_BASES]; s[7] = c->text_bytes; s[8] = h_stats[GS_MISSING];
    *out = c.release();
    return GK_OK;
}

int gk_gfa_stats(const gk_gfa *c, uint64_t *stats9) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, "gk_gfa_stats: null gfa handle");
    if (!stats9) return fail(c->ctx, GK_E_INVALID, "gk_gfa_stats: stats9 is NULL");
    for (int i = 0; i < 9; i++) stats9[i] = c->stats[i];
    return GK_OK;
}

int gk_gfa_last_ms(const gk_gfa *c, float *ms4) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, "gk_gfa_last_ms: null gfa handle");
    if (!ms4) return fail(c->ctx, GK_E_INVALID, "gk_gfa_last_ms: ms4 is NULL");
    for (int i = 0; i < 4; i++) ms4[i] = c->ts.last_ms[i];
    return GK_OK;
}

int gk_gfa_read(gk_gfa *c, uint64_t offset, char *buf, uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (int rc = gfa_live(c, "gk_gfa_read")) return rc;
    gk_ctx *ctx = c->ctx;
    if (offset > c->text_bytes) return fail(ctx, GK_E_INVALID, "gk_gfa_read: the offset lies beyond the text");
    const u64 want = std::min<u64>(cap, c->text_bytes - offset);
    if (want && !buf) return fail(ctx, GK_E_INVALID, "gk_gfa_read: buf is NULL");
    u64 done = 0;
    bool sink_failed = false;
    if (int rc = text_stream(&c->ts, c->text_bytes, offset, want, "gk_gfa", gfa_emit(c), [&](const char *p, u64 m) { std::memcpy(buf + done, p, m); done += m; return true; }, &sink_failed)) return rc;
    if (n) *n = done;
    return GK_OK;
}

int gk_gfa_write(gk_gfa *c, const char *path) {
    if (int rc = gfa_live(c, "gk_gfa_write")) return rc;
    gk_ctx *ctx = c->ctx;
    if (!path) return fail(ctx, GK_E_INVALID, "gk_gfa_write: path is NULL");
    return text_write_file(&c->ts, c->text_bytes, path, "gk_gfa", "gk_gfa_write", gfa_emit(c));
}

}  // extern "C"
