// gk_place.hip — placements and the judge: where every edge of a graph lies on a reference genome, and every junction of a scaffold
// plan held against those placements.  Both rules are this project's own and stated in include/genome_amd.h ("placements", "the
// judge"); tests/judge_ref.py restates them.
//
// Reference: none.  CheckGraph.scala asks whether a window of the genome is in the graph; nothing there asks where an edge lies.
//
// k_place_windows is k_fa_windows' shape (gk_fasta.hip): a slice of the record's characters staged in LDS with a k-1 halo, a lane
// owns PL_RUN consecutive window starts and rolls the window and its reverse complement together (append_base / prepend_base).
// What it adds: two getAll probes per window (gk_vmap_probe.h), and the hits folded before they reach HBM.  Adjacent windows hit
// the same edge on the same diagonal, so a lane keeps one open (edge, count, min, max) per strand and only a change of edge inside
// its run costs atomics; at the end the open runs of a wave's lanes are folded again (a segmented suffix reduction over equal
// neighbouring keys, six shuffle steps) and each segment's head issues ONE triple: a 32-bit add, a 64-bit min, a 64-bit max.
// On a genome of long edges that is about one triple per strand per 1024 windows.  LDS: the 4 KiB + halo of text only.
// k_place_classify: one lane per edge id reads the six words of its record and leaves class, record, position and the two counts;
// the class counts by ballot.  k_judge: one lane per segment of the plan, the junction's index from a scan over the edge
// segments; 18 (kind, class) counts by ballot, one atomic per wave and non-zero count.
#include <algorithm>
#include <string>
#include <vector>

#include "gk_scan.h"
#include "gk_text.h"
#include "gk_thread_common.h"

namespace {

constexpr u64 PL_SLICE_DEFAULT = 64ull << 20;          // characters per device slice
constexpr u32 PL_RUN = 16;                             // consecutive window starts per lane
constexpr u32 PL_WT = 256 * PL_RUN;                    // per workgroup
constexpr u64 PL_BIAS = 1ull << 39;                    // a candidate is stored as coordinate + 2^39 in the low 40 bits
constexpr u64 PL_COORD_MASK = (1ull << 40) - 1;
constexpr u64 PL_MAX_RECORDS = 1ull << 24;
enum { PC_VALID = 0, PC_WINDOWS = 1, PC_FWD = 2, PC_REV = 6, PC_BAD = 10, PC_N = 12 };       // device counters of the placement pass
enum { LC_ABSENT = 0, LC_REPETITIVE = 1, LC_AT_NODE = 2, LC_EDGE = 3 };
enum { PE_UNPLACED = 0, PE_BOTH = 1, PE_SCATTERED = 2, PE_FORWARD = 3, PE_REVERSE = 4, PE_FWD_BASES = 5, PE_REV_BASES = 6, PE_SATURATED = 7, PE_N = 8 };
enum { JC_UNJUDGED = 0, JC_OTHER_RECORD = 1, JC_STRAND = 2, JC_ORDER = 3, JC_DISTANCE = 4, JC_CORRECT = 5, JC_N = 6 };
enum { JK_ADJACENT = 0, JK_GAPPED = 1, JK_OVERLAPPED = 2, JK_N = 3 };
enum { JD_SUM = JK_N * JC_N, JD_MAX, JD_JUDGED, JD_CLEAN, JD_N };                              // device counters of the judge
constexpr int PLACE_NSTATS = 20, JUDGE_NSTATS = 29;

// the table: strand s of edge e at s * ne + e
struct PlaceView { u32 *cnt; unsigned long long *mn, *mx; uint8_t *sat; u64 ne; };
struct Fold { u32 key, cnt; u64 mn, mx; };

__device__ __forceinline__ u32 pl_code(u32 c) { return c == 'A' ? 0u : c == 'G' ? 1u : c == 'C' ? 2u : c == 'T' ? 3u : 4u; }

__device__ __forceinline__ void pl_flush(const PlaceView &pv, u32 strand, u32 rec, const Fold &f) {
    if (f.key == NONE) return;
    const u64 at = (u64)strand * pv.ne + f.key;
    const u32 old = atomicAdd(&pv.cnt[at], f.cnt);
    // Saturation.  The adds to a word are totally ordered, so the count passes 2^32-1 iff one of them wraps, and the lane whose add wraps
    // sees it in the value returned: the flag is set iff the count overflowed.  The store is a plain byte store that races only with
    // stores of the same value 1 from other waves (nothing ever clears it), and it is read by a later launch: the race is harmless.
    if (old + f.cnt < old) pv.sat[at] = 1;
    atomicMin(&pv.mn[at], (unsigned long long)(((u64)rec << 40) | f.mn));
    atomicMax(&pv.mx[at], (unsigned long long)(((u64)rec << 40) | f.mx));
}
__device__ __forceinline__ void pl_push(const PlaceView &pv, u32 strand, u32 rec, Fold &f, u32 e, u64 cand) {
    if (f.key == e) { f.cnt++; f.mn = min(f.mn, cand); f.mx = max(f.mx, cand); return; }
    pl_flush(pv, strand, rec, f);
    f.key = e; f.cnt = 1; f.mn = f.mx = cand;
}
// The open runs of the wave's 64 lanes: neighbours with the same key are one segment; lane l ends up with the fold of
// [l, end of its segment], so a segment's first lane holds all of it.  Every lane of the wave must call this.
__device__ __forceinline__ void pl_wave_flush(const PlaceView &pv, u32 strand, u32 rec, Fold f) {
    const int lane = threadIdx.x & 63;
    const u32 prev = __shfl_up(f.key, 1);
    const bool head = lane == 0 || prev != f.key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int seg_end = above ? lane + __ffsll((long long)above) - 1 : 63;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 oc = __shfl_down(f.cnt, d);
        const unsigned long long omn = __shfl_down((unsigned long long)f.mn, d), omx = __shfl_down((unsigned long long)f.mx, d);
        if (lane + d <= seg_end) { f.cnt += oc; f.mn = min(f.mn, (u64)omn); f.mx = max(f.mx, (u64)omx); }
    }
    if (head) pl_flush(pv, strand, rec, f);
}

// one lookup: its class, and for an `edge` hit the edge and the distance.  The position is untrusted (k_check_positions' test,
// bound first): one that names nothing live in this graph raises *bad and is dropped before any edge array is indexed by it.
template <int W>
__device__ __forceinline__ u32 pl_lookup(const Table<W> &pm, const GraphView &g, Kmer<W> x, u32 *e, u64 *d, unsigned long long *bad) {
    u64 v = 0;
    const u32 n = vmap_count_one(pm, x, &v);
    if (n == 0) return LC_ABSENT;
    if (n > 1) return LC_REPETITIVE;
    if (!GK_POS_IS_EDGE(v)) return LC_AT_NODE;
    const u32 id = GK_POS_ID(v);
    if (!(id < g.n_edges && g.e_alive[id] && (u64)GK_POS_DIST(v) < g.e_len[id])) { *bad = 1ull; *e = NONE; return LC_EDGE; }
    *e = id; *d = GK_POS_DIST(v);
    return LC_EDGE;
}

// T[0 .. L) = the slice with its halo: T[i] is character x0 + i of record `rec`; the first `halo` characters were counted by the
// slice before.  Every window start 0 .. L - k is evaluated here and nowhere else.
template <int W>
__global__ __launch_bounds__(256) void k_place_windows(Table<W> pm, GraphView g, int k, const uint8_t *__restrict__ T, u64 L, u64 halo, u64 x0, u32 rec,
                                                       PlaceView pv, unsigned long long *ctr) {
    __shared__ u32 s_txt[(PL_WT + 128) / 4];
    const u64 P = L >= (u64)k ? L - (u64)k + 1 : 0;
    const u64 pb = (u64)blockIdx.x * PL_WT;
    const u64 cend = umin(L, pb + PL_WT + (u64)k - 1);
    u64 a0 = 0;
    if (pb < cend) a0 = stage_tile(s_txt, T, pb, cend);
    __syncthreads();
    const uint8_t *sc = reinterpret_cast<const uint8_t *>(s_txt);
    const u64 p = pb + (u64)threadIdx.x * PL_RUN;
    Fold ff{NONE, 0u, ~0ull, 0ull}, fr{NONE, 0u, ~0ull, 0ull};
    u64 cf = 0, cr = 0, cvw = 0;                              // four 16-bit class counts per strand; valid | windows << 16
    if (p < L) {
        Kmer<W> km{}, rc{};
        u32 good = 0;
        if (p < P)
            for (int j = 0; j < k - 1; j++) {
                const u32 c = pl_code(sc[p + j - a0]);
                km = append_base(km, (int)(c & 3u), k);
                rc = prepend_base((int)(3u - (c & 3u)), rc, k);
                good = c < 4u ? good + 1 : 0;
            }
        for (u32 r = 0; r < PL_RUN && p + r < L; r++) {
            const u64 q = p + r;
            if (q >= halo && pl_code(sc[q - a0]) < 4u) cvw += 1;
            if (q >= P) continue;
            const u32 c = pl_code(sc[q + k - 1 - a0]);
            km = append_base(km, (int)(c & 3u), k);
            rc = prepend_base((int)(3u - (c & 3u)), rc, k);
            good = c < 4u ? good + 1 : 0;
            if (good < (u32)k) continue;
            cvw += 1ull << 16;
            const u64 x = x0 + q;
            u32 e = NONE;
            u64 d = 0;
            u32 cls = pl_lookup(pm, g, km, &e, &d, &ctr[PC_BAD]);
            cf += 1ull << (16 * cls);
            if (e != NONE) pl_push(pv, 0u, rec, ff, e, PL_BIAS + x - d);
            e = NONE;
            cls = pl_lookup(pm, g, rc, &e, &d, &ctr[PC_BAD]);
            cr += 1ull << (16 * cls);
            if (e != NONE) pl_push(pv, 1u, rec, fr, e, PL_BIAS + x + d + (u64)k - 1);
        }
    }
    pl_wave_flush(pv, 0u, rec, ff);
    pl_wave_flush(pv, 1u, rec, fr);
    cf = wave_sum(cf); cr = wave_sum(cr); cvw = wave_sum(cvw);               // (64 lanes x 16 windows: every field stays below 2^16)
    if ((threadIdx.x & 63) == 0) {
        if (cvw & 0xffffu) atomicAdd(&ctr[PC_VALID], (unsigned long long)(cvw & 0xffffu));
        if (cvw >> 16) atomicAdd(&ctr[PC_WINDOWS], (unsigned long long)(cvw >> 16));
        for (int c = 0; c < 4; c++) {
            const u64 a = (cf >> (16 * c)) & 0xffffu, b = (cr >> (16 * c)) & 0xffffu;
            if (a) atomicAdd(&ctr[PC_FWD + c], (unsigned long long)a);
            if (b) atomicAdd(&ctr[PC_REV + c], (unsigned long long)b);
        }
    }
}

// one lane per edge id: the edge class, and what gk_placements_edges hands out
__global__ __launch_bounds__(BLOCK) void k_place_classify(GraphView g, PlaceView pv, uint8_t *__restrict__ cls, u32 *__restrict__ prec, long long *__restrict__ ppos,
                                                          u32 *__restrict__ wf, u32 *__restrict__ wr, unsigned long long *st) {
    u32 wc[5] = {}, nsat = 0;
    unsigned long long fb = 0, rb = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < pv.ne; base += (u64)gridDim.x * BLOCK) {      // (uniform over the wave)
        const u64 e = base + threadIdx.x;
        u32 c = 5;                                   // 5: no live edge
        bool sat = false;
        unsigned long long pb = 0;
        if (e < pv.ne) {
            const bool sf = pv.sat[e] != 0, sr = pv.sat[pv.ne + e] != 0;
            const u32 nf = sf ? 0xffffffffu : pv.cnt[e], nr = sr ? 0xffffffffu : pv.cnt[pv.ne + e];
            u32 rec = 0;
            long long pos = 0;
            if (g.e_alive[e]) {
                sat = sf || sr;
                if (!nf && !nr) c = PE_UNPLACED;
                else if (nf && nr) c = PE_BOTH;
                else {
                    const u64 at = nf ? e : pv.ne + e;
                    const u64 mn = pv.mn[at], mx = pv.mx[at];
                    if (mn != mx) c = PE_SCATTERED;
                    else {
                        c = nf ? PE_FORWARD : PE_REVERSE;
                        rec = (u32)(mn >> 40);
                        pos = (long long)(mn & PL_COORD_MASK) - (long long)PL_BIAS;
                        pb = (unsigned long long)g.k + g.e_len[e];
                    }
                }
            }
            cls[e] = c == 5 ? (uint8_t)PE_UNPLACED : (uint8_t)c;
            prec[e] = rec; ppos[e] = pos; wf[e] = c == 5 ? 0u : nf; wr[e] = c == 5 ? 0u : nr;
        }
#pragma unroll
        for (u32 q = 0; q < 5; q++) wc[q] += (u32)__popcll(__ballot(c == q));
        nsat += (u32)__popcll(__ballot(sat));
        fb += wave_sum(c == PE_FORWARD ? pb : 0ull);
        rb += wave_sum(c == PE_REVERSE ? pb : 0ull);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (u32 q = 0; q < 5; q++) if (wc[q]) atomicAdd(&st[q], (unsigned long long)wc[q]);
        if (fb) atomicAdd(&st[PE_FWD_BASES], fb);
        if (rb) atomicAdd(&st[PE_REV_BASES], rb);
        if (nsat) atomicAdd(&st[PE_SATURATED], (unsigned long long)nsat);
    }
}

__global__ __launch_bounds__(BLOCK) void k_place_gather(const u32 *__restrict__ ids, u64 n, const uint8_t *__restrict__ cls, const u32 *__restrict__ prec,
                                                        const long long *__restrict__ ppos, const u32 *__restrict__ wf, const u32 *__restrict__ wr,
                                                        uint8_t *o_cls, u32 *o_rec, long long *o_pos, u32 *o_wf, u32 *o_wr) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u32 e = ids[i];                        // (below the bound: checked on the host)
        o_cls[i] = cls[e]; o_rec[i] = prec[e]; o_pos[i] = ppos[e]; o_wf[i] = wf[e]; o_wr[i] = wr[e];
    }
}

// ---- the judge ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_judge_flags(const u32 *__restrict__ seg_edge, u64 nseg, u32 *__restrict__ flag) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < nseg; i += (u64)gridDim.x * BLOCK) flag[i] = seg_edge[i] != NONE;
}

// One lane per segment i.  An edge segment whose record goes on is the first row of a junction; the second row is segment i + 1,
// or i + 2 behind an N run.  The junction's index is (edge segments before i) - (records before i's): every record before it
// has one junction less than it has rows.
__global__ __launch_bounds__(BLOCK) void k_judge(GraphView g, ScafRows p, const unsigned long long *__restrict__ rowrank, const uint8_t *__restrict__ pcls,
                                                 const u32 *__restrict__ prec, const long long *__restrict__ ppos, u64 tol, uint8_t *__restrict__ o_cls,
                                                 long long *__restrict__ o_err, u32 *__restrict__ rec_judged, u32 *__restrict__ rec_misjoin, unsigned long long *st) {
    u32 wc[JK_N * JC_N] = {};
    unsigned long long esum = 0, emax = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < p.segs; base += (u64)gridDim.x * BLOCK) {     // (uniform over the wave)
        const u64 i = base + threadIdx.x;
        u32 code = JK_N * JC_N;                      // no junction
        unsigned long long aerr = 0;
        if (i < p.segs && p.seg_edge[i] != NONE) {
            u64 lo = 0, hi = p.records;              // the record: the last r with rec_seg[r] <= i
            while (hi - lo > 1) {
                const u64 mid = lo + (hi - lo) / 2;
                if (p.rec_seg[mid] <= i) lo = mid; else hi = mid;
            }
            const u64 r = lo, send = p.rec_seg[r + 1];
            u64 j = i + 1;
            u32 kind = JK_N;
            if (j < send && p.seg_edge[j] == NONE) { j++; kind = JK_GAPPED; }
            if (j < send) {
                const u32 e = p.seg_edge[i], f = p.seg_edge[j];
                if (kind == JK_N) kind = g.e_end[e] == g.e_start[f] ? JK_ADJACENT : JK_OVERLAPPED;
                const u32 ce = pcls[e], cf = pcls[f];
                u32 cls;
                long long err = 0;
                if ((ce != PE_FORWARD && ce != PE_REVERSE) || (cf != PE_FORWARD && cf != PE_REVERSE)) cls = JC_UNJUDGED;
                else if (prec[e] != prec[f]) cls = JC_OTHER_RECORD;
                else if (ce != cf) cls = JC_STRAND;
                else {
                    const long long se = p.seg_skip[i], sf = p.seg_skip[j];
                    const long long dscaf = (long long)p.seg_start[j] - (long long)p.seg_start[i];
                    const long long dref = ce == PE_FORWARD ? (ppos[f] + sf) - (ppos[e] + se) : (ppos[e] - se) - (ppos[f] - sf);
                    err = dscaf - dref;
                    const unsigned long long a = err < 0 ? (unsigned long long)(-err) : (unsigned long long)err;
                    if (dref <= 0) cls = JC_ORDER;
                    else if (kind == JK_GAPPED ? a > tol : err != 0) cls = JC_DISTANCE;
                    else { cls = JC_CORRECT; if (kind == JK_GAPPED) aerr = a; }
                }
                const u64 jx = rowrank[i] - r;
                o_cls[jx] = (uint8_t)cls; o_err[jx] = err;
                if (cls != JC_UNJUDGED) rec_judged[r] = 1u;
                if (cls >= JC_OTHER_RECORD && cls <= JC_DISTANCE) rec_misjoin[r] = 1u;
                code = kind * JC_N + cls;
            }
        }
#pragma unroll
        for (u32 c = 0; c < JK_N * JC_N; c++) wc[c] += (u32)__popcll(__ballot(code == c));
        esum += wave_sum(aerr);
        for (int d = 32; d; d >>= 1) aerr = max(aerr, (unsigned long long)__shfl_xor(aerr, d));
        emax = max(emax, aerr);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (u32 c = 0; c < JK_N * JC_N; c++) if (wc[c]) atomicAdd(&st[c], (unsigned long long)wc[c]);
        if (esum) atomicAdd(&st[JD_SUM], esum);
        if (emax) atomicMax(&st[JD_MAX], emax);
    }
}
// the chain records: those with a judged junction, those without a misjoin
__global__ __launch_bounds__(BLOCK) void k_judge_records(const u32 *__restrict__ rec_judged, const u32 *__restrict__ rec_misjoin, u64 chain_recs, unsigned long long *st) {
    u32 nj = 0, nc = 0;
    for (u64 base = (u64)blockIdx.x * BLOCK; base < chain_recs; base += (u64)gridDim.x * BLOCK) {
        const u64 r = base + threadIdx.x;
        nj += (u32)__popcll(__ballot(r < chain_recs && rec_judged[r] != 0));
        nc += (u32)__popcll(__ballot(r < chain_recs && rec_misjoin[r] == 0));
    }
    if ((threadIdx.x & 63) == 0) {
        if (nj) atomicAdd(&st[JD_JUDGED], (unsigned long long)nj);
        if (nc) atomicAdd(&st[JD_CLEAN], (unsigned long long)nc);
    }
}

}  // namespace

struct gk_placements {
    gk_ctx *ctx = nullptr;
    gk_graph *g = nullptr;
    gk_vmap *vm = nullptr;
    int k = 0, W = 1;
    u64 epoch = 0, ne = 0;
    bool failed = false, classified = false;
    u64 records = 0, bases = 0;
    u32 *d_cnt = nullptr;                        // the table (PlaceView)
    unsigned long long *d_mn = nullptr, *d_mx = nullptr;
    uint8_t *d_sat = nullptr;
    unsigned long long *d_ctr = nullptr;         // PC_N words
    // per edge id, made by the first stats / edges / judge after the last record (k_place_classify)
    uint8_t *d_cls = nullptr;
    u32 *d_rec = nullptr, *d_wf = nullptr, *d_wr = nullptr;
    long long *d_pos = nullptr;
    u64 stats[PLACE_NSTATS] = {};
    TextUpload up;
    float ms[4] = {0, 0, 0, 0};
};

namespace {

u64 pl_slice_max(const gk_ctx *ctx) { return ctx->hook_place_slice > 0 ? (u64)ctx->hook_place_slice : PL_SLICE_DEFAULT; }
PlaceView pl_view(const gk_placements *p) { return PlaceView{p->d_cnt, p->d_mn, p->d_mx, p->d_sat, p->ne}; }

int pl_live(const gk_placements *p, const char *who) {
    if (!p || !p->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null placements handle");
    const hipError_t e = hipSetDevice(p->ctx->device);
    if (e != hipSuccess) return hip_fail(p->ctx, e, "hipSetDevice");
    if (p->g->epoch != p->epoch) return fail(p->ctx, GK_E_STATE, std::string(who) + ": the graph was edited after the placements were created");
    return GK_OK;
}
int pl_fail(gk_placements *p, int code, const std::string &msg) {
    p->failed = true;
    return fail(p->ctx, code, msg);
}
#define PL_HIP(p, call)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess) { (p)->failed = true; return gk::hip_fail((p)->ctx, e__, #call); } \
    } while (0)

// the records of one call, slice by slice
int pl_run(gk_placements *p, const char *bases, u64 n) {
    gk_ctx *ctx = p->ctx;
    const int k = p->k;
    const u64 slice_max = pl_slice_max(ctx), cap = std::min<u64>(n, slice_max) + 64;      // a slice and its halo (k - 1 <= 63)
    const int nbuf = n > slice_max ? 2 : 1;
    const bool pinned = TextUpload::is_pinned(bases);
    double up_ms = 0, look_ms = 0;
    DevScratch tmp(ctx);
    uint8_t *tb[2] = {nullptr, nullptr};
    for (int i = 0; i < nbuf; i++) tmp.get(&tb[i], std::max<u64>(cap + 64, 1ull << 20));      // (a block of 1 MiB is pooled)
    if (tmp.error() != hipSuccess) { p->failed = true; return hip_fail(ctx, tmp.error(), "gk_placements_add_record: slice buffers"); }
    void *slots = nullptr;
    uint32_t nb2 = 1, lnb1 = 0;
    vmap_table(p->vm, &slots, &nb2, &lnb1);
    const TimedSection kt{ctx};
    auto halo_of = [&](u64 s0) { return std::min<u64>((u64)k - 1, s0); };
    int b = 0, rc = GK_OK;
    u64 s0 = 0;
    // (every slice after the first brings its halo: ask for the largest upload now, not for a second, larger pair of buffers later)
    if (!pinned && n > slice_max) { if ((rc = p->up.reserve(ctx, slice_max + 63))) { p->failed = true; return rc; } }
    if ((rc = p->up.upload(ctx, 0, tb[0], bases, std::min<u64>(n, slice_max), pinned, &up_ms))) { p->failed = true; return rc; }
    while (s0 < n) {
        const u64 len = std::min<u64>(n - s0, slice_max), halo = halo_of(s0), L = halo + len;
        PL_HIP(p, hipStreamWaitEvent(ctx->stream, p->up.up1[b], 0));
        PL_HIP(p, kt.start());
        const unsigned grid = (unsigned)((L + PL_WT - 1) / PL_WT);
        GK_BY_W(p->W, hipLaunchKernelGGL(k_place_windows<W>, dim3(grid), dim3(256), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u}, p->g->v, k,
                                         tb[b], L, halo, s0 - halo, (u32)p->records, pl_view(p), p->d_ctr));
        PL_HIP(p, hipGetLastError());
        // (the next slice goes up on the copy stream beside this one's kernel: the other buffer is free)
        const u64 s1 = s0 + len;
        if (s1 < n) {
            const u64 h1 = halo_of(s1), len1 = std::min<u64>(n - s1, slice_max);
            if ((rc = p->up.upload(ctx, 1 - b, tb[1 - b], bases + (s1 - h1), h1 + len1, pinned, &up_ms))) { p->failed = true; return rc; }
        }
        if ((rc = kt.end(&look_ms))) { p->failed = true; return rc; }
        {
            float t = 0;
            PL_HIP(p, hipEventElapsedTime(&t, p->up.up0[b], p->up.up1[b]));
            up_ms += t;
        }
        s0 = s1;
        b = 1 - b;
    }
    PL_HIP(p, hipStreamSynchronize(ctx->copy_stream));
    p->ms[0] = (float)up_ms; p->ms[2] = (float)look_ms;
    return GK_OK;
}

// class, record, position and counts of every edge id, and the stats; once per set of records
int pl_classify(gk_placements *pc, const char *who) {
    gk_placements *p = pc;
    if (p->classified) return GK_OK;
    gk_ctx *ctx = p->ctx;
    DevScratch tmp(ctx);
    unsigned long long *d_st = nullptr, h_st[PE_N] = {}, h_ctr[PC_N] = {};
    tmp.zeroed(&d_st, PE_N);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), (std::string(who) + ": scratch").c_str());
    if (p->ne)
        hipLaunchKernelGGL(k_place_classify, dim3(ggrid(ctx, p->ne)), dim3(BLOCK), 0, ctx->stream, p->g->v, pl_view(p), p->d_cls, p->d_rec, p->d_pos, p->d_wf, p->d_wr, d_st);
    GK_HIP(ctx, read_back(ctx, {{h_st, d_st, sizeof(h_st)}, {h_ctr, p->d_ctr, sizeof(h_ctr)}}));
    u64 *st = p->stats;
    st[0] = p->records; st[1] = p->bases; st[2] = h_ctr[PC_VALID]; st[3] = h_ctr[PC_WINDOWS];
    for (int c = 0; c < 4; c++) { st[4 + c] = h_ctr[PC_FWD + c]; st[8 + c] = h_ctr[PC_REV + c]; }
    for (int c = 0; c < 5; c++) st[12 + c] = h_st[c];
    st[17] = h_st[PE_FWD_BASES]; st[18] = h_st[PE_REV_BASES]; st[19] = h_st[PE_SATURATED];
    p->classified = true;
    return GK_OK;
}

}  // namespace

extern "C" {

void gk_placements_destroy(gk_placements *p) {
    if (!p) return;
    gk_ctx *ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    for (void *q : {(void *)p->d_cnt, (void *)p->d_mn, (void *)p->d_mx, (void *)p->d_sat, (void *)p->d_ctr, (void *)p->d_cls, (void *)p->d_rec, (void *)p->d_wf,
                    (void *)p->d_wr, (void *)p->d_pos})
        (void)pool_free(ctx, q);
    p->up.destroy();
    delete p;
}

int gk_placements_create(gk_graph *g, gk_vmap *positions, gk_placements **out) {
    if (!out) return fail(g ? g->ctx : nullptr, GK_E_INVALID, "gk_placements_create: out is NULL");
    *out = nullptr;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (!positions) return fail(ctx, GK_E_INVALID, "gk_placements_create: null position map");
    if (vmap_ctx(positions) != ctx) return fail(ctx, GK_E_INVALID, "gk_placements_create: the position map lives on another context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, "gk_placements_create: the position map has another k");
    gk_placements *p = new gk_placements;
    p->ctx = ctx; p->g = g; p->vm = positions; p->k = g->k; p->W = words_for_k(g->k); p->epoch = g->epoch; p->ne = g->v.n_edges;
    const u64 m = std::max<u64>(p->ne, 1);
    hipError_t e = p->up.create();
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_cnt, 2 * m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_mn, 2 * m * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_mx, 2 * m * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_sat, 2 * m);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_ctr, PC_N * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_cls, m);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_rec, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_wf, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_wr, m * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &p->d_pos, m * 8);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_cnt, 0, 2 * m * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_mn, 0xff, 2 * m * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_mx, 0, 2 * m * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_sat, 0, 2 * m, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_ctr, 0, PC_N * 8, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { const int rc = hip_fail(ctx, e, "gk_placements_create"); gk_placements_destroy(p); return rc; }
    *out = p;
    return GK_OK;
}

int gk_placements_add_record(gk_placements *p, const char *bases, uint64_t n) {
    if (int rc = pl_live(p, "gk_placements_add_record")) return rc;
    gk_ctx *ctx = p->ctx;
    if (p->failed) return fail(ctx, GK_E_STATE, "gk_placements_add_record: the handle failed earlier (see the first error); destroy it");
    if (!bases && n) return fail(ctx, GK_E_INVALID, "gk_placements_add_record: null bases");
    if (p->records >= PL_MAX_RECORDS) return pl_fail(p, GK_E_CAPACITY, "gk_placements_add_record: more than 2^24 records");
    if (n >= PL_BIAS) return pl_fail(p, GK_E_CAPACITY, "gk_placements_add_record: a record of 2^39 bases or more");
    const auto t_call = clk::now();
    p->ms[0] = p->ms[1] = p->ms[2] = 0;
    p->classified = false;
    if (n) { if (int rc = pl_run(p, bases, n)) return rc; }
    unsigned long long bad = 0;
    PL_HIP(p, read_back(ctx, &bad, p->d_ctr + PC_BAD));
    if (bad) return pl_fail(p, GK_E_STATE, "gk_placements_add_record: the position map names an edge that is not live in this graph (a stale map)");
    p->records++;
    p->bases += n;
    p->ms[3] = (float)ms_since(t_call);
    return GK_OK;
}

int gk_placements_stats(const gk_placements *p, uint64_t *stats) {
    if (int rc = pl_live(p, "gk_placements_stats")) return rc;
    if (!stats) return fail(p->ctx, GK_E_INVALID, "gk_placements_stats: stats is NULL");
    if (int rc = pl_classify(const_cast<gk_placements *>(p), "gk_placements_stats")) return rc;
    for (int i = 0; i < PLACE_NSTATS; i++) stats[i] = p->stats[i];
    return GK_OK;
}

int gk_placements_edges(const gk_placements *p, const uint32_t *edge_ids, uint64_t n, uint8_t *cls, uint32_t *record, int64_t *pos, uint32_t *windows_fwd,
                        uint32_t *windows_rev) {
    if (int rc = pl_live(p, "gk_placements_edges")) return rc;
    gk_ctx *ctx = p->ctx;
    if (n == 0) return GK_OK;
    if (!edge_ids) return fail(ctx, GK_E_INVALID, "gk_placements_edges: edge_ids is NULL");
    for (u64 i = 0; i < n; i++)
        if (edge_ids[i] >= p->ne) return fail(ctx, GK_E_INVALID, "gk_placements_edges: edge id " + std::to_string(edge_ids[i]) + " is not below the bound " + std::to_string(p->ne));
    if (int rc = pl_classify(const_cast<gk_placements *>(p), "gk_placements_edges")) return rc;
    DevScratch tmp(ctx);
    u32 *d_ids = nullptr, *o_rec = nullptr, *o_wf = nullptr, *o_wr = nullptr;
    uint8_t *o_cls = nullptr;
    long long *o_pos = nullptr;
    tmp.upload(&d_ids, edge_ids, n);
    tmp.get(&o_cls, n); tmp.get(&o_rec, n); tmp.get(&o_pos, n); tmp.get(&o_wf, n); tmp.get(&o_wr, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_placements_edges: scratch");
    hipLaunchKernelGGL(k_place_gather, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, d_ids, (u64)n, p->d_cls, p->d_rec, p->d_pos, p->d_wf, p->d_wr, o_cls, o_rec, o_pos,
                       o_wf, o_wr);
    GK_HIP(ctx, read_back(ctx, {{cls, o_cls, (size_t)n}, {record, o_rec, (size_t)n * 4}, {pos, o_pos, (size_t)n * 8}, {windows_fwd, o_wf, (size_t)n * 4},
                                {windows_rev, o_wr, (size_t)n * 4}}));
    return GK_OK;
}

int gk_placements_last_ms(const gk_placements *p, float *ms4) {
    if (!p) return fail(nullptr, GK_E_INVALID, "gk_placements_last_ms: null handle");
    if (!ms4) return fail(p->ctx, GK_E_INVALID, "gk_placements_last_ms: null buffer");
    for (int i = 0; i < 4; i++) ms4[i] = p->ms[i];
    return GK_OK;
}

int gk_scaffolds_judge(const gk_scaffolds *s, const gk_placements *p, uint64_t tol, uint8_t *cls, int64_t *err, uint64_t cap, uint64_t *n, uint64_t *stats) {
    if (n) *n = 0;
    if (stats) for (int i = 0; i < JUDGE_NSTATS; i++) stats[i] = 0;
    if (!s) return fail(p ? p->ctx : nullptr, GK_E_INVALID, "gk_scaffolds_judge: null scaffolds handle");
    ScafRows rows{};
    scaffolds_rows(s, &rows);
    if (!rows.ctx) return fail(nullptr, GK_E_INVALID, "gk_scaffolds_judge: null scaffolds handle");
    if (!p || !p->ctx) return fail(rows.ctx, GK_E_INVALID, "gk_scaffolds_judge: null placements handle");
    gk_ctx *ctx = p->ctx;
    if (rows.ctx != ctx || rows.g != p->g) return fail(ctx, GK_E_INVALID, "gk_scaffolds_judge: the plan and the placements are of different graphs or contexts");
    if (!n || !stats) return fail(ctx, GK_E_INVALID, "gk_scaffolds_judge: n or stats is NULL");
    if (int rc = pl_live(p, "gk_scaffolds_judge")) return rc;
    if (rows.epoch != p->g->epoch) return fail(ctx, GK_E_STATE, "gk_scaffolds_judge: the graph was edited after the plan was made");
    if (int rc = pl_classify(const_cast<gk_placements *>(p), "gk_scaffolds_judge")) return rc;
    const u64 nj = rows.rows - rows.records;                 // a record of m rows has m - 1 junctions, and no record is empty
    unsigned long long h_st[JD_N] = {};
    DevScratch tmp(ctx);
    uint8_t *d_cls = nullptr;
    long long *d_err = nullptr;
    if (nj) {
        u32 *d_flag = nullptr, *d_judged = nullptr, *d_mis = nullptr;
        unsigned long long *d_rank = nullptr, *d_st = nullptr;
        tmp.get(&d_flag, rows.segs);
        tmp.get(&d_rank, rows.segs + 1);
        tmp.get(&d_cls, nj);
        tmp.get(&d_err, nj);
        tmp.zeroed(&d_judged, rows.chain_recs);
        tmp.zeroed(&d_mis, rows.chain_recs);
        tmp.zeroed(&d_st, JD_N);
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_scaffolds_judge: scratch");
        hipLaunchKernelGGL(k_judge_flags, dim3(ggrid(ctx, rows.segs)), dim3(BLOCK), 0, ctx->stream, rows.seg_edge, rows.segs, d_flag);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, tmp, d_flag, rows.segs, d_rank));
        hipLaunchKernelGGL(k_judge, dim3(ggrid(ctx, rows.segs)), dim3(BLOCK), 0, ctx->stream, p->g->v, rows, d_rank, p->d_cls, p->d_rec, p->d_pos, (u64)tol, d_cls, d_err,
                           d_judged, d_mis, d_st);
        hipLaunchKernelGGL(k_judge_records, dim3(ggrid(ctx, rows.chain_recs)), dim3(BLOCK), 0, ctx->stream, d_judged, d_mis, rows.chain_recs, d_st);
        GK_HIP(ctx, read_back(ctx, {{h_st, d_st, sizeof(h_st)}}));
    } else h_st[JD_CLEAN] = rows.chain_recs;
    *n = nj;
    stats[0] = nj;
    for (int kd = 0; kd < JK_N; kd++)
        for (int c = 0; c < JC_N; c++) { stats[7 + kd * JC_N + c] = h_st[kd * JC_N + c]; stats[1 + c] += h_st[kd * JC_N + c]; }
    stats[25] = h_st[JD_SUM]; stats[26] = h_st[JD_MAX]; stats[27] = h_st[JD_JUDGED]; stats[28] = h_st[JD_CLEAN];
    if (nj > cap) return fail(ctx, GK_E_CAPACITY, "gk_scaffolds_judge: room for " + std::to_string(cap) + " junctions, " + std::to_string(nj) + " needed");
    if (nj == 0) return GK_OK;
    if (!cls || !err) return fail(ctx, GK_E_INVALID, "gk_scaffolds_judge: an output array is NULL");
    GK_HIP(ctx, read_back(ctx, {{cls, d_cls, (size_t)nj}, {err, d_err, (size_t)nj * 8}}));
    return GK_OK;
}

}  // extern "C"
