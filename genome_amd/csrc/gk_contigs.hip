// gk_contigs.hip — the assembly as FASTA text, written on the device: one record per live edge, one strand per contig.
//
// Reference: GraphSimplifier.scala:338-347 prints every edge's seq before a ">abacaba<i>" line, both strands, without the start
// k-mer (Graph::writeContigs in host/genome.hpp is its literal twin and stays).  The rule here is this project's own and stated in
// include/genome_amd.h ("contigs: this project's own rule"); tests/contigs_ref.py restates it.
//
// Three steps.  k_contig_classify: one wave per live edge compares the path with its reverse complement and stops at the first
// difference; a lane sizes the record.  (With a count table the sums come from gk_coverage.hip's pass over the selected edges and
// k_contig_cov adds the cov= field.)  Two scans (gk_scan.h) and k_contig_compact leave (id, byte offset[, q]) per record: the
// plan.  k_contig_emit is output-centric: it is handed a byte range of the text and every lane produces one aligned 8-byte word
// of it, found by a binary search in the record offsets once per wave, so chunked writes and reads at any offset are the same
// launch.  No LDS, no atomics in the emit kernel.
//
// Roofline: the emit kernel reads 2 bits and writes 8 (plus the line ends) per base: it is a streaming write of the text.
#include <memory>

#include "gk_fastaout.h"
#include "gk_scan.h"

// device counters of a plan: the four classes, bases of the records, windows missing from the table, "a record passes 2^32-1 bytes"
enum { CS_SHORT = 0, CS_FORWARD, CS_SELF, CS_REVERSE, CS_BASES, CS_MISSING, CS_OVERFLOW, CS_N };

// ---------------------------------------------------------------------------------------------
// classification and sizing: one wave per live edge
// ---------------------------------------------------------------------------------------------
// cls[e] = the class, want[e] / sel[e] = 1 for a record, size[e] = the bytes of its text without a cov= field (0: no record)
__global__ __launch_bounds__(BLOCK) void k_contig_classify(GraphView g, u64 min_len, u32 line_width, int strands, uint8_t *__restrict__ cls,
                                                           uint8_t *__restrict__ want, u32 *__restrict__ sel, u32 *__restrict__ size,
                                                           unsigned long long *stats) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    unsigned long long cnt[4] = {0, 0, 0, 0}, bases = 0, over = 0;
    for (u64 e = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e < g.n_edges; e += waves) {      // (uniform over the wave)
        if (!g.e_alive[e]) {
            if (lane == 0) { cls[e] = CLS_DEAD; want[e] = 0; sel[e] = 0; size[e] = 0; }
            continue;
        }
        const u64 n = (u64)g.k + g.e_len[e];
        const uint8_t c = wave_contig_class(g, e, min_len);
        if (lane == 0) {
            const bool rec = c == CLS_FORWARD || c == CLS_SELF || (c == CLS_REVERSE && strands == 2);
            u64 bytes = 0;
            if (rec) {
                bytes = (u64)rec_hdr(e, n, 0, false).len + body_bytes(n, line_width);
                if (bytes > 0xfffffff0ull) { over = 1; bytes = 0; }      // (room for the cov= field below 2^32)
                else bases += n;
            }
            cls[e] = c; want[e] = rec && bytes; sel[e] = rec && bytes; size[e] = (u32)bytes;
            cnt[c - CLS_SHORT]++;
        }
    }
    if (lane == 0) {
        for (int i = 0; i < 4; i++) if (cnt[i]) atomicAdd(&stats[CS_SHORT + i], cnt[i]);
        if (bases) atomicAdd(&stats[CS_BASES], bases);
        if (over) atomicAdd(&stats[CS_OVERFLOW], over);
    }
}
// with a count table: q = floor(100 * sum / kmers) per record and the cov= field's bytes; the windows the table does not hold.
// 100 * sum may pass 2^64, so the quotient is taken in two parts: 100 * (sum / kmers) + 100 * (sum % kmers) / kmers, where
// sum / kmers is a mean of 32-bit counts and sum % kmers < kmers < 2^57.
__global__ __launch_bounds__(BLOCK) void k_contig_cov(GraphView g, EdgeCov cov, const uint8_t *__restrict__ want, u64 *__restrict__ q, u32 *__restrict__ size,
                                                      unsigned long long *stats) {
    const u64 stride = (u64)gridDim.x * BLOCK;
    for (u64 e0 = (u64)blockIdx.x * BLOCK; e0 < g.n_edges; e0 += stride) {      // (uniform over the wave: every lane takes the shuffles)
        const u64 e = e0 + threadIdx.x;
        unsigned long long miss = 0;
        if (e < g.n_edges && want[e]) {
            const u64 kmers = g.e_len[e] + 1, sum = cov.sum[e];
            const u64 v = 100 * (sum / kmers) + 100 * (sum % kmers) / kmers;
            q[e] = v;
            size[e] += (u32)(5 + dec_digits(v / 100) + 3);
            miss = cov.miss[e];
        }
        for (int d = 32; d; d >>= 1) miss += __shfl_down(miss, d);
        if ((threadIdx.x & 63) == 0 && miss) atomicAdd(&stats[CS_MISSING], miss);
    }
}
// the records in ascending edge id: (id, byte offset[, q]); rec_off[records] = the text's size
__global__ __launch_bounds__(BLOCK) void k_contig_compact(u64 n_edges, const u32 *__restrict__ sel, const unsigned long long *__restrict__ rank,
                                                          const unsigned long long *__restrict__ off, const u64 *__restrict__ q, u32 *__restrict__ rec_id,
                                                          unsigned long long *__restrict__ rec_off, u64 *__restrict__ rec_q) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e <= n_edges; e += (u64)gridDim.x * BLOCK) {
        if (e == n_edges) { rec_off[rank[e]] = off[e]; continue; }
        if (!sel[e]) continue;
        const u64 r = rank[e];
        rec_id[r] = (u32)e;
        rec_off[r] = off[e];
        if (rec_q) rec_q[r] = q[e];
    }
}

// ---------------------------------------------------------------------------------------------
// emission: a byte range of the text
// ---------------------------------------------------------------------------------------------
struct ContigPlan {
    const u32 *id;
    const unsigned long long *off;       // [records + 1]
    const u64 *q;                        // nullptr without a count table
    u64 records;
    u32 line_width;
};
// Bytes [t0, t1) of the text, t0 < t1 <= off[records].  `out` is 8-byte aligned and holds text byte t at out[t - (t0 & ~7)]: a
// word of the text that is aligned in the text is aligned in memory.  Items in text order: the bytes before the first whole word,
// the whole words, the bytes after the last; a lane takes one item and stores it once.
__global__ __launch_bounds__(BLOCK) void k_contig_emit(GraphView g, ContigPlan p, u64 t0, u64 t1, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const u64 base = t0 & ~(u64)7;
    const u64 a0 = min(t1, (t0 + 7) & ~(u64)7), a1 = max(a0, t1 & ~(u64)7);                // whole words: [a0, a1)
    const u64 nhead = a0 - t0, nwords = (a1 - a0) >> 3, items = nhead + nwords + (t1 - a1);
    const bool has_cov = p.q != nullptr;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 tile = ((u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * 64; tile < items; tile += waves * 64) {
        // the record of the wave's first byte: the last r with off[r] <= pos (pos < off[records])
        const u64 wpos = tile < nhead ? t0 + tile : tile < nhead + nwords ? a0 + 8 * (tile - nhead) : a1 + (tile - nhead - nwords);
        u64 lo = 0, hi = p.records;
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            if (p.off[mid] <= wpos) lo = mid; else hi = mid;
        }
        const u64 item = tile + (u64)lane;
        if (item >= items) continue;
        const bool word = item >= nhead && item < nhead + nwords;
        const u64 pos = item < nhead ? t0 + item : word ? a0 + 8 * (item - nhead) : a1 + (item - nhead - nwords);
        const int nb = word ? 8 : 1;
        // walk forward from the wave's record
        u64 r = lo;
        while (p.off[r + 1] <= pos) r++;
        u64 bits = 0, begin = 0, end = 0, nlo = 0, nhi = 0, bi = 0;
        u32 col = 0;
        const uint8_t *seq = nullptr;
        RecHdr h{};
        bool fresh = true, body_init = true;
        for (int b = 0; b < nb; b++) {
            const u64 at = pos + (u64)b;
            if (!fresh && at >= end) { r++; fresh = true; }
            if (fresh) {
                const u32 e = p.id[r];
                const u32 s = g.e_start[e];
                begin = p.off[r]; end = p.off[r + 1];
                h = rec_hdr(e, (u64)g.k + g.e_len[e], has_cov ? p.q[r] : 0, has_cov);
                nlo = g.node_lo[s]; nhi = g.k > 32 ? g.node_hi[s] : 0ull;
                seq = g.pool + g.e_off[e];
                fresh = false; body_init = true;
            }
            const u32 rel = (u32)(at - begin);                           // (a record is shorter than 2^32 bytes: the plan refuses others)
            char ch;
            if (rel < h.len) ch = hdr_byte(h, rel, has_cov);
            else {
                if (body_init) {                                         // one division per item; the bytes after it step
                    const u32 j = rel - h.len;
                    const u32 line = p.line_width ? j / (p.line_width + 1) : 0u;
                    col = j - line * (p.line_width + 1);
                    bi = j - line;
                    body_init = false;
                }
                if ((p.line_width && col == p.line_width) || bi == h.n) { ch = '\n'; col = 0; }
                else { ch = "AGCT"[path_base(nlo, nhi, seq, g.k, bi)]; bi++; col++; }
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
struct gk_contigs {
    gk_ctx *ctx = nullptr;
    gk_graph *g = nullptr;
    u64 epoch = 0;                       // the graph's when the plan was made: any edit since makes the plan stale
    u32 line_width = 0;
    u64 stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 records = 0, text_bytes = 0;
    // the plan, on the device: what the text is a pure function of
    u32 *d_id = nullptr;
    unsigned long long *d_off = nullptr;
    u64 *d_q = nullptr;
    TextStream ts;                       // the chunk buffers, made by the first read / write, and the times of the last one
};

namespace {

int contigs_live(const gk_contigs *c, const char *who) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null contigs handle");
    const hipError_t e = hipSetDevice(c->ctx->device);
    if (e != hipSuccess) return hip_fail(c->ctx, e, "hipSetDevice");
    if (c->g->epoch != c->epoch) return fail(c->ctx, GK_E_STATE, std::string(who) + ": the graph was edited after the plan was made");
    return GK_OK;
}

// the launch of k_contig_emit for bytes [t, t1) of the text (gk_fastaout.h: text_stream)
auto contigs_emit(gk_contigs *c) {
    return [c](u64 t, u64 t1, u64 items, uint8_t *out) {
        const ContigPlan plan{c->d_id, c->d_off, c->d_q, c->records, c->line_width};
        hipLaunchKernelGGL(k_contig_emit, dim3(ggrid(c->ctx, items)), dim3(BLOCK), 0, c->ctx->stream, c->g->v, plan, t, t1, out);
    };
}

}  // namespace

extern "C" {

void gk_contigs_destroy(gk_contigs *c) {
    if (!c) return;
    if (c->ctx) {
        (void)hipSetDevice(c->ctx->device);
        text_free_buffers(&c->ts);
        (void)pool_free(c->ctx, c->d_id);
        (void)pool_free(c->ctx, c->d_off);
        (void)pool_free(c->ctx, c->d_q);
    }
    delete c;
}

int gk_graph_contigs_plan(gk_graph *g, gk_map *counts, uint64_t min_len, uint32_t line_width, int strands, gk_contigs **out) {
    if (!out) return fail(g ? g->ctx : nullptr, GK_E_INVALID, "gk_graph_contigs_plan: out is NULL");
    *out = nullptr;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (strands != 1 && strands != 2) return fail(ctx, GK_E_INVALID, "gk_graph_contigs_plan: strands is 1 (one record per contig) or 2 (both strands)");
    if (line_width > 0x7fffffffu) return fail(ctx, GK_E_INVALID, "gk_graph_contigs_plan: line_width beyond 2^31-1");
    if (counts) { if (int rc = check_counts(g, counts, "gk_graph_contigs_plan")) return rc; }
    const GraphView &v = g->v;
    std::unique_ptr<gk_contigs, void (*)(gk_contigs *)> c(new gk_contigs, gk_contigs_destroy);
    c->ctx = ctx; c->ts.ctx = ctx; c->g = g; c->epoch = g->epoch; c->line_width = line_width;
    if (v.n_edges == 0) { *out = c.release(); return GK_OK; }
    const u64 ne = v.n_edges;
    DevScratch tmp(ctx);
    uint8_t *d_cls = nullptr, *d_want = nullptr;
    u32 *d_sel = nullptr, *d_size = nullptr;
    u64 *d_q = nullptr;
    unsigned long long *d_off = nullptr, *d_rank = nullptr, *d_stats = nullptr, h_stats[CS_N] = {}, h_records = 0, h_bytes = 0;
    tmp.get(&d_cls, ne);
    tmp.get(&d_want, ne);
    tmp.get(&d_sel, ne);
    tmp.get(&d_size, ne);
    tmp.get(&d_off, ne + 1);
    tmp.get(&d_rank, ne + 1);
    if (counts) tmp.get(&d_q, ne);
    tmp.zeroed(&d_stats, CS_N);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_contigs_plan: per-edge scratch");
    hipLaunchKernelGGL(k_contig_classify, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, (u64)min_len, (u32)line_width, strands, d_cls, d_want,
                       d_sel, d_size, d_stats);
    GK_HIP(ctx, hipGetLastError());
    if (counts) {
        EdgeCov cov{};
        if (int rc = coverage_pass(g, counts, tmp, d_want, &cov)) return rc;
        hipLaunchKernelGGL(k_contig_cov, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, v, cov, d_want, d_q, d_size, d_stats);
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, scan_counts(ctx, tmp, d_size, ne, d_off));
    GK_HIP(ctx, scan_counts(ctx, tmp, d_sel, ne, d_rank));
    GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}, {&h_records, d_rank + ne, 8}, {&h_bytes, d_off + ne, 8}}));
    if (h_stats[CS_OVERFLOW]) return fail(ctx, GK_E_CAPACITY, "gk_graph_contigs_plan: a record of 2^32 bytes or more");
    // the plan: (id, offset[, q]) per record
    tmp.get(&c->d_id, h_records);
    tmp.get(&c->d_off, h_records + 1);
    if (counts) tmp.get(&c->d_q, h_records);
    if (tmp.error() != hipSuccess) { c->d_id = nullptr; c->d_off = nullptr; c->d_q = nullptr; return hip_fail(ctx, tmp.error(), "gk_graph_contigs_plan: the plan"); }
    hipLaunchKernelGGL(k_contig_compact, dim3(ggrid(ctx, ne + 1)), dim3(BLOCK), 0, ctx->stream, ne, d_sel, d_rank, d_off, d_q, c->d_id, c->d_off, c->d_q);
    const hipError_t e = read_back(ctx, {});
    if (e != hipSuccess) { c->d_id = nullptr; c->d_off = nullptr; c->d_q = nullptr; return hip_fail(ctx, e, "gk_graph_contigs_plan: compaction"); }
    tmp.take(c->d_id);
    tmp.take(c->d_off);
    if (c->d_q) tmp.take(c->d_q);
    c->records = h_records; c->text_bytes = h_bytes;
    u64 *s = c->stats;
    s[1] = h_stats[CS_SHORT]; s[2] = h_stats[CS_FORWARD]; s[3] = h_stats[CS_SELF]; s[4] = h_stats[CS_REVERSE];
    s[0] = s[1] + s[2] + s[3] + s[4];
    s[5] = h_records; s[6] = h_stats[CS_BASES]; s[7] = h_bytes; s[8] = h_stats[CS_MISSING];
    *out = c.release();
    return GK_OK;
}

int gk_contigs_stats(const gk_contigs *c, uint64_t *stats9) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, "gk_contigs_stats: null contigs handle");
    if (!stats9) return fail(c->ctx, GK_E_INVALID, "gk_contigs_stats: stats9 is NULL");
    for (int i = 0; i < 9; i++) stats9[i] = c->stats[i];
    return GK_OK;
}

int gk_contigs_last_ms(const gk_contigs *c, float *ms4) {
    if (!c || !c->ctx) return fail(nullptr, GK_E_INVALID, "gk_contigs_last_ms: null contigs handle");
    if (!ms4) return fail(c->ctx, GK_E_INVALID, "gk_contigs_last_ms: ms4 is NULL");
    for (int i = 0; i < 4; i++) ms4[i] = c->ts.last_ms[i];
    return GK_OK;
}

int gk_contigs_read(gk_contigs *c, uint64_t offset, char *buf, uint64_t cap, uint64_t *n) {
    if (n) *n = 0;
    if (int rc = contigs_live(c, "gk_contigs_read")) return rc;
    gk_ctx *ctx = c->ctx;
    if (offset > c->text_bytes) return fail(ctx, GK_E_INVALID, "gk_contigs_read: the offset lies beyond the text");
    const u64 want = std::min<u64>(cap, c->text_bytes - offset);
    if (want && !buf) return fail(ctx, GK_E_INVALID, "gk_contigs_read: buf is NULL");
    u64 done = 0;
    bool sink_failed = false;
    if (int rc = text_stream(&c->ts, c->text_bytes, offset, want, "gk_contigs", contigs_emit(c), [&](const char *p, u64 m) { std::memcpy(buf + done, p, m); done += m; return true; }, &sink_failed)) return rc;
    if (n) *n = done;
    return GK_OK;
}

int gk_contigs_write(gk_contigs *c, const char *path) {
    if (int rc = contigs_live(c, "gk_contigs_write")) return rc;
    gk_ctx *ctx = c->ctx;
    if (!path) return fail(ctx, GK_E_INVALID, "gk_contigs_write: path is NULL");
    return text_write_file(&c->ts, c->text_bytes, path, "gk_contigs", "gk_contigs_write", contigs_emit(c));
}

}  // extern "C"
