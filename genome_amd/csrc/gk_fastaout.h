// gk_fastaout.h — what the two FASTA writers share (gk_contigs.hip: one record per edge; gk_scaffolds.hip: one record per chain).
// Device: the decimal digits of a header, the ">e<id> len=<n>" header of an edge's record, the size of a wrapped body and base i
// of an edge's path.  Host: TextStream, the chunked double-buffered way a text that a kernel emits by byte range reaches a sink.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <string>

#include "gk_graph.h"

// ---------------------------------------------------------------------------------------------
// the text of one record, from its numbers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int dec_digits(u64 v) {
    int d = 1;
    while (v >= 10) { v /= 10; d++; }
    return d;
}
// digit `pos` (0 = the most significant) of v, which has ndig digits
__device__ __forceinline__ char dec_digit_at(u64 v, int ndig, int pos) {
    for (int i = ndig - 1 - pos; i > 0; i--) v /= 10;
    return (char)('0' + (int)(v % 10));
}
// ">e<id> len=<n>[ cov=<q/100>.<q%100, two digits>]\n"
struct RecHdr {
    u64 id, n, q;
    int di, dn, dq;
    u32 len;
};
__device__ __forceinline__ RecHdr rec_hdr(u64 id, u64 n, u64 q, bool has_cov) {
    RecHdr h;
    h.id = id; h.n = n; h.q = q;
    h.di = dec_digits(id); h.dn = dec_digits(n); h.dq = has_cov ? dec_digits(q / 100) : 0;
    h.len = (u32)(2 + h.di + 5 + h.dn + (has_cov ? 5 + h.dq + 3 : 0) + 1);
    return h;
}
__device__ __forceinline__ char hdr_byte(const RecHdr &h, u32 p, bool has_cov) {
    if (p < 2) return p ? 'e' : '>';
    p -= 2;
    if (p < (u32)h.di) return dec_digit_at(h.id, h.di, (int)p);
    p -= (u32)h.di;
    if (p < 5) return " len="[p];
    p -= 5;
    if (p < (u32)h.dn) return dec_digit_at(h.n, h.dn, (int)p);
    p -= (u32)h.dn;
    if (has_cov) {
        if (p < 5) return " cov="[p];
        p -= 5;
        if (p < (u32)h.dq) return dec_digit_at(h.q / 100, h.dq, (int)p);
        p -= (u32)h.dq;
        if (p == 0) return '.';
        if (p == 1) return (char)('0' + (int)(h.q % 100) / 10);
        if (p == 2) return (char)('0' + (int)(h.q % 10));
    }
    return '\n';
}
// the n bases and their line ends: a '\n' after every line_width bases (0: none) and after the last base, never two in a row
__device__ __forceinline__ u64 body_bytes(u64 n, u32 line_width) { return n + (line_width ? (n + line_width - 1) / line_width : 1); }
// base i of the path start k-mer ++ seq
__device__ __forceinline__ int path_base(u64 nlo, u64 nhi, const uint8_t *__restrict__ seq, int k, u64 i) {
    if (i >= (u64)k) return pool_get(seq, 0, i - (u64)k);
    return (int)((i < 32 ? nlo >> (2 * i) : nhi >> (2 * (i - 32))) & 3);
}

// The contigs' classes (include/genome_amd.h, "contigs": short, then forward / self_twin / reverse by comparing the path with its
// reverse complement), shared by the contig plan (gk_contigs.hip) and the multi-k seeding (gk_multik.hip).
static constexpr uint8_t CLS_DEAD = 0, CLS_SHORT = 1, CLS_FORWARD = 2, CLS_SELF = 3, CLS_REVERSE = 4;
// the class of LIVE edge e, by one wave: every lane of the wave calls it with the same e and gets the answer; 64 bases of each
// strand per step, it stops at the first difference
__device__ __forceinline__ uint8_t wave_contig_class(const GraphView &g, u64 e, u64 min_len) {
    const int lane = threadIdx.x & 63;
    const u64 n = (u64)g.k + g.e_len[e];
    if (n < min_len) return CLS_SHORT;
    const u32 s = g.e_start[e];
    const u64 nlo = g.node_lo[s], nhi = g.k > 32 ? g.node_hi[s] : 0ull;
    const uint8_t *seq = g.pool + g.e_off[e];
    const u64 half = (n + 1) / 2;                            // (an odd n differs at its middle base at the latest: 3 - b != b)
    for (u64 i0 = 0; i0 < half; i0 += 64) {
        const u64 i = i0 + (u64)lane;
        int a = 0, b = 0;
        if (i < half) { a = path_base(nlo, nhi, seq, g.k, i); b = 3 - path_base(nlo, nhi, seq, g.k, n - 1 - i); }
        const unsigned long long differ = __ballot(a != b);
        if (differ) return __shfl(a < b ? 1 : 0, __ffsll((long long)differ) - 1) ? CLS_FORWARD : CLS_REVERSE;
    }
    return CLS_SELF;
}

// ---------------------------------------------------------------------------------------------
// host side: a text emitted by byte range, streamed to a sink
// ---------------------------------------------------------------------------------------------
namespace {

constexpr u64 TEXT_CHUNK_DEFAULT = 64ull << 20;

// text bytes per device chunk: a multiple of 8, the "contigs_chunk_bytes" switch or 64 MiB
inline u64 text_chunk(const gk_ctx *ctx) {
    const u64 c = ctx->hook_contigs_chunk > 0 ? (u64)ctx->hook_contigs_chunk : TEXT_CHUNK_DEFAULT;
    return std::max<u64>(8, c & ~(u64)7);
}

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// two device chunks and two pinned staging buffers of buf_bytes each, made by the first read / write of a plan
struct TextStream {
    gk_ctx *ctx = nullptr;
    uint8_t *d_buf[2] = {nullptr, nullptr};
    void *h_buf[2] = {nullptr, nullptr};
    hipEvent_t ev_k0[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr};      // a chunk's kernel begins / ends, its copy has landed
    u64 buf_bytes = 0;
    float last_ms[4] = {0, 0, 0, 0};     // the last read / write: emit kernels (device events), waits for copies, the sink, the whole call
};

inline void text_free_buffers(TextStream *c) {
    for (int i = 0; i < 2; i++) {
        if (c->ev_k0[i]) { (void)hipEventSynchronize(c->ev_k0[i]); (void)hipEventDestroy(c->ev_k0[i]); c->ev_k0[i] = nullptr; }
        if (c->ev_k[i]) { (void)hipEventSynchronize(c->ev_k[i]); (void)hipEventDestroy(c->ev_k[i]); c->ev_k[i] = nullptr; }
        if (c->ev_c[i]) { (void)hipEventSynchronize(c->ev_c[i]); (void)hipEventDestroy(c->ev_c[i]); c->ev_c[i] = nullptr; }
        if (c->d_buf[i]) { (void)pool_free(c->ctx, c->d_buf[i]); c->d_buf[i] = nullptr; }
        if (c->h_buf[i]) { (void)gk_host_free(c->ctx, c->h_buf[i]); c->h_buf[i] = nullptr; }
    }
    c->buf_bytes = 0;
}

// the chunk buffers for pieces of at most `chunk` bytes of a text of text_bytes (a piece may start up to 7 bytes into its first word)
inline int text_buffers(TextStream *c, u64 text_bytes, u64 chunk, const char *who) {
    gk_ctx *ctx = c->ctx;
    const u64 want = std::min(chunk, (text_bytes + 7) & ~(u64)7) + 8;
    if (c->buf_bytes == want) return GK_OK;
    text_free_buffers(c);
    for (int i = 0; i < 2; i++) {
        const hipError_t e = pool_malloc(ctx, &c->d_buf[i], want);
        if (e != hipSuccess) { (void)hipGetLastError(); text_free_buffers(c); return hip_fail(ctx, e, (std::string(who) + ": device chunk").c_str()); }
        if (int rc = gk_host_alloc(ctx, want, &c->h_buf[i])) { text_free_buffers(c); return rc; }
        hipError_t e2 = hipEventCreate(&c->ev_k0[i]);
        if (e2 == hipSuccess) e2 = hipEventCreate(&c->ev_k[i]);
        if (e2 == hipSuccess) e2 = hipEventCreateWithFlags(&c->ev_c[i], hipEventDisableTiming);
        if (e2 != hipSuccess) { text_free_buffers(c); return hip_fail(ctx, e2, (std::string(who) + ": events").c_str()); }
    }
    c->buf_bytes = want;
    return GK_OK;
}

// Bytes [offset, offset + n) of a text of text_bytes through `sink`, in order, in pieces of at most the chunk size.  `emit(t, t1,
// items, out)` launches, on the context's stream, the kernel that writes bytes [t, t1) to `out` (8-byte aligned; text byte x at
// out[x - (t & ~7)]) in `items` work items: the bytes before the first whole word, the whole words, the bytes after the last.
// Piece i + 1 is emitted on the context's stream while piece i is copied to its pinned buffer on the copy stream and handed to the
// sink.  A sink that returns false ends the stream (*sink_failed).
template <class Emit, class Sink> int text_stream(TextStream *c, u64 text_bytes, u64 offset, u64 n, const char *who, Emit &&emit, Sink &&sink, bool *sink_failed) {
    gk_ctx *ctx = c->ctx;
    *sink_failed = false;
    for (float &m : c->last_ms) m = 0;
    if (n == 0) return GK_OK;
    const double t_call = now_ms();
    double t_wait = 0, t_sink = 0;
    float t_kernels = 0;
    const u64 chunk = text_chunk(ctx);
    if (int rc = text_buffers(c, text_bytes, chunk, who)) return rc;
    // pieces end on multiples of the chunk size in the text, so that all but the first start on a word
    const u64 end = offset + n;
    auto piece_end = [&](u64 t) { return std::min(end, (t / chunk + 1) * chunk); };
    auto issue = [&](u64 t, int slot) -> hipError_t {
        const u64 t1 = piece_end(t);
        const u64 a0 = std::min(t1, (t + 7) & ~(u64)7), a1 = std::max(a0, t1 & ~(u64)7);
        hipError_t e = hipEventRecord(c->ev_k0[slot], ctx->stream);
        if (e != hipSuccess) return e;
        emit(t, t1, (a0 - t) + ((a1 - a0) >> 3) + (t1 - a1), c->d_buf[slot]);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(c->ev_k[slot], ctx->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, c->ev_k[slot], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(c->h_buf[slot], c->d_buf[slot] + (t & 7), t1 - t, hipMemcpyDeviceToHost, ctx->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(c->ev_c[slot], ctx->copy_stream);
        ctx->copy_other_pending = true;                      // (the copy stream reads a pooled block: pool_free waits for it)
        return e;
    };
    hipError_t he = issue(offset, 0);
    int slot = 0;
    for (u64 t = offset; t < end && he == hipSuccess; slot ^= 1) {
        const u64 t1 = piece_end(t);
        if (t1 < end) he = issue(t1, slot ^ 1);
        if (he != hipSuccess) break;
        double t_ = now_ms();
        he = hipEventSynchronize(c->ev_c[slot]);
        t_wait += now_ms() - t_;
        float k_ms = 0;
        if (he == hipSuccess) he = hipEventElapsedTime(&k_ms, c->ev_k0[slot], c->ev_k[slot]);
        if (he != hipSuccess) break;
        t_kernels += k_ms;
        t_ = now_ms();
        const bool ok = sink((const char *)c->h_buf[slot], t1 - t);
        t_sink += now_ms() - t_;
        if (!ok) { *sink_failed = true; break; }
        t = t1;
    }
    // nothing of this call is left in flight, whatever ended the loop
    const hipError_t e1 = hipStreamSynchronize(ctx->stream), e2 = hipStreamSynchronize(ctx->copy_stream);
    if (he == hipSuccess) he = e1 != hipSuccess ? e1 : e2;
    if (he != hipSuccess) return hip_fail(ctx, he, (std::string(who) + ": emit").c_str());
    c->last_ms[0] = t_kernels; c->last_ms[1] = (float)t_wait; c->last_ms[2] = (float)t_sink; c->last_ms[3] = (float)(now_ms() - t_call);
    return GK_OK;
}

inline bool write_all(int fd, const char *p, u64 n) {
    while (n) {
        const ssize_t w = ::write(fd, p, std::min<u64>(n, 1ull << 30));
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (u64)w;
    }
    return true;
}

inline int sys_fail(gk_ctx *ctx, const std::string &what, const std::string &path) {
    return fail(ctx, GK_E_INVALID, what + " " + path + ": " + std::strerror(errno));
}

// the whole text to `path`, through path + ".tmp" and a rename: a failed write leaves nothing at path
template <class Emit> int text_write_file(TextStream *c, u64 text_bytes, const char *path, const char *stream_who, const char *who, Emit &&emit) {
    gk_ctx *ctx = c->ctx;
    const std::string w(who), p(path), tmp = p + ".tmp";
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return sys_fail(ctx, w + ": cannot open", tmp);
    bool sink_failed = false;
    int en = 0;
    const int rc = text_stream(c, text_bytes, 0, text_bytes, stream_who, emit, [&](const char *q, u64 m) { if (write_all(fd, q, m)) return true; en = errno; return false; }, &sink_failed);
    if (::close(fd) != 0 && !sink_failed) { sink_failed = true; en = errno; }
    if (rc) { ::unlink(tmp.c_str()); return rc; }
    if (sink_failed) { ::unlink(tmp.c_str()); errno = en; return sys_fail(ctx, w + ": cannot write", tmp); }
    if (std::rename(tmp.c_str(), p.c_str()) != 0) { en = errno; ::unlink(tmp.c_str()); errno = en; return sys_fail(ctx, w + ": cannot rename to", p); }
    return GK_OK;
}

}  // namespace
