// gk_fastq.hip — FASTQ text to `.bin` read records on the device: Convert2bin (S/scripts/Convert2bin.scala:25-87), and the same
// parse feeding the k-mer count straight from HBM.  The conversion rules, with this converter's deviations, are in
// include/genome_amd.h ("FASTQ").
//
// One device chunk = the bytes carried from the last chunk (an incomplete record) + the next slice of the caller's text:
//   k_fq_terms (pass 0)     a workgroup per 16 KiB tile, staged in LDS with 16-byte loads: terminator bytes counted by ballot
//   scan_counts             tile counts -> tile offsets (gk_scan.h); the host reads the line count
//   k_fq_terms (pass 1)     the same tiles write their terminator positions (ballot + popcount compaction): E[line] = end of line
//   k_fq_plan               one lane: the records this chunk completes, the ones it emits, where the carry starts, end-of-input rules
//   k_fq_records            one wave per record: sequence / quality bounds from E, first non-ACGT base of each half by ballot,
//                           bytes >= 0x80, mate lengths; the first bad record by atomicMin
//   k_fq_pairs              one lane per pair: bytes and windows per mate, statistics (pairs after the first bad record emit nothing)
//   scan_counts             bytes per mate -> output offsets (and windows per mate -> window prefix, count path)
//   k_fq_pack               one wave per mate: length byte + ceil(len/4) bytes of 2-bit codes, u32 offset table
// The host learns the chunk's last complete record from the line count (4 lines per record) — it never scans the text — and
// the tail from there on is copied device to device in front of the next slice, which is uploaded on the copy stream beside
// this chunk's kernels.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "gk_text.h"

namespace {

constexpr u64 FQ_MAX_RECORD = 64ull << 20;              // one record's text at most (a deliberate limit; GK_E_FORMAT beyond)
constexpr u64 FQ_SLICE_DEFAULT = 128ull << 20;          // text bytes uploaded per device chunk
constexpr u64 FQ_HEAD_MIN = 1ull << 20;                 // room in front of a slice for the carried tail (grows on demand)
constexpr u64 FQ_NO_ERR = ~0ull;

// error kinds, low 3 bits of the error word (record << 3 | kind): the smallest record wins, then the smallest kind
enum : u32 { FE_LONG = 1, FE_HIGH = 2, FE_BIG = 3, FE_TAIL = 4, FE_ODD = 5 };
const char *fq_err_text(u32 kind) {
    switch (kind) {
        case FE_LONG: return "a mate longer than 255 bases (the .bin length byte cannot hold it)";
        case FE_HIGH: return "a byte >= 0x80 in a sequence or quality line (the converter reads ASCII only)";
        case FE_BIG: return "a record of more than 64 MiB of text";
        case FE_TAIL: return "the input ends inside a record (2 or 3 of its 4 lines)";
        case FE_ODD: return "interleaved input ends with an odd number of records (the last has no mate)";
    }
    return "malformed record";
}

struct FqPlan {                  // k_fq_plan -> host
    u64 lines;                   // lines of the chunk (a non-empty unterminated tail at end of input included)
    u64 recs;                    // complete records
    u64 recs_emit;               // of them, the ones whose pairs this chunk emits
    u64 carry_start;             // first byte not consumed by this chunk
};
struct FqSum {                   // per chunk: the first error, and the emitted pairs' statistics
    unsigned long long err;
    unsigned long long pairs, short_pairs, kmers;
};
struct FqHost {                  // pinned landing area of the per-chunk reads
    unsigned long long terms;
    FqPlan plan;
    FqSum sum;
    unsigned long long out_bytes, windows;
};

__device__ __forceinline__ bool fq_acgt(u32 c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
__device__ __forceinline__ u32 fq_code(u32 c) { return c == 'G' ? 1u : c == 'C' ? 2u : c == 'T' ? 3u : 0u; }     // A0 G1 C2 T3

// one lane: which records the chunk completes and emits, and the end-of-input rules (Convert2bin.scala:51-73)
__global__ void k_fq_plan(const uint8_t *__restrict__ T, u64 n, u32 *__restrict__ E, u64 terms, int last, int interleaved, u64 rec_base,
                          FqPlan *__restrict__ plan, FqSum *__restrict__ sum) {
    u64 L = terms;
    // a '\r' that is the chunk's last byte may be the first half of a "\r\n" whose '\n' has not arrived: that line is not complete
    if (!last && L > 0 && E[L - 1] == n - 1 && T[n - 1] == '\r') L--;
    if (last && fq_line_start(T, n, E, L) < n) E[L++] = (u32)n;          // a non-empty unterminated tail is a line
    const u64 R = L / 4;
    u64 err = FQ_NO_ERR;
    u64 Re = interleaved ? (R & ~1ull) : R;
    if (last) {
        if (L % 4 >= 2) err = ((rec_base + R) << 3) | FE_TAIL;               // (a lone header line is ignored: L % 4 == 1)
        if (interleaved && (R & 1)) err = umin(err, ((rec_base + R - 1) << 3) | FE_ODD);
    } else {
        const u64 partial = fq_line_start(T, n, E, 4 * R);
        if (n - partial > FQ_MAX_RECORD) err = umin(err, ((rec_base + R) << 3) | FE_BIG);
    }
    plan->lines = L;
    plan->recs = R;
    plan->recs_emit = Re;
    plan->carry_start = last ? n : fq_line_start(T, n, E, 4 * Re);
    sum->err = err;
    sum->pairs = sum->short_pairs = sum->kmers = 0;
}

// the first non-ACGT position of [a, a + lim), lim <= 256; lim if none (one wave, ballot per 64 bytes)
__device__ __forceinline__ u32 fq_mate_len(const uint8_t *__restrict__ T, u64 a, u32 lim, int lane) {
    for (u32 o = 0; o < lim; o += 64) {
        const u32 i = o + lane;
        const unsigned long long bad = __ballot(i < lim && !fq_acgt(T[a + i]));
        if (bad) return o + (u32)(__ffsll((long long)bad) - 1);
    }
    return lim;
}
__device__ __forceinline__ bool fq_any_high(const uint8_t *__restrict__ T, u64 a, u64 b, int lane) {
    bool hi = false;
    for (u64 x = a + lane; x < b; x += 64) hi |= T[x] >= 0x80;
    return __ballot(hi) != 0;
}

// one wave per complete record: lines 4r .. 4r+3 = header, sequence, separator, quality (header and separator not inspected)
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_records(const uint8_t *__restrict__ T, u64 n, const u32 *__restrict__ E, u64 R, int split_at,
                                                          u64 rec_base, u32 *__restrict__ mlen, u32 *__restrict__ mstart, FqSum *__restrict__ sum) {
    const u64 r = (u64)blockIdx.x * (FQ_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    const u64 l0 = 4 * r;
    const u64 hs = fq_line_start(T, n, E, l0), ss = fq_line_start(T, n, E, l0 + 1), se = E[l0 + 1];
    const u64 qs = fq_line_start(T, n, E, l0 + 3), qe = umin(E[l0 + 3], n), rend = fq_line_start(T, n, E, l0 + 4);
    const u64 slen = se - ss, qlen = qe - qs;
    u32 kind = 0;
    u32 len[2] = {0, 0};
    u64 st[2] = {ss, ss};
    if (rend - hs > FQ_MAX_RECORD) kind = FE_BIG;         // (its lines are not scanned)
    else {
        if (fq_any_high(T, ss, se, lane) || fq_any_high(T, qs, qe, lane)) kind = FE_HIGH;
        // mates: splitAt(split_at) of both lines (:59, :61); the mate = takeWhile ACGT over zip(sequence half, quality half) (:40-49)
        const u64 h1s = split_at ? umin(split_at, slen) : slen, h1q = split_at ? umin(split_at, qlen) : qlen;
        const u64 cap[2] = {umin(h1s, h1q), umin(slen - h1s, qlen - h1q)};
        st[1] = ss + h1s;
        const int nm = split_at ? 2 : 1;
        for (int h = 0; h < nm; h++) {
            len[h] = fq_mate_len(T, st[h], (u32)umin(cap[h], 256), lane);
            if (len[h] > 255) { len[h] = 255; if (!kind) kind = FE_LONG; }
        }
    }
    if (lane == 0) {
        if (split_at) {
            mlen[2 * r] = len[0]; mstart[2 * r] = (u32)st[0];
            mlen[2 * r + 1] = len[1]; mstart[2 * r + 1] = (u32)st[1];
        } else {
            mlen[r] = len[0]; mstart[r] = (u32)st[0];
        }
        if (kind) atomicMin(&sum->err, ((rec_base + r) << 3) | kind);
    }
}

__device__ __forceinline__ u64 fq_wave_sum(u64 v) {
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// one lane per pair (mates 2p, 2p+1): a pair is emitted when all its records precede the first bad one and it is among the first
// max_pairs of the input; bytes per mate = 1 + ceil(len/4) (0 if not emitted), windows for the map's k, statistics for k_stats
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_pairs(u64 npairs, const u32 *__restrict__ mlen, int recs_per_pair, u64 rec_base, u64 pair_base,
                                                        u64 max_pairs, int k_stats, int k_map, u32 *__restrict__ bytes, u32 *__restrict__ win,
                                                        FqSum *__restrict__ sum) {
    __shared__ u64 s_red[3][FQ_BLOCK / 64];
    const u64 p = (u64)blockIdx.x * FQ_BLOCK + threadIdx.x;
    const u64 err_rec = sum->err >> 3;
    u64 pairs = 0, shorts = 0, kmers = 0;
    if (p < npairs) {
        const u64 last_rec = rec_base + (p + 1) * recs_per_pair - 1;
        const bool emit = last_rec < err_rec && (max_pairs == 0 || pair_base + p < max_pairs);
        const u32 l1 = mlen[2 * p], l2 = mlen[2 * p + 1];
        bytes[2 * p] = emit ? 1 + (l1 + 3) / 4 : 0;
        bytes[2 * p + 1] = emit ? 1 + (l2 + 3) / 4 : 0;
        if (win) {
            win[2 * p] = emit && (int)l1 >= k_map ? l1 - k_map + 1 : 0;
            win[2 * p + 1] = emit && (int)l2 >= k_map ? l2 - k_map + 1 : 0;
        }
        if (emit) {
            pairs = 1;
            shorts = ((int)l1 < k_stats || (int)l2 < k_stats) ? 1 : 0;
            kmers = ((int)l1 >= k_stats ? l1 - k_stats + 1 : 0) + ((int)l2 >= k_stats ? l2 - k_stats + 1 : 0);
        }
    }
    pairs = fq_wave_sum(pairs); shorts = fq_wave_sum(shorts); kmers = fq_wave_sum(kmers);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_red[0][wave] = pairs; s_red[1][wave] = shorts; s_red[2][wave] = kmers; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const u64 v = s_red[threadIdx.x][0] + s_red[threadIdx.x][1] + s_red[threadIdx.x][2] + s_red[threadIdx.x][3];
        if (v) atomicAdd(threadIdx.x == 0 ? &sum->pairs : threadIdx.x == 1 ? &sum->short_pairs : &sum->kmers, (unsigned long long)v);
    }
}

// one wave per mate: [len:u8] + ceil(len/4) bytes, 2-bit codes LSB-first (Convert2bin.scala:35-38); off32 = the u32 offset table
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_pack(const uint8_t *__restrict__ T, u64 nm, const u32 *__restrict__ mlen, const u32 *__restrict__ mstart,
                                                       const u32 *__restrict__ bytes, const unsigned long long *__restrict__ off64,
                                                       uint8_t *__restrict__ out, u64 out_cap, u32 *__restrict__ off32) {
    const u64 m = (u64)blockIdx.x * (FQ_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= nm) return;
    const u64 o = off64[m];
    if (lane == 0) {
        off32[m] = (u32)o;
        if (m == nm - 1) off32[nm] = (u32)off64[nm];
    }
    if (!bytes[m] || o + bytes[m] > out_cap) return;      // (cannot happen: every record writes at most its text's bytes)
    const u32 len = mlen[m];
    const u64 a = mstart[m];
    if (lane == 0) out[o] = (uint8_t)len;
    if ((u32)lane < (len + 3) / 4) {
        u32 v = 0;
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const u32 i = 4 * lane + j;
            if (i < len) v |= fq_code(T[a + i]) << (2 * j);
        }
        out[o + 1 + lane] = (uint8_t)v;
    }
}

// batch boundaries of the count path: b[j] = first mate whose window prefix reaches j * per (b[0] = 0, b[nb] = nm), with the prefix
__global__ void k_fq_cut(const unsigned long long *__restrict__ wpre, u64 nm, u64 per, u64 nb, unsigned long long *__restrict__ cut) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nb) return;
    u64 b;
    if (j == 0) b = 0;
    else if (j == nb) b = nm;
    else {
        u64 lo = 0, hi = nm;
        const u64 want = j * per;
        while (lo < hi) { const u64 mid = (lo + hi) / 2; if (wpre[mid] < want) lo = mid + 1; else hi = mid; }
        b = lo;
    }
    cut[2 * j] = b;
    cut[2 * j + 1] = wpre[b];
}


}  // namespace

struct gk_fastq {
    gk_ctx *ctx = nullptr;
    int split_at = 36, k_stats = 23;
    u64 max_pairs = 0;
    bool failed = false, finished = false;
    // text: two device buffers of [head | slice | slack]; the carried tail sits right in front of the slice
    uint8_t *buf[2] = {nullptr, nullptr};
    u64 head[2] = {0, 0}, slice_cap[2] = {0, 0};
    int cur = 0;
    u64 carry = 0;
    // the slice already on its way into buf[b] (prefetched by the previous chunk of the same call)
    const char *pf_src[2] = {nullptr, nullptr};
    u64 pf_bytes[2] = {0, 0};
    TextUpload up;                                // the copy-stream upload into buf[b] (gk_text.h)
    bool up_timed[2] = {false, false};
    // parse scratch (pooled, grown on demand)
    u32 *d_tile_cnt = nullptr; size_t tile_cap = 0;
    unsigned long long *d_tile_off = nullptr; size_t tile_off_cap = 0;
    u64 *d_scan = nullptr; size_t scan_cap = 0;
    u32 *d_E = nullptr; size_t e_cap = 0;
    u32 *d_mlen = nullptr, *d_mstart = nullptr, *d_bytes = nullptr, *d_win = nullptr, *d_off32 = nullptr;
    unsigned long long *d_off64 = nullptr, *d_wpre = nullptr;
    size_t mate_cap = 0;                          // entries of every per-mate array
    unsigned long long *d_cut = nullptr; size_t cut_cap = 0;
    uint8_t *d_out = nullptr; size_t out_cap = 0;
    FqPlan *d_plan = nullptr;
    FqSum *d_sum = nullptr;
    FqHost *h = nullptr;
    // statistics
    u64 pairs = 0, short_pairs = 0, kmers = 0, text_bytes = 0, records = 0, pairs_seen = 0;
    float ms[4] = {0, 0, 0, 0};
};

namespace {

template <class T>
int fq_grow(gk_ctx *ctx, T **p, size_t *cap, size_t want) {
    if (*cap >= want && *p) return GK_OK;
    want = std::max(want, *cap + *cap / 2);
    if (*p) GK_HIP(ctx, pool_free(ctx, *p));
    *p = nullptr;
    *cap = 0;
    GK_HIP(ctx, pool_malloc(ctx, p, want * sizeof(T)));
    *cap = want;
    return GK_OK;
}

// every per-mate array holds at least `want` entries
int fq_mates(gk_fastq *fq, size_t want) {
    gk_ctx *ctx = fq->ctx;
    if (fq->mate_cap >= want) return GK_OK;
    want = std::max(want, fq->mate_cap + fq->mate_cap / 2);
    u32 **a32[] = {&fq->d_mlen, &fq->d_mstart, &fq->d_bytes, &fq->d_win, &fq->d_off32};
    unsigned long long **a64[] = {&fq->d_off64, &fq->d_wpre};
    fq->mate_cap = 0;
    for (u32 **p : a32) { if (*p) GK_HIP(ctx, pool_free(ctx, *p)); *p = nullptr; }
    for (unsigned long long **p : a64) { if (*p) GK_HIP(ctx, pool_free(ctx, *p)); *p = nullptr; }
    for (u32 **p : a32) GK_HIP(ctx, pool_malloc(ctx, p, want * sizeof(u32)));
    for (unsigned long long **p : a64) GK_HIP(ctx, pool_malloc(ctx, p, want * sizeof(unsigned long long)));
    fq->mate_cap = want;
    return GK_OK;
}

u64 fq_slice(const gk_fastq *fq) { return fq->ctx->hook_fastq_chunk > 0 ? (u64)fq->ctx->hook_fastq_chunk : FQ_SLICE_DEFAULT; }

// buffer b must take `carry` bytes in front of a slice of `slice` bytes; a re-allocation drops whatever was prefetched into it
// and, with keep, moves the carried tail that already sits in front of the old slice
int fq_text_buffer(gk_fastq *fq, int b, u64 carry, u64 slice, bool keep) {
    gk_ctx *ctx = fq->ctx;
    if (fq->buf[b] && fq->head[b] >= carry + 64 && fq->slice_cap[b] >= slice) return GK_OK;
    const u64 head = std::max<u64>(std::max<u64>(fq->head[b], FQ_HEAD_MIN), pow2ceil(carry + 64));
    const u64 sl = std::max<u64>(fq->slice_cap[b], slice);
    GK_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    uint8_t *nbuf = nullptr;
    GK_HIP(ctx, pool_malloc(ctx, &nbuf, head + sl + 64));
    if (keep && carry && fq->buf[b])
        GK_HIP(ctx, hipMemcpyAsync(nbuf + head - carry, fq->buf[b] + fq->head[b] - carry, carry, hipMemcpyDeviceToDevice, ctx->stream));
    if (fq->buf[b]) GK_HIP(ctx, pool_free(ctx, fq->buf[b]));       // (waits for the context's streams: the move has landed)
    fq->buf[b] = nbuf; fq->head[b] = head; fq->slice_cap[b] = sl; fq->pf_src[b] = nullptr;
    return GK_OK;
}

// text [src, src + bytes) on its way to buf[b] + head[b], and remembered: the chunk that wants exactly this slice finds it there
int fq_prefetch(gk_fastq *fq, int b, const char *src, u64 bytes, bool pinned, double *host_ms) {
    fq->pf_src[b] = src; fq->pf_bytes[b] = bytes;
    fq->up_timed[b] = false;
    if (!bytes) return GK_OK;
    if (int rc = fq->up.upload(fq->ctx, b, fq->buf[b] + fq->head[b], src, bytes, pinned, host_ms)) return rc;
    fq->up_timed[b] = true;
    return GK_OK;
}

int fq_fail(gk_fastq *fq, int code, const std::string &msg) {
    fq->failed = true;
    return fail(fq->ctx, code, msg);
}

// the shared body of gk_fastq_convert / gk_fastq_count: every completed pair goes to `sink` (host buffer or map)
int fq_run(gk_fastq *fq, const char *text, size_t nbytes, int last, uint8_t *bin_out, size_t *bin_bytes, gk_map *m, uint64_t *occ_out) {
    gk_ctx *ctx = fq->ctx;
    const auto t_call = clk::now();
    double up_ms = 0, kern_ms = 0, sink_ms = 0;
    const bool pinned = nbytes && TextUpload::is_pinned(text);
    const u64 slice_max = fq_slice(fq);
    u64 pos = 0;
    size_t written = 0;
    int rc = GK_OK;
    if (m) { if ((rc = map_count_begin(m))) return fq_fail(fq, rc, ctx->err); }
    const TimedSection kt{ctx};
    do {
        const u64 slice = std::min<u64>(nbytes - pos, slice_max);
        const bool is_last = last && pos + slice == nbytes;
        const int b = fq->cur;
        if ((rc = fq_text_buffer(fq, b, fq->carry, slice, true))) return fq_fail(fq, rc, ctx->err);
        if (!(fq->pf_src[b] == text + pos && fq->pf_bytes[b] == slice)) {
            if ((rc = fq_prefetch(fq, b, text + pos, slice, pinned, &up_ms))) return fq_fail(fq, rc, ctx->err);
        }
        fq->pf_src[b] = nullptr;
        if (fq->up_timed[b]) GK_HIP(ctx, hipStreamWaitEvent(ctx->stream, fq->up.up1[b], 0));
        const u64 n = fq->carry + slice;
        const uint8_t *T = fq->buf[b] + fq->head[b] - fq->carry;
        // ---- line ends
        const u64 ntiles = (n + FQ_TILE - 1) / FQ_TILE;
        if ((rc = fq_grow(ctx, &fq->d_tile_cnt, &fq->tile_cap, ntiles + 1)) || (rc = fq_grow(ctx, &fq->d_tile_off, &fq->tile_off_cap, ntiles + 2)) ||
            (rc = fq_grow(ctx, &fq->d_scan, &fq->scan_cap, (size_t)(n / (2 * SCAN_CHUNK) + 4))))
            return fq_fail(fq, rc, ctx->err);
        GK_HIP(ctx, kt.start());
        if (ntiles) hipLaunchKernelGGL((k_fq_terms<0>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, fq->d_tile_cnt, nullptr, nullptr);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, fq->d_tile_cnt, ntiles, fq->d_tile_off, fq->d_scan));
        GK_HIP(ctx, hipMemcpyAsync(&fq->h->terms, fq->d_tile_off + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = kt.end(&kern_ms))) return fq_fail(fq, rc, ctx->err);
        const u64 terms = fq->h->terms;
        if (fq->up_timed[b]) {
            float t = 0;
            GK_HIP(ctx, hipEventElapsedTime(&t, fq->up.up0[b], fq->up.up1[b]));
            up_ms += t;
            fq->up_timed[b] = false;
        }
        // (the next slice of this call goes up beside the rest of this chunk: its buffer is free, its head region is written last)
        const u64 next_pos = pos + slice, next_slice = std::min<u64>(nbytes - next_pos, slice_max);
        if ((rc = fq_grow(ctx, &fq->d_E, &fq->e_cap, terms + 2))) return fq_fail(fq, rc, ctx->err);
        GK_HIP(ctx, kt.start());
        if (ntiles) hipLaunchKernelGGL((k_fq_terms<1>), dim3((unsigned)ntiles), dim3(FQ_BLOCK), 0, ctx->stream, T, n, nullptr, fq->d_tile_off, fq->d_E);
        hipLaunchKernelGGL(k_fq_plan, dim3(1), dim3(1), 0, ctx->stream, T, n, fq->d_E, terms, is_last ? 1 : 0, fq->split_at ? 0 : 1, fq->records,
                           fq->d_plan, fq->d_sum);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, hipMemcpyAsync(&fq->h->plan, fq->d_plan, sizeof(FqPlan), hipMemcpyDeviceToHost, ctx->stream));
        if (next_slice && fq->buf[1 - b] && fq->slice_cap[1 - b] >= next_slice) {
            if ((rc = fq_prefetch(fq, 1 - b, text + next_pos, next_slice, pinned, &up_ms))) return fq_fail(fq, rc, ctx->err);
        }
        if ((rc = kt.end(&kern_ms))) return fq_fail(fq, rc, ctx->err);
        const FqPlan plan = fq->h->plan;
        // ---- records, pairs, offsets, pack
        const u64 npairs = fq->split_at ? plan.recs_emit : plan.recs_emit / 2;
        const u64 nm_parsed = fq->split_at ? 2 * plan.recs : plan.recs;
        const u64 nm = 2 * npairs;
        if ((rc = fq_mates(fq, std::max(nm_parsed, nm) + 2))) return fq_fail(fq, rc, ctx->err);
        if ((rc = fq_grow(ctx, &fq->d_scan, &fq->scan_cap, (size_t)(nm / SCAN_CHUNK + 4)))) return fq_fail(fq, rc, ctx->err);
        // output: never more bytes than the chunk's text (header comment of gk_fastq_convert)
        if ((rc = fq_grow(ctx, &fq->d_out, &fq->out_cap, (size_t)n + 64))) return fq_fail(fq, rc, ctx->err);
        GK_HIP(ctx, kt.start());
        if (plan.recs)
            hipLaunchKernelGGL(k_fq_records, dim3((unsigned)((plan.recs + 3) / 4)), dim3(FQ_BLOCK), 0, ctx->stream, T, n, fq->d_E, plan.recs, fq->split_at,
                               fq->records, fq->d_mlen, fq->d_mstart, fq->d_sum);
        if (npairs)
            hipLaunchKernelGGL(k_fq_pairs, dim3((unsigned)((npairs + FQ_BLOCK - 1) / FQ_BLOCK)), dim3(FQ_BLOCK), 0, ctx->stream, npairs, fq->d_mlen,
                               fq->split_at ? 1 : 2, fq->records, fq->pairs_seen, fq->max_pairs, fq->k_stats, m ? m->k : 0, fq->d_bytes,
                               m ? fq->d_win : nullptr, fq->d_sum);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, scan_counts(ctx, fq->d_bytes, nm, fq->d_off64, fq->d_scan));
        if (m) GK_HIP(ctx, scan_counts(ctx, fq->d_win, nm, fq->d_wpre, fq->d_scan));
        if (nm)
            hipLaunchKernelGGL(k_fq_pack, dim3((unsigned)((nm + 3) / 4)), dim3(FQ_BLOCK), 0, ctx->stream, T, nm, fq->d_mlen, fq->d_mstart, fq->d_bytes,
                               fq->d_off64, fq->d_out, (u64)fq->out_cap, fq->d_off32);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, hipMemcpyAsync(&fq->h->sum, fq->d_sum, sizeof(FqSum), hipMemcpyDeviceToHost, ctx->stream));
        GK_HIP(ctx, hipMemcpyAsync(&fq->h->out_bytes, fq->d_off64 + nm, 8, hipMemcpyDeviceToHost, ctx->stream));
        if (m) GK_HIP(ctx, hipMemcpyAsync(&fq->h->windows, fq->d_wpre + nm, 8, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = kt.end(&kern_ms))) return fq_fail(fq, rc, ctx->err);
        const FqSum sum = fq->h->sum;
        const u64 out_bytes = fq->h->out_bytes;
        // ---- the completed pairs to their sink (pairs after the first bad record emitted nothing: a prefix of the mates)
        const auto t_sink = clk::now();
        const u64 good_mates = 2 * sum.pairs;
        if (out_bytes > n) return fq_fail(fq, GK_E_STATE, "gk_fastq: output bound violated (internal error)");
        if (bin_out && out_bytes) {
            GK_HIP(ctx, hipMemcpy(bin_out + written, fq->d_out, out_bytes, hipMemcpyDeviceToHost));
            written += out_bytes;
        }
        if (m && good_mates) {
            const u64 windows = fq->h->windows;
            const u64 limit = map_window_limit(m);
            if (windows <= limit) {
                if ((rc = map_count_framed_dev(m, fq->d_out, fq->d_off32, good_mates, windows, 1.0))) return fq_fail(fq, rc, ctx->err);
            } else {
                const u64 per = limit - 255, nb = (windows + per - 1) / per;
                if ((rc = fq_grow(ctx, &fq->d_cut, &fq->cut_cap, 2 * (nb + 1)))) return fq_fail(fq, rc, ctx->err);
                hipLaunchKernelGGL(k_fq_cut, dim3((unsigned)((nb + 1 + 255) / 256)), dim3(256), 0, ctx->stream, fq->d_wpre, good_mates, per, nb, fq->d_cut);
                std::vector<unsigned long long> cut(2 * (nb + 1));
                GK_HIP(ctx, read_back(ctx, cut.data(), fq->d_cut, cut.size()));
                for (u64 j = 0; j < nb; j++) {
                    const u64 b0 = cut[2 * j], b1 = cut[2 * j + 2];
                    if (b1 <= b0) continue;
                    if ((rc = map_count_framed_dev(m, fq->d_out, fq->d_off32 + b0, b1 - b0, cut[2 * j + 3] - cut[2 * j + 1], (double)(nb - j))))
                        return fq_fail(fq, rc, ctx->err);
                }
            }
        }
        sink_ms += ms_since(t_sink);
        fq->pairs += sum.pairs; fq->short_pairs += sum.short_pairs; fq->kmers += sum.kmers;
        if (sum.err != FQ_NO_ERR) {
            fq->carry = 0;
            if (bin_bytes) *bin_bytes = written;
            fq->ms[0] = (float)up_ms; fq->ms[1] = (float)kern_ms; fq->ms[2] = (float)sink_ms; fq->ms[3] = (float)ms_since(t_call);
            return fq_fail(fq, GK_E_FORMAT, "FASTQ record " + std::to_string(sum.err >> 3) + ": " + fq_err_text((u32)(sum.err & 7)));
        }
        fq->records += plan.recs_emit;
        fq->pairs_seen += npairs;
        fq->text_bytes += plan.carry_start;
        // ---- the tail in front of the next slice
        const u64 new_carry = n - plan.carry_start;
        const int nb_ = 1 - b;
        if ((rc = fq_text_buffer(fq, nb_, new_carry, next_slice, false))) return fq_fail(fq, rc, ctx->err);
        if (new_carry)
            GK_HIP(ctx, hipMemcpyAsync(fq->buf[nb_] + fq->head[nb_] - new_carry, T + plan.carry_start, new_carry, hipMemcpyDeviceToDevice, ctx->stream));
        fq->carry = new_carry;
        fq->cur = nb_;
        pos = next_pos;
    } while (pos < nbytes);
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (last) { fq->finished = true; fq->carry = 0; }
    if (bin_bytes) *bin_bytes = written;
    if (m) { if ((rc = map_count_end(m, occ_out))) return fq_fail(fq, rc, ctx->err); }
    fq->ms[0] = (float)up_ms; fq->ms[1] = (float)kern_ms; fq->ms[2] = (float)sink_ms; fq->ms[3] = (float)ms_since(t_call);
    return GK_OK;
}

int fq_check_call(gk_fastq *fq, const char *text, size_t nbytes) {
    if (!fq) return fail(nullptr, GK_E_INVALID, "gk_fastq: null handle");
    if (fq->failed) return fail(fq->ctx, GK_E_STATE, "gk_fastq: the handle failed earlier (see the first error); destroy it");
    if (fq->finished) return fail(fq->ctx, GK_E_STATE, "gk_fastq: the input has ended (last != 0 was passed)");
    if (!text && nbytes) return fail(fq->ctx, GK_E_INVALID, "gk_fastq: null text");
    return GK_OK;
}

}  // namespace

extern "C" {

int gk_fastq_create(gk_ctx *ctx, int split_at, int k_stats, uint64_t max_pairs, gk_fastq **out) {
    if (!ctx || !out) return fail(ctx, GK_E_INVALID, "gk_fastq_create: null argument");
    *out = nullptr;
    if (split_at < 0 || split_at > 4096) return fail(ctx, GK_E_INVALID, "gk_fastq_create: split_at must be 0 (interleaved) or 1..4096");
    if (k_stats < 1 || k_stats > 255) return fail(ctx, GK_E_INVALID, "gk_fastq_create: k_stats must be 1..255");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    gk_fastq *fq = new gk_fastq;
    fq->ctx = ctx; fq->split_at = split_at; fq->k_stats = k_stats; fq->max_pairs = max_pairs;
    hipError_t e = fq->up.create();
    if (e == hipSuccess) e = pool_malloc(ctx, &fq->d_plan, sizeof(FqPlan));
    if (e == hipSuccess) e = pool_malloc(ctx, &fq->d_sum, sizeof(FqSum));
    if (e == hipSuccess) e = hipHostMalloc((void **)&fq->h, sizeof(FqHost), 0);
    if (e != hipSuccess) { const int rc = hip_fail(ctx, e, "gk_fastq_create"); gk_fastq_destroy(fq); return rc; }
    *out = fq;
    return GK_OK;
}

void gk_fastq_destroy(gk_fastq *fq) {
    if (!fq) return;
    gk_ctx *ctx = fq->ctx;
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    void *dev[] = {fq->buf[0], fq->buf[1], fq->d_tile_cnt, fq->d_tile_off, fq->d_scan, fq->d_E, fq->d_mlen, fq->d_mstart, fq->d_bytes, fq->d_win,
                   fq->d_off32, fq->d_off64, fq->d_wpre, fq->d_cut, fq->d_out, fq->d_plan, fq->d_sum};
    for (void *p : dev) (void)pool_free(ctx, p);
    fq->up.destroy();
    if (fq->h) (void)hipHostFree(fq->h);
    delete fq;
}

int gk_fastq_convert(gk_fastq *fq, const char *text, size_t nbytes, int last, uint8_t *bin_out, size_t bin_cap, size_t *bin_bytes) {
    if (int rc = fq_check_call(fq, text, nbytes)) return rc;
    if (bin_bytes) *bin_bytes = 0;
    if (!bin_bytes) return fail(fq->ctx, GK_E_INVALID, "gk_fastq_convert: bin_bytes is NULL");
    const u64 bound = fq->carry + nbytes;
    if (bound && !bin_out) return fail(fq->ctx, GK_E_INVALID, "gk_fastq_convert: bin_out is NULL");
    if (bin_cap < bound)
        return fail(fq->ctx, GK_E_CAPACITY, "gk_fastq_convert: bin_cap " + std::to_string(bin_cap) + " < carried + nbytes = " + std::to_string(bound));
    GK_HIP(fq->ctx, hipSetDevice(fq->ctx->device));
    if (!nbytes && !last) return GK_OK;
    return fq_run(fq, text, nbytes, last, bin_out, bin_bytes, nullptr, nullptr);
}

int gk_fastq_count(gk_fastq *fq, gk_map *m, const char *text, size_t nbytes, int last, uint64_t *occurrences) {
    if (int rc = fq_check_call(fq, text, nbytes)) return rc;
    if (occurrences) *occurrences = 0;
    if (!m) return fail(fq->ctx, GK_E_INVALID, "gk_fastq_count: null map");
    if (m->ctx != fq->ctx) return fail(fq->ctx, GK_E_INVALID, "gk_fastq_count: the map lives on another context");
    GK_HIP(fq->ctx, hipSetDevice(fq->ctx->device));
    if (!nbytes && !last) return GK_OK;
    return fq_run(fq, text, nbytes, last, nullptr, nullptr, m, occurrences);
}

int gk_fastq_stats(const gk_fastq *fq, uint64_t *pairs, uint64_t *short_pairs, uint64_t *kmers, uint64_t *text_bytes, uint64_t *carried_bytes) {
    if (!fq) return fail(nullptr, GK_E_INVALID, "gk_fastq_stats: null handle");
    if (pairs) *pairs = fq->pairs;
    if (short_pairs) *short_pairs = fq->short_pairs;
    if (kmers) *kmers = fq->kmers;
    if (text_bytes) *text_bytes = fq->text_bytes;
    if (carried_bytes) *carried_bytes = fq->carry;
    return GK_OK;
}

int gk_fastq_last_ms(const gk_fastq *fq, float *ms4) {
    if (!fq) return fail(nullptr, GK_E_INVALID, "gk_fastq_last_ms: null handle");
    if (!ms4) return fail(fq->ctx, GK_E_INVALID, "gk_fastq_last_ms: null buffer");
    for (int i = 0; i < 4; i++) ms4[i] = fq->ms[i];
    return GK_OK;
}

}  // extern "C"
