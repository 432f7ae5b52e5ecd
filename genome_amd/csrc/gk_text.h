// gk_text.h — what the FASTQ parser (gk_fastq.hip) and the FASTA check (gk_fasta.hip) share.  Device: line ends of a text tile —
// the terminator passes over 16 KiB tiles staged in LDS, and the start of line j from the terminator array they write.
// Host: the slice upload on the copy stream (TextUpload) and the event-timed section of kernels (TimedSection).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstring>

#include "gk_scan.h"
#include "gk_tile.h"

namespace {

constexpr u32 FQ_TILE = 16384;                          // text bytes per workgroup of the line-end passes
constexpr u32 FQ_BLOCK = 256;

__device__ __forceinline__ u64 umin(u64 a, u64 b) { return a < b ? a : b; }

// first byte of line j: 0, or past line j-1's terminator ("\r\n" is one; E == n marks an unterminated last line)
__device__ __forceinline__ u64 fq_line_start(const uint8_t *__restrict__ T, u64 n, const u32 *__restrict__ E, u64 j) {
    if (j == 0) return 0;
    const u64 e = E[j - 1];
    if (e >= n) return n;
    return e + ((T[e] == '\r' && e + 1 < n && T[e + 1] == '\n') ? 2 : 1);
}

// pass 0: terminators per tile; pass 1: their positions at tile_off[tile].  A terminator is the byte a line ends at: '\r', or
// '\n' not preceded by '\r' (Java BufferedReader.readLine).  The byte before the tile comes along for that look-back.
template <int PASS>
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_terms(const uint8_t *__restrict__ T, u64 n, u32 *__restrict__ tile_cnt,
                                                        const unsigned long long *__restrict__ tile_off, u32 *__restrict__ E) {
    __shared__ u32 s_tile[(FQ_TILE + 64) / 4];
    __shared__ u32 s_wcnt[FQ_BLOCK / 64];
    const u64 g0 = (u64)blockIdx.x * FQ_TILE, g1 = umin(n, g0 + FQ_TILE);
    const u64 a0 = stage_tile(s_tile, T, g0 ? g0 - 1 : 0, g1);
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(s_tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr u32 PER_WAVE = FQ_TILE / (FQ_BLOCK / 64);
    const u64 w0 = g0 + (u64)wave * PER_WAVE;
    auto is_term = [&](u64 x) -> bool {
        if (x >= g1) return false;
        const u32 c = tb[x - a0];
        return c == '\r' || (c == '\n' && !(x > 0 && tb[x - 1 - a0] == '\r'));
    };
    u32 cnt = 0;
    for (u32 s = 0; s < PER_WAVE; s += 64) cnt += (u32)__popcll(__ballot(is_term(w0 + s + lane)));
    if (PASS == 0) {
        if (lane == 0) s_wcnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        return;
    }
    if (lane == 0) s_wcnt[wave] = cnt;
    __syncthreads();
    u64 o = tile_off[blockIdx.x];
    for (int w = 0; w < wave; w++) o += s_wcnt[w];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (u32 s = 0; s < PER_WAVE; s += 64) {
        const u64 x = w0 + s + lane;
        const bool t = is_term(x);
        const unsigned long long mask = __ballot(t);
        if (t) E[o + (u64)__popcll(mask & below)] = (u32)x;
        o += (u64)__popcll(mask);
    }
}

// ---- host half ----------------------------------------------------------------------------------------------------------------
using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }

// Uploads of text slices into the two device buffers of a stage: on the copy stream, between the event pair up0[b] / up1[b]
// (the consumer waits for up1[b] and reads the pair's time).  Pageable text goes through one of two pinned staging buffers,
// grown on demand to a power of two.
struct TextUpload {
    hipEvent_t up0[2] = {nullptr, nullptr}, up1[2] = {nullptr, nullptr};
    uint8_t *h_stage[2] = {nullptr, nullptr};
    u64 h_stage_cap = 0;

    hipError_t create() {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            e = hipEventCreate(&up0[i]);
            if (e == hipSuccess) e = hipEventCreate(&up1[i]);
        }
        return e;
    }
    void destroy() {
        for (int i = 0; i < 2; i++) {
            if (h_stage[i]) (void)hipHostFree(h_stage[i]);
            if (up0[i]) (void)hipEventDestroy(up0[i]);
            if (up1[i]) (void)hipEventDestroy(up1[i]);
        }
    }
    static bool is_pinned(const void *p) {
        unsigned int flags = 0;
        const bool ok = hipHostGetFlags(&flags, const_cast<void *>(p)) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    // the two pinned staging buffers hold at least `bytes` each (a caller that knows its largest upload asks once, up front)
    int reserve(gk_ctx *ctx, u64 bytes) {
        if (h_stage_cap >= bytes) return GK_OK;
        GK_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
        for (int i = 0; i < 2; i++) { if (h_stage[i]) (void)hipHostFree(h_stage[i]); h_stage[i] = nullptr; }
        h_stage_cap = 0;
        const u64 cap = pow2ceil(std::max<u64>(bytes, 4096));
        for (int i = 0; i < 2; i++) GK_HIP(ctx, hipHostMalloc((void **)&h_stage[i], cap, 0));
        h_stage_cap = cap;
        return GK_OK;
    }
    // text [src, src + bytes) -> d_dst; *host_ms grows by the time of the host's copy into the staging buffer
    int upload(gk_ctx *ctx, int b, void *d_dst, const char *src, u64 bytes, bool pinned, double *host_ms) {
        const void *from = src;
        if (!pinned) {
            if (int rc = reserve(ctx, bytes)) return rc;
            const auto t0 = clk::now();
            memcpy(h_stage[b], src, bytes);
            *host_ms += ms_since(t0);
            from = h_stage[b];
        }
        GK_HIP(ctx, hipEventRecord(up0[b], ctx->copy_stream));
        GK_HIP(ctx, hipMemcpyAsync(d_dst, from, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
        GK_HIP(ctx, hipEventRecord(up1[b], ctx->copy_stream));
        return GK_OK;
    }
};

// A section of work on ctx->stream between the context's event pair: end() waits for it and adds its time to *acc_ms.
struct TimedSection {
    gk_ctx *ctx;
    hipError_t start() const { return hipEventRecord(ctx->ev0, ctx->stream); }
    int end(double *acc_ms) const {
        GK_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        GK_HIP(ctx, hipEventSynchronize(ctx->ev1));
        float t = 0;
        GK_HIP(ctx, hipEventElapsedTime(&t, ctx->ev0, ctx->ev1));
        *acc_ms += t;
        return GK_OK;
    }
};

}  // namespace
