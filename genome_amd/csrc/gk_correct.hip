// gk_correct.hip — spectral correction of the reads themselves: a base under a run of weak k-mers is replaced when exactly one
// replacement makes every k-mer of the run solid.  The rule is this project's own and stated in include/genome_amd.h
// (gk_reads_correct); tests/correct_ref.py restates it.
//
// Reference: none.  GraphBuilder.scala:30 hardcodes rounds = 3 and lives with the k true k-mers every wrong base costs.
//
// Roofline: one independent random table probe per window of every read, and 3 * m more for every run of m weak windows whose
// shape is accepted (m <= k): the random-load rate of HBM, as k_cov_* (gk_coverage.hip).  The records themselves are read and
// written once, 16 bytes at a time; no global atomics but ten per workgroup for the statistics.
#include <algorithm>

#include "gk_binstream.h"
#include "gk_graph.h"

// ---------------------------------------------------------------------------------------------
// 256-bit sets of window positions (a record holds at most 255 - k + 1 <= 254 windows), wave-uniform, in registers: every
// index below is a compile-time constant after unrolling
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int first_set_from(const u64 (&w)[4], int from) {      // the first set bit at or after `from`; 256 if none
    int r = 256;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        const int lo = from - 64 * j;                        // bits of word j below `lo` do not count
        const u64 v = lo >= 64 ? 0ull : lo > 0 ? w[j] & (~0ull << lo) : w[j];
        if (v) r = 64 * j + __ffsll((unsigned long long)v) - 1;
    }
    return r;
}
// read[i] ^= d in a window (d = old base ^ new base); in its reverse complement the same d lands at k - 1 - i (complement is ^ 3)
__device__ __forceinline__ Kmer<1> flip_base(Kmer<1> x, int i, u64 d) { return Kmer<1>{x.lo ^ (d << (2 * i))}; }
__device__ __forceinline__ Kmer<2> flip_base(Kmer<2> x, int i, u64 d) {
    return i < 32 ? Kmer<2>{x.lo ^ (d << (2 * i)), x.hi} : Kmer<2>{x.lo, x.hi ^ (d << (2 * (i - 32)))};
}

struct CorrectCounts { u32 reads, shrt, windows, weak, runs, corrected, ambiguous, unresolved, skipped, changed; };

// One record, one wave (every branch below is wave-uniform except where a lane owns a window).  `ro` = the record's byte offset
// in the tile.  Runs never share a window and the base a run may change lies in its own windows only: what later runs read from
// the tile is what the input held.
template <int W, class S>
__device__ __forceinline__ void correct_record(const Table<W, S> &t, bool empty, u32 *tile, u32 ro, int len, int k, u32 solid, CorrectCounts &st) {
    uint8_t *tb = reinterpret_cast<uint8_t *>(tile);
    const int lane = threadIdx.x & 63;
    const int n = len - k + 1;
    st.reads++;
    st.shrt += n <= 0 ? 1u : 0u;
    if (n <= 0) return;
    const u32 bit0 = (ro + 1) * 8;
    // phase 1: the solid flags of the input's windows, one lane per window
    u64 weak[4], rest[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int left = n - 64 * j;
        u64 s = 0;
        if (left > 0) {
            const int p = 64 * j + lane;
            bool ok = false;
            if (p < n && !empty) {
                const Kmer<W> x = tile_kmer(tile, bit0 + 2 * p, k, (Kmer<W> *)nullptr);
                ok = window_count(t, x, revcomp(x, k)) >= solid;
            }
            s = __ballot(ok);
        }
        weak[j] = left <= 0 ? 0ull : ~s & low_mask(left);
        rest[j] = ~weak[j];                                  // solid windows, and everything from n on: where a weak run ends
        st.weak += (u32)__popcll(weak[j]);
    }
    st.windows += (u32)n;
    // phase 2: the weak runs [a, b]
    bool changed = false;
    for (int a = first_set_from(weak, 0); a < 256;) {
        const int e = first_set_from(rest, a);               // <= n <= 254
        const int b = e - 1, m = e - a;
        st.runs++;
        int p = -1;                                          // the one base that lies in exactly the windows a .. b
        if (a == 0 && b == n - 1) p = -1;
        else if (a == 0) { if (m <= k) p = b; }
        else if (b == n - 1) { if (m <= k) p = a + k - 1; }
        else if (m == k) p = b;
        int nvalid = -1;                                     // -1: skipped for its shape
        if (p >= 0) {
            // 3 x m (replacement, window) pairs over the lanes; a pair votes against its replacement when its window stays weak
            u32 invalid = 0;
            for (int i0 = 0; i0 < 3 * m; i0 += 64) {
                const int i = i0 + lane;
                int c = 3;
                bool bad = false;
                if (i < 3 * m) {
                    c = i / m;
                    const int w = a + (i - c * m);
                    Kmer<W> x = tile_kmer(tile, bit0 + 2 * w, k, (Kmer<W> *)nullptr);
                    Kmer<W> rc = revcomp(x, k);
                    x = flip_base(x, p - w, (u64)(c + 1));
                    rc = flip_base(rc, k - 1 - (p - w), (u64)(c + 1));
                    bad = window_count(t, x, rc) < solid;
                }
                if (__ballot(bad && c == 0)) invalid |= 1u;
                if (__ballot(bad && c == 1)) invalid |= 2u;
                if (__ballot(bad && c == 2)) invalid |= 4u;
            }
            nvalid = 3 - __popc(invalid);
            if (nvalid == 1) {
                const u32 d = invalid == 6u ? 1u : invalid == 5u ? 2u : 3u;
                if (lane == 0) tb[ro + 1 + (p >> 2)] ^= (uint8_t)(d << ((p & 3) * 2));
                // (a later run of this record may read the word this byte lies in)
                wave_sync();
                changed = true;
            }
        }
        // (sums, not branches: increments on different branches meet in one dynamically indexed store, which costs scratch)
        st.skipped += nvalid < 0 ? 1u : 0u;
        st.unresolved += nvalid == 0 ? 1u : 0u;
        st.corrected += nvalid == 1 ? 1u : 0u;
        st.ambiguous += nvalid > 1 ? 1u : 0u;
        a = first_set_from(weak, e);
    }
    st.changed += changed ? 1u : 0u;
}

// A workgroup stages 64 records in LDS (gk_tile.h), its four waves take them one at a time, and the tile goes out again: only
// the bytes of the tile's own records [gb, ge) are written, never the 16-byte widening of the staging — which is what lets
// `out` be `rec` itself (another workgroup owns the bytes beside this tile).
template <int W, class S>
__global__ __launch_bounds__(BLOCK) void k_correct_reads(Table<W, S> t, int k, u32 empty, const uint8_t *rec, uint8_t *out, u64 nreads,
                                                         const u32 *__restrict__ off, u32 stride, WindowLimits lim, u32 solid,
                                                         unsigned long long *stats) {
    __shared__ __attribute__((aligned(16))) u32 tile[TILE_WORDS];
    __shared__ unsigned long long s_stats[GK_CORRECT_NSTATS];
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < GK_CORRECT_NSTATS) s_stats[threadIdx.x] = 0;
    CorrectCounts st{};
    const bool vec = ((((uintptr_t)out) ^ ((uintptr_t)rec)) & 15) == 0;      // the staging aligned the tile for `rec`
    const u64 ntiles = (nreads + TILE_READS - 1) / TILE_READS;
    for (u64 ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {                 // (uniform over the workgroup: the barriers are safe)
        const u64 r0 = ti * TILE_READS;
        const int nr = (int)min((u64)TILE_READS, nreads - r0);
        const u64 gb = off ? (u64)off[r0] : r0 * stride, ge = off ? (u64)off[r0 + nr] : (r0 + nr) * stride;
        const u64 a0 = stage_tile(tile, rec, gb, ge);
        __syncthreads();
        for (int r = wave; r < nr; r += BLOCK / 64) {
            const u32 ro = (u32)((off ? (u64)off[r0 + r] : (r0 + r) * stride) - a0);
            correct_record<W, S>(t, empty != 0u, tile, ro, record_len(tb, ro, lim), k, solid, st);
        }
        __syncthreads();
        // LDS bytes [lo, hi) are this tile's own; whole 16-byte vectors of them go out as such when `out` is aligned as `rec` is
        const u32 lo = (u32)(gb - a0), hi = (u32)(ge - a0);
        u32 v0 = (lo + 15u) >> 4, v1 = hi >> 4;
        if (!vec || v0 >= v1) v0 = v1 = hi >> 4;                              // no vector part: [lo, hi) byte by byte
        uint8_t *ob = out + (i64)a0;
        if (v0 < v1) {
            const uint4 *src = reinterpret_cast<const uint4 *>(tile);
            uint4 *dst = reinterpret_cast<uint4 *>(ob);
            for (u32 i = v0 + threadIdx.x; i < v1; i += BLOCK) dst[i] = src[i];
            for (u32 q = lo + threadIdx.x; q < v0 * 16u; q += BLOCK) ob[q] = tb[q];
            for (u32 q = v1 * 16u + threadIdx.x; q < hi; q += BLOCK) ob[q] = tb[q];
        } else {
            for (u32 q = lo + threadIdx.x; q < hi; q += BLOCK) ob[q] = tb[q];
        }
        __syncthreads();                                                      // before the next tile is staged over this one
    }
    // the counters are wave-uniform: lane 0 of every wave adds them up in LDS, then one global atomic per counter and workgroup
    if (lane == 0) {
        const u32 v[GK_CORRECT_NSTATS] = {st.reads, st.shrt, st.windows, st.weak, st.runs, st.corrected, st.ambiguous, st.unresolved, st.skipped, st.changed};
#pragma unroll
        for (int i = 0; i < GK_CORRECT_NSTATS; i++) if (v[i]) atomicAdd(&s_stats[i], (unsigned long long)v[i]);
    }
    __syncthreads();
    if (threadIdx.x < GK_CORRECT_NSTATS && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// one launch over records resident in HBM: `src` as the count kernels take it (fixed stride, or the offset table of a framing
// the host has walked); stream-ordered, no sync.  d_stats: GK_CORRECT_NSTATS counters the launch adds to.
static int correct_launch(gk_map *counts, const ReadSrc &src, uint8_t *d_out, u32 solid, u32 *d_bad, unsigned long long *d_stats) {
    gk_ctx *ctx = counts->ctx;
    const u64 ntiles = (src.nreads + TILE_READS - 1) / TILE_READS;
    const int grid = (int)std::min<u64>(ntiles, grid_cap(ctx));
    const WindowLimits lim{src.max_len, d_bad};
    // a new or cleared map is an empty table whose slots hold void bytes: every window is weak, and the slots are not read
    const u32 empty = counts->pending_clear ? 1u : 0u;
    GK_BY_SLOT(counts, {
        const Table<W, S> t{reinterpret_cast<S *>(counts->slots), counts->nb2, counts->lnb1, counts->k == 64 ? 1u : 0u, counts->dirty ? 1u : 0u};
        hipLaunchKernelGGL((k_correct_reads<W, S>), dim3(grid), dim3(BLOCK), 0, ctx->stream, t, counts->k, empty, src.rec, d_out, (u64)src.nreads, src.off,
                           src.stride, lim, solid, d_stats);
    });
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}

static int check_correct_args(gk_map *counts, uint32_t solid, uint64_t *stats, const char *who) {
    if (stats) for (int i = 0; i < GK_CORRECT_NSTATS; i++) stats[i] = 0;
    if (!counts || !counts->ctx) return fail(nullptr, GK_E_INVALID, std::string(who) + ": null map handle");
    gk_ctx *ctx = counts->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    if (solid == 0) return fail(ctx, GK_E_INVALID, std::string(who) + ": solid must be at least 1 (no k-mer has count 0)");
    return GK_OK;
}

extern "C" {

int gk_reads_correct_dev(gk_map *counts, const void *dev_records, uint64_t nreads, int read_len, uint32_t solid, void *dev_out, uint64_t *stats) {
    if (int rc = check_correct_args(counts, solid, stats, "gk_reads_correct_dev")) return rc;
    gk_ctx *ctx = counts->ctx;
    if (nreads && (!dev_records || !dev_out)) return fail(ctx, GK_E_INVALID, "gk_reads_correct_dev: null records");
    if (int rc = check_read_len(ctx, read_len)) return rc;
    if (nreads == 0) return GK_OK;
    const ReadSrc src = ReadSrc::fixed(dev_records, nreads, read_len);
    const uintptr_t in0 = (uintptr_t)dev_records, out0 = (uintptr_t)dev_out, span = (uintptr_t)(nreads * src.stride);
    if (in0 != out0 && in0 < out0 + span && out0 < in0 + span)
        return fail(ctx, GK_E_INVALID, "gk_reads_correct_dev: dev_out overlaps dev_records without being the same buffer");
    DevScratch tmp(ctx);
    unsigned long long *d_stats = nullptr, h_stats[GK_CORRECT_NSTATS] = {};
    GK_HIP(ctx, tmp.zeroed(&d_stats, GK_CORRECT_NSTATS));
    if (int rc = correct_launch(counts, src, (uint8_t *)dev_out, solid, ctx->d_flags, d_stats)) return rc;
    GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}}));
    if (stats) for (int i = 0; i < GK_CORRECT_NSTATS; i++) stats[i] = h_stats[i];
    return ctx_check_format(ctx);
}

int gk_reads_correct(gk_map *counts, const uint8_t *bin_host, size_t nbytes, uint64_t nreads, uint32_t solid, uint8_t *bin_out, uint64_t *stats) {
    if (int rc = check_correct_args(counts, solid, stats, "gk_reads_correct")) return rc;
    gk_ctx *ctx = counts->ctx;
    if (nreads && (!bin_host || !bin_out)) return fail(ctx, GK_E_INVALID, "gk_reads_correct: null stream");
    // the framing, walked on the host before anything is written
    size_t end = 0;
    if (int rc = bin_walk(ctx, bin_host, nbytes, nreads, &end)) return rc;
    unsigned long long h_stats[GK_CORRECT_NSTATS] = {};
    if (end) {
        DevScratch tmp(ctx);
        unsigned long long *d_stats = nullptr;
        GK_HIP(ctx, tmp.zeroed(&d_stats, GK_CORRECT_NSTATS));
        // a piece is corrected in place in its staging area and comes back to bin_out at the offset it came from
        if (int rc = bin_feed(ctx, tmp, bin_host, end, [&](const ReadSrc &src, uint8_t *d_area, const BinPiece &piece, D2H *back) {
                *back = {bin_out + piece.begin, d_area, piece.bytes};
                return correct_launch(counts, src, d_area, solid, nullptr, d_stats);
            }))
            return rc;
        GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}}));
    }
    if (bin_out != bin_host && nbytes > end) std::copy(bin_host + end, bin_host + nbytes, bin_out + end);     // bytes behind the last record
    if (stats) for (int i = 0; i < GK_CORRECT_NSTATS; i++) stats[i] = h_stats[i];
    return GK_OK;
}

}  // extern "C"
