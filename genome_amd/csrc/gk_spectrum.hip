// gk_spectrum.hip — the k-mer count spectrum of a table (how many distinct k-mers occur exactly c times) in one streaming pass
// over the slots, and the rule that picks deleteAll's cutoff from it.
//
// Reference: GraphBuilder.scala:30 hardcodes `rounds = 3` for FreqFilter.extractFilteredKmers (S/data/FreqFilter.scala:25, :55);
// the reference has no spectrum.  The rules of the three entry points are in include/genome_amd.h.
//
// Roofline: k_spectrum reads every slot once (12, 16 or 24 bytes) and writes nothing but its histogram: HBM streaming.
#include <vector>

#include "gk_internal.h"
#include "gk_tile.h"

using namespace gk;

// Counts below SPEC_LDS_BINS are histogrammed in LDS per workgroup (32 KiB of the CU's 160: five workgroups, 20 waves, stay resident) and
// flushed with one 64-bit global atomic per non-empty (workgroup, bin); counts beyond go straight to the global histogram with
// one atomic each (a k-mer seen 8192 times and more: a handful per genome).  Count 1 — most of a real table, nearly all of an
// error-rich one — never meets an LDS atomic per lane: a wave counts its singletons by ballot and adds them once (64 lanes
// adding to ONE LDS word serialise; DESIGN.md section 3 "The spectrum").
// An LDS bin is 32 bits: a workgroup sees capacity / grid slots, far below 2^32 for any table that fits the device.
static constexpr u32 SPEC_LDS_BINS = 8192;
static constexpr int SPEC_UNROLL = 4;      // slots per lane and trip, their loads issued back to back

template <int W, class S>
__global__ __launch_bounds__(BLOCK) void k_spectrum(const S *__restrict__ slots, u64 ncap, u32 bins, unsigned long long *hist,
                                                    unsigned long long *out /* distinct, occurrences, largest count */) {
    __shared__ u32 lh[SPEC_LDS_BINS];
    for (u32 b = threadIdx.x; b < SPEC_LDS_BINS; b += BLOCK) lh[b] = 0u;
    __syncthreads();
    const u32 top = bins - 1u;             // the overflow bin
    const int lane = threadIdx.x & 63;
    unsigned long long live = 0, sum = 0;
    u32 mx = 0;
    // (the trip count is uniform over a wave: the ballots below see all 64 lanes)
    for (u64 base = (u64)blockIdx.x * (BLOCK * SPEC_UNROLL); base < ncap; base += (u64)gridDim.x * (BLOCK * SPEC_UNROLL)) {
        u32 c[SPEC_UNROLL];
#pragma unroll
        for (int u = 0; u < SPEC_UNROLL; u++) {
            const u64 i = base + (u64)u * BLOCK + threadIdx.x;
            c[u] = i < ncap && slot_live(&slots[i]) ? slot_count(&slots[i]) : 0u;      // (a live slot's count is at least 1)
        }
#pragma unroll
        for (int u = 0; u < SPEC_UNROLL; u++) {
            const u32 b = c[u] < top ? c[u] : top;
            live += c[u] != 0u;
            sum += c[u];
            mx = c[u] > mx ? c[u] : mx;
            const unsigned long long ones = __ballot(b == 1u);
            if (lane == 0 && ones) atomicAdd(&lh[1], (u32)__popcll(ones));
            if (b > 1u) {
                if (b < SPEC_LDS_BINS) atomicAdd(&lh[b], 1u);
                else atomicAdd(&hist[b], 1ull);
            }
        }
    }
    __syncthreads();
    const u32 nl = bins < SPEC_LDS_BINS ? bins : SPEC_LDS_BINS;
    for (u32 b = threadIdx.x; b < nl; b += BLOCK)
        if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
    for (int d = 32; d; d >>= 1) {
        live += __shfl_down(live, d); sum += __shfl_down(sum, d);
        const u32 o = __shfl_down(mx, d);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        if (live) { atomicAdd(&out[0], live); atomicAdd(&out[1], sum); atomicMax(&out[2], (unsigned long long)mx); }
    }
}

extern "C" {

int gk_map_spectrum(gk_map *m, uint64_t *hist, uint32_t bins, uint64_t *distinct, uint64_t *occurrences, uint32_t *max_count) {
    if (!m || !m->ctx) return fail(nullptr, GK_E_INVALID, "null map handle");
    gk_ctx *ctx = m->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    if (!hist) return fail(ctx, GK_E_INVALID, "gk_map_spectrum: hist is NULL");
    if (bins < 2 || bins > (1u << 20)) return fail(ctx, GK_E_INVALID, "gk_map_spectrum: bins must be 2 .. 1<<20");
    for (uint32_t b = 0; b < bins; b++) hist[b] = 0;
    unsigned long long h3[3] = {0, 0, 0};
    // A new or cleared map holds void bytes until something materialises the deferred clear: it is empty, and its slots are
    // not read (nor cleared: the next partitioned insert still builds every segment from empty).
    if (!m->pending_clear) {
        DevScratch tmp(ctx);
        unsigned long long *d = nullptr;                 // [bins] histogram, then distinct, occurrences, largest count
        GK_HIP(ctx, tmp.get(&d, (uint64_t)bins + 3));
        GK_HIP(ctx, hipMemsetAsync(d, 0, ((size_t)bins + 3) * 8, ctx->stream));
        const u64 per_block = (u64)BLOCK * SPEC_UNROLL;
        u64 blocks = (m->capacity + per_block - 1) / per_block;
        const u64 cap_blocks = grid_cap(ctx);             // grid-stride; the LDS histogram lets five be resident per CU
        const int grid = (int)(blocks < 1 ? 1 : blocks < cap_blocks ? blocks : cap_blocks);
        GK_BY_SLOT(m, hipLaunchKernelGGL((k_spectrum<W, S>), dim3(grid), dim3(BLOCK), 0, ctx->stream, (const S *)m->slots, m->capacity, bins, d, d + bins));
        GK_HIP(ctx, hipGetLastError());
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histogram is read back in place");
        GK_HIP(ctx, read_back(ctx, {{hist, d, (size_t)bins * 8}, {h3, d + bins, sizeof(h3)}}));
    }
    if (distinct) *distinct = h3[0];
    if (occurrences) *occurrences = h3[1];
    if (max_count) *max_count = (uint32_t)h3[2];
    return GK_OK;
}

// Pure host code: no context, no device.
int gk_spectrum_cutoff(const uint64_t *hist, uint32_t bins, uint32_t min_count, uint32_t *valley, uint32_t *peak, uint64_t *genome_size) {
    if (!hist) return fail(nullptr, GK_E_INVALID, "gk_spectrum_cutoff: hist is NULL");
    if (bins < 2 || bins > (1u << 20)) return fail(nullptr, GK_E_INVALID, "gk_spectrum_cutoff: bins must be 2 .. 1<<20");
    if (min_count < 1) return fail(nullptr, GK_E_INVALID, "gk_spectrum_cutoff: min_count must be at least 1 (no key has count 0)");
    uint32_t v = 0, p = 0;
    uint64_t g = 0;
    const uint64_t last = (uint64_t)bins - 2;            // the last counted bin; hist[bins - 1] (overflow) is never looked at
    uint64_t r = 0;
    bool rise = false;
    for (uint64_t c = min_count; c + 1 <= last; c++)
        if (hist[c] < hist[c + 1]) { r = c; rise = true; break; }
    if (rise) {
        p = (uint32_t)(r + 1);
        for (uint64_t c = r + 2; c <= last; c++)
            if (hist[c] > hist[p]) p = (uint32_t)c;
        v = min_count;
        for (uint64_t c = (uint64_t)min_count + 1; c <= p; c++)
            if (hist[c] < hist[v]) v = (uint32_t)c;
        unsigned __int128 s = 0;
        for (uint64_t c = v; c <= last; c++) s += (unsigned __int128)c * hist[c];
        g = (uint64_t)(s / p);
    }
    if (valley) *valley = v;
    if (peak) *peak = p;
    if (genome_size) *genome_size = g;
    return GK_OK;
}

}  // extern "C"
