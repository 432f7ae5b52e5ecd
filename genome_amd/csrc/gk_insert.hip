// gk_insert.hip — the fragment lengths of a paired-end library, measured on the graph: the histogram of the distances `annotate`
// (S/scripts/GraphSimplifier.scala:192-206) computes and throws away, and the rule that reads the range of the walks from it.
//
// Reference: GraphSimplifier.scala:146 hardcodes `180 to 250`; the reference estimates nothing.  The rules of the two entry
// points are in include/genome_amd.h ("the insert range").  The front end (keys cut from the stream, the four getAll as one
// batch in HBM, the position check) is gk_graph_walk_pairs' own: pairs_front (gk_pairs.hip).
//
// Roofline: k_pair_distances reads the CSR of the lookups once (two offsets and, for a placed orientation, two values) and one
// edge length per counted orientation; it writes nothing but its histogram.
#include <vector>

#include "gk_graph.h"

// Distances below PD_LDS_BINS are histogrammed in LDS per workgroup and flushed with one 64-bit global atomic per non-empty
// (workgroup, bin); larger ones go straight to the global histogram with one atomic each.  16 KiB: the eight 256-thread
// workgroups a CU holds (32 waves) fit its 160 KiB of LDS together, so the histogram costs no occupancy; a library's fragments
// spread over a hundred bins or so, and 4096 bases is beyond any short-read library's insert (a mate-pair library's kilobases
// take the global path: they spread over thousands of bins, where one address is no longer hot).
// An LDS bin is 32 bits: a workgroup sees norient / grid orientations, far below 2^32 for any batch that fits the device.
static constexpr u32 PD_LDS_BINS = 4096;
static constexpr u32 PD_MAX_LIST = 16;            // |P1|, |P2| beyond this: `repetitive` (the work of one lane is bounded by 16 x 16)
enum { PD_UNPLACED = 1, PD_REPETITIVE, PD_APART, PD_AMBIGUOUS, PD_REVERSED, PD_BEYOND, PD_NEAR_END, PD_COUNTED, PD_NCLASS };

// One lane per pair orientation o: P1 = vals[off[2o] .. off[2o+1]), P2 = vals[off[2o+1] .. off[2o+2]) (PairFront).
__global__ __launch_bounds__(BLOCK) void k_pair_distances(GraphView g, const unsigned long long *__restrict__ off, const u64 *__restrict__ vals, u64 norient, int k,
                                                          u32 bins, unsigned long long *hist, unsigned long long *classes) {
    __shared__ u32 lh[PD_LDS_BINS];
    __shared__ u32 lc[PD_NCLASS];
    for (u32 b = threadIdx.x; b < PD_LDS_BINS; b += BLOCK) lh[b] = 0u;
    if (threadIdx.x < PD_NCLASS) lc[threadIdx.x] = 0u;
    __syncthreads();
    const long max_dist = (long)bins - 1;
    u32 wc[PD_NCLASS] = {};                  // this wave's class counts (the same in every lane: sums of ballots)
    // (the trip count is uniform over a wave: the ballots below see all 64 lanes)
    for (u64 base = (u64)blockIdx.x * BLOCK; base < norient; base += (u64)gridDim.x * BLOCK) {
        const u64 o = base + threadIdx.x;
        u32 cls = 0;                         // 0: a lane past the end
        long D = 0;
        if (o < norient) {
            const u64 a0 = off[2 * o], a1 = off[2 * o + 1], a2 = off[2 * o + 2];
            const u64 n1 = a1 - a0, n2 = a2 - a1;
            if (n1 == 0 || n2 == 0) cls = PD_UNPLACED;
            else if (n1 > PD_MAX_LIST || n2 > PD_MAX_LIST) cls = PD_REPETITIVE;
            else {
                u32 nc = 0;
                u64 ca = 0, cb = 0;          // the first combination on one edge
                for (u64 i = 0; i < n1; i++) {
                    const u64 va = vals[a0 + i];
                    if (!GK_POS_IS_EDGE(va)) continue;
                    for (u64 j = 0; j < n2; j++) {
                        const u64 vb = vals[a1 + j];
                        if (!GK_POS_IS_EDGE(vb) || GK_POS_ID(vb) != GK_POS_ID(va)) continue;
                        if (nc == 0) { ca = va; cb = vb; }
                        nc++;
                    }
                }
                if (nc == 0) cls = PD_APART;
                else if (nc >= 2) cls = PD_AMBIGUOUS;
                else {
                    D = (long)GK_POS_DIST(cb) - (long)GK_POS_DIST(ca) + k;
                    if (D < k) cls = PD_REVERSED;
                    else if (D > max_dist) cls = PD_BEYOND;
                    else if ((long)GK_POS_DIST(ca) + max_dist - k >= (long)g.e_len[GK_POS_ID(ca)]) cls = PD_NEAR_END;      // (k_check_positions: the id is a live edge)
                    else cls = PD_COUNTED;
                }
            }
        }
#pragma unroll
        for (u32 c = 1; c < PD_NCLASS; c++) wc[c] += (u32)__popcll(__ballot(cls == c));
        if (cls == PD_COUNTED) {
            if (D < (long)PD_LDS_BINS) atomicAdd(&lh[D], 1u);
            else atomicAdd(&hist[D], 1ull);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (u32 c = 1; c < PD_NCLASS; c++) if (wc[c]) atomicAdd(&lc[c], wc[c]);
    }
    __syncthreads();
    const u32 nl = bins < PD_LDS_BINS ? bins : PD_LDS_BINS;
    for (u32 b = threadIdx.x; b < nl; b += BLOCK)
        if (lh[b]) atomicAdd(&hist[b], (unsigned long long)lh[b]);
    if (threadIdx.x >= 1 && threadIdx.x < PD_NCLASS && lc[threadIdx.x]) {
        atomicAdd(&classes[threadIdx.x], (unsigned long long)lc[threadIdx.x]);
        atomicAdd(&classes[0], (unsigned long long)lc[threadIdx.x]);
    }
}

extern "C" {

int gk_graph_pair_distances(gk_graph *g, gk_vmap *positions, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint32_t bins, uint64_t *hist,
                            uint64_t *classes) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    const char *who = "gk_graph_pair_distances";
    if (!positions || !hist || !classes || (!bin && nbytes)) return fail(ctx, GK_E_INVALID, std::string(who) + ": null argument");
    if (vmap_ctx(positions) != ctx) return fail(ctx, GK_E_INVALID, std::string(who) + ": the position map must live on the graph's context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, std::string(who) + ": the position map has another k");
    if (bins < 2 || bins > 65536) return fail(ctx, GK_E_INVALID, std::string(who) + ": bins must be 2 .. 65536");
    for (uint32_t b = 0; b < bins; b++) hist[b] = 0;
    for (int c = 0; c < 9; c++) classes[c] = 0;
    DevScratch tmp(ctx);
    PairFront F;
    if (int rc = pairs_front(g, positions, bin, nbytes, npairs, who, tmp, F)) return rc;
    if (F.nq == 0) return GK_OK;
    if (int rc = pairs_front_checked(ctx, F, who)) return rc;         // the kernel reads e_len by the positions' edge ids
    const u64 norient = F.nq / 2;
    unsigned long long *d = nullptr;                 // [bins] histogram, then the nine classes
    GK_HIP(ctx, tmp.get(&d, (uint64_t)bins + 9));
    GK_HIP(ctx, hipMemsetAsync(d, 0, ((size_t)bins + 9) * 8, ctx->stream));
    hipLaunchKernelGGL(k_pair_distances, dim3(ggrid(ctx, norient)), dim3(BLOCK), 0, ctx->stream, g->v, F.d_off, F.d_vals, norient, g->k, bins, d, d + bins);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histogram is read back in place");
    GK_HIP(ctx, read_back(ctx, {{hist, d, (size_t)bins * 8}, {classes, d + bins, 9 * 8}}));
    return GK_OK;
}

// Pure host code: no context, no device.
int gk_insert_range(const uint64_t *hist, uint32_t bins, uint32_t trim_permille, uint64_t min_observations, uint32_t *range_lo, uint32_t *range_hi,
                    uint32_t *median) {
    if (!hist) return fail(nullptr, GK_E_INVALID, "gk_insert_range: hist is NULL");
    if (bins < 2 || bins > 65536) return fail(nullptr, GK_E_INVALID, "gk_insert_range: bins must be 2 .. 65536");
    if (trim_permille > 499) return fail(nullptr, GK_E_INVALID, "gk_insert_range: trim_permille must be 0 .. 499");
    unsigned __int128 n = 0;
    for (uint32_t b = 0; b < bins; b++) n += hist[b];
    uint32_t lo = 0, hi = 0, med = 0;
    if (n >= (min_observations > 1 ? min_observations : 1)) {
        const unsigned __int128 t_lo = (unsigned __int128)trim_permille * n, t_hi = (unsigned __int128)(1000 - trim_permille) * n;
        unsigned __int128 cum = 0;
        bool have_lo = false, have_hi = false, have_med = false;
        for (uint32_t b = 0; b < bins && !have_hi; b++) {
            cum += hist[b];
            if (!have_lo && 1000 * cum > t_lo) { lo = b; have_lo = true; }
            if (!have_med && 2 * cum >= n) { med = b; have_med = true; }
            if (1000 * cum >= t_hi) { hi = b; have_hi = true; }
        }
    }
    if (range_lo) *range_lo = lo;
    if (range_hi) *range_hi = hi;
    if (median) *median = med;
    return GK_OK;
}

}  // extern "C"
