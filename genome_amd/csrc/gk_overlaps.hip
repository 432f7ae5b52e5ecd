// gk_overlaps.hip — overlap detection: where the last o bases of a chain member's path equal the first o bases of the next member's,
// exactly, for exactly one o the gap estimate allows, the junction is an overlap of o bases, so that the scaffold text writes those
// bases once instead of twice with N between them.
//
// The rule is this project's own and stated in include/genome_amd.h ("overlap detection"); tests/overlaps_ref.py restates it.  The
// chain list comes from gk_scaffold_chains or gk_graph_fill_gaps and goes on, with the overlaps, to gk_graph_scaffolds_plan_overlaps;
// its front end, the check included, is gk_chains.h's.
//
// k_chain_junctions by OvlRule: adjacent / out_of_range / to be searched; a scan compacts the junctions to search.
// k_ovl_search: one wave per junction packs the two ends into four 64-bit words each in LDS; a lane tests the candidates
// lo + lane and lo + lane + 64 by a multi-word shift, mask and compare; the hits are counted by ballot.  k_ovl_stats: a reduction
// over the classes.  Nothing but scratch is written on the device; the host copies out after one read-back.
#include <vector>

#include "gk_chains.h"
#include "gk_fastaout.h"
#include "gk_scan.h"

static_assert(GK_OVERLAP_MAX == 127, "a side is four 64-bit words of 2-bit codes, two bases per lane; the candidates fit two rounds of a wave");
static constexpr int OVL_STATS = 7;
static constexpr int OVL_WORDS = 4;
// device counters of a call: the five classes in the order of the GK_OVL_* codes, then the overlapped bases
enum { OS_ADJACENT = 0, OS_OUT_OF_RANGE, OS_NONE, OS_AMBIGUOUS, OS_OVERLAP, OS_BASES, OS_N };

// the candidates lo .. hi of a junction whose members' paths hold pe and pf bases (|G| and tol are below 2^31)
__device__ __forceinline__ void ovl_range(long long G, long long tol, u32 min_overlap, u32 max_overlap, u64 pe, u64 pf, long long *lo, long long *hi) {
    *lo = max((long long)min_overlap, -G - tol);
    *hi = min(min((long long)max_overlap, -G + tol), (long long)min(min(pe, pf) - 1, (u64)GK_OVERLAP_MAX));
}

// a junction that is neither adjacent nor out of the gap's range (behind a clean check: it reads the members' lengths): with a
// candidate, none so far and to be searched
struct OvlRule {
    long long tol;
    u32 min_overlap, max_overlap;
    __device__ u32 decide(const GraphView &g, u32 e, u32 f, long long G, uint8_t *cls) const {
        long long a, b;
        ovl_range(G, tol, min_overlap, max_overlap, (u64)g.k + g.e_len[e], (u64)g.k + g.e_len[f], &a, &b);
        *cls = a <= b ? GK_OVL_NONE : GK_OVL_OUT_OF_RANGE;
        return a <= b;
    }
};

// ---------------------------------------------------------------------------------------------
// the search: one wave per junction, the two ends in LDS
// ---------------------------------------------------------------------------------------------
// Bases first .. first + n - 1 (n <= 127) of edge x's path as 2-bit codes, base first + i at bits 2i of the 256: lane l takes
// bases 2l and 2l + 1, sixteen lanes make a word by an OR over their group, the group's first lane stores it.
__device__ __forceinline__ void ovl_pack(const GraphView &g, u32 x, u64 first, u32 n, u64 *words) {
    const int lane = threadIdx.x & 63;
    const u32 s = g.e_start[x];
    const u64 nlo = g.node_lo[s], nhi = g.k > 32 ? g.node_hi[s] : 0ull;
    const uint8_t *seq = g.pool + g.e_off[x];
    u64 v = 0;
    for (u32 b = 0; b < 2; b++) {
        const u32 i = 2 * (u32)lane + b;
        if (i < n) v |= (u64)path_base(nlo, nhi, seq, g.k, first + i) << (4 * (lane & 15) + 2 * b);
    }
    for (int d = 1; d < 16; d <<= 1) v |= __shfl_xor(v, d);
    if ((lane & 15) == 0) words[lane >> 4] = v;
}
// are bases [from, from + o) of side E the bases [0, o) of side F?  1 <= o, from + o <= 127.
__device__ __forceinline__ bool ovl_equal(const u64 *E, const u64 *F, u32 from, u32 o) {
    const u32 ws = (2 * from) >> 6, bs = (2 * from) & 63;
    bool same = true;
    for (u32 i = 0; i < OVL_WORDS; i++) {
        if (64 * i >= 2 * o) break;
        const u64 a = i + ws < OVL_WORDS ? E[i + ws] >> bs : 0ull;
        const u64 b = bs && i + ws + 1 < OVL_WORDS ? E[i + ws + 1] << (64 - bs) : 0ull;
        const u32 bits = min(2 * o - 64 * i, 64u);
        const u64 mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
        same &= ((a | b) & mask) == (F[i] & mask);
    }
    return same;
}

__global__ __launch_bounds__(BLOCK) void k_ovl_search(GraphView g, const u32 *__restrict__ members, const long long *__restrict__ gap, long long tol, u32 min_overlap,
                                                     u32 max_overlap, const u32 *__restrict__ flags, const u32 *__restrict__ list,
                                                     const unsigned long long *__restrict__ nsearch, uint8_t *__restrict__ jclass, u32 *__restrict__ overlap) {
    __shared__ u64 lds[BLOCK / 64][2 * OVL_WORDS];
    if (chains_bad(flags)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 *E = lds[wave], *F = lds[wave] + OVL_WORDS;
    const u64 ns = *nsearch, waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 w = (u64)blockIdx.x * (BLOCK / 64) + wave; w < ns; w += waves) {       // (uniform over the wave)
        const u32 j = list[w];
        const u32 e = members[j], f = members[j + 1];
        const u64 pe = (u64)g.k + g.e_len[e], pf = (u64)g.k + g.e_len[f];
        long long lo, hi;
        ovl_range(gap[j], tol, min_overlap, max_overlap, pe, pf, &lo, &hi);      // 1 <= lo <= hi <= 127: OvlRule
        const u32 ne = (u32)min(pe, (u64)GK_OVERLAP_MAX), nf = (u32)min(pf, (u64)GK_OVERLAP_MAX);
        ovl_pack(g, e, pe - ne, ne, E);
        ovl_pack(g, f, 0, nf, F);
        wave_sync();
        u32 hits = 0, hit = 0;
        for (u32 round = 0; round < 2; round++) {
            const long long o = lo + lane + 64 * round;
            const unsigned long long found = __ballot(o <= hi && ovl_equal(E, F, ne - (u32)o, (u32)o));
            if (found && !hits) hit = (u32)lo + 64 * round + (u32)__ffsll((long long)found) - 1;
            hits += (u32)__popcll(found);
            if (lo + 64 * (round + 1) > hi) break;
        }
        if (lane == 0) {
            jclass[j] = hits == 0 ? GK_OVL_NONE : hits > 1 ? GK_OVL_AMBIGUOUS : GK_OVL_OVERLAP;
            overlap[j] = hits == 1 ? hit : 0u;
        }
        wave_sync();                                     // the next junction reuses the words
    }
}

// ---------------------------------------------------------------------------------------------
// stats
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_ovl_stats(u64 nm, const u32 *__restrict__ flags, const uint8_t *__restrict__ jclass, const u32 *__restrict__ overlap,
                                                    unsigned long long *stats) {
    if (chains_bad(flags)) return;
    unsigned long long st[OS_N] = {};
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nm; j += (u64)gridDim.x * BLOCK) {
        const uint8_t cls = jclass[j];
        for (int c = 0; c < OS_BASES; c++) st[c] += cls == GK_OVL_ADJACENT + c;
        st[OS_BASES] += overlap[j];
    }
    for (int i = 0; i < OS_N; i++) {
        const unsigned long long v = wave_sum(st[i]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[i], v);
    }
}

extern "C" {

int gk_graph_overlap_gaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, uint64_t tol, uint32_t min_overlap,
                          uint32_t max_overlap, uint32_t *overlap, uint8_t *jclass, uint64_t *stats7) {
    const char *who = "gk_graph_overlap_gaps";
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (tol > 0x7fffffffull) return fail(ctx, GK_E_INVALID, std::string(who) + ": tol beyond 2^31-1");
    if (min_overlap < 1 || min_overlap > GK_OVERLAP_MAX) return fail(ctx, GK_E_INVALID, std::string(who) + ": min_overlap outside 1 .. " + std::to_string(GK_OVERLAP_MAX));
    if (max_overlap < min_overlap || max_overlap > GK_OVERLAP_MAX)
        return fail(ctx, GK_E_INVALID, std::string(who) + ": max_overlap outside min_overlap .. " + std::to_string(GK_OVERLAP_MAX));
    if (!stats7) return fail(ctx, GK_E_INVALID, std::string(who) + ": stats7 is NULL");
    if (nchains == 0) {                                      // (no chain, no member)
        for (int i = 0; i < OVL_STATS; i++) stats7[i] = 0;
        return GK_OK;
    }
    if (!overlap || !jclass) return fail(ctx, GK_E_INVALID, std::string(who) + ": overlap or jclass is NULL");
    const GraphView &v = g->v;
    DevScratch tmp(ctx);
    ChainList cl;
    if (int rc = chains_begin(who, g, tmp, members, chain_off, nchains, gap, SF_N, &cl)) return rc;
    const u64 nm = cl.nm;
    u32 *d_search = nullptr, *d_list = nullptr, *d_overlap = nullptr, h_flags[SF_N] = {};
    uint8_t *d_jclass = nullptr;
    unsigned long long *d_rank = nullptr, *d_stats = nullptr, h_stats[OS_N] = {};
    tmp.zeroed(&d_stats, OS_N);
    tmp.get(&d_jclass, nm);
    tmp.zeroed(&d_overlap, nm);                              // (zero: only the search writes it)
    tmp.zeroed(&d_search, nm);                               // (zero: behind a raised flag nothing writes it, and the scan still runs)
    tmp.get(&d_rank, nm + 1);
    tmp.get(&d_list, nm);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_overlap_gaps: scratch");
    // the junctions behind the check; every later kernel returns at once behind a raised flag
    hipLaunchKernelGGL(k_chain_junctions<OvlRule>, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, v, cl.d_members, cl.d_chain_off, (u64)nchains, nm, cl.d_gap,
                       OvlRule{(long long)tol, min_overlap, max_overlap}, cl.d_flags, d_jclass, d_search);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_search, nm, d_rank));
    hipLaunchKernelGGL(k_chain_list, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, nm, cl.d_flags, d_search, d_rank, d_list);
    hipLaunchKernelGGL(k_ovl_search, dim3(ggrid(ctx, (nm - nchains) * 64)), dim3(BLOCK), 0, ctx->stream, v, cl.d_members, cl.d_gap, (long long)tol, min_overlap, max_overlap,
                       cl.d_flags, d_list, d_rank + nm, d_jclass, d_overlap);
    hipLaunchKernelGGL(k_ovl_stats, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, nm, cl.d_flags, d_jclass, d_overlap, d_stats);
    std::vector<u32> h_overlap(nm);
    std::vector<uint8_t> h_jclass(nm);
    GK_HIP(ctx, read_back(ctx, {{h_flags, cl.d_flags, sizeof(h_flags)}, {h_stats, d_stats, sizeof(h_stats)}, {h_overlap.data(), d_overlap, nm * 4},
                                {h_jclass.data(), d_jclass, nm}}));
    if (int rc = chains_failed(who, ctx, h_flags, true)) return rc;
    stats7[0] = 0;
    for (int i = 0; i < OS_BASES; i++) { stats7[1 + i] = h_stats[i]; stats7[0] += h_stats[i]; }
    stats7[6] = h_stats[OS_BASES];
    std::copy(h_overlap.begin(), h_overlap.end(), overlap);
    std::copy(h_jclass.begin(), h_jclass.end(), jclass);
    return GK_OK;
}

}  // extern "C"
