// gk_chains.h — the front end of a call that takes a chain list: gk_graph_scaffolds_plan[_overlaps] (gk_scaffolds.hip),
// gk_graph_fill_gaps (gk_fillgaps.hip) and gk_graph_overlap_gaps (gk_overlaps.hip).
//
// `members`, `chain_off` and `gap` are the caller's and are not trusted: no chain is empty, chain_off starts at 0 and ascends,
// every member is a live edge and occurs once.  The ids index device arrays, so NO KERNEL READS A MEMBER'S LENGTH BEFORE
// k_scaf_check HAS PASSED: chains_begin makes the host-side checks, uploads the list and queues k_scaf_check; every kernel behind
// it opens with chains_unchecked / chains_bad and returns at once behind a raised flag; chains_failed turns the flags read back
// into the call's error.  k_chain_junctions classes the junction after every member for the stages that search some of them
// (fill, overlap), by a stage's rule; k_chain_list compacts the junctions to search.
#pragma once

#include "gk_graph.h"

// error flags of the check and of the passes behind it (a stage's own flags follow SF_N)
enum { SF_BAD_ID = 0, SF_DUPLICATE, SF_CHAIN, SF_GAP, SF_OVERFLOW, SF_OVERLAP, SF_N };

// ---------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------
// k_scaf_check raised a flag: the members' ids may index nothing (the guard of the kernels that raise SF_GAP themselves)
__device__ __forceinline__ bool chains_unchecked(const u32 *flags) { return flags[SF_BAD_ID] | flags[SF_DUPLICATE] | flags[SF_CHAIN]; }
__device__ __forceinline__ bool chains_bad(const u32 *flags) { return chains_unchecked(flags) | flags[SF_GAP]; }
// the chain of member j: the last c with chain_off[c] <= j
__device__ __forceinline__ u64 chain_of_member(const unsigned long long *__restrict__ chain_off, u64 nchains, u64 j) {
    u64 lo = 0, hi = nchains;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (chain_off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// one lane per member claims its edge's owner word (a second claim is a duplicate); one lane per chain looks at its bounds
static __global__ __launch_bounds__(BLOCK) void k_scaf_check(GraphView g, const u32 *__restrict__ members, const unsigned long long *__restrict__ chain_off, u64 nchains,
                                                             u64 nm, u32 *owner, u32 *flags) {
    const u64 items = max(nm, nchains);
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < items; i += (u64)gridDim.x * BLOCK) {
        if (i < nchains && !(chain_off[i] < chain_off[i + 1])) flags[SF_CHAIN] = 1;      // (empty, or not ascending)
        if (i < nm) {
            const u32 e = members[i];
            if ((u64)e >= g.n_edges || !g.e_alive[e]) flags[SF_BAD_ID] = 1;
            else if (atomicCAS(&owner[e], 0u, 1u) != 0u) flags[SF_DUPLICATE] = 1;
        }
    }
}

// The junction after member j, one lane per member, behind a clean check: the last of its chain, adjacent in the graph, or by
// `rule.decide(g, e, f, G, &cls)` — the class of a junction between e and f that is not adjacent and whose gap G fits
// +-(2^31-1) (any other raises SF_GAP: the call fails and the class is not read), and whether it is to be searched.
static_assert(GK_FILL_LAST == 0 && GK_OVL_LAST == 0 && GK_FILL_ADJACENT == 1 && GK_OVL_ADJACENT == 1, "k_chain_junctions writes the two classes the stages share");
template <class Rule>
static __global__ __launch_bounds__(BLOCK) void k_chain_junctions(GraphView g, const u32 *__restrict__ members, const unsigned long long *__restrict__ chain_off, u64 nchains,
                                                                  u64 nm, const long long *__restrict__ gap, Rule rule, u32 *flags, uint8_t *__restrict__ jclass,
                                                                  u32 *__restrict__ search) {
    if (chains_unchecked(flags)) return;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nm; j += (u64)gridDim.x * BLOCK) {
        uint8_t cls = GK_FILL_LAST;
        u32 s = 0;
        if (j + 1 != chain_off[chain_of_member(chain_off, nchains, j) + 1]) {
            const u32 e = members[j], f = members[j + 1];
            if (g.e_end[e] == g.e_start[f]) cls = GK_FILL_ADJACENT;
            else {
                const long long G = gap[j];
                if (G > 0x7fffffffll || G < -0x7fffffffll) flags[SF_GAP] = 1;
                else s = rule.decide(g, e, f, G, &cls);
            }
        }
        jclass[j] = cls; search[j] = s;
    }
}
static __global__ __launch_bounds__(BLOCK) void k_chain_list(u64 nm, const u32 *__restrict__ flags, const u32 *__restrict__ search, const unsigned long long *__restrict__ rank,
                                                             u32 *__restrict__ list) {
    if (chains_bad(flags)) return;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nm; j += (u64)gridDim.x * BLOCK)
        if (search[j]) list[rank[j]] = (u32)j;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct ChainList {                       // a call's chain list on the device, in the call's DevScratch
    u64 nchains = 0, nm = 0;             // nm: members
    u32 *d_members = nullptr, *d_owner = nullptr, *d_flags = nullptr;      // owner: a word per edge id, 1 for a member behind the check
    long long *d_gap = nullptr;
    unsigned long long *d_chain_off = nullptr;
};

// The host-side checks of the list, its upload into `tmp`, zeroed owner and flags (`nflags` >= SF_N words) and k_scaf_check, queued.
// A list without members passes (the scaffold plan still writes the edges in no chain; the other entries return before this).
static int chains_begin(const char *who, gk_graph *g, DevScratch &tmp, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap,
                        int nflags, ChainList *cl) {
    gk_ctx *ctx = g->ctx;
    const u64 ne = g->v.n_edges;
    if (nchains && !chain_off) return fail(ctx, GK_E_INVALID, std::string(who) + ": chain_off is NULL");
    // an edge occurs once at most and no chain is empty: more chains or members than edge ids cannot be right
    if (nchains > ne) return fail(ctx, GK_E_INVALID, std::string(who) + ": more chains than edge ids");
    const u64 nm = nchains ? chain_off[nchains] : 0;
    if (nchains && (chain_off[0] != 0 || nm < nchains || nm > ne)) return fail(ctx, GK_E_INVALID, std::string(who) + ": chain_off does not start at 0, holds an empty chain, or lists more members than there are edge ids");
    if (nm && (!members || !gap)) return fail(ctx, GK_E_INVALID, std::string(who) + ": members or gap is NULL");
    cl->nchains = nchains; cl->nm = nm;
    const u64 zero_off[1] = {0};
    if (nm) { tmp.upload(&cl->d_members, members, nm); tmp.upload(&cl->d_gap, gap, nm); }
    else { tmp.get(&cl->d_members, 1); tmp.get(&cl->d_gap, 1); }
    tmp.upload(&cl->d_chain_off, nchains ? chain_off : zero_off, nchains + 1);
    tmp.zeroed(&cl->d_owner, ne);
    tmp.zeroed(&cl->d_flags, nflags);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), (std::string(who) + ": scratch").c_str());
    hipLaunchKernelGGL(k_scaf_check, dim3(ggrid(ctx, std::max(nm, (u64)nchains))), dim3(BLOCK), 0, ctx->stream, g->v, cl->d_members, cl->d_chain_off, (u64)nchains, nm,
                       cl->d_owner, cl->d_flags);
    return GK_OK;
}

// the call's error if a flag of the list is up.  `gap_both_sides`: the stage refused a gap below -(2^31-1) too (the plan clamps it)
static int chains_failed(const char *who, gk_ctx *ctx, const u32 *h_flags, bool gap_both_sides) {
    if (h_flags[SF_CHAIN]) return fail(ctx, GK_E_INVALID, std::string(who) + ": an empty chain, or a chain_off that does not ascend");
    if (h_flags[SF_BAD_ID]) return fail(ctx, GK_E_INVALID, std::string(who) + ": a member that is no live edge of this graph");
    if (h_flags[SF_DUPLICATE]) return fail(ctx, GK_E_INVALID, std::string(who) + ": an edge occurs twice in the chains");
    if (h_flags[SF_GAP]) return fail(ctx, GK_E_INVALID, std::string(who) + (gap_both_sides ? ": a gap beyond +-(2^31-1) at a junction that is not adjacent" : ": a gap above 2^31-1"));
    return GK_OK;
}
