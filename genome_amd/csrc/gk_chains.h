// gk_chains.h — the check of a chain list (members, chain_off) that gk_scaffolds.hip, gk_fillgaps.hip and gk_overlaps.hip share: it runs before any
// kernel reads a member's length, and its owner words say afterwards which edges are members.
#pragma once

#include "gk_graph.h"

// error flags of the check and of the passes behind it
enum { SF_BAD_ID = 0, SF_DUPLICATE, SF_CHAIN, SF_GAP, SF_OVERFLOW, SF_OVERLAP, SF_N };

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
