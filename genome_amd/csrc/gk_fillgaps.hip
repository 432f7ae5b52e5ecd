// gk_fillgaps.hip — gap filling: where the graph holds exactly one path of the right length between two consecutive members of a
// chain, the path's edges become members, so that the scaffold text joins them instead of writing N.
//
// The rule is this project's own and stated in include/genome_amd.h ("gap filling"); tests/fillgaps_ref.py restates it.  The chain
// list comes from gk_scaffold_chains and goes on to gk_graph_scaffolds_plan; its front end, the check included, is gk_chains.h's.
//
// k_chain_junctions by FillRule: adjacent / B < 1 / to be searched; a scan compacts the junctions to search.
// k_fill_search: one wave per junction builds the tree of bounded paths in LDS, level by level, forward from end(e) and, only if
// that tree outgrows max_paths, backward from start(f); hits are counted by ballot and a unique one is unwound into HBM.
// k_fill_uses: one atomic add per path edge.  k_fill_resolve: shared or filled, the output count per member and the stats.  A scan
// and k_fill_write place the members.  Nothing but scratch is written on the device; the host copies out after one read-back.
#include <vector>

#include "gk_chains.h"
#include "gk_scan.h"

static_assert(GK_FILL_MAX_PATHS <= 0xffff, "a parent index is 16 bits, 0xffff the root");
static_assert(GK_FILL_MAX_EDGES <= 64, "a path is unwound by one wave");
static constexpr uint8_t FC_UNIQUE = 7;                      // a candidate, between the search and the resolution
static constexpr uint16_t FILL_ROOT = 0xffff;
static constexpr int FILL_STATS = 10;
// device counters of a call; the flag behind the check's: a write beyond the output's bound (cannot happen by the rule)
enum { FS_ADJACENT = 0, FS_OVERFLOW, FS_NONE, FS_AMBIGUOUS, FS_SHARED, FS_FILLED, FS_EDGES, FS_BASES, FS_BACKWARD, FS_N };
enum { FF_INTERNAL = SF_N, FF_N };

// a junction that is neither adjacent nor out of the gap's range: none so far; B < 1 leaves nothing to search
struct FillRule {
    long long tol;
    __device__ u32 decide(const GraphView &g, u32, u32, long long G, uint8_t *cls) const {
        *cls = GK_FILL_NONE;
        return G + tol + (long long)g.k >= 1;
    }
};

// ---------------------------------------------------------------------------------------------
// the search: one wave per junction, the tree in LDS
// ---------------------------------------------------------------------------------------------
struct FillTree {                                            // entry i: a path, by its last edge and the entry of the path without it
    u32 edge[GK_FILL_MAX_PATHS];
    u32 sum[GK_FILL_MAX_PATHS];                              // (B < 2^32: |G| and tol are below 2^31)
    uint16_t parent[GK_FILL_MAX_PATHS];
};
struct FillFound { u32 hits, idx, depth; bool over; };       // uniform over the wave; idx / depth: the first hit's entry and edges

// FWD: all paths from `root` along out-edges; else all edge sequences backwards from `root` along in-edges.  Sum <= B, at most
// max_edges edges.  A hit ends (starts) in `target` with sum >= smin.  Stops with `over` the moment the entries pass max_paths.
template <bool FWD>
__device__ FillFound fill_tree(FillTree &T, const GraphView &g, const unsigned long long *__restrict__ in_off, const u32 *__restrict__ in_list, u32 root, u32 target,
                               u32 B, u32 smin, u32 max_edges, u32 max_paths) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    FillFound r{0, 0, 0, false};
    u32 n = 0, f0 = 0, f1 = 0;                               // entries; the frontier [f0, f1): the paths of level - 1 edges
    for (u32 level = 1; level <= max_edges; level++) {
        const u32 nf = level == 1 ? 1u : f1 - f0, n0 = n;
        for (u32 base = 0; base < nf; base += 64) {
            const u32 i = base + (u32)lane;
            u32 psum = 0, cnt = 0;
            u64 beg = 0;
            uint16_t pidx = FILL_ROOT;
            if (i < nf) {
                u32 node = root;
                if (level > 1) {
                    const u32 pe = T.edge[f0 + i];
                    node = FWD ? g.e_end[pe] : g.e_start[pe];
                    psum = T.sum[f0 + i]; pidx = (uint16_t)(f0 + i);
                }
                beg = FWD ? (u64)node * 4 : in_off[node];
                cnt = FWD ? 4u : (u32)(in_off[node + 1] - in_off[node]);      // (an in-list may be longer than four on an edited graph)
            }
            for (u32 s = 0; __any(s < cnt); s++) {
                bool ok = false;
                u32 c = NONE, csum = 0;
                if (s < cnt) {
                    c = FWD ? g.out_edge[beg + s] : in_list[beg + s];
                    // (backward: an edge displaced from its start node's out-edge word by gk_graph_replace_start is on no path, as forward)
                    if (c != NONE && g.e_alive[c] && (FWD || g.out_edge[(u64)g.e_start[c] * 4 + g.e_first[c]] == c)) {
                        const u64 len = g.e_len[c];
                        if (len <= (u64)(B - psum)) { ok = true; csum = psum + (u32)len; }
                    }
                }
                const unsigned long long mask = __ballot(ok);
                if (!mask) continue;
                const u32 at = n + (u32)__popcll(mask & below);
                if (ok && at < max_paths) { T.edge[at] = c; T.sum[at] = csum; T.parent[at] = pidx; }
                const unsigned long long hit = __ballot(ok && (FWD ? g.e_end[c] : g.e_start[c]) == target && csum >= smin);
                if (hit) {
                    if (!r.hits) { r.idx = (u32)__shfl((int)at, __ffsll((long long)hit) - 1); r.depth = level; }
                    r.hits += (u32)__popcll(hit);
                }
                n += (u32)__popcll(mask);
                if (n > max_paths) { r.over = true; return r; }
            }
        }
        wave_sync();                                    // the next level reads what this one appended
        f0 = n0; f1 = n;
        if (f0 == f1) break;
    }
    return r;
}

__global__ __launch_bounds__(BLOCK) void k_fill_search(GraphView g, const unsigned long long *__restrict__ in_off, const u32 *__restrict__ in_list,
                                                       const u32 *__restrict__ members, const long long *__restrict__ gap, long long tol, u32 max_edges,
                                                       u32 max_paths, const u32 *__restrict__ flags, const u32 *__restrict__ list,
                                                       const unsigned long long *__restrict__ nsearch, uint8_t *__restrict__ jclass, long long *__restrict__ jlen,
                                                       u32 *__restrict__ plen, uint8_t *__restrict__ back, u32 *__restrict__ path) {
    __shared__ FillTree lds[BLOCK / 64];
    if (chains_bad(flags)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FillTree &T = lds[wave];
    const u64 ns = *nsearch, waves = (u64)gridDim.x * (BLOCK / 64);
    for (u64 w = (u64)blockIdx.x * (BLOCK / 64) + wave; w < ns; w += waves) {       // (uniform over the wave)
        const u32 j = list[w];
        const u32 from = g.e_end[members[j]], to = g.e_start[members[j + 1]];
        const long long G = gap[j], k = g.k;
        const u32 B = (u32)(G + tol + k);                    // 1 .. 2^32-1: FillRule
        const u32 smin = (u32)max(G - tol + k, 0ll);         // L >= G - tol; L <= G + tol is sum <= B
        FillFound r = fill_tree<true>(T, g, in_off, in_list, from, to, B, smin, max_edges, max_paths);
        const bool backward = r.over;
        if (backward) {
            wave_sync();
            r = fill_tree<false>(T, g, in_off, in_list, to, from, B, smin, max_edges, max_paths);
        }
        if (lane == 0) {
            const uint8_t cls = r.over ? GK_FILL_OVERFLOW : r.hits == 0 ? GK_FILL_NONE : r.hits > 1 ? GK_FILL_AMBIGUOUS : FC_UNIQUE;
            jclass[j] = cls; back[j] = backward;
            if (cls == FC_UNIQUE) {                          // through the parents: last edge first in the forward tree, first edge first in the backward one
                u32 *p = path + (u64)j * max_edges;
                u32 at = r.idx;
                for (u32 i = 0; i < r.depth; i++) { p[backward ? i : r.depth - 1 - i] = T.edge[at]; at = T.parent[at]; }
                plen[j] = r.depth;
                jlen[j] = (long long)T.sum[r.idx] - k;
            }
        }
        wave_sync();                                    // the next junction reuses the tree
    }
}

// ---------------------------------------------------------------------------------------------
// uses, resolution, write-out
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_fill_uses(u64 nm, u32 max_edges, const u32 *__restrict__ flags, const uint8_t *__restrict__ jclass,
                                                     const u32 *__restrict__ plen, const u32 *__restrict__ path, u32 *use) {
    if (chains_bad(flags)) return;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < nm * max_edges; t += (u64)gridDim.x * BLOCK) {
        const u64 j = t / max_edges;
        if (jclass[j] == FC_UNIQUE && t - j * max_edges < plen[j]) atomicAdd(&use[path[t]], 1u);
    }
}
// a candidate is shared iff an edge of its path is a member (owner) or is used twice (by another candidate, or by this one)
__global__ __launch_bounds__(BLOCK) void k_fill_resolve(u64 nm, u32 max_edges, long long k, const u32 *__restrict__ flags, const u32 *__restrict__ owner,
                                                        const u32 *__restrict__ use, const u32 *__restrict__ plen, const u32 *__restrict__ path,
                                                        const long long *__restrict__ jlen, const uint8_t *__restrict__ back, uint8_t *__restrict__ jclass,
                                                        u32 *__restrict__ cnt, unsigned long long *stats) {
    if (chains_bad(flags)) return;
    unsigned long long st[FS_N] = {};
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nm; j += (u64)gridDim.x * BLOCK) {
        uint8_t cls = jclass[j];
        const u32 m = plen[j];
        if (cls == FC_UNIQUE) {
            bool shared = false;
            for (u32 i = 0; i < m; i++) { const u32 x = path[j * max_edges + i]; shared |= owner[x] != 0 || use[x] > 1; }
            jclass[j] = cls = shared ? GK_FILL_SHARED : GK_FILL_FILLED;
        }
        cnt[j] = 1 + (cls == GK_FILL_FILLED ? m : 0u);
        if (cls != GK_FILL_LAST) st[cls - GK_FILL_ADJACENT]++;
        if (cls == GK_FILL_FILLED) { st[FS_EDGES] += m; st[FS_BASES] += (unsigned long long)(jlen[j] + k); }
        st[FS_BACKWARD] += back[j];
    }
    for (int i = 0; i < FS_N; i++) {
        const unsigned long long v = wave_sum(st[i]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[i], v);
    }
}
// out_at = the scan of cnt; `cap` = the room of out_members / out_gap
__global__ __launch_bounds__(BLOCK) void k_fill_write(u64 nm, u64 nchains, u32 max_edges, long long k, u32 *flags, const u32 *__restrict__ members,
                                                      const unsigned long long *__restrict__ chain_off, const long long *__restrict__ gap,
                                                      const uint8_t *__restrict__ jclass, const u32 *__restrict__ plen, const u32 *__restrict__ path,
                                                      const unsigned long long *__restrict__ out_at, u64 cap, u32 *__restrict__ out_members,
                                                      long long *__restrict__ out_gap, unsigned long long *__restrict__ out_chain_off) {
    if (chains_bad(flags)) return;
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < max(nm, nchains + 1); j += (u64)gridDim.x * BLOCK) {
        if (j <= nchains) out_chain_off[j] = out_at[chain_off[j]];
        if (j >= nm) continue;
        const u64 o = out_at[j];
        const bool filled = jclass[j] == GK_FILL_FILLED;
        const u32 m = filled ? plen[j] : 0u;
        if (o + m >= cap) { flags[FF_INTERNAL] = 1; continue; }
        out_members[o] = members[j]; out_gap[o] = filled ? -k : gap[j];
        for (u32 i = 0; i < m; i++) { out_members[o + 1 + i] = path[j * max_edges + i]; out_gap[o + 1 + i] = -k; }
    }
}

extern "C" {

int gk_graph_fill_gaps(gk_graph *g, const uint32_t *members, const uint64_t *chain_off, uint64_t nchains, const int64_t *gap, uint64_t tol, uint32_t max_edges,
                       uint32_t max_paths, uint32_t *out_members, int64_t *out_gap, uint64_t members_cap, uint64_t *out_chain_off, uint8_t *jclass, int64_t *jlen,
                       uint64_t *n_members, uint64_t *stats10) {
    const char *who = "gk_graph_fill_gaps";
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (tol > 0x7fffffffull) return fail(ctx, GK_E_INVALID, std::string(who) + ": tol beyond 2^31-1");
    if (max_edges < 1 || max_edges > GK_FILL_MAX_EDGES) return fail(ctx, GK_E_INVALID, std::string(who) + ": max_edges outside 1 .. " + std::to_string(GK_FILL_MAX_EDGES));
    if (max_paths < 1 || max_paths > GK_FILL_MAX_PATHS) return fail(ctx, GK_E_INVALID, std::string(who) + ": max_paths outside 1 .. " + std::to_string(GK_FILL_MAX_PATHS));
    if (!out_chain_off || !n_members || !stats10) return fail(ctx, GK_E_INVALID, std::string(who) + ": out_chain_off, n_members or stats10 is NULL");
    if (nchains == 0) {                                      // (no chain, no member)
        out_chain_off[0] = 0; *n_members = 0;
        for (int i = 0; i < FILL_STATS; i++) stats10[i] = 0;
        return GK_OK;
    }
    if (!jclass || !jlen) return fail(ctx, GK_E_INVALID, std::string(who) + ": jclass or jlen is NULL");
    const GraphView &v = g->v;
    DevScratch tmp(ctx);
    ChainList cl;
    if (int rc = chains_begin(who, g, tmp, members, chain_off, nchains, gap, FF_N, &cl)) return rc;
    const u64 ne = v.n_edges, nm = cl.nm;
    // no edge is written twice (a filled path's edges are no members and lie on no other filled path): the output fits the edge ids
    const u64 cap = std::min<u64>(ne, nm + (nm - nchains) * max_edges);
    u32 *d_search = nullptr, *d_list = nullptr, *d_plen = nullptr, *d_path = nullptr, *d_use = nullptr, *d_cnt = nullptr, *d_out_members = nullptr, *d_in_list = nullptr,
        h_flags[FF_N] = {};
    uint8_t *d_jclass = nullptr, *d_back = nullptr;
    long long *d_jlen = nullptr, *d_out_gap = nullptr;
    unsigned long long *d_rank = nullptr, *d_out_at = nullptr, *d_out_chain_off = nullptr, *d_stats = nullptr, *d_in_off = nullptr, h_stats[FS_N] = {}, h_n = 0;
    tmp.zeroed(&d_use, ne);
    tmp.zeroed(&d_stats, FS_N);
    tmp.get(&d_jclass, nm);
    tmp.zeroed(&d_back, nm);                                 // (zero: only the search writes these three, and only where it has something to say)
    tmp.zeroed(&d_jlen, nm);
    tmp.zeroed(&d_plen, nm);
    tmp.zeroed(&d_search, nm);                               // (zero, like cnt: behind a raised flag nothing writes them, and the scans still run)
    tmp.get(&d_rank, nm + 1);
    tmp.get(&d_list, nm);
    tmp.get(&d_path, nm * max_edges);                        // max_edges ids per junction, used or not: 64 bytes each at the default 16
    tmp.zeroed(&d_cnt, nm);
    tmp.get(&d_out_at, nm + 1);
    tmp.get(&d_out_members, cap);
    tmp.get(&d_out_gap, cap);
    tmp.get(&d_out_chain_off, nchains + 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_graph_fill_gaps: scratch");
    if (int rc = graph_in_lists(g, tmp, who, &d_in_off, &d_in_list)) return rc;
    // the junctions behind the check; every later kernel returns at once behind a raised flag
    hipLaunchKernelGGL(k_chain_junctions<FillRule>, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, v, cl.d_members, cl.d_chain_off, (u64)nchains, nm, cl.d_gap,
                       FillRule{(long long)tol}, cl.d_flags, d_jclass, d_search);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_search, nm, d_rank));
    hipLaunchKernelGGL(k_chain_list, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, nm, cl.d_flags, d_search, d_rank, d_list);
    hipLaunchKernelGGL(k_fill_search, dim3(ggrid(ctx, (nm - nchains) * 64)), dim3(BLOCK), 0, ctx->stream, v, d_in_off, d_in_list, cl.d_members, cl.d_gap, (long long)tol,
                       max_edges, max_paths, cl.d_flags, d_list, d_rank + nm, d_jclass, d_jlen, d_plen, d_back, d_path);
    hipLaunchKernelGGL(k_fill_uses, dim3(ggrid(ctx, nm * max_edges)), dim3(BLOCK), 0, ctx->stream, nm, max_edges, cl.d_flags, d_jclass, d_plen, d_path, d_use);
    hipLaunchKernelGGL(k_fill_resolve, dim3(ggrid(ctx, nm)), dim3(BLOCK), 0, ctx->stream, nm, max_edges, (long long)v.k, cl.d_flags, cl.d_owner, d_use, d_plen, d_path, d_jlen,
                       d_back, d_jclass, d_cnt, d_stats);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_cnt, nm, d_out_at));
    hipLaunchKernelGGL(k_fill_write, dim3(ggrid(ctx, std::max(nm, (u64)nchains + 1))), dim3(BLOCK), 0, ctx->stream, nm, (u64)nchains, max_edges, (long long)v.k, cl.d_flags,
                       cl.d_members, cl.d_chain_off, cl.d_gap, d_jclass, d_plen, d_path, d_out_at, cap, d_out_members, d_out_gap, d_out_chain_off);
    std::vector<u32> h_members(cap);
    std::vector<long long> h_gap(cap), h_jlen(nm);
    std::vector<unsigned long long> h_chain_off(nchains + 1);
    std::vector<uint8_t> h_jclass(nm);
    GK_HIP(ctx, read_back(ctx, {{h_flags, cl.d_flags, sizeof(h_flags)}, {h_stats, d_stats, sizeof(h_stats)}, {&h_n, d_out_at + nm, 8}, {h_members.data(), d_out_members, cap * 4},
                                {h_gap.data(), d_out_gap, cap * 8}, {h_chain_off.data(), d_out_chain_off, (nchains + 1) * 8}, {h_jclass.data(), d_jclass, nm},
                                {h_jlen.data(), d_jlen, nm * 8}}));
    if (int rc = chains_failed(who, ctx, h_flags, true)) return rc;
    if (h_flags[FF_INTERNAL] || h_n > cap) return fail(ctx, GK_E_STATE, std::string(who) + ": the filled chains outgrew the edge ids (internal error)");
    if (members_cap >= h_n && (!out_members || !out_gap)) return fail(ctx, GK_E_INVALID, std::string(who) + ": out_members or out_gap is NULL");
    u64 st[FILL_STATS] = {};
    for (int i = 0; i < 6; i++) { st[1 + i] = h_stats[i]; st[0] += h_stats[i]; }
    st[7] = h_stats[FS_EDGES]; st[8] = h_stats[FS_BASES]; st[9] = h_stats[FS_BACKWARD];
    *n_members = h_n;
    for (int i = 0; i < FILL_STATS; i++) stats10[i] = st[i];
    if (members_cap < h_n) return fail(ctx, GK_E_CAPACITY, std::string(who) + ": need room for " + std::to_string(h_n) + " members");
    std::copy(h_members.begin(), h_members.begin() + h_n, out_members);
    std::copy(h_gap.begin(), h_gap.begin() + h_n, out_gap);
    std::copy(h_chain_off.begin(), h_chain_off.end(), out_chain_off);
    std::copy(h_jclass.begin(), h_jclass.end(), jclass);
    std::copy(h_jlen.begin(), h_jlen.end(), jlen);
    return GK_OK;
}

}  // extern "C"
