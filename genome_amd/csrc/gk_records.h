// gk_records.h — a table's records as planes, grouped by owner rank (gk_links.h: rec_bucket), for the two tables that travel
// that way: the link table (gk_links.hip) and the span table (gk_spans.hip).  support_bucket's three launches (gk_pairs.hip) with
// a third plane and the table read through a source type:
//   struct Src { u64 cap; __device__ bool get(u64 slot, const RecCanon &c, u64 *key, u32 *cnt, u64 *x) const; }
// get: false for a free slot, and for a record that names an edge outside the canonical numbering (it raises *c.bad).
#pragma once

#include <vector>

#include "gk_graph.h"
#include "gk_links.h"
#include "gk_scan.h"

namespace gk {
struct RecCanon { const u32 *canon; const uint8_t *dup; u64 nmap; u32 *bad; };
// local edge id -> canonical id; NONE, and *bad raised, for an id that is dead, out of range or a duplicate path.  No map: the id.
__device__ __forceinline__ u32 rec_canon_id(const RecCanon &c, u32 id) {
    if (!c.canon) return id;
    const u32 v = id < c.nmap && !c.dup[id] ? c.canon[id] : NONE;
    if (v == NONE) *c.bad = 1u;
    return v;
}
// The owner rank of a record: splitmix64's finalizer over the key plane, NOT mix64, by which the shard tables place their keys
// (sup_owner's reason, gk_pairs.hip).
__device__ __forceinline__ u32 rec_owner(u64 key, u32 P) {
    key ^= key >> 30; key *= 0xbf58476d1ce4e5b9ULL;
    key ^= key >> 27; key *= 0x94d049bb133111ebULL;
    key ^= key >> 31;
    return (u32)(((key >> 32) * (u64)P) >> 32);
}
// the live slots of workgroup w's contiguous `chunk` of the table, counted per owner in LDS -> counts[p * nwg + w]
template <class Src>
__global__ __launch_bounds__(BLOCK) void k_rec_bucket_count(Src s, u64 chunk, u32 P, RecCanon c, u32 *__restrict__ counts) {
    __shared__ u32 hist[64];
    for (u32 p = threadIdx.x; p < 64; p += BLOCK) hist[p] = 0;
    __syncthreads();
    const u64 a = (u64)blockIdx.x * chunk, b = min(a + chunk, s.cap);
    for (u64 i = a + threadIdx.x; i < b; i += BLOCK) {
        u64 key, x;
        u32 cnt;
        if (s.get(i, c, &key, &cnt, &x)) atomicAdd(&hist[rec_owner(key, P)], 1u);
    }
    __syncthreads();
    for (u32 p = threadIdx.x; p < P; p += BLOCK) counts[(u64)p * gridDim.x + blockIdx.x] = hist[p];
}
// the same slots again, each record written at its (owner, workgroup) offset + its rank among them (an LDS cursor), plane by plane
template <class Src>
__global__ __launch_bounds__(BLOCK) void k_rec_bucket_scatter(Src s, u64 chunk, u32 P, RecCanon c, const unsigned long long *__restrict__ off, RecPlanes out) {
    __shared__ u32 cursor[64];
    for (u32 p = threadIdx.x; p < 64; p += BLOCK) cursor[p] = 0;
    __syncthreads();
    const u64 a = (u64)blockIdx.x * chunk, b = min(a + chunk, s.cap);
    for (u64 i = a + threadIdx.x; i < b; i += BLOCK) {
        u64 key, x;
        u32 cnt;
        if (!s.get(i, c, &key, &cnt, &x)) continue;
        const u32 p = rec_owner(key, P);
        const u64 at = off[(u64)p * gridDim.x + blockIdx.x] + atomicAdd(&cursor[p], 1u);
        out.key[at] = key;
        out.cnt[at] = cnt;
        out.x[at] = x;
    }
}
static __global__ void k_rec_regions(const unsigned long long *off, u64 nwg, u32 P, unsigned long long *region) {
    for (u32 p = threadIdx.x; p <= P; p += blockDim.x) region[p] = off[(u64)p * nwg];
}
// canonical ids of the key plane (and, x_is_edge, of the extra plane) back to this replica's ids, in place
static __global__ __launch_bounds__(BLOCK) void k_rec_uncanon(RecPlanes p, u64 n, bool x_is_edge, const u32 *__restrict__ inv, u64 nlive, u32 *bad) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) {
        const u64 key = p.key[i], a = key >> 32, b = key & 0xffffffffull, x = x_is_edge ? p.x[i] : 0;
        if (a >= nlive || b >= nlive || x >= nlive) { *bad = 1u; continue; }
        p.key[i] = ((u64)inv[a] << 32) | inv[b];
        if (x_is_edge) p.x[i] = inv[x];
    }
}

template <class Src>
int records_bucket(gk_ctx *ctx, const Src &s, int P, const RecPlanes &out, u64 room, u64 *region, const u32 *canon, const uint8_t *dup, u64 nmap, const char *what) {
    if (P < 1 || P > 64) return fail(ctx, GK_E_INVALID, "records_bucket: 1..64 owners (the world limit of gk_dist_create)");
    for (int p = 0; p <= P; p++) region[p] = 0;
    if (s.cap == 0) return GK_OK;
    const u64 nwg = (u64)ggrid(ctx, s.cap), chunk = (s.cap + nwg - 1) / nwg, n = nwg * (u64)P;
    DevScratch tmp(ctx);
    u32 *d_counts = nullptr, *d_bad = nullptr, h_bad = 0;
    unsigned long long *d_off = nullptr, *d_region = nullptr;
    tmp.get(&d_counts, n);
    tmp.get(&d_off, n + 1);
    tmp.get(&d_region, (u64)P + 1);
    tmp.zeroed(&d_bad, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "records_bucket: scratch");
    const RecCanon c{canon, dup, nmap, d_bad};
    hipLaunchKernelGGL(k_rec_bucket_count<Src>, dim3((unsigned)nwg), dim3(BLOCK), 0, ctx->stream, s, chunk, (u32)P, c, d_counts);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_counts, n, d_off));
    hipLaunchKernelGGL(k_rec_regions, dim3(1), dim3(64), 0, ctx->stream, d_off, nwg, (u32)P, d_region);
    std::vector<unsigned long long> h(P + 1);
    GK_HIP(ctx, read_back(ctx, {{h.data(), d_region, (size_t)(P + 1) * 8}, {&h_bad, d_bad, 4}}));
    if (h_bad) return fail(ctx, GK_E_STATE, std::string(what) + " name an edge that is dead in this graph, or whose path another live edge has too");
    if (h[P] > room) return fail(ctx, GK_E_STATE, "records_bucket: " + std::to_string(h[P]) + " live slots, room for " + std::to_string(room));
    if (h[P]) {
        hipLaunchKernelGGL(k_rec_bucket_scatter<Src>, dim3((unsigned)nwg), dim3(BLOCK), 0, ctx->stream, s, chunk, (u32)P, c, d_off, out);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, hipStreamSynchronize(ctx->stream));         // (the scratch goes with this scope)
    }
    for (int p = 0; p <= P; p++) region[p] = h[p];
    return GK_OK;
}
inline int records_uncanon(gk_ctx *ctx, const RecPlanes &p, u64 n, bool x_is_edge, const u32 *d_inv, u64 nlive) {
    if (n == 0) return GK_OK;
    DevScratch tmp(ctx);
    u32 *d_bad = nullptr, h_bad = 0;
    GK_HIP(ctx, tmp.zeroed(&d_bad, 1));
    hipLaunchKernelGGL(k_rec_uncanon, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, p, n, x_is_edge, d_inv, nlive, d_bad);
    GK_HIP(ctx, read_back(ctx, &h_bad, d_bad));
    if (h_bad) return fail(ctx, GK_E_STATE, "records_uncanon: a record outside the canonical edge numbering");
    return GK_OK;
}
}  // namespace gk
