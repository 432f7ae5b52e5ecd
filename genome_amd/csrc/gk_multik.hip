// gk_multik.hip — multi-k assembly: the contigs of a graph of one k, cut into the k-mers of a larger k and added to a count table
// (the k-iteration of IDBA / SPAdes: the small-k contigs carry the connectivity across coverage dips into the large-k table).
//
// Reference: none; the reference builds its graph at one k.  The rule is this project's own and stated in include/genome_amd.h
// ("multi-k"); tests/multik_ref.py restates it.
//
// k_mk_classify: one wave per live edge takes the contigs' class (gk_fastaout.h: wave_contig_class, the contig plan's comparison)
// and a lane sizes the edge: its runs of MK_RUN consecutive windows and what the last run lacks.  Two scans (gk_scan.h) give every
// edge its first run and the keys before it.  k_mk_emit is run-centric: a lane takes one run, finds its edge by binary search in the
// run offsets, builds the first window from the node k-mer and the pool (window_at, no per-base loop), rolls window and reverse
// complement through the rest and stores canonical keys and the weight, densely.  The host loop hands a bounded chunk of runs at a
// time to the table's insert of counted device keys (map_add_counted_keys_dev), so scratch does not grow with the graph and an
// edge of 10^7 bases is spread over the device like any other.  Integers only; no LDS and no atomics in the emit kernel.
//
// Roofline: the emission reads 2 bits and writes 8 or 16 bytes + 4 per window; the insert behind it is one random table update per
// window — the random-access rate of HBM, as gk_graph_edge_coverage's one probe per window over the same graph.
#include <algorithm>

#include "gk_fastaout.h"
#include "gk_scan.h"

static constexpr u64 MK_RUN = 16;                    // consecutive windows of one contig per lane
static constexpr u64 MK_CHUNK_WINDOWS = 1ull << 24;  // windows per chunk of the host loop: 320 MiB of keys and counts at 16-byte keys
// device counters of a call: the four classes, the windows, "an edge of more than 2^32-1 runs"
enum { MS_SHORT = 0, MS_FORWARD, MS_SELF, MS_REVERSE, MS_WINDOWS, MS_OVERFLOW, MS_N };

// runs[e] = the runs of edge e (0: dead, short or reverse), pad[e] = 16 * runs - windows: what its last run lacks
__global__ __launch_bounds__(BLOCK) void k_mk_classify(GraphView g, int k2, u32 *__restrict__ runs, u32 *__restrict__ pad, unsigned long long *stats) {
    const int lane = threadIdx.x & 63;
    const u64 waves = (u64)gridDim.x * (BLOCK / 64);
    unsigned long long cnt[4] = {0, 0, 0, 0}, windows = 0, over = 0;
    for (u64 e = (u64)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); e < g.n_edges; e += waves) {      // (uniform over the wave)
        if (!g.e_alive[e]) {
            if (lane == 0) { runs[e] = 0; pad[e] = 0; }
            continue;
        }
        const uint8_t c = wave_contig_class(g, e, (u64)k2);
        if (lane == 0) {
            u64 r = 0, p = 0;
            if (c == CLS_FORWARD || c == CLS_SELF) {
                const u64 nwin = (u64)g.k + g.e_len[e] - (u64)k2 + 1;
                r = (nwin + MK_RUN - 1) / MK_RUN;
                if (r > 0xffffffffull) { over = 1; r = 0; }
                else { p = r * MK_RUN - nwin; windows += nwin; }
            }
            runs[e] = (u32)r; pad[e] = (u32)p;
            cnt[c - CLS_SHORT]++;
        }
    }
    if (lane == 0) {
        for (int i = 0; i < 4; i++) if (cnt[i]) atomicAdd(&stats[MS_SHORT + i], cnt[i]);
        if (windows) atomicAdd(&stats[MS_WINDOWS], windows);
        if (over) atomicAdd(&stats[MS_OVERFLOW], over);
    }
}

struct MkPlan {
    const unsigned long long *run_off;   // [n_edges + 1]: the first run of every edge; run_off[n_edges] = all runs
    const unsigned long long *pad_off;   // [n_edges + 1]: what the last runs of the edges before it lack
};
// the key index of run r's first window: the last e in [0, n_edges] with run_off[e] <= r owns it (n_edges: r = all runs), and
// every run before r is full but the last runs of the edges before e
__device__ __forceinline__ u64 mk_run_pos(const MkPlan &p, u64 n_edges, u64 r, u64 *edge) {
    u64 lo = 0, hi = n_edges + 1;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (p.run_off[mid] <= r) lo = mid; else hi = mid;
    }
    *edge = lo;
    return r * MK_RUN - p.pad_off[lo];
}
template <int W> __device__ __forceinline__ void mk_store(u64 *__restrict__ keys, i32 *__restrict__ counts, u64 at, Kmer<W> x, Kmer<W> rc, u32 weight) {
    const bool fwd = ref_hash(x) < ref_hash(rc);             // (FreqFilter's rule: a tie goes to the reverse complement)
    const Kmer<W> y = fwd ? x : rc;
    if constexpr (W == 1) keys[at] = y.lo;
    else { keys[2 * at] = y.lo; keys[2 * at + 1] = y.hi; }
    counts[at] = (i32)weight;
}
// Runs [r0, r1) of the plan, r0 < r1 <= all runs; pos0 = the key index of run r0's first window.  keys / counts receive the windows
// of these runs densely, in run order; *pos1 = the key index of run r1's first window (the keys written: *pos1 - pos0).
template <int W>
__global__ __launch_bounds__(BLOCK) void k_mk_emit(GraphView g, MkPlan p, int k2, u32 weight, u64 r0, u64 r1, u64 pos0, u64 *__restrict__ keys,
                                                   i32 *__restrict__ counts, unsigned long long *pos1) {
    const u64 gid = (u64)blockIdx.x * BLOCK + threadIdx.x;
    u64 e;
    if (gid == 0) *pos1 = mk_run_pos(p, g.n_edges, r1, &e);
    for (u64 r = r0 + gid; r < r1; r += (u64)gridDim.x * BLOCK) {
        const u64 at = mk_run_pos(p, g.n_edges, r, &e) - pos0;
        const u64 nwin = (u64)g.k + g.e_len[e] - (u64)k2 + 1;
        const u64 d0 = (r - p.run_off[e]) * MK_RUN, d1 = min(d0 + MK_RUN, nwin);
        const u32 s = g.e_start[e];
        const Kmer<2> node{g.node_lo[s], g.k > 32 ? g.node_hi[s] : 0ull};
        const uint8_t *seq = g.pool + g.e_off[e];
        Kmer<W> x = window_at<W>(node, seq, g.k, k2, d0), rc = revcomp(x, k2);
        mk_store<W>(keys, counts, at, x, rc, weight);
        // window d + 1 ends with base d + k2 of the path: k2 > k, so it is base q = d + k2 - k of the edge, one pool byte per four steps
        u64 q = d0 + (u64)(k2 - g.k);
        u32 byte = (q & 3) && d0 + 1 < d1 ? seq[q >> 2] : 0u;
        for (u64 d = d0; d + 1 < d1; d++, q++) {
            if ((q & 3) == 0) byte = seq[q >> 2];
            const int b = (int)(byte >> ((q & 3) * 2)) & 3;
            x = append_base(x, b, k2);
            rc = prepend_base(3 - b, rc, k2);
            mk_store<W>(keys, counts, at + (d + 1 - d0), x, rc, weight);
        }
    }
}

extern "C" {

int gk_map_add_graph_paths(gk_map *dst, gk_graph *g, uint32_t weight, uint64_t *stats6) {
    if (stats6) for (int i = 0; i < 6; i++) stats6[i] = 0;
    if (!dst || !dst->ctx) return fail(g ? g->ctx : nullptr, GK_E_INVALID, "gk_map_add_graph_paths: null map handle");
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (dst->ctx != ctx) return fail(ctx, GK_E_INVALID, "gk_map_add_graph_paths: the map belongs to another context");
    if (dst->k <= g->k) return fail(ctx, GK_E_INVALID, "gk_map_add_graph_paths: the map's k must be larger than the graph's");
    if (weight == 0 || weight > 65535) return fail(ctx, GK_E_INVALID, "gk_map_add_graph_paths: weight is 1..65535");
    ctx->multik_last_chunks = 0;
    const GraphView &v = g->v;
    const u64 ne = v.n_edges;
    if (ne == 0) return GK_OK;
    const int k2 = dst->k;
    DevScratch tmp(ctx);
    u32 *d_runs = nullptr, *d_pad = nullptr;
    unsigned long long *d_roff = nullptr, *d_poff = nullptr, *d_stats = nullptr, *d_pos1 = nullptr, h_stats[MS_N] = {}, h_runs = 0;
    tmp.get(&d_runs, ne);
    tmp.get(&d_pad, ne);
    tmp.get(&d_roff, ne + 1);
    tmp.get(&d_poff, ne + 1);
    tmp.zeroed(&d_stats, MS_N);
    tmp.get(&d_pos1, 1);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_map_add_graph_paths: per-edge scratch");
    hipLaunchKernelGGL(k_mk_classify, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, k2, d_runs, d_pad, d_stats);
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, scan_counts(ctx, tmp, d_runs, ne, d_roff));
    GK_HIP(ctx, scan_counts(ctx, tmp, d_pad, ne, d_poff));
    GK_HIP(ctx, read_back(ctx, {{h_stats, d_stats, sizeof(h_stats)}, {&h_runs, d_roff + ne, 8}}));
    if (h_stats[MS_OVERFLOW]) return fail(ctx, GK_E_CAPACITY, "gk_map_add_graph_paths: an edge of 2^36 windows or more");
    // the chunks: a bounded number of runs each, their keys and counts in two buffers reused by every chunk
    const u64 cw = ctx->hook_multik_chunk_windows > 0 ? (u64)ctx->hook_multik_chunk_windows : MK_CHUNK_WINDOWS;      // ("test_multik_chunk_windows")
    const u64 chunk_runs = std::max<u64>(1, cw / MK_RUN);
    const u64 buf_keys = std::min<u64>(chunk_runs, h_runs) * MK_RUN;
    u64 *d_keys = nullptr;
    i32 *d_counts = nullptr;
    if (h_runs) {
        tmp.get(&d_keys, buf_keys * (u64)dst->W);
        tmp.get(&d_counts, buf_keys);
        if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_map_add_graph_paths: key buffer");
    }
    const MkPlan plan{d_roff, d_poff};
    unsigned long long pos0 = 0, pos1 = 0;
    for (u64 r0 = 0; r0 < h_runs; r0 += chunk_runs) {
        const u64 r1 = std::min(r0 + chunk_runs, (u64)h_runs);
        GK_BY_W(dst->W, hipLaunchKernelGGL((k_mk_emit<W>), dim3(ggrid(ctx, r1 - r0)), dim3(BLOCK), 0, ctx->stream, v, plan, k2, (u32)weight, r0, r1, (u64)pos0,
                                           d_keys, d_counts, d_pos1));
        GK_HIP(ctx, read_back(ctx, &pos1, d_pos1));
        if (pos1 < pos0 || pos1 - pos0 > buf_keys) return fail(ctx, GK_E_STATE, "gk_map_add_graph_paths: the run offsets are inconsistent");
        if (int rc = map_add_counted_keys_dev(dst, d_keys, d_counts, pos1 - pos0)) return rc;
        pos0 = pos1;
        ctx->multik_last_chunks++;
    }
    if (stats6) {
        stats6[1] = h_stats[MS_SHORT]; stats6[2] = h_stats[MS_FORWARD]; stats6[3] = h_stats[MS_SELF]; stats6[4] = h_stats[MS_REVERSE];
        stats6[0] = stats6[1] + stats6[2] + stats6[3] + stats6[4];
        stats6[5] = h_stats[MS_WINDOWS];
    }
    return GK_OK;
}

}  // extern "C"
