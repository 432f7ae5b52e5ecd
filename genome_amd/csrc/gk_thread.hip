// gk_thread.hip — reads threaded through the graph: every window of every read is looked up in the position map, and a window
// that is a node's k-mer names the in-edge the read arrived by and the out-edge it left by: support[(in, out)] += 1.  The rule is
// this project's own and stated in include/genome_amd.h (gk_graph_thread_reads); tests/thread_ref.py restates it.
//
// Reference: none.  GraphSimplifier.scala:213-217 looks at p1.take(k) and p2.take(k) of a pair and drops the rest of both mates.
//
// Shape: k_correct_reads' (gk_correct.hip).  A workgroup stages 64 records in LDS, a wave takes a record, its lanes take windows
// 64 at a time.  One bit-range extraction gives window i of the read and, reverse-complemented, window n-1-i of the other strand;
// both go to the position map (gk_vmap_probe.h), and what comes back — nothing, several positions, or the one — is left in a
// per-wave LDS array, 2 strands x 256 windows x 8 bytes.  After a wave barrier the lanes whose window is a node read their two
// neighbours from LDS and the node's edges from the graph arrays.
// Bound: two random position-map probes per window (~1.3 sectors each: the HBM random-access rate, as k_fa_windows); the
// liveness check of a position reads e_alive / e_len or node_alive at an id that is the same for the lanes along one edge; the
// graph is otherwise touched at node windows only (out_edge, e_len, e_end), and the support table once per crossing.
// Contention: at high coverage thousands of reads cross one node, so one counter takes thousands of atomics.  Every crossing is
// one atomic of its own lane.  Combining the equal keys of a wave's trip first (a ballot loop over the trip's distinct keys, one
// lane adding per key) was measured and does not pay: a wave holds ONE read, which rarely crosses one (in, out) pair twice, so
// there is nothing to combine and the loop serialises the trip's adds — 22.5 ms against 7.6 ms where every read crosses nodes
// (8 x 10^5 reads of a 2 kbp genome), no difference on a 4 Mbp genome (profiles/r11).  The loop stays behind the test-build
// switch "thread_combine" = 1 as the A/B.
#include <algorithm>
#include <memory>

#include "gk_binstream.h"
#include "gk_support.h"
#include "gk_thread_common.h"

namespace {

constexpr int TH_NSTATS = 7;

struct ThreadCounts { u32 reads, inner, cls[5]; };

// One record, one wave.  pos[s][i] = what window i of strand s found.
template <int W>
__device__ __forceinline__ void thread_record(const Table<W> &pm, const GraphView &g, const u32 *tile, u32 ro, int len, int k, u64 (*pos)[TH_MAXW],
                                              const SupView &sup, bool combine, u32 *bad, ThreadCounts &st) {
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int lane = threadIdx.x & 63;
    if (len < k + 2) return;                                  // no inner window
    const int n = len - k + 1;
    const u32 bit0 = (ro + 1) * 8;
    st.reads++;
    st.inner += 2u * (u32)(n - 2);
    // phase 1: both strands' positions, one lane per window of the read
    for (int p = lane; p < n; p += 64) {
        const Kmer<W> x = tile_kmer(tile, bit0 + 2 * p, k, (Kmer<W> *)nullptr);
        pos[0][p] = thread_lookup(pm, g, x, bad);
        pos[1][n - 1 - p] = thread_lookup(pm, g, revcomp(x, k), bad);
    }
    wave_sync();
    // phase 2: the class of every inner window of either strand (the loops are wave-uniform, a lane may have no window)
    for (int s = 0; s < 2; s++)
        for (int i0 = 1; i0 < n - 1; i0 += 64) {
            const int i = i0 + lane;
            int cls = -1;
            u64 key = 0;
            if (i < n - 1) cls = thread_window_class(g, tb, ro, len, k, s, i, pos[s], &key);
#pragma unroll
            for (int c = 0; c < 5; c++) st.cls[c] += (u32)__popcll(__ballot(cls == c));
            if (combine) {
                // (A/B) equal keys of this trip as one add by the first lane that holds the key
                unsigned long long todo = __ballot(cls == TC_CROSSING);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const u64 k0 = (u64)__shfl((unsigned long long)key, leader);
                    const unsigned long long same = __ballot(cls == TC_CROSSING && key == k0);
                    if (lane == leader) sup_add_checked(sup, k0, (u32)__popcll(same));
                    todo &= ~same;
                }
            } else if (cls == TC_CROSSING) sup_add_checked(sup, key, 1u);
        }
    wave_sync();                                       // before the next record's positions land in `pos`
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_thread_reads(Table<W> pm, GraphView g, int k, const uint8_t *rec, u64 nreads, const u32 *__restrict__ off, u32 stride,
                                                        WindowLimits lim, SupView sup, u32 combine, u32 *bad, unsigned long long *stats) {
    __shared__ __attribute__((aligned(16))) u32 tile[TILE_WORDS];
    __shared__ u64 pos[BLOCK / 64][2][TH_MAXW];
    __shared__ unsigned long long s_stats[TH_NSTATS];
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < TH_NSTATS) s_stats[threadIdx.x] = 0;
    ThreadCounts st{};
    const u64 ntiles = (nreads + TILE_READS - 1) / TILE_READS;
    for (u64 ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {                 // (uniform over the workgroup: the barriers are safe)
        const u64 r0 = ti * TILE_READS;
        const int nr = (int)min((u64)TILE_READS, nreads - r0);
        const u64 gb = off ? (u64)off[r0] : r0 * stride, ge = off ? (u64)off[r0 + nr] : (r0 + nr) * stride;
        const u64 a0 = stage_tile(tile, rec, gb, ge);
        __syncthreads();
        for (int r = wave; r < nr; r += BLOCK / 64) {
            const u32 ro = (u32)((off ? (u64)off[r0 + r] : (r0 + r) * stride) - a0);
            thread_record<W>(pm, g, tile, ro, record_len(tb, ro, lim), k, pos[wave], sup, combine != 0u, bad, st);
        }
        __syncthreads();                                                      // before the next tile is staged over this one
    }
    // the counters are wave-uniform: lane 0 of every wave adds them up in LDS, then one global atomic per counter and workgroup
    if (lane == 0) {
        const u32 v[TH_NSTATS] = {st.reads, st.inner, st.cls[TC_OFF], st.cls[TC_REPEATED], st.cls[TC_ON_EDGE], st.cls[TC_BROKEN], st.cls[TC_CROSSING]};
#pragma unroll
        for (int i = 0; i < TH_NSTATS; i++) if (v[i]) atomicAdd(&s_stats[i], (unsigned long long)v[i]);
    }
    __syncthreads();
    if (threadIdx.x < TH_NSTATS && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// the state of one call: a support of its own that the launches count into, the flags and the statistics
struct ThreadCall {
    gk_graph *g;
    gk_vmap *pm;
    gk_support *local = nullptr;
    u32 *d_bad = nullptr;
    unsigned long long *d_stats = nullptr;
};

SupView thread_sup_view(const gk_support *s) { return SupView{s->d_keys, s->d_cnt, s->cap - 1, s->d_ctr}; }

int thread_check_args(gk_graph *g, gk_vmap *positions, gk_support *sup, uint64_t *stats7, const char *who) {
    if (stats7) for (int i = 0; i < TH_NSTATS; i++) stats7[i] = 0;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    const std::string w(who);
    if (!positions || !sup) return fail(ctx, GK_E_INVALID, w + ": null argument");
    if (vmap_ctx(positions) != ctx || sup->ctx != ctx) return fail(ctx, GK_E_INVALID, w + ": the position map and the support must live on the graph's context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, w + ": the position map has another k");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    return GK_OK;
}

int thread_begin(ThreadCall &c, DevScratch &tmp) {
    gk_ctx *ctx = c.g->ctx;
    if (int rc = gk_support_create(ctx, &c.local)) return rc;
    // a crossing is (in-edge, out-edge) of one node: at most 4 out-edges behind every edge, at most 16 pairs at every node
    const GraphView &v = c.g->v;
    if (int rc = support_reserve(c.local, std::min<u64>(4 * v.n_edges, 16 * v.n_nodes))) return rc;
    GK_HIP(ctx, tmp.zeroed(&c.d_bad, 1));
    GK_HIP(ctx, tmp.zeroed(&c.d_stats, TH_NSTATS));
    return GK_OK;
}

// one launch over records resident in HBM; stream-ordered, no sync
int thread_launch(const ThreadCall &c, const ReadSrc &src, u32 *d_fmt) {
    gk_ctx *ctx = c.g->ctx;
    const u64 ntiles = (src.nreads + TILE_READS - 1) / TILE_READS;
    const int grid = (int)std::min<u64>(ntiles, grid_cap(ctx));
    const WindowLimits lim{src.max_len, d_fmt};
    void *slots = nullptr;
    uint32_t nb2 = 1, lnb1 = 0;
    vmap_table(c.pm, &slots, &nb2, &lnb1);
    const int k = c.g->k;
    const u32 combine = ctx->hook_thread_combine > 0 ? 1u : 0u;
    GK_BY_W(c.g->W, hipLaunchKernelGGL(k_thread_reads<W>, dim3(grid), dim3(BLOCK), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u},
                                       c.g->v, k, src.rec, (u64)src.nreads, src.off, src.stride, lim, thread_sup_view(c.local), combine, c.d_bad, c.d_stats));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}

// the end of a call whose launches are queued: the flags, then the call's counts into `sup` through gk_support_merge, which
// refuses before it writes if a count would wrap
int thread_end(const ThreadCall &c, gk_support *sup, bool dev_format, uint64_t *stats7, const char *who) {
    gk_ctx *ctx = c.g->ctx;
    const std::string w(who);
    unsigned long long h_stats[TH_NSTATS] = {}, h_ctr[5] = {};
    u32 h_bad = 0;
    GK_HIP(ctx, read_back(ctx, {{h_stats, c.d_stats, sizeof(h_stats)}, {&h_bad, c.d_bad, 4}, {h_ctr, c.local->d_ctr, sizeof(h_ctr)}}));
    if (dev_format) { if (int rc = ctx_check_format(ctx)) return rc; }
    if (h_bad) return fail(ctx, GK_E_STATE, w + ": the position map does not belong to this graph (rebuild it after edits)");
    if (h_ctr[3]) return fail(ctx, GK_E_CAPACITY, w + ": the support table filled up (internal sizing error)");
    if (h_ctr[4]) return fail(ctx, GK_E_CAPACITY, w + ": a count would pass 2^32-1; nothing was added");
    if (int rc = gk_support_merge(sup, c.local)) return rc;
    if (stats7) for (int i = 0; i < TH_NSTATS; i++) stats7[i] = h_stats[i];
    return GK_OK;
}

}  // namespace

extern "C" {

int gk_graph_thread_reads_dev(gk_graph *g, gk_vmap *positions, gk_support *sup, const void *dev_records, uint64_t nreads, int read_len, uint64_t *stats7) {
    if (int rc = thread_check_args(g, positions, sup, stats7, "gk_graph_thread_reads_dev")) return rc;
    gk_ctx *ctx = g->ctx;
    if (nreads && !dev_records) return fail(ctx, GK_E_INVALID, "gk_graph_thread_reads_dev: null records");
    if (int rc = check_read_len(ctx, read_len)) return rc;
    if (nreads == 0) return GK_OK;
    ThreadCall c{g, positions};
    DevScratch tmp(ctx);
    int rc = thread_begin(c, tmp);
    std::unique_ptr<gk_support, void (*)(gk_support *)> own(c.local, gk_support_destroy);
    if (rc) return rc;
    if ((rc = thread_launch(c, ReadSrc::fixed(dev_records, nreads, read_len), ctx->d_flags))) return rc;
    return thread_end(c, sup, true, stats7, "gk_graph_thread_reads_dev");
}

int gk_graph_thread_reads(gk_graph *g, gk_vmap *positions, gk_support *sup, const uint8_t *bin, size_t nbytes, uint64_t nreads, uint64_t *stats7) {
    if (int rc = thread_check_args(g, positions, sup, stats7, "gk_graph_thread_reads")) return rc;
    gk_ctx *ctx = g->ctx;
    if (nreads && !bin) return fail(ctx, GK_E_INVALID, "gk_graph_thread_reads: null stream");
    if (nreads == 0) return GK_OK;
    // the framing, walked on the host before anything is launched
    size_t end = 0;
    if (int rc = bin_walk(ctx, bin, nbytes, nreads, &end)) return rc;
    ThreadCall c{g, positions};
    DevScratch tmp(ctx);
    int rc = thread_begin(c, tmp);
    std::unique_ptr<gk_support, void (*)(gk_support *)> own(c.local, gk_support_destroy);
    if (rc) return rc;
    // nothing comes back from a piece: the feeder's end of a piece is the plain wait for the main stream
    if ((rc = bin_feed(ctx, tmp, bin, end, [&](const ReadSrc &src, uint8_t *, const BinPiece &, D2H *) { return thread_launch(c, src, nullptr); }))) return rc;
    return thread_end(c, sup, false, stats7, "gk_graph_thread_reads");
}

}  // extern "C"
