// gk_spans.hip — reads followed across a whole edge: for every edge m a read crosses from end to end, the in-edge e it arrived by and
// the out-edge f it left by: spans[(e, m, f)] += 1.  That is the evidence for a repeat longer than k, which is an edge between two
// nodes and which the per-node support of gk_graph_thread_reads cannot resolve.  The rule is this project's own and stated in
// include/genome_amd.h (gk_graph_thread_spans); tests/spans_ref.py restates it.  The edit that uses the table,
// gk_graph_split_edges_by_spans, stands beside the node split in gk_pairs.hip.
//
// Reference: none.  GraphSimplifier.scala:272-316 resolves per node.
//
// Shape: k_thread_reads' (gk_thread.hip), whose lookup, window classes and wave sync come from gk_thread_common.h.  A workgroup
// stages 64 records in LDS, a wave takes a record, its lanes take windows 64 at a time; phase 1 leaves both strands' positions in
// LDS (two position-map probes per window), phase 2 classifies the inner windows as k_thread_reads does and leaves every window's
// crossing key, or none, in a second LDS array.  Phase 3 starts after a wave barrier, when ALL trips of phase 2 have written: the
// lane that owns a crossing at window j reads window j - len_m, which lies up to 252 windows and so up to four trips back.
// The windows between the two crossings are checked by a loop of the owning lane over the positions in LDS, which stops at the
// first window that is not the next step along m.  The other way, a per-window "continues the previous window's edge" flag and a
// wave prefix count of the breaks, was not built: it costs every window of every record a flag and every trip a scan with a carry
// from the trip before, while the loop costs only the crossings, of which a record has a handful, LDS reads only.
// Bound: as k_thread_reads, two random position-map probes per window; the span table is touched once per span.
#include <algorithm>
#include <memory>

#include "gk_binstream.h"
#include "gk_records.h"
#include "gk_spans.h"
#include "gk_support.h"
#include "gk_thread_common.h"

namespace {

constexpr int SP_NSTATS = 5;
constexpr u64 XK_NONE = ~0ull;                 // a window that is no crossing (0xffffffff is not an edge id)
enum { SC_SPAN = 0, SC_INTERRUPTED = 1, SC_OPEN = 2 };

struct SpanCounts { u32 reads, cross, cls[3]; };

// sup_add_checked for a triple: the slot of (e, m, 0), (e, m, 1), ... whose f plane holds f or takes it
__device__ __forceinline__ void span_add(const SpanView &t, u32 e, u32 m, u32 f, u32 c) {
    const u64 base = ((u64)e << 33) | ((u64)m << 2);
    for (u64 slot = 0; slot < 4; slot++) {
        const u64 key = base | slot;
        u64 i = mix64(key) & t.mask, n = 0;
        bool other = false;
        for (; n <= t.mask; n++) {
            u64 cur = t.keys[i];
            if (cur == SUP_EMPTY) {
                cur = atomicCAS(reinterpret_cast<unsigned long long *>(&t.keys[i]), (unsigned long long)SUP_EMPTY, (unsigned long long)key);
                if (cur == SUP_EMPTY) cur = key;
            }
            if (cur == key) {
                const u32 had = atomicCAS(&t.f[i], NONE, f);
                if (had == NONE) atomicAdd(&t.ctr[0], 1ull);
                if (had == NONE || had == f) {
                    const u32 old = atomicAdd(&t.cnt[i], c);
                    if (old + c < old) t.ctr[4] = 1;
                    return;
                }
                other = true;                                 // this slot is another out-edge's: the next one
                break;
            }
            i = (i + 1) & t.mask;
        }
        if (!other) { t.ctr[3] = 1; return; }
    }
    t.ctr[5] = 1;
}

// One record, one wave.  pos[s][i] = what window i of strand s found, xk[s][i] = its crossing key or XK_NONE.
template <int W>
__device__ __forceinline__ void spans_record(const Table<W> &pm, const GraphView &g, const u32 *tile, u32 ro, int len, int k, u64 (*pos)[TH_MAXW],
                                             u64 (*xk)[TH_MAXW], const SpanView &t, u32 *bad, SpanCounts &st) {
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int lane = threadIdx.x & 63;
    if (len < k + 2) return;                                  // no inner window
    const int n = len - k + 1;
    const u32 bit0 = (ro + 1) * 8;
    st.reads++;
    // phase 1: both strands' positions, one lane per window of the read
    for (int p = lane; p < n; p += 64) {
        const Kmer<W> x = tile_kmer(tile, bit0 + 2 * p, k, (Kmer<W> *)nullptr);
        pos[0][p] = thread_lookup(pm, g, x, bad);
        pos[1][n - 1 - p] = thread_lookup(pm, g, revcomp(x, k), bad);
    }
    wave_sync();
    // phase 2: every inner window's crossing key, or none (the loops are wave-uniform, a lane may have no window)
    for (int s = 0; s < 2; s++)
        for (int i0 = 1; i0 < n - 1; i0 += 64) {
            const int i = i0 + lane;
            bool cross = false;
            if (i < n - 1) {
                u64 key = 0;
                cross = thread_window_class(g, tb, ro, len, k, s, i, pos[s], &key) == TC_CROSSING;
                xk[s][i] = cross ? key : XK_NONE;
            }
            st.cross += (u32)__popcll(__ballot(cross));
        }
    wave_sync();                                       // window j - len_m may lie in any earlier trip: all of them have written
    // phase 3: the lane that owns a crossing at j looks back over the edge it arrived by
    for (int s = 0; s < 2; s++)
        for (int j0 = 1; j0 < n - 1; j0 += 64) {
            const int j = j0 + lane;
            int cls = -1;
            const u64 kj = j < n - 1 ? xk[s][j] : XK_NONE;
            if (kj != XK_NONE) {
                const u32 m = (u32)(kj >> 32);
                const u64 len_m = g.e_len[m];
                if (len_m >= (u64)j) cls = SC_OPEN;            // j - len_m < 1: the read began inside m or at its start node
                else {
                    const int i = j - (int)len_m;
                    const u64 ki = xk[s][i];
                    bool ok = ki != XK_NONE && (u32)ki == m;
                    for (int w = i + 1; ok && w < j; w++) ok = pos[s][w] == thread_edge_pos(m, (u64)(w - i));
                    cls = ok ? SC_SPAN : SC_INTERRUPTED;
                    if (ok) span_add(t, (u32)(ki >> 32), m, (u32)kj, 1u);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) st.cls[c] += (u32)__popcll(__ballot(cls == c));
        }
    wave_sync();                                       // before the next record's positions land in `pos`
}

template <int W>
__global__ __launch_bounds__(BLOCK) void k_thread_spans(Table<W> pm, GraphView g, int k, const uint8_t *rec, u64 nreads, const u32 *__restrict__ off, u32 stride,
                                                        WindowLimits lim, SpanView t, u32 *bad, unsigned long long *stats) {
    __shared__ __attribute__((aligned(16))) u32 tile[TILE_WORDS];
    __shared__ u64 pos[BLOCK / 64][2][TH_MAXW];
    __shared__ u64 xk[BLOCK / 64][2][TH_MAXW];
    __shared__ unsigned long long s_stats[SP_NSTATS];
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < SP_NSTATS) s_stats[threadIdx.x] = 0;
    SpanCounts st{};
    const u64 ntiles = (nreads + TILE_READS - 1) / TILE_READS;
    for (u64 ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {                 // (uniform over the workgroup: the barriers are safe)
        const u64 r0 = ti * TILE_READS;
        const int nr = (int)min((u64)TILE_READS, nreads - r0);
        const u64 gb = off ? (u64)off[r0] : r0 * stride, ge = off ? (u64)off[r0 + nr] : (r0 + nr) * stride;
        const u64 a0 = stage_tile(tile, rec, gb, ge);
        __syncthreads();
        for (int r = wave; r < nr; r += BLOCK / 64) {
            const u32 ro = (u32)((off ? (u64)off[r0 + r] : (r0 + r) * stride) - a0);
            spans_record<W>(pm, g, tile, ro, record_len(tb, ro, lim), k, pos[wave], xk[wave], t, bad, st);
        }
        __syncthreads();                                                      // before the next tile is staged over this one
    }
    // the counters are wave-uniform: lane 0 of every wave adds them up in LDS, then one global atomic per counter and workgroup
    if (lane == 0) {
        const u32 v[SP_NSTATS] = {st.reads, st.cross, st.cls[SC_SPAN], st.cls[SC_INTERRUPTED], st.cls[SC_OPEN]};
#pragma unroll
        for (int i = 0; i < SP_NSTATS; i++) if (v[i]) atomicAdd(&s_stats[i], (unsigned long long)v[i]);
    }
    __syncthreads();
    if (threadIdx.x < SP_NSTATS && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// growth, merge and gk_spans_add: live slots, or a list, through the same insert
__global__ __launch_bounds__(BLOCK) void k_span_rehash(const u64 *okeys, const u32 *of, const u32 *ocnt, u64 ocap, SpanView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ocap; i += (u64)gridDim.x * BLOCK)
        if (okeys[i] != SUP_EMPTY) span_add(t, (u32)(okeys[i] >> 33), (u32)(okeys[i] >> 2) & 0x7fffffffu, of[i], ocnt[i]);
}
__global__ __launch_bounds__(BLOCK) void k_span_add_list(const u32 *e, const u32 *m, const u32 *f, const u32 *cnt, u64 n, SpanView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) span_add(t, e[i], m[i], f[i], cnt[i]);
}

// the sum of the live counts: one LDS add per lane that holds any, one global atomic per workgroup
__global__ __launch_bounds__(BLOCK) void k_span_sum(const u64 *keys, const u32 *cnt, u64 cap, unsigned long long *out) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    unsigned long long v = 0;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < cap; i += (u64)gridDim.x * BLOCK)
        if (keys[i] != SUP_EMPTY) v += cnt[i];
    if (v) atomicAdd(&s_sum, v);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(out, s_sum);
}

SpanView span_view(const gk_spans *s) { return SpanView{s->d_keys, s->d_f, s->d_cnt, s->cap - 1, s->d_ctr}; }

void spans_free_table(gk_spans *s) {
    gk_ctx *ctx = s->ctx;
    (void)pool_free(ctx, s->d_keys); (void)pool_free(ctx, s->d_f); (void)pool_free(ctx, s->d_cnt);
    s->d_keys = nullptr; s->d_f = nullptr; s->d_cnt = nullptr; s->cap = 0;
}

// an EMPTY table's room for `want` distinct triples at load <= 0.5 (a power of two of slots)
int spans_alloc(gk_spans *s, u64 want) {
    gk_ctx *ctx = s->ctx;
    const u64 need = pow2ceil(std::max<u64>(2 * want + 1024, 4096));
    hipError_t e = pool_malloc(ctx, &s->d_keys, need * 8);
    if (e == hipSuccess) e = pool_malloc(ctx, &s->d_f, need * 4);
    if (e == hipSuccess) e = pool_malloc(ctx, &s->d_cnt, need * 4);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_keys, 0xff, need * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_f, 0xff, need * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_cnt, 0, need * 4, ctx->stream);
    if (e != hipSuccess) { spans_free_table(s); return hip_fail(ctx, e, "gk_spans: table"); }
    s->cap = need;
    return GK_OK;
}

using LocalSpans = std::unique_ptr<gk_spans, void (*)(gk_spans *)>;

// dst += src, with dst unchanged on any error: both go into a fresh table, which dst takes only once no flag is raised
int spans_merge(gk_spans *dst, const gk_spans *src, const char *who) {
    gk_ctx *ctx = dst->ctx;
    const std::string w(who);
    unsigned long long hs = 0, hd = 0, flags[3] = {0, 0, 0};
    GK_HIP(ctx, read_back(ctx, {{&hs, src->d_ctr, 8}, {&hd, dst->d_ctr, 8}}));
    if (!src->cap || !hs) return GK_OK;
    gk_spans *t = nullptr;
    if (int rc = gk_spans_create(ctx, &t)) return rc;
    LocalSpans own(t, gk_spans_destroy);
    if (int rc = spans_alloc(t, hd + hs)) return rc;
    if (dst->cap && hd) hipLaunchKernelGGL(k_span_rehash, dim3(ggrid(ctx, dst->cap)), dim3(BLOCK), 0, ctx->stream, dst->d_keys, dst->d_f, dst->d_cnt, dst->cap, span_view(t));
    hipLaunchKernelGGL(k_span_rehash, dim3(ggrid(ctx, src->cap)), dim3(BLOCK), 0, ctx->stream, src->d_keys, src->d_f, src->d_cnt, src->cap, span_view(t));
    GK_HIP(ctx, hipGetLastError());
    GK_HIP(ctx, read_back(ctx, flags, t->d_ctr + 3, 3));
    if (flags[0]) return fail(ctx, GK_E_CAPACITY, w + ": the span table filled up (internal sizing error)");
    if (flags[1]) return fail(ctx, GK_E_CAPACITY, w + ": a count would pass 2^32-1; nothing was added");
    if (flags[2]) return fail(ctx, GK_E_INVALID, w + ": more than four out-edges behind one (in-edge, edge); nothing was added");
    std::swap(dst->d_keys, t->d_keys); std::swap(dst->d_f, t->d_f); std::swap(dst->d_cnt, t->d_cnt); std::swap(dst->cap, t->cap);
    std::swap(dst->d_ctr, t->d_ctr);
    return GK_OK;
}

// the state of one call: a table of its own that the launches count into, the flags and the statistics
struct SpanCall {
    gk_graph *g;
    gk_vmap *pm;
    gk_spans *local = nullptr;
    u32 *d_bad = nullptr;
    unsigned long long *d_stats = nullptr;
};

int spans_check_args(gk_graph *g, gk_vmap *positions, gk_spans *spans, uint64_t *stats5, const char *who) {
    if (stats5) for (int i = 0; i < SP_NSTATS; i++) stats5[i] = 0;
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    const std::string w(who);
    if (!positions || !spans) return fail(ctx, GK_E_INVALID, w + ": null argument");
    if (vmap_ctx(positions) != ctx || spans->ctx != ctx) return fail(ctx, GK_E_INVALID, w + ": the position map and the spans must live on the graph's context");
    if (vmap_k(positions) != g->k) return fail(ctx, GK_E_KLEN, w + ": the position map has another k");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    return GK_OK;
}

int spans_begin(SpanCall &c, DevScratch &tmp, u64 nreads) {
    gk_ctx *ctx = c.g->ctx;
    if (int rc = gk_spans_create(ctx, &c.local)) return rc;
    // a span is (in-edge, m, out-edge): an in-edge has at most 4 edges m behind it, and at most 4 spans lie behind every
    // (in-edge, m); a record adds at most one span per inner window and strand
    if (int rc = spans_alloc(c.local, std::min<u64>(16 * c.g->v.n_edges, 2 * (u64)TH_MAXW * nreads))) return rc;
    GK_HIP(ctx, tmp.zeroed(&c.d_bad, 1));
    GK_HIP(ctx, tmp.zeroed(&c.d_stats, SP_NSTATS));
    return GK_OK;
}

// one launch over records resident in HBM; stream-ordered, no sync
int spans_launch(const SpanCall &c, const ReadSrc &src, u32 *d_fmt) {
    gk_ctx *ctx = c.g->ctx;
    const u64 ntiles = (src.nreads + TILE_READS - 1) / TILE_READS;
    const int grid = (int)std::min<u64>(ntiles, grid_cap(ctx));
    const WindowLimits lim{src.max_len, d_fmt};
    void *slots = nullptr;
    uint32_t nb2 = 1, lnb1 = 0;
    vmap_table(c.pm, &slots, &nb2, &lnb1);
    const int k = c.g->k;
    GK_BY_W(c.g->W, hipLaunchKernelGGL(k_thread_spans<W>, dim3(grid), dim3(BLOCK), 0, ctx->stream, Table<W>{(Slot<W> *)slots, nb2, lnb1, k == 64 ? 1u : 0u, 0u},
                                       c.g->v, k, src.rec, (u64)src.nreads, src.off, src.stride, lim, span_view(c.local), c.d_bad, c.d_stats));
    GK_HIP(ctx, hipGetLastError());
    return GK_OK;
}

// the end of a call whose launches are queued: the flags, then the call's counts into `spans` through spans_merge
int spans_end(const SpanCall &c, gk_spans *spans, bool dev_format, uint64_t *stats5, const char *who) {
    gk_ctx *ctx = c.g->ctx;
    const std::string w(who);
    unsigned long long h_stats[SP_NSTATS] = {}, h_ctr[6] = {};
    u32 h_bad = 0;
    GK_HIP(ctx, read_back(ctx, {{h_stats, c.d_stats, sizeof(h_stats)}, {&h_bad, c.d_bad, 4}, {h_ctr, c.local->d_ctr, sizeof(h_ctr)}}));
    if (dev_format) { if (int rc = ctx_check_format(ctx)) return rc; }
    if (h_bad) return fail(ctx, GK_E_STATE, w + ": the position map does not belong to this graph (rebuild it after edits)");
    if (h_ctr[3]) return fail(ctx, GK_E_CAPACITY, w + ": the span table filled up (internal sizing error)");
    if (h_ctr[5]) return fail(ctx, GK_E_STATE, w + ": more than four out-edges behind one (in-edge, edge): the position map does not belong to this graph");
    if (h_ctr[4]) return fail(ctx, GK_E_CAPACITY, w + ": a count would pass 2^32-1; nothing was added");
    if (int rc = spans_merge(spans, c.local, who)) return rc;
    if (stats5) for (int i = 0; i < SP_NSTATS; i++) stats5[i] = h_stats[i];
    return GK_OK;
}

// ---- the span table's records as planes (gk_links.h): key plane (e << 32 | m), extra plane f ----------------------------------
struct SpanSrc {
    const u64 *keys; const u32 *f; const u32 *cnt; u64 cap;
    __device__ __forceinline__ bool get(u64 i, const RecCanon &c, u64 *key, u32 *n, u64 *x) const {
        const u64 k = keys[i];
        if (k == SUP_EMPTY || f[i] == NONE) return false;
        const u32 e = rec_canon_id(c, (u32)(k >> 33)), m = rec_canon_id(c, (u32)(k >> 2) & 0x7fffffffu), o = rec_canon_id(c, f[i]);
        if (e == NONE || m == NONE || o == NONE) return false;
        *key = ((u64)e << 32) | m; *n = cnt[i]; *x = o;
        return true;
    }
};
__global__ __launch_bounds__(BLOCK) void k_span_add_planes(RecPlanes p, u64 n, SpanView t) {
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * BLOCK) span_add(t, (u32)(p.key[i] >> 32), (u32)p.key[i], (u32)p.x[i], p.cnt[i]);
}

}  // namespace

namespace gk {
template <> gk_ctx *rec_ctx<gk_spans>(const gk_spans *s) { return s->ctx; }
template <> int rec_distinct<gk_spans>(const gk_spans *s, u64 *n) {
    unsigned long long h = 0;
    GK_HIP(s->ctx, read_back(s->ctx, &h, s->d_ctr));
    *n = h;
    return GK_OK;
}
template <> int rec_bucket<gk_spans>(gk_spans *s, int P, const RecPlanes &out, u64 room, u64 *region, const u32 *canon, const uint8_t *dup, u64 nmap) {
    return records_bucket(s->ctx, SpanSrc{s->d_keys, s->d_f, s->d_cnt, s->cap}, P, out, room, region, canon, dup, nmap, "the spans");
}
template <> int rec_insert<gk_spans>(gk_spans *s, const RecPlanes &in, u64 n, bool *overflow) {
    gk_ctx *ctx = s->ctx;
    *overflow = false;
    if (n == 0) return GK_OK;
    u64 have = 0;
    if (int rc = rec_distinct(s, &have)) return rc;
    if (s->cap < 2 * (have + n)) return fail(ctx, GK_E_STATE, "rec_insert: the span table was not made for " + std::to_string(have + n) + " triples");
    hipLaunchKernelGGL(k_span_add_planes, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, in, n, span_view(s));
    unsigned long long fl[3] = {0, 0, 0};                      // [3] table full, [4] a count wrapped, [5] a fifth out-edge
    GK_HIP(ctx, read_back(ctx, fl, s->d_ctr + 3, 3));
    if (fl[0]) return fail(ctx, GK_E_CAPACITY, "the span table filled up (internal sizing error)");
    if (fl[2]) return fail(ctx, GK_E_STATE, "more than four out-edges behind one (in-edge, edge) over the ranks: the spans do not belong to this graph");
    *overflow = fl[1] != 0;
    return GK_OK;
}
template <> int rec_uncanon<gk_spans>(gk_ctx *ctx, const RecPlanes &p, u64 n, const u32 *d_inv, u64 nlive) { return records_uncanon(ctx, p, n, true, d_inv, nlive); }
template <> int rec_new<gk_spans>(gk_ctx *ctx, u64 want, u64, gk_spans **out) {
    if (int rc = gk_spans_create(ctx, out)) return rc;
    return spans_alloc(*out, want);
}
template <> void rec_free<gk_spans>(gk_spans *s) { gk_spans_destroy(s); }
template <> int rec_adopt<gk_spans>(gk_spans *s, gk_spans *t) {
    GK_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));
    std::swap(s->d_keys, t->d_keys); std::swap(s->d_f, t->d_f); std::swap(s->d_cnt, t->d_cnt); std::swap(s->cap, t->cap); std::swap(s->d_ctr, t->d_ctr);
    return GK_OK;
}

int spans_to_host(const gk_spans *s, std::vector<u32> &e, std::vector<u32> &m, std::vector<u32> &f, std::vector<u32> &count) {
    gk_ctx *ctx = s->ctx;
    e.clear(); m.clear(); f.clear(); count.clear();
    if (!s->cap) return GK_OK;
    std::vector<u64> k(s->cap);
    std::vector<u32> pf(s->cap), c(s->cap);
    GK_HIP(ctx, read_back(ctx, {{k.data(), s->d_keys, s->cap * 8}, {pf.data(), s->d_f, s->cap * 4}, {c.data(), s->d_cnt, s->cap * 4}}));
    for (u64 i = 0; i < s->cap; i++)
        if (k[i] != SUP_EMPTY) { e.push_back((u32)(k[i] >> 33)); m.push_back((u32)(k[i] >> 2) & 0x7fffffffu); f.push_back(pf[i]); count.push_back(c[i]); }
    return GK_OK;
}
}  // namespace gk

extern "C" {

int gk_spans_create(gk_ctx *ctx, gk_spans **out) {
    if (!ctx || !out) return fail(ctx, GK_E_INVALID, "gk_spans_create: null argument");
    *out = nullptr;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    gk_spans *s = new gk_spans();
    s->ctx = ctx;
    hipError_t e = pool_malloc(ctx, &s->d_ctr, 64);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_ctr, 0, 64, ctx->stream);
    if (e != hipSuccess) { (void)pool_free(ctx, s->d_ctr); delete s; return hip_fail(ctx, e, "gk_spans_create"); }
    *out = s;
    return GK_OK;
}

void gk_spans_destroy(gk_spans *s) {
    if (!s) return;
    gk_ctx *ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    spans_free_table(s);
    (void)pool_free(ctx, s->d_ctr);
    delete s;
}

int gk_spans_size(const gk_spans *s, uint64_t *triples, uint64_t *observations) {
    if (!s) return fail(nullptr, GK_E_INVALID, "null spans handle");
    GK_HIP(s->ctx, hipSetDevice(s->ctx->device));
    gk_ctx *ctx = s->ctx;
    // the distinct triples are counted as they are inserted (ctr[0]); the observations are summed on the device
    unsigned long long held = 0, total = 0;
    DevScratch tmp(ctx);
    unsigned long long *d_total = nullptr;
    if (observations && s->cap) {
        GK_HIP(ctx, tmp.zeroed(&d_total, 1));
        hipLaunchKernelGGL(k_span_sum, dim3(ggrid(ctx, s->cap)), dim3(BLOCK), 0, ctx->stream, s->d_keys, s->d_cnt, s->cap, d_total);
        GK_HIP(ctx, hipGetLastError());
        GK_HIP(ctx, read_back(ctx, {{&held, s->d_ctr, 8}, {&total, d_total, 8}}));
    } else {
        GK_HIP(ctx, read_back(ctx, &held, s->d_ctr, 1));
    }
    if (triples) *triples = held;
    if (observations) *observations = total;
    return GK_OK;
}

int gk_spans_export(const gk_spans *s, uint32_t *e, uint32_t *m, uint32_t *f, uint32_t *count, uint64_t cap, uint64_t *n) {
    if (!s) return fail(nullptr, GK_E_INVALID, "null spans handle");
    gk_ctx *ctx = s->ctx;
    GK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<u32> ve, vm, vf, vc;
    if (int rc = spans_to_host(s, ve, vm, vf, vc)) return rc;
    const u64 live = ve.size();
    if (n) *n = live;
    if (live > cap) return fail(ctx, GK_E_CAPACITY, "gk_spans_export: need room for " + std::to_string(live) + " triples");
    if (live && (!e || !m || !f || !count)) return fail(ctx, GK_E_INVALID, "gk_spans_export: null argument");
    for (u64 i = 0; i < live; i++) { e[i] = ve[i]; m[i] = vm[i]; f[i] = vf[i]; count[i] = vc[i]; }
    return GK_OK;
}

int gk_spans_add(gk_spans *s, const uint32_t *e, const uint32_t *m, const uint32_t *f, const uint32_t *count, uint64_t n) {
    if (!s) return fail(nullptr, GK_E_INVALID, "null spans handle");
    gk_ctx *ctx = s->ctx;
    if (n == 0) return GK_OK;
    if (!e || !m || !f || !count) return fail(ctx, GK_E_INVALID, "gk_spans_add: null argument");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    for (u64 i = 0; i < n; i++)
        if (e[i] >= 0x7fffffffu || m[i] >= 0x7fffffffu || f[i] >= 0x7fffffffu) return fail(ctx, GK_E_INVALID, "gk_spans_add: an edge id is below 2^31 - 1");
    // the list goes into a table of its own (duplicates add up there, checked), which is then merged
    gk_spans *t = nullptr;
    if (int rc = gk_spans_create(ctx, &t)) return rc;
    LocalSpans own(t, gk_spans_destroy);
    if (int rc = spans_alloc(t, n)) return rc;
    DevScratch tmp(ctx);
    u32 *d_e = nullptr, *d_m = nullptr, *d_f = nullptr, *d_c = nullptr;
    tmp.upload(&d_e, e, n);
    tmp.upload(&d_m, m, n);
    tmp.upload(&d_f, f, n);
    tmp.upload(&d_c, count, n);
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_spans_add: upload");
    hipLaunchKernelGGL(k_span_add_list, dim3(ggrid(ctx, n)), dim3(BLOCK), 0, ctx->stream, d_e, d_m, d_f, d_c, (u64)n, span_view(t));
    GK_HIP(ctx, hipGetLastError());
    unsigned long long fl[3] = {0, 0, 0};                      // [3] table full, [4] a count wrapped, [5] a fifth out-edge
    GK_HIP(ctx, read_back(ctx, fl, t->d_ctr + 3, 3));
    if (fl[0]) return fail(ctx, GK_E_CAPACITY, "gk_spans_add: the span table filled up (internal sizing error)");
    if (fl[1]) return fail(ctx, GK_E_CAPACITY, "gk_spans_add: a count of the list would pass 2^32-1; nothing was added");
    if (fl[2]) return fail(ctx, GK_E_INVALID, "gk_spans_add: more than four out-edges behind one (in-edge, edge); nothing was added");
    return spans_merge(s, t, "gk_spans_add");
}

int gk_graph_thread_spans_dev(gk_graph *g, gk_vmap *positions, gk_spans *spans, const void *dev_records, uint64_t nreads, int read_len, uint64_t *stats5) {
    if (int rc = spans_check_args(g, positions, spans, stats5, "gk_graph_thread_spans_dev")) return rc;
    gk_ctx *ctx = g->ctx;
    if (nreads && !dev_records) return fail(ctx, GK_E_INVALID, "gk_graph_thread_spans_dev: null records");
    if (int rc = check_read_len(ctx, read_len)) return rc;
    if (nreads == 0) return GK_OK;
    SpanCall c{g, positions};
    DevScratch tmp(ctx);
    int rc = spans_begin(c, tmp, nreads);
    LocalSpans own(c.local, gk_spans_destroy);
    if (rc) return rc;
    if ((rc = spans_launch(c, ReadSrc::fixed(dev_records, nreads, read_len), ctx->d_flags))) return rc;
    return spans_end(c, spans, true, stats5, "gk_graph_thread_spans_dev");
}

int gk_graph_thread_spans(gk_graph *g, gk_vmap *positions, gk_spans *spans, const uint8_t *bin, size_t nbytes, uint64_t nreads, uint64_t *stats5) {
    if (int rc = spans_check_args(g, positions, spans, stats5, "gk_graph_thread_spans")) return rc;
    gk_ctx *ctx = g->ctx;
    if (nreads && !bin) return fail(ctx, GK_E_INVALID, "gk_graph_thread_spans: null stream");
    if (nreads == 0) return GK_OK;
    // the framing, walked on the host before anything is launched
    size_t end = 0;
    if (int rc = bin_walk(ctx, bin, nbytes, nreads, &end)) return rc;
    SpanCall c{g, positions};
    DevScratch tmp(ctx);
    int rc = spans_begin(c, tmp, nreads);
    LocalSpans own(c.local, gk_spans_destroy);
    if (rc) return rc;
    if ((rc = bin_feed(ctx, tmp, bin, end, [&](const ReadSrc &src, uint8_t *, const BinPiece &, D2H *) { return spans_launch(c, src, nullptr); }))) return rc;
    return spans_end(c, spans, false, stats5, "gk_graph_thread_spans");
}

}  // extern "C"
