// gk_testhooks.hip — what ONLY the test build of the library has (libgenome_amd_test.so = the product's objects + this one):
//   * gk_ctx_set_option and the environment switches read at gk_ctx_create: A/B switches of the kernels, test hooks that stage
//     the large-table paths on small tables or inject failures;
//   * gk_test_grid_cap_uses: how many launches "test_max_grid" has sized on a context (the switch's echo);
//   * gk_test_prefilter_chunks: the chunks a singleton pre-filter handle has staged and run ("test_max_stage" / "test_prefilter_chunk_windows"' echo);
//   * gk_test_multik_chunks: the chunks the last gk_map_add_graph_paths on a context ran ("test_multik_chunk_windows"' echo);
//   * gk_test_part_plan: what the partitioned insert would choose for a table geometry and a set of switches (part_choose's echo, no device);
//   * gk_test_support_last_walk: which walker (device kernel / host fallback) did the orientations of the last gk_graph_walk_pairs;
//   * gk_test_scan_counts: gk_scan.h's scan_counts over counts from the host, between guard words (either overload);
//   * gk_test_slot_ranks: the pointer-jumping build's slot -> rank structure of a map's table (gk_graph.hip: rank_build);
//   * gk_test_skm_route_offsets: the super-k-mer routing over an offset table (gk_skm.hip: k_skm_route<SLOT, true>), in one process;
//   * gk_dist_create_loopback: a transport whose ranks are threads of ONE process on ONE device, so that gk_dist_* runs with
//     world > 1 on a one-GPU box (RCCL refuses two ranks on one device).
// The product library (libgenome_amd.so) links none of this; its header is include/genome_amd.h, this file's is
// include/genome_amd_test.h.  The tests load the test build through GK_LIB_PATH (tests/conftest.py).
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "gk_dist.h"
#include "gk_graph.h"
#include "gk_links.h"
#include "gk_scan.h"
#include "gk_support.h"
#include "../../include/genome_amd_test.h"

using namespace gk;

extern "C" {

void gk_testhooks_env(gk_ctx *ctx) {
    ctx->hook_no_reserve = getenv("GK_TEST_NO_RESERVE") != nullptr;
    ctx->hook_host_ragged = getenv("GK_HOST_RAGGED") != nullptr;
    ctx->hook_part_exact = getenv("GK_PART_EXACT") != nullptr;
    if (const char *u = getenv("GK_P45_STRIPES")) ctx->hook_p45_stripes = atoi(u);
    if (const char *u = getenv("GK_MIN_LNB1")) ctx->hook_min_lnb1 = std::max(0, std::min((int)gk::MAX_LNB1, atoi(u)));      // (tests: the whole suite over 512 / 1024 L1 buckets)
    if (const char *u = getenv("GK_GRAPH_UNITIGS")) ctx->hook_unitigs = !strcmp(u, "walk") ? 1 : !strcmp(u, "pj") ? 2 : 0;
    if (const char *u = getenv("GK_GRAPH_MBT")) ctx->hook_graph_mbt = atoi(u);            // (tests: the whole graph suite over the bucketed table)
}

int gk_ctx_set_option(gk_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return fail(ctx, GK_E_INVALID, "gk_ctx_set_option: null argument");
    const std::string n(name);
    if (n == "test_no_reserve") ctx->hook_no_reserve = value != 0;
    else if (n == "host_ragged") ctx->hook_host_ragged = value != 0;
    else if (n == "part_exact") ctx->hook_part_exact = value != 0;
    else if (n == "graph_unitigs") {
        if (value < 0 || value > 2) return fail(ctx, GK_E_INVALID, "graph_unitigs: 0 auto, 1 walk, 2 pointer jumping");
        ctx->hook_unitigs = (int)value;
    } else if (n == "p4_direct") ctx->hook_p4_direct = value < 0 ? -1 : value != 0;
    else if (n == "p2_wide") ctx->hook_p2_wide = value < 0 ? -1 : value != 0;
    else if (n == "p2_sorted") ctx->hook_p2_sorted = value < 0 ? -1 : value != 0;
    else if (n == "p4_wide") ctx->hook_p4_wide = value < 0 ? -1 : (value >= 2 ? 2 : value != 0);
    else if (n == "p45_stripes") ctx->hook_p45_stripes = (int)value;
    else if (n == "p24_pieces") ctx->hook_p24_pieces = (int)value;
    else if (n == "dist_exchange_ahead") ctx->hook_dist_ahead = (int)value;
    else if (n == "test_dist_small_send") ctx->hook_dist_small_send = (int)std::max<int64_t>(0, value);
    else if (n == "target_load_pct") {
        // (max_load is 0.8: a table sized for a load at or above it grows for ever or fills a segment)
        if (value != 0 && value != -1 && (value < 10 || value > 75)) return fail(ctx, GK_E_INVALID, "target_load_pct: 0 / -1 default, else 10..75");
        ctx->hook_target_load_pct = value > 0 ? (int)value : 0;
    }
    else if (n == "cc_find") ctx->hook_cc_find = (int)value;
    else if (n == "test_dist_fail_classify") ctx->hook_dist_fail_classify = (int)value;
    else if (n == "test_dist_fail_reduce") ctx->hook_dist_fail_reduce = (int)value;
    else if (n == "test_dist_fail_exchange") ctx->hook_dist_fail = value > 0 ? -(int)value : (int)value;
    else if (n == "test_max_nb2") ctx->hook_max_nb2 = (int)std::max<int64_t>(0, value);
    else if (n == "min_lnb1") {
        if (value < 0 || value > (int64_t)gk::MAX_LNB1) return fail(ctx, GK_E_INVALID, "min_lnb1: 0..10");
        ctx->hook_min_lnb1 = (int)value;
    }
    else if (n == "p4_grid") ctx->hook_p4_grid = (int)value;
    else if (n == "graph_walk_queue") ctx->hook_walk_queue = (int)value;
    else if (n == "graph_mbt") ctx->hook_graph_mbt = (int)value;
    else if (n == "graph_mbt_keys") ctx->hook_graph_mbt_keys = (int)std::max<int64_t>(16, value);
    else if (n == "pairs_host") ctx->hook_pairs_host = (int)value;
    else if (n == "thread_combine") ctx->hook_thread_combine = value < 0 ? -1 : value != 0;
    else if (n == "host_prefetch") ctx->hook_host_prefetch = (int)value;
    else if (n == "test_max_stage") ctx->hook_max_stage = (int64_t)std::max<int64_t>(0, value);
    else if (n == "test_pairs_small_sets") ctx->hook_pairs_small_sets = (int)value;
    else if (n == "filter_classic") ctx->hook_filter_classic = (int)value;
    else if (n == "graph_load_pct") {
        if (value != 0 && value != -1 && (value < 10 || value > 75)) return fail(ctx, GK_E_INVALID, "graph_load_pct: 0 / -1 default, else 10..75");
        ctx->hook_graph_load_pct = value > 0 ? (int)value : -1;
    }
    else if (n == "test_fastq_chunk") ctx->hook_fastq_chunk = (int64_t)std::max<int64_t>(0, value);
    else if (n == "test_max_grid") {
        if (value < 0) return fail(ctx, GK_E_INVALID, "test_max_grid: 0 off, else the most workgroups of a grid-stride launch");
        ctx->hook_max_grid = (int)std::min<int64_t>(value, 1 << 30);
    }
    else if (n == "test_place_slice") ctx->hook_place_slice = (int64_t)std::max<int64_t>(0, value);
    else if (n == "test_prefilter_chunk_windows") ctx->hook_pf_chunk_windows = (int64_t)std::max<int64_t>(0, value);
    else if (n == "test_multik_chunk_windows") ctx->hook_multik_chunk_windows = (int64_t)std::max<int64_t>(0, value);
    else if (n == "contigs_chunk_bytes") ctx->hook_contigs_chunk = (int64_t)std::max<int64_t>(0, value);
    else if (n == "twin_key_bits") {
        if (value < 0 || value > 128) return fail(ctx, GK_E_INVALID, "twin_key_bits: 0..128");
        ctx->hook_twin_key_bits = (int)value;
    }
    else if (n == "fine_exact") ctx->hook_fine_exact = value < 0 ? -1 : value != 0;
    else return fail(ctx, GK_E_INVALID, "gk_ctx_set_option: unknown option '" + n + "'");
    return GK_OK;
}

int gk_test_grid_cap_uses(const gk_ctx *ctx, uint64_t *uses) {
    if (!ctx || !uses) return fail(ctx, GK_E_INVALID, "gk_test_grid_cap_uses: null argument");
    *uses = ctx->hook_max_grid_uses;
    return GK_OK;
}

int gk_test_prefilter_chunks(const gk_prefilter *pf, uint64_t *host_fixed, uint64_t *host_offsets, uint64_t *dev_pass2, uint64_t *pass2_launches) {
    if (!pf) return fail(nullptr, GK_E_INVALID, "gk_test_prefilter_chunks: null filter handle");
    uint64_t c[4];
    prefilter_chunk_counts(pf, c);
    if (host_fixed) *host_fixed = c[0];
    if (host_offsets) *host_offsets = c[1];
    if (dev_pass2) *dev_pass2 = c[2];
    if (pass2_launches) *pass2_launches = c[3];
    return GK_OK;
}

int gk_test_multik_chunks(const gk_ctx *ctx, uint64_t *chunks) {
    if (!ctx || !chunks) return fail(ctx, GK_E_INVALID, "gk_test_multik_chunks: null argument");
    *chunks = ctx->multik_last_chunks;
    return GK_OK;
}

int gk_test_part_plan(const gk_test_part_in *in, gk_test_part_out *out) {
    if (!in || !out) return fail(nullptr, GK_E_INVALID, "gk_test_part_plan: null argument");
    if ((in->W != 1 && in->W != 2) || in->lnb1 < 0 || in->lnb1 > (int)gk::MAX_LNB1 || in->source < PART_SRC_DEVICE || in->source > PART_SRC_KEYS)
        return fail(nullptr, GK_E_INVALID, "gk_test_part_plan: W 1 / 2, lnb1 0..10, source 0..4");
    PartInput pi;
    pi.W = in->W; pi.lnb1 = in->lnb1; pi.nb2 = in->nb2; pi.source = in->source; pi.max_windows = in->max_windows;
    pi.from_empty = in->from_empty != 0; pi.verify_uniform = in->verify_uniform != 0; pi.estimate = in->estimate != 0; pi.fine_exact = in->fine_exact != 0;
    pi.part_exact = in->part_exact != 0;
    pi.p4_wide = in->p4_wide; pi.p4_direct = in->p4_direct; pi.p2_wide = in->p2_wide; pi.p2_sorted = in->p2_sorted;
    pi.p45_stripes = in->p45_stripes; pi.p24_pieces = in->p24_pieces; pi.p4_grid = in->p4_grid; pi.max_nb2 = in->test_max_nb2;
    const PartChoice c = part_choose(pi);
    memset(out, 0, sizeof *out);
    auto echo = [&](const P4Form *f, gk_test_part_form *o) {
        strncpy(o->name, f->name, sizeof o->name - 1);
        o->chunk_keys = f->chunk_keys(); o->threads = (uint32_t)f->threads; o->lds_bytes = f->lds(in->nb2, 1u << in->lnb1);
    };
    echo(c.p4_op, &out->p4_op);
    echo(c.p4_exact, &out->p4_exact);
    strncpy(out->p2, c.p2, sizeof out->p2 - 1);
    out->supported = c.supported; out->op1 = c.op1; out->fine_exact = c.fine_exact; out->sync_between = c.sync_between; out->pipelined = c.pipelined;
    out->stripes = c.fine_exact ? 1 : c.op_stripes;
    return GK_OK;
}

int gk_test_support_last_walk(const gk_support *s, uint64_t *orientations, uint64_t *overflowed) {
    if (!s) return fail(nullptr, GK_E_INVALID, "gk_test_support_last_walk: null support handle");
    if (orientations) *orientations = s->last_orientations;
    if (overflowed) *overflowed = s->last_overflow;
    return GK_OK;
}

// d_out (n + 1 words) and d_sums (exactly n / SCAN_CHUNK + 2 words) each lie between two guards of SCAN_GUARD words inside one
// allocation of their own, and the whole allocation starts as 0xA5 bytes: a word of the result the scan did not write shows in
// the comparison, a write beside the result in *guard_hits.
static constexpr u64 SCAN_GUARD = 64, SCAN_FILL = 0xA5A5A5A5A5A5A5A5ull;
int gk_test_scan_counts(gk_ctx *ctx, const uint32_t *in_host, uint64_t n, int via_scratch, uint64_t *out_host, uint64_t *guard_hits) {
    if (!ctx || !out_host || !guard_hits || (n && !in_host)) return fail(ctx, GK_E_INVALID, "gk_test_scan_counts: null argument");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    const u64 nsums = n / SCAN_CHUNK + 2, out_words = n + 1 + 2 * SCAN_GUARD, sums_words = nsums + 2 * SCAN_GUARD;
    DevScratch tmp(ctx);
    u32 *d_in = nullptr;
    u64 *out_blk = nullptr, *sums_blk = nullptr;
    if (n) tmp.upload(&d_in, in_host, n);
    tmp.get(&out_blk, out_words);
    if (!via_scratch) tmp.get(&sums_blk, sums_words);
    if (tmp.error() == hipSuccess) tmp.note(hipMemsetAsync(out_blk, 0xA5, out_words * 8, ctx->stream));
    if (tmp.error() == hipSuccess && sums_blk) tmp.note(hipMemsetAsync(sums_blk, 0xA5, sums_words * 8, ctx->stream));
    if (tmp.error() != hipSuccess) return hip_fail(ctx, tmp.error(), "gk_test_scan_counts: buffers");
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(out_blk + SCAN_GUARD);
    const hipError_t es = via_scratch ? scan_counts(ctx, tmp, d_in, n, d_out) : scan_counts(ctx, d_in, n, d_out, sums_blk + SCAN_GUARD);
    if (es != hipSuccess) return hip_fail(ctx, es, "gk_test_scan_counts: scan");
    u64 guards[4 * SCAN_GUARD];
    for (u64 &g : guards) g = SCAN_FILL;          // (the two of d_sums stay so under via_scratch)
    const size_t gb = SCAN_GUARD * 8;
    const u64 *sums_hi = sums_blk ? sums_blk + SCAN_GUARD + nsums : nullptr;
    const hipError_t e = read_back(ctx, {{out_host, d_out, (n + 1) * 8}, {guards, out_blk, gb}, {guards + SCAN_GUARD, out_blk + SCAN_GUARD + n + 1, gb},
                                         {sums_blk ? guards + 2 * SCAN_GUARD : nullptr, sums_blk, gb},
                                         {sums_hi ? guards + 3 * SCAN_GUARD : nullptr, sums_hi, gb}});
    if (e != hipSuccess) return hip_fail(ctx, e, "gk_test_scan_counts: read back");
    u64 hits = 0;
    for (u64 g : guards) hits += g != SCAN_FILL;
    *guard_hits = hits;
    return GK_OK;
}

int gk_test_edge_path_keys(gk_graph *g, uint64_t *h1, uint64_t *h2, uint32_t *canon, uint8_t *dup, uint64_t *nlive, uint64_t *fingerprint) {
    if (!g || !g->ctx) return fail(nullptr, GK_E_INVALID, "gk_test_edge_path_keys: null graph handle");
    gk_ctx *ctx = g->ctx;
    if (!h1 || !h2 || !canon || !dup || !nlive || !fingerprint) return fail(ctx, GK_E_INVALID, "gk_test_edge_path_keys: null argument");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    DevScratch keep(ctx);
    u32 *d_canon = nullptr, *d_inv = nullptr;
    uint8_t *d_dup = nullptr;
    u64 *d_h1 = nullptr, *d_h2 = nullptr, n = 0, fp = 0;
    if (int rc = graph_edge_pathkeys(g, keep, &d_canon, &d_inv, &d_dup, &n, &fp, &d_h1, &d_h2)) return rc;
    const size_t ne = g->v.n_edges;
    if (ne) GK_HIP(ctx, read_back(ctx, {{h1, d_h1, ne * 8}, {h2, d_h2, ne * 8}, {canon, d_canon, ne * 4}, {dup, d_dup, ne}}));
    *nlive = n; *fingerprint = fp;
    return GK_OK;
}

int gk_test_slot_ranks(gk_map *map, uint64_t *masks, uint64_t *bases, uint64_t cap_blocks, uint64_t *nblk, uint64_t *total) {
    if (!map || !map->ctx) return fail(nullptr, GK_E_INVALID, "gk_test_slot_ranks: null map handle");
    if (!masks || !bases || !nblk || !total) return fail(map->ctx, GK_E_INVALID, "gk_test_slot_ranks: null argument");
    return graph_slot_ranks(map, masks, bases, cap_blocks, nblk, total);
}

// gk_shard_superkmers_dev's three steps over the offset-table overload of the launch (the product reaches it through gk_dist_* only)
int gk_test_skm_route_offsets(gk_ctx *ctx, int k, const void *dev_records, const uint32_t *dev_offsets, uint64_t nreads, uint64_t windows, int P,
                              void *dev_out, uint64_t out_cap_records, uint64_t *rec_counts_host, uint64_t *kmer_counts_host) {
    if (!ctx) return fail(nullptr, GK_E_INVALID, "null ctx");
    if (!rec_counts_host || !kmer_counts_host) return fail(ctx, GK_E_INVALID, "gk_test_skm_route_offsets: null argument");
    if (!ctx->skm_counts) GK_HIP(ctx, pool_malloc(ctx, &ctx->skm_counts, SKM_COUNT_WORDS * sizeof(unsigned long long)));
    unsigned long long h[SKM_COUNT_WORDS];
    if (int rc = skm_route_launch(ctx, ctx->stream, (unsigned long long *)ctx->skm_counts, h, k, dev_records, dev_offsets, nreads, windows, P, dev_out, out_cap_records)) return rc;
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return skm_route_finish(ctx, h, nreads && windows, P, out_cap_records, rec_counts_host, kmer_counts_host);
}

}  // extern "C"

// ---- loopback transport (tests): the ranks of one "node" are threads of ONE process on ONE device --------------------------
// RCCL refuses two ranks on one GPU, and only one GPU is reachable from the build box: gk_dist_create_loopback gives every
// rank a handle whose sends, receives and reductions go through this hub instead — device-to-device copies between the
// ranks' buffers, matched pairwise in posting order like RCCL's — so that the exchange logic of gk_dist_* (sizes, regions,
// buffer rotation, the order of operations across ranks) runs with world > 1 before it ever meets a real communicator.  It is
// STRICTER than RCCL in two ways that make it a better test: a group's end blocks until every peer has posted the matching
// operation (an inconsistent order of operations across ranks deadlocks here at once), and a send whose size differs from
// the matching receive is an error.
namespace {
struct LoopHub {
    std::mutex mu;
    std::condition_variable cv;
    int world = 0, refs = 0;
    struct Op { void *ptr; size_t bytes; hipStream_t stream; hipEvent_t ready; bool *done; int *err; };
    std::deque<Op> sends[64][64], recvs[64][64];          // [src][dst], in posting order
    // reductions / gathers: one at a time, every rank contributes
    unsigned long long gen = 0;
    int arrived = 0;
    std::vector<double> contrib[64];                      // (any length: a spectrum reduces a histogram)
    std::vector<double> result;
    bool result_ok = true;                                // false: the ranks disagreed about the length (RCCL would hang): every rank gets an error
    std::vector<hipEvent_t> events;                       // every event the transport made; destroyed with the hub
    ~LoopHub() { for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e); }
};
std::mutex g_hubs_mu;
std::map<std::string, std::shared_ptr<LoopHub>> g_hubs;
}  // namespace


namespace {
struct LoopState {
    std::shared_ptr<LoopHub> hub;
    std::string key;
    struct Posted { bool send; void *ptr; size_t bytes; int peer; hipStream_t stream; };
    std::vector<Posted> group;                       // the operations of the group being built
    ~LoopState() {
        std::lock_guard<std::mutex> lk(g_hubs_mu);
        if (hub && --hub->refs == 0) g_hubs.erase(key);
    }
};
size_t dtype_bytes(int dt) { return dt == XP_UINT64 || dt == XP_FLOAT64 ? 8 : 1; }
int loop_group_start(gk_dist *d) { static_cast<LoopState *>(d->xstate.get())->group.clear(); return XP_SUCCESS; }
int loop_send(gk_dist *d, const void *p, size_t count, int dt, int peer, hipStream_t st) {
    static_cast<LoopState *>(d->xstate.get())->group.push_back({true, const_cast<void *>(p), count * dtype_bytes(dt), peer, st});
    return XP_SUCCESS;
}
int loop_recv(gk_dist *d, void *p, size_t count, int dt, int peer, hipStream_t st) {
    static_cast<LoopState *>(d->xstate.get())->group.push_back({false, p, count * dtype_bytes(dt), peer, st});
    return XP_SUCCESS;
}
int loop_group_end(gk_dist *d) {
    LoopState &ls = *static_cast<LoopState *>(d->xstate.get());
    LoopHub &h = *ls.hub;
    const size_t n = ls.group.size();
    std::unique_ptr<bool[]> done(new bool[n]());
    int err = 0;
    std::unique_lock<std::mutex> lk(h.mu);
    for (size_t i = 0; i < n; i++) {
        const LoopState::Posted &o = ls.group[i];
        hipEvent_t ev = nullptr;
        if (o.send) {                                 // the data is ready once the sender's stream reaches this point
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, o.stream) != hipSuccess) err = 1;
            h.events.push_back(ev);
            h.sends[d->rank][o.peer].push_back({o.ptr, o.bytes, o.stream, ev, &done[i], &err});
        } else {
            h.recvs[o.peer][d->rank].push_back({o.ptr, o.bytes, o.stream, nullptr, &done[i], &err});
        }
    }
    // match whatever can be matched (any thread may complete any pair), then wait for the rest of this group
    auto match_all = [&]() {
        for (int s = 0; s < h.world; s++)
            for (int r = 0; r < h.world; r++)
                while (!h.sends[s][r].empty() && !h.recvs[s][r].empty()) {
                    LoopHub::Op a = h.sends[s][r].front(), b = h.recvs[s][r].front();
                    h.sends[s][r].pop_front(); h.recvs[s][r].pop_front();
                    int e = 0;
                    if (a.bytes != b.bytes) e = 2;                               // RCCL would hang or corrupt here
                    else if (a.bytes) {
                        hipEvent_t copied = nullptr;
                        if (hipStreamWaitEvent(b.stream, a.ready, 0) != hipSuccess) e = 1;
                        if (!e && hipMemcpyAsync(b.ptr, a.ptr, a.bytes, hipMemcpyDeviceToDevice, b.stream) != hipSuccess) e = 1;
                        // the sender may reuse its buffer only after the copy: its stream waits for it
                        if (!e && (hipEventCreateWithFlags(&copied, hipEventDisableTiming) != hipSuccess || hipEventRecord(copied, b.stream) != hipSuccess ||
                                   hipStreamWaitEvent(a.stream, copied, 0) != hipSuccess)) e = 1;
                        if (copied) h.events.push_back(copied);
                    }
                    if (e) { *a.err = e; *b.err = e; }
                    *a.done = true; *b.done = true;
                }
    };
    auto all_done = [&]() { for (size_t i = 0; i < n; i++) if (!done[i]) return false; return true; };
    match_all();
    h.cv.notify_all();
    while (!all_done()) {
        h.cv.wait(lk);
        match_all();
        h.cv.notify_all();
    }
    lk.unlock();
    ls.group.clear();
    return err ? 3 /* ncclInternalError */ : XP_SUCCESS;
}
static int loop_collective(gk_dist *d, const void *in, void *out, size_t n, int dt, int op, bool gather, hipStream_t st) {
    LoopHub &h = *static_cast<LoopState *>(d->xstate.get())->hub;
    if (n < 1 || (gather && n != 1)) return 3;
    std::vector<double> mine(n);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(mine.data(), in, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    size_t nres = gather ? (size_t)h.world : n;
    std::vector<double> res(nres);
    {
        std::unique_lock<std::mutex> lk(h.mu);
        const unsigned long long gen = h.gen;
        h.contrib[d->rank] = mine;
        if (++h.arrived == h.world) {
            h.result.assign(nres, 0.0);
            h.result_ok = true;
            for (int r = 0; r < h.world; r++) h.result_ok = h.result_ok && h.contrib[r].size() == n;
            for (size_t i = 0; i < nres && h.result_ok; i++) {
                if (gather) { memcpy(&h.result[i], &h.contrib[i][0], 8); continue; }
                if (dt == XP_FLOAT64) {
                    double acc = h.contrib[0][i];
                    for (int r = 1; r < h.world; r++) acc = op == XP_MAX ? std::max(acc, h.contrib[r][i]) : acc + h.contrib[r][i];
                    h.result[i] = acc;
                } else {
                    unsigned long long acc = 0, v;
                    for (int r = 0; r < h.world; r++) { memcpy(&v, &h.contrib[r][i], 8); acc = op == XP_MAX ? std::max(acc, v) : acc + v; }
                    memcpy(&h.result[i], &acc, 8);
                }
            }
            h.arrived = 0;
            h.gen++;
            h.cv.notify_all();
        } else {
            h.cv.wait(lk, [&]() { return h.gen != gen; });
        }
        if (!h.result_ok || h.result.size() != nres) return 3;
        memcpy(res.data(), h.result.data(), nres * 8);
    }
    return hipMemcpyAsync(out, res.data(), nres * 8, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? XP_SUCCESS : 3;
}
int loop_all_reduce(gk_dist *d, const void *in, void *out, size_t n, int dt, int op, hipStream_t st) { return loop_collective(d, in, out, n, dt, op, false, st); }
int loop_all_gather(gk_dist *d, const void *in, void *out, size_t n, int dt, hipStream_t st) { return loop_collective(d, in, out, n, dt, XP_SUM, true, st); }
std::string loop_error_text(int) { return "transport error (loopback: a send and its receive differ in size, the ranks of a reduction differ in length, or a HIP call failed)"; }
void loop_close(gk_dist *d) { d->xstate.reset(); }
const Transport LOOP_TRANSPORT = {loop_group_start, loop_send, loop_recv, loop_group_end, loop_all_reduce, loop_all_gather, loop_error_text, loop_close};
}  // namespace

extern "C" int gk_dist_create_loopback(gk_ctx *ctx, int rank, int world, const void *id128, gk_dist **out) {
    if (!ctx || !out || !id128) return fail(ctx, GK_E_INVALID, "gk_dist_create_loopback: null argument");
    *out = nullptr;
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return fail(ctx, GK_E_INVALID, "gk_dist_create_loopback: need 0 <= rank < world <= 64");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    // the ranks of one loopback "node" find each other by the id (any 128 bytes every rank was given alike)
    auto ls = std::make_shared<LoopState>();
    ls->key.assign((const char *)id128, 128);
    {
        std::lock_guard<std::mutex> lk(g_hubs_mu);
        std::shared_ptr<LoopHub> &h = g_hubs[ls->key];
        if (!h) { h = std::make_shared<LoopHub>(); h->world = world; }
        if (h->world != world) return fail(ctx, GK_E_INVALID, "gk_dist_create_loopback: the ranks of one id disagree about the world size");
        h->refs++;
        ls->hub = h;
    }
    gk_dist *d = nullptr;
    if (int rc = dist_create_common(ctx, rank, world, &d)) return rc;
    d->xport = &LOOP_TRANSPORT;
    d->xstate = ls;
    *out = d;
    return GK_OK;
}
