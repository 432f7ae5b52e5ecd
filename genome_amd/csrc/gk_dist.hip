// gk_dist.hip — PartitionedDNAMap across the GPUs of one node, behind the C-ABI: one rank per GPU, one table partition
// per rank, k-mers routed to their owner with ONE all-to-all over RCCL/xGMI per batch.
//
// Reference path replaced (S/ = /root/reference/src/main/scala/ru/ifmo/genome/):
//   PartitionedDNAMap.update / update1   S/ds/PartitionedDNAMap.scala:37-47   gk_dist_count_reads_dev (route -> exchange -> owner count)
//   PartitionedDNAMap.partition          :60-63                               gk_owner_of (strand-symmetric minimizer, gk_device.h)
//   PartitionedDNAMap.size               :31                                  gk_dist_size (all-reduce of one integer)
//   deleteAll / mapReduce scatter-gather :49-58                               local calls on every rank's gk_map (no data exchange)
//   "the whole k-mer set" for Graph.buildGraph (Graph.scala:269)              gk_dist_gather_map (all-gather of the survivors, device to device)
//
// The reference sends one Akka message per k-mer occurrence (driver -> owner actor).  Here a rank turns its reads into
// SUPER-K-MER records grouped by owner (gk_skm.hip: ~2 bits per base instead of 8/16 bytes per k-mer), exchanges the
// per-owner (records, k-mers) counts, then the records — sizes are exact, nothing is padded or packed: region p of the
// send buffer goes straight to rank p with ncclSend, what arrives lands back to back — and counts what it received with
// the same pipeline as reads (gk_map_count_superkmers_dev).  xGMI is point to point (7 links per GPU): an all-to-all puts
// one peer on each link, which is why this is a grouped send/recv and not a ring collective.
//
// RCCL is loaded at run time (dlopen), so the library has no link-time dependency on it: a single-GPU user never needs
// it, and a process that already holds an RCCL (PyTorch bundles one) shares that copy.
#include <dlfcn.h>
#include <time.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gk_binstream.h"
#include "gk_dist.h"
#include "gk_graph.h"
#include "gk_links.h"
#include "gk_support.h"
#include "gk_tile.h"

using namespace gk;

// ---- the handful of RCCL entry points used (rccl.h: NCCL-compatible ABI) ---------------------------------------------
namespace {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
enum { ncclSuccess = 0 };
enum { ncclInt8 = 0, ncclUint8 = 1, ncclUint64 = 5, ncclFloat64 = 8 };      // ncclDataType_t
enum { ncclSum = 0, ncclMax = 2 };                                           // ncclRedOp_t

struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(ncclUniqueId *) = nullptr;
    int (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*Send)(const void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
};

Rccl *rccl() {
    static Rccl r;
    static bool tried = false;
    if (tried) return &r;
    tried = true;
    // an RCCL this process already holds (PyTorch's) first, then the ROCm one
    for (const char *name : {"librccl.so", "librccl.so.1"}) {
        r.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
        if (r.lib) break;
    }
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        if (r.lib) break;
        r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    }
    if (!r.lib) { r.why = std::string("cannot load librccl: ") + dlerror(); return &r; }
    auto sym = [&](const char *n) { void *p = dlsym(r.lib, n); if (!p && r.why.empty()) r.why = std::string("librccl lacks ") + n; return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    return &r;
}
}  // namespace

static void helper_main(gk_dist *d) {
    (void)hipSetDevice(d->ctx->device);
    std::unique_lock<std::mutex> lk(d->wmu);
    for (;;) {
        d->wcv.wait(lk, [&]() { return d->job_pending || d->quit; });
        if (d->quit) return;
        std::function<void()> f = std::move(d->job);
        d->job_pending = false; d->job_running = true;
        lk.unlock();
        f();
        lk.lock();
        d->job_running = false;
        d->wcv.notify_all();
    }
}
static void helper_submit(gk_dist *d, std::function<void()> f) {
    std::unique_lock<std::mutex> lk(d->wmu);
    if (!d->worker.joinable()) d->worker = std::thread(helper_main, d);
    d->job = std::move(f);
    d->job_pending = true;
    d->wcv.notify_all();
}
static void helper_wait(gk_dist *d) {
    std::unique_lock<std::mutex> lk(d->wmu);
    d->wcv.wait(lk, [&]() { return !d->job_pending && !d->job_running; });
}
static void helper_stop(gk_dist *d) {
    {
        std::unique_lock<std::mutex> lk(d->wmu);
        d->wcv.wait(lk, [&]() { return !d->job_pending && !d->job_running; });
        d->quit = true;
        d->wcv.notify_all();
    }
    if (d->worker.joinable()) d->worker.join();
}
// buffers the helper thread replaced: their frees wait for the owner thread (pool_free synchronises the context's streams)
static void drain_garbage(gk_dist *d) {
    gk_ctx *ctx = d->ctx;
    std::vector<void *> g;
    { std::lock_guard<std::mutex> lk(d->wmu); g.swap(d->garbage); }
    for (void *p : g) (void)pool_free(ctx, p);
}

static thread_local const gk_dist *tl_dist = nullptr;       // whose transport explains an error code (set by dist_check)
static std::string comm_error_text(int code) {
    if (tl_dist && tl_dist->xport) return tl_dist->xport->error_text(code);
    Rccl *r = rccl();
    return r->GetErrorString ? r->GetErrorString(code) : "RCCL error";
}
#define GK_NCCL(ctx, call)                                                                                        \
    do {                                                                                                          \
        int r__ = (call);                                                                                         \
        if (r__ != ncclSuccess)                                                                                   \
            return gk::fail((ctx), GK_E_COMM, std::string(#call) + ": " + comm_error_text(r__)); \
    } while (0)

// ---- the RCCL transport -----------------------------------------------------------------------------------------------------
namespace {
int rccl_group_start(gk_dist *) { return rccl()->GroupStart(); }
int rccl_send(gk_dist *d, const void *p, size_t count, int dt, int peer, hipStream_t st) { return rccl()->Send(p, count, dt, peer, (ncclComm_t)d->comm, st); }
int rccl_recv(gk_dist *d, void *p, size_t count, int dt, int peer, hipStream_t st) { return rccl()->Recv(p, count, dt, peer, (ncclComm_t)d->comm, st); }
int rccl_group_end(gk_dist *) { return rccl()->GroupEnd(); }
int rccl_all_reduce(gk_dist *d, const void *in, void *out, size_t n, int dt, int op, hipStream_t st) { return rccl()->AllReduce(in, out, n, dt, op, (ncclComm_t)d->comm, st); }
int rccl_all_gather(gk_dist *d, const void *in, void *out, size_t n, int dt, hipStream_t st) { return rccl()->AllGather(in, out, n, dt, (ncclComm_t)d->comm, st); }
std::string rccl_error_text(int code) { Rccl *r = rccl(); return r->GetErrorString ? r->GetErrorString(code) : "RCCL error"; }
void rccl_close(gk_dist *d) { if (d->comm && rccl()->CommDestroy) (void)rccl()->CommDestroy((ncclComm_t)d->comm); d->comm = nullptr; }
const Transport RCCL_TRANSPORT = {rccl_group_start, rccl_send, rccl_recv, rccl_group_end, rccl_all_reduce, rccl_all_gather, rccl_error_text, rccl_close};
}  // namespace
static int xGroupStart(gk_dist *d) { return d->xport->group_start(d); }
static int xSend(gk_dist *d, const void *p, size_t count, int dt, int peer, hipStream_t st) { return d->xport->send(d, p, count, dt, peer, st); }
static int xRecv(gk_dist *d, void *p, size_t count, int dt, int peer, hipStream_t st) { return d->xport->recv(d, p, count, dt, peer, st); }
static int xGroupEnd(gk_dist *d) { return d->xport->group_end(d); }
static int xAllReduce(gk_dist *d, const void *in, void *out, size_t n, int dt, int op, hipStream_t st) { return d->xport->all_reduce(d, in, out, n, dt, op, st); }
static int xAllGather(gk_dist *d, const void *in, void *out, size_t n_per_rank, int dt, hipStream_t st) { return d->xport->all_gather(d, in, out, n_per_rank, dt, st); }

static int dist_check(const gk_dist *d) {
    if (!d || !d->ctx || !d->xport) return fail(nullptr, GK_E_INVALID, "null or closed gk_dist handle");
    tl_dist = d;
    hipError_t e = hipSetDevice(d->ctx->device);
    if (e != hipSuccess) return hip_fail(d->ctx, e, "hipSetDevice");
    return GK_OK;
}

static double now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

extern "C" {

int gk_dist_unique_id(void *id128) {
    if (!id128) return fail(nullptr, GK_E_INVALID, "gk_dist_unique_id: null buffer");
    Rccl *r = rccl();
    if (!r->why.empty()) return fail(nullptr, GK_E_COMM, r->why);
    ncclUniqueId id;
    GK_NCCL(nullptr, r->GetUniqueId(&id));
    memcpy(id128, id.internal, 128);
    return GK_OK;
}

}  // extern "C"
namespace gk {
int dist_create_common(gk_ctx *ctx, int rank, int world, gk_dist **out) {
    *out = nullptr;
    gk_dist *d = new gk_dist();
    d->ctx = ctx; d->rank = rank; d->world = world;
    hipError_t e = pool_malloc(ctx, &d->d_cnt, 8 * 64 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void **)&d->h_cnt, 8 * 64 * sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) e = pool_malloc(ctx, &d->d_route_cnt, gk_dist::NROUTE * SKM_COUNT_WORDS * sizeof(unsigned long long));
    for (int i = 0; i < gk_dist::NROUTE && e == hipSuccess; i++) e = hipEventCreateWithFlags(&d->route_done[i], hipEventDisableTiming);
    for (int i = 0; i < gk_dist::NROUTE && e == hipSuccess; i++) e = hipEventCreateWithFlags(&d->exch_done[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void **)&d->h_route_cnt, gk_dist::NROUTE * SKM_COUNT_WORDS * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) { int c = hip_fail(ctx, e, "gk_dist_create"); gk_dist_destroy(d); return c; }
    *out = d;
    return GK_OK;
}
}  // namespace gk
extern "C" {

int gk_dist_create(gk_ctx *ctx, int rank, int world, const void *id128, gk_dist **out) {
    if (!ctx || !out || !id128) return fail(ctx, GK_E_INVALID, "gk_dist_create: null argument");
    *out = nullptr;
    if (world < 1 || world > 64 || rank < 0 || rank >= world) return fail(ctx, GK_E_INVALID, "gk_dist_create: need 0 <= rank < world <= 64");
    Rccl *r = rccl();
    if (!r->why.empty()) return fail(ctx, GK_E_COMM, r->why);
    GK_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    memcpy(id.internal, id128, 128);
    ncclComm_t comm = nullptr;
    const int rc = r->CommInitRank(&comm, world, id, rank);
    if (rc != ncclSuccess) return fail(ctx, GK_E_COMM, std::string("ncclCommInitRank: ") + (r->GetErrorString ? r->GetErrorString(rc) : "error"));
    gk_dist *d = nullptr;
    if (int c = dist_create_common(ctx, rank, world, &d)) { if (r->CommDestroy) (void)r->CommDestroy(comm); return c; }
    d->xport = &RCCL_TRANSPORT;
    d->comm = comm;
    *out = d;
    return GK_OK;
}

void gk_dist_destroy(gk_dist *d) {
    if (!d) return;
    gk_ctx *ctx = d->ctx;
    helper_stop(d);
    if (ctx) { (void)hipSetDevice(ctx->device); drain_garbage(d); }
    if (d->ctx) { (void)hipSetDevice(d->ctx->device); (void)hipStreamSynchronize(d->ctx->stream); }
    if (d->comm_stream) (void)hipStreamSynchronize(d->comm_stream);
    if (d->xport && d->xport->close) d->xport->close(d);
    if (d->ctx && d->ctx->copy_stream) (void)hipStreamSynchronize(d->ctx->copy_stream);
    for (int i = 0; i < gk_dist::NROUTE; i++) (void)pool_free(ctx, d->d_sendbuf[i]);
    for (int i = 0; i < 2; i++) (void)pool_free(ctx, d->d_recv[i]);
    for (int i = 0; i < gk_dist::NROUTE; i++) { (void)pool_free(ctx, d->d_stage[i]); (void)pool_free(ctx, d->d_stage_offs[i]); }
    for (int i = 0; i < gk_dist::NROUTE; i++) if (d->route_done[i]) (void)hipEventDestroy(d->route_done[i]);
    for (int i = 0; i < gk_dist::NROUTE; i++) if (d->exch_done[i]) (void)hipEventDestroy(d->exch_done[i]);
    if (d->join) (void)hipEventDestroy(d->join);
    if (d->comm_stream) (void)hipStreamDestroy(d->comm_stream);
    (void)pool_free(ctx, d->d_route_cnt);
    if (d->h_route_cnt) (void)hipHostFree(d->h_route_cnt);
    (void)pool_free(ctx, d->d_cnt);
    if (d->h_cnt) (void)hipHostFree(d->h_cnt);
    delete d;
}

int gk_dist_rank(const gk_dist *d) { return d ? d->rank : -1; }
int gk_dist_world(const gk_dist *d) { return d ? d->world : 0; }

// The collectives below run on the context's stream; a batch whose exchange was posted ahead (gk_dist_count_routed) may still
// be on the wire on the communication stream, and two operations of one communicator must not run side by side.
static int dist_quiesce(gk_dist *d) {
    GK_HIP(d->ctx, hipStreamSynchronize(d->comm_stream));
    return GK_OK;
}

int gk_dist_barrier(gk_dist *d) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (int rc = dist_quiesce(d)) return rc;
    GK_HIP(ctx, hipMemsetAsync(d->d_cnt, 0, 8, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt, d->d_cnt, 1, ncclUint64, ncclSum, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GK_OK;
}

int gk_dist_allreduce_f64(gk_dist *d, double *values, int n, int op_max) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (!values || n < 1 || n > 32) return fail(ctx, GK_E_INVALID, "gk_dist_allreduce_f64: 1..32 values");
    if (int rc = dist_quiesce(d)) return rc;
    double *dv = reinterpret_cast<double *>(d->d_cnt);
    GK_HIP(ctx, hipMemcpyAsync(dv, values, n * 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, dv, dv, (size_t)n, ncclFloat64, op_max ? ncclMax : ncclSum, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(values, dv, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GK_OK;
}

int gk_dist_size(gk_dist *d, gk_map *local, uint64_t *total) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (!local || !total) return fail(ctx, GK_E_INVALID, "gk_dist_size: null argument");
    if (int rc = dist_quiesce(d)) return rc;
    unsigned long long v = local->size;
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt, &v, 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt, d->d_cnt, 1, ncclUint64, ncclSum, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(&v, d->d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *total = v;
    return GK_OK;
}

// The spectrum of the whole map on every rank.  The status round comes FIRST, on the handle's own words (they exist whatever
// fails here): a rank that could not take its spectrum, or has no room for the histogram, says so beside its largest count, and
// the histogram is only reduced once every rank is known to hold one.  The results are read without a launch check in between
// (a check could fail one rank in a round the others passed).
int gk_dist_spectrum(gk_dist *d, gk_map *local, uint64_t *hist, uint32_t bins, uint64_t *distinct, uint64_t *occurrences, uint32_t *max_count) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    const char *who = "gk_dist_spectrum: ";
    if (!hist) return fail(ctx, GK_E_INVALID, std::string(who) + "hist is NULL");
    if (bins < 2 || bins > (1u << 20)) return fail(ctx, GK_E_INVALID, std::string(who) + "bins must be 2 .. 1<<20");
    if (int rc = dist_quiesce(d)) return rc;
    int my_rc = GK_OK;
    std::string my_err;
    auto local_rc = [&](int rc) { if (rc != GK_OK && my_rc == GK_OK) { my_rc = rc; my_err = ctx->err; } };
    std::vector<unsigned long long> h((size_t)bins + 2, 0ull);       // hist, distinct, occurrences
    uint32_t mx = 0;
    if (!local) local_rc(fail(ctx, GK_E_INVALID, std::string(who) + "null map"));
    else if (local->ctx != ctx) local_rc(fail(ctx, GK_E_INVALID, std::string(who) + "the map must live on the handle's context"));
    else {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "one histogram type");
        local_rc(gk_map_spectrum(local, reinterpret_cast<uint64_t *>(h.data()), bins, reinterpret_cast<uint64_t *>(&h[bins]),
                                 reinterpret_cast<uint64_t *>(&h[(size_t)bins + 1]), &mx));
    }
    DevScratch buf(ctx);
    unsigned long long *d_h = nullptr;
    if (buf.get(&d_h, h.size()) != hipSuccess) local_rc(fail(ctx, GK_E_HIP, std::string(who) + "no room for the histogram"));
    unsigned long long w[2] = {mx, my_rc ? 1ull : 0ull};
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt, w, 16, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt, d->d_cnt + 2, 2, XP_UINT64, XP_MAX, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(w, d->d_cnt + 2, 16, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (w[1]) return my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, std::string(who) + "a rank could not take the spectrum of its partition; every rank gave up");
    GK_HIP(ctx, hipMemcpyAsync(d_h, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d_h, d_h, h.size(), XP_UINT64, XP_SUM, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(h.data(), d_h, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t b = 0; b < bins; b++) hist[b] = h[b];
    if (distinct) *distinct = h[bins];
    if (occurrences) *occurrences = h[(size_t)bins + 1];
    if (max_count) *max_count = (uint32_t)w[0];
    return GK_OK;
}

// The fragment-length histogram of every rank's pairs on every rank: gk_dist_spectrum's shape.  The status round comes first, on
// the handle's own words; the histogram and the classes travel as one array once every rank is known to hold them.
int gk_dist_pair_distances(gk_dist *d, gk_graph *g, gk_vmap *positions, const uint8_t *bin, size_t nbytes, uint64_t npairs, uint32_t bins, uint64_t *hist,
                           uint64_t *classes) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    const char *who = "gk_dist_pair_distances: ";
    if (!hist || !classes) return fail(ctx, GK_E_INVALID, std::string(who) + "hist or classes is NULL");
    if (bins < 2 || bins > 65536) return fail(ctx, GK_E_INVALID, std::string(who) + "bins must be 2 .. 65536");
    if (int rc = dist_quiesce(d)) return rc;
    int my_rc = GK_OK;
    std::string my_err;
    auto local_rc = [&](int rc) { if (rc != GK_OK && my_rc == GK_OK) { my_rc = rc; my_err = ctx->err; } };
    std::vector<unsigned long long> h((size_t)bins + 9, 0ull);       // hist, then the nine classes
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "one histogram type");
    if (!g) local_rc(fail(ctx, GK_E_INVALID, std::string(who) + "null graph"));
    else if (!positions) local_rc(fail(ctx, GK_E_INVALID, std::string(who) + "null position map"));
    else local_rc(gk_graph_pair_distances(g, positions, bin, nbytes, npairs, bins, reinterpret_cast<uint64_t *>(h.data()), reinterpret_cast<uint64_t *>(&h[bins])));
    DevScratch buf(ctx);
    unsigned long long *d_h = nullptr;
    if (buf.get(&d_h, h.size()) != hipSuccess) local_rc(fail(ctx, GK_E_HIP, std::string(who) + "no room for the histogram"));
    unsigned long long w = my_rc ? 1ull : 0ull;
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt, &w, 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt, d->d_cnt + 2, 1, XP_UINT64, XP_MAX, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(&w, d->d_cnt + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (w) return my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, std::string(who) + "a rank could not take the distances of its pairs; every rank gave up");
    GK_HIP(ctx, hipMemcpyAsync(d_h, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d_h, d_h, h.size(), XP_UINT64, XP_SUM, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(h.data(), d_h, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t b = 0; b < bins; b++) hist[b] = h[b];
    for (int c = 0; c < 9; c++) classes[c] = h[(size_t)bins + c];
    return GK_OK;
}

static int dist_grow(gk_ctx *ctx, uint8_t **buf, u64 *have, u64 want_records, int slot) {
    if (*have >= want_records && *buf) return GK_OK;
    if (*buf) { GK_HIP(ctx, hipStreamSynchronize(ctx->stream)); GK_HIP(ctx, pool_free(ctx, *buf)); }
    *buf = nullptr; *have = 0;
    GK_HIP(ctx, pool_malloc(ctx, buf, std::max<u64>(want_records, 1) * (u64)slot + 64));
    *have = want_records;
    return GK_OK;
}

static u64 route_want_records(int k, int P, u64 nreads, int read_len) {
    // a run of same-owner windows is about half a minimizer window long; a region that turns out too small is reported with
    // the size it needs and the route is taken again
    const u64 nk = read_len >= k ? (u64)(read_len - k + 1) : 0;
    const double per_read = std::max(2.0, (double)nk / std::max(1.0, (k - 9) / 2.0)) * 1.5 + 1.0;
    return std::max<u64>((u64)1024 * P, (u64)((double)nreads * per_read) / P * P);
}
// the same for a ragged batch, from the window total its host walk counted (not nreads x the longest read's windows)
static u64 route_want_records_ragged(int k, int P, u64 nreads, u64 windows) {
    const double runs = std::max(2.0 * (double)nreads, (double)windows / std::max(1.0, (k - 9) / 2.0));
    return std::max<u64>((u64)1024 * P, (u64)(runs * 1.5 + (double)nreads) / P * P);
}
// launch (or re-launch) route slot b's kernel on the context's second stream, in its batch's framing
static int route_launch(gk_dist *d, int b) {
    gk_ctx *ctx = d->ctx;
    const gk_dist::Route &rt = d->route[b];
    unsigned long long *d_rc = d->d_route_cnt + b * SKM_COUNT_WORDS, *h_rc = d->h_route_cnt + b * SKM_COUNT_WORDS;
    ctx->copy_other_pending = true;
    if (rt.offsets) return skm_route_launch(ctx, ctx->copy_stream, d_rc, h_rc, rt.k, rt.records, rt.offsets, rt.nreads, rt.windows, d->world, d->d_sendbuf[b], d->send_cap[b]);
    return skm_route_launch(ctx, ctx->copy_stream, d_rc, h_rc, rt.k, rt.records, rt.nreads, rt.read_len, d->world, d->d_sendbuf[b], d->send_cap[b]);
}
static bool route_has_windows(const gk_dist::Route &rt) { return rt.nreads && (rt.offsets ? rt.windows > 0 : rt.read_len >= rt.k); }

// Begin a route: fixed stride (offsets == nullptr), or the offset framing of a host-walked ragged batch.  carry_rc != 0: this rank
// has already failed this batch (its records could not be staged) — the batch is begun empty, carrying the failure, and its
// gk_dist_count_routed tells every rank, which all drop it together.
static int route_begin_impl(gk_dist *d, int k, const void *dev_records, const uint32_t *dev_offsets, uint64_t nreads, int read_len, uint64_t windows,
                            int carry_rc = GK_OK, const std::string &carry_err = std::string()) {
    gk_ctx *ctx = d->ctx;
    constexpr int NR = gk_dist::NROUTE;
    drain_garbage(d);
    if (d->npending >= NR) return fail(ctx, GK_E_STATE, "gk_dist_route_begin: three routes are already waiting (gk_dist_count_routed consumes one)");
    if (!dev_records && nreads && !carry_rc) return fail(ctx, GK_E_INVALID, "gk_dist_route_begin: null records");
    if (read_len < 0 || read_len > 255) return fail(ctx, GK_E_FORMAT, "read_len must be 0..255 (one length byte per record)");
    if (!k_supported(k)) return fail(ctx, GK_E_UNSUPPORTED_K, "k=" + std::to_string(k) + " unsupported");
    const int P = d->world, slot = gk_skm_slot_bytes(k);
    if (d->slot != slot) {       // key width changed: the buffers were sized in other slots
        if (d->npending) return fail(ctx, GK_E_KLEN, "gk_dist_route_begin: a route for another key width is still waiting");
        GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        GK_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
        GK_HIP(ctx, hipStreamSynchronize(d->comm_stream));
        for (int i = 0; i < NR; i++) { if (d->d_sendbuf[i]) GK_HIP(ctx, pool_free(ctx, d->d_sendbuf[i])); d->d_sendbuf[i] = nullptr; d->send_cap[i] = 0; }
        for (int i = 0; i < 2; i++) { if (d->d_recv[i]) GK_HIP(ctx, pool_free(ctx, d->d_recv[i])); d->d_recv[i] = nullptr; d->recv_records[i] = 0; }
        d->slot = slot;
    }
    const int b = (d->head + d->npending) % NR;
    // (the buffer's previous batch was counted before this slot could come round again: its records have left)
    u64 want = std::max(dev_offsets ? route_want_records_ragged(k, P, nreads, windows) : route_want_records(k, P, nreads, read_len), d->send_cap[b]);
    if (ctx->hook_dist_small_send > 0) {      // test hook: THIS route gets a send buffer of so many records — the in-place re-route must repair it
        GK_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
        if (d->d_sendbuf[b]) { GK_HIP(ctx, pool_free(ctx, d->d_sendbuf[b])); d->d_sendbuf[b] = nullptr; d->send_cap[b] = 0; }
        want = (u64)std::max(ctx->hook_dist_small_send, P);
        ctx->hook_dist_small_send = 0;
    }
    gk_dist::Route &rt = d->route[b];
    rt = gk_dist::Route();
    rt.k = k; rt.read_len = read_len; rt.records = dev_records; rt.nreads = nreads;
    rt.offsets = dev_offsets; rt.windows = windows;
    // A failure from here on is THIS RANK'S ALONE, and its peers are going to exchange this batch: the batch is begun all the
    // same, carrying the failure, and gk_dist_count_routed tells everybody (status word of the counts exchange).
    int rc = carry_rc;
    if (rc) { rt.records = nullptr; rt.offsets = nullptr; rt.nreads = 0; rt.windows = 0; }
    if (!rc) rc = dist_grow(ctx, &d->d_sendbuf[b], &d->send_cap[b], want, slot);
    if (!rc) rc = route_launch(d, b);
    if (rc) { rt.settled = true; rt.local_rc = rc; rt.local_err = carry_rc ? carry_err : ctx->err; (void)hipGetLastError(); }
    GK_HIP(ctx, hipEventRecord(d->route_done[b], ctx->copy_stream));
    d->npending++;
    return GK_OK;
}

// Route this rank's reads for a later gk_dist_count_routed on the context's second stream and return at once: the routing
// kernel (0.6 ms per 10^6 reads, issue-bound) then overlaps whatever the main stream is doing — in a streaming loop, the
// owner pipeline of an earlier batch.  The records buffer must stay valid until the batch's gk_dist_count_routed returns.
int gk_dist_route_begin(gk_dist *d, int k, const void *dev_records, uint64_t nreads, int read_len) {
    if (int rc = dist_check(d)) return rc;
    return route_begin_impl(d, k, dev_records, nullptr, nreads, read_len, 0);
}

// Owner thread: wait for route slot b's kernel, take the route again (bigger, in place) while a region was too small, and
// fix this rank's verdict on its half of the batch.  ms += the wait.
static void route_settle(gk_dist *d, int b, float *ms) {
    gk_ctx *ctx = d->ctx;
    gk_dist::Route &rt = d->route[b];
    if (rt.settled) return;
    const double t0 = now_ms();
    const int P = d->world, slot = d->slot;
    const unsigned long long *h_rc = d->h_route_cnt + b * SKM_COUNT_WORDS;
    int rrc = GK_OK;
    hipError_t e = hipEventSynchronize(d->route_done[b]);            // this route only: later ones may already be queued behind it
    if (e != hipSuccess) rrc = hip_fail(ctx, e, "gk_dist: waiting for the route");
    if (!rrc) rrc = skm_route_finish(ctx, h_rc, route_has_windows(rt), P, d->send_cap[b], rt.recs, rt.kmers);
    for (int attempt = 0; rrc == GK_E_CAPACITY && attempt < 4; attempt++) {       // a region was too small: route again, in place, bigger
        u64 worst = 0;
        for (int p = 0; p < P; p++) worst = std::max<u64>(worst, rt.recs[p]);
        const u64 want = std::max<u64>(d->send_cap[b] * 2, (worst + worst / 8 + 1024) * P);
        if ((e = hipStreamSynchronize(ctx->copy_stream)) != hipSuccess) { rrc = hip_fail(ctx, e, "gk_dist: re-route"); break; }   // (later routes share the stream)
        if ((rrc = dist_grow(ctx, &d->d_sendbuf[b], &d->send_cap[b], want, slot)) != GK_OK) break;
        if ((rrc = route_launch(d, b)) != GK_OK) break;
        if ((e = hipStreamSynchronize(ctx->copy_stream)) != hipSuccess) { rrc = hip_fail(ctx, e, "gk_dist: re-route"); break; }
        rrc = skm_route_finish(ctx, h_rc, true, P, d->send_cap[b], rt.recs, rt.kmers);
    }
    if (!rrc && ctx->hook_dist_fail) {        // test hook: this rank alone fails this batch, as an allocation or a hopeless route would
        rrc = fail(ctx, ctx->hook_dist_fail, "injected failure (test_dist_fail_exchange)");
        ctx->hook_dist_fail = 0;
    }
    rt.local_rc = rrc;
    if (rrc) rt.local_err = ctx->err;
    rt.settled = true;
    *ms += (float)(now_ms() - t0);
}

// Counts and records of route slot b (settled) over RCCL, on the communication stream — on the owner thread or on the
// helper.  Touches neither the context's error string nor its streams nor the pool's frees.  Three steps, and every rank
// takes the same ones whatever happens to it locally:
//   1. counts: (records, k-mers, STATUS) to every peer — a rank whose route failed says so here and sends nothing; if any
//      status is set, every rank drops the batch after this step;
//   2. room for what is coming, then one max-reduction of "I could not make room": any rank -> every rank drops the batch;
//   3. payload: region p -> rank p straight out of the send buffer, arrivals back to back in the receive buffer that is not
//      being counted.  exch_done[b] fires when they have arrived.
// Returns 0 with rt.exchanged set, or the code the batch's count_routed will report (rt.error / rt.error_text).
static int dist_exchange(gk_dist *d, int b, float *ms) {
    gk_ctx *ctx = d->ctx;
    gk_dist::Route &rt = d->route[b];
    const int P = d->world, slot = d->slot;
    const double t1 = now_ms();
    hipStream_t cs = d->comm_stream;
    auto give_up = [&](int code, const std::string &text) { rt.error = code; rt.error_text = text; *ms += (float)(now_ms() - t1); return code; };
    auto hip_text = [](hipError_t e, const char *what) { (void)hipGetLastError(); return std::string(what) + ": " + hipGetErrorString(e); };
    // ---- 1. counts + status
    const u64 region = d->send_cap[b] / (u64)P;
    u64 sent = 0;
    unsigned long long *h_in = d->h_cnt, *h_out = d->h_cnt + 3 * 64, *d_in = d->d_cnt, *d_out = d->d_cnt + 3 * 64;
    for (int p = 0; p < P; p++) {
        h_in[3 * p] = rt.local_rc ? 0 : rt.recs[p];
        h_in[3 * p + 1] = rt.local_rc ? 0 : rt.kmers[p];
        h_in[3 * p + 2] = rt.local_rc ? (unsigned long long)(-rt.local_rc) : 0ull;
        sent += h_in[3 * p + 1];
    }
    hipError_t e = hipMemcpyAsync(d_in, h_in, 3 * P * 8, hipMemcpyHostToDevice, cs);
    if (e != hipSuccess) return give_up(GK_E_HIP, hip_text(e, "gk_dist: counts upload") + " (before anything was posted: the peers will wait; destroy the communicator)");
    int grc = xGroupStart(d);
    for (int p = 0; p < P && grc == ncclSuccess; p++) {
        grc = xSend(d, d_in + 3 * p, 3, ncclUint64, p, cs);
        if (grc == ncclSuccess) grc = xRecv(d, d_out + 3 * p, 3, ncclUint64, p, cs);
    }
    { const int gend = xGroupEnd(d); if (grc == ncclSuccess) grc = gend; }          // (a group that was opened is always closed)
    if (grc != ncclSuccess) return give_up(GK_E_COMM, "counts exchange: " + comm_error_text(grc));
    e = hipMemcpyAsync(h_out, d_out, 3 * P * 8, hipMemcpyDeviceToHost, cs);
    if (e == hipSuccess) e = hipStreamSynchronize(cs);                              // (also: the previous batch's records have arrived)
    if (e != hipSuccess) return give_up(GK_E_HIP, hip_text(e, "gk_dist: counts download"));
    u64 nrec_in = 0, nkm_in = 0;
    int bad_rank = -1;
    for (int p = 0; p < P; p++) {
        nrec_in += h_out[3 * p]; nkm_in += h_out[3 * p + 1];
        if (h_out[3 * p + 2] && bad_rank < 0) bad_rank = p;
    }
    if (bad_rank >= 0) {
        std::string text = "rank " + std::to_string(bad_rank) + " could not route its share of this batch (status " + std::to_string(-(long long)h_out[3 * bad_rank + 2]) +
                           "): every rank dropped the batch";
        if (rt.local_rc) text += "; this rank: " + rt.local_err;
        return give_up(GK_E_COMM, text);
    }
    // ---- 2. room for the arrivals (the buffer that is NOT being counted: the batch counted two exchanges ago has returned)
    const int rb = (int)(d->nexchanged & 1);
    unsigned long long noroom = 0;
    std::string noroom_text;
    if (nrec_in > d->recv_records[rb] || !d->d_recv[rb]) {
        const u64 want = std::max<u64>(nrec_in + nrec_in / 8, 1024);
        uint8_t *nb = nullptr;
        e = pool_malloc(ctx, &nb, want * (u64)slot + 64);                         // (the pool: a mutex, no stream is waited for)
        if (e == hipSuccess) {
            if (d->d_recv[rb]) { std::lock_guard<std::mutex> lk(d->wmu); d->garbage.push_back(d->d_recv[rb]); }
            d->d_recv[rb] = nb; d->recv_records[rb] = want;
        } else { noroom = 1; noroom_text = hip_text(e, "gk_dist: receive buffer"); }
    }
    unsigned long long *d_flag = d->d_cnt + 6 * 64, *h_flag = d->h_cnt + 6 * 64;
    h_flag[0] = noroom;
    e = hipMemcpyAsync(d_flag, h_flag, 8, hipMemcpyHostToDevice, cs);
    if (e != hipSuccess) return give_up(GK_E_HIP, hip_text(e, "gk_dist: ready flag"));
    grc = xAllReduce(d, d_flag, d_flag + 1, 1, ncclUint64, ncclMax, cs);
    if (grc != ncclSuccess) return give_up(GK_E_COMM, "ready reduction: " + comm_error_text(grc));
    e = hipMemcpyAsync(h_flag + 1, d_flag + 1, 8, hipMemcpyDeviceToHost, cs);
    if (e == hipSuccess) e = hipStreamSynchronize(cs);
    if (e != hipSuccess) return give_up(GK_E_HIP, hip_text(e, "gk_dist: ready flag"));
    if (h_flag[1]) return give_up(GK_E_COMM, "a rank had no room for the records addressed to it: every rank dropped the batch" + (noroom ? "; this rank: " + noroom_text : std::string()));
    // ---- 3. payload
    grc = xGroupStart(d);
    u64 roff = 0;
    for (int p = 0; p < P && grc == ncclSuccess; p++) {
        if (rt.recs[p]) grc = xSend(d, d->d_sendbuf[b] + (u64)p * region * slot, (size_t)rt.recs[p] * slot, ncclUint8, p, cs);
        if (h_out[3 * p] && grc == ncclSuccess) grc = xRecv(d, d->d_recv[rb] + roff * slot, (size_t)h_out[3 * p] * slot, ncclUint8, p, cs);
        roff += h_out[3 * p];
    }
    { const int gend = xGroupEnd(d); if (grc == ncclSuccess) grc = gend; }
    if (grc != ncclSuccess) return give_up(GK_E_COMM, "record exchange: " + comm_error_text(grc));
    e = hipEventRecord(d->exch_done[b], cs);
    if (e != hipSuccess) return give_up(GK_E_HIP, hip_text(e, "gk_dist: exchange event"));
    rt.exchanged = true; rt.rbuf = rb; rt.nrec_in = nrec_in; rt.nkm_in = nkm_in; rt.sent = sent;
    d->nexchanged++;
    *ms += (float)(now_ms() - t1);
    return GK_OK;
}

// The rest of the oldest batch begun by gk_dist_route_begin: exchange counts and records (unless that was done ahead), count
// what arrived.  With THREE batches begun, the exchange of the next one is posted first, so that its records travel while
// this batch is being counted (the rule depends on the number of begun batches only, never on timing: every rank issues
// the same sequence of RCCL operations).
int gk_dist_count_routed(gk_dist *d, gk_map *local, uint64_t *occurrences_sent, uint64_t *occurrences_owned) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    constexpr int NR = gk_dist::NROUTE;
    if (occurrences_sent) *occurrences_sent = 0;
    if (occurrences_owned) *occurrences_owned = 0;
    drain_garbage(d);
    if (!d->npending) return fail(ctx, GK_E_STATE, "gk_dist_count_routed: no route was begun (gk_dist_route_begin)");
    const int b = d->head;
    if (!local || local->ctx != ctx) return fail(ctx, GK_E_INVALID, "gk_dist_count_routed: the local map must live on the handle's context");
    if (local->k != d->route[b].k) return fail(ctx, GK_E_KLEN, "gk_dist_count_routed: the route was begun for another k");
    const double t0 = now_ms();
    float ms_route = 0, ms_exch = 0;
    auto drop_head = [&]() { d->head = (d->head + 1) % NR; d->npending--; };
    // (whatever this batch's own fate, the collective steps below are taken: the peers take them too)
    if (!d->route[b].exchanged && !d->route[b].error) {
        route_settle(d, b, &ms_route);
        (void)dist_exchange(d, b, &ms_exch);           // a failure is in route[b].error
    }
    // With three batches begun, the NEXT batch's exchange runs on the helper thread beside this batch's owner count: its host
    // side alone (RCCL group launches and two round trips for the sizes, 0.4-0.6 ms) would otherwise sit in front of the
    // owner pipeline's launches.  Its route is settled HERE first (a re-route allocates and waits for the context's second
    // stream: the owner thread's business).  The helper is the only thread that touches the communicator until it is waited for.
    bool helping = false;
    float hms = 0;
    if (d->npending >= NR && ctx->hook_dist_ahead != 0) {        // ("dist_exchange_ahead" = 0: the plain order, for A/B and as a fallback)
        const int b1 = (b + 1) % NR;
        if (!d->route[b1].exchanged && !d->route[b1].error) {
            route_settle(d, b1, &ms_route);
            helper_submit(d, [d, b1, &hms]() { (void)dist_exchange(d, b1, &hms); });
            helping = true;
        }
    }
    struct Join { gk_dist *d; bool on; ~Join() { if (on) helper_wait(d); } } join_helper{d, helping};
    const gk_dist::Route rt = d->route[b];
    drop_head();
    if (rt.error) return fail(ctx, rt.error, "gk_dist_count_routed: " + rt.error_text);     // (a batch that could not be exchanged is dropped — on every rank)
    const double t2 = now_ms();
    // ---- the owner counts what it received: the records ARE short reads (stream-ordered behind the receives)
    GK_HIP(ctx, hipStreamWaitEvent(ctx->stream, d->exch_done[b], 0));
    uint64_t occ = 0;
    if (rt.nrec_in) { if (int rc = gk_map_count_superkmers_dev(local, d->d_recv[rt.rbuf], rt.nrec_in, rt.nkm_in, &occ)) return rc; }
    else GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double t3 = now_ms();
    if (helping) { helper_wait(d); join_helper.on = false; }
    const double t4 = now_ms();
    // {waiting for routes, exchanges done in front of the count, owner count, total}; [1] also carries what the helper's
    // exchange took beyond the owner count (0 when it was hidden completely)
    d->last_ms[0] = ms_route; d->last_ms[1] = ms_exch + (float)(t4 - t3); d->last_ms[2] = (float)(t3 - t2); d->last_ms[3] = (float)(t4 - t0);
    d->last_helper_ms = hms;
    if (occurrences_sent) *occurrences_sent = rt.sent;
    if (occurrences_owned) *occurrences_owned = occ;
    return GK_OK;
}

int gk_dist_count_reads_dev(gk_dist *d, gk_map *local, const void *dev_records, uint64_t nreads, int read_len,
                            uint64_t *occurrences_sent, uint64_t *occurrences_owned) {
    if (int rc = dist_check(d)) return rc;
    if (occurrences_sent) *occurrences_sent = 0;
    if (occurrences_owned) *occurrences_owned = 0;
    if (!local || local->ctx != d->ctx) return fail(d->ctx, GK_E_INVALID, "gk_dist_count_reads_dev: the local map must live on the handle's context");
    if (int rc = gk_dist_route_begin(d, local->k, dev_records, nreads, read_len)) return rc;
    return gk_dist_count_routed(d, local, occurrences_sent, occurrences_owned);
}

// FreqFilter.add over this rank's HOST `.bin` stream (ragged or not), every k-mer counted by its owner.
//   1. the whole stream's framing is walked on the host and cut into chunks by gk_map_count_reads' rules (map_cut_chunk)
//      before anything moves;
//   2. ONE all-gather of (status | chunk count): a malformed stream anywhere -> GK_E_FORMAT on every rank, nothing moved, every
//      `local` untouched; else every rank runs max(chunk count) rounds — a rank out of chunks routes empty batches — so that all
//      of them issue the same sequence of transport operations;
//   3. the rounds stream through route_begin / count_routed three batches deep: chunk i+1 (and i+2) is uploaded and routed on
//      the context's second stream while chunk i is exchanged and counted.  A run of equal-length records takes the fixed-stride
//      route, a ragged chunk the offset-framed one (its offset table travels with it).
// A rank that fails a round after streaming began (an exchange dropped by agreement, a HIP error) begins its remaining batches
// empty and carrying the failure: its peers learn it from the status word of the next counts exchange, every rank goes through
// every round without a payload, and every rank returns an error.  `local` then holds an unspecified subset of the counts.
int gk_dist_count_reads(gk_dist *d, gk_map *local, const uint8_t *bin, size_t nbytes, uint64_t nreads, uint64_t *occurrences_sent,
                        uint64_t *occurrences_owned) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    constexpr int NR = gk_dist::NROUTE;
    if (occurrences_sent) *occurrences_sent = 0;
    if (occurrences_owned) *occurrences_owned = 0;
    drain_garbage(d);
    // ---- 1. this rank's verdict on its own stream (a failure here is announced in step 2, never returned before it)
    int my_rc = GK_OK;
    std::vector<BinChunk> chunks;            // (a run of equal-length records carries no offset table)
    if (!local || local->ctx != ctx) my_rc = fail(ctx, GK_E_INVALID, "gk_dist_count_reads: the local map must live on the handle's context");
    else if (!bin && nreads) my_rc = fail(ctx, GK_E_INVALID, "gk_dist_count_reads: null stream");
    else if (d->npending) my_rc = fail(ctx, GK_E_STATE, "gk_dist_count_reads: routes begun with gk_dist_route_begin are still waiting");
    else if (!k_supported(local->k)) my_rc = fail(ctx, GK_E_UNSUPPORTED_K, "k=" + std::to_string(local->k) + " unsupported");
    size_t pos = 0;
    u64 r = 0;
    while (!my_rc && r < nreads) {
        int err = 0;
        BinChunk c = map_cut_chunk(local, bin, nbytes, nreads, pos, r, true, &err);
        if (err) {
            my_rc = bin_truncated(ctx, err, c.r_begin + c.offs.size());
            break;
        }
        if (!c.valid) break;
        pos += c.bytes; r += c.reads;
        if (c.uniform && c.first_len >= 0 && !ctx->hook_host_ragged) { c.offs.clear(); c.offs.shrink_to_fit(); }
        else if (c.offs.empty()) {        // (host_ragged: a run of equal-length records goes the offset-framed way too)
            const u32 rb = 1 + (u32)(c.first_len + 3) / 4;
            c.offs.resize(c.reads + 1);
            for (u64 i = 0; i <= c.reads; i++) c.offs[i] = (u32)(i * rb);
        }
        chunks.push_back(std::move(c));
    }
    const std::string my_err = my_rc ? ctx->err : std::string();
    // ---- 2. every rank's status and chunk count, in one collective
    if (int rc = dist_quiesce(d)) return rc;
    constexpr unsigned long long BAD = 1ull << 63;
    const unsigned long long word = my_rc ? BAD | (unsigned long long)(-(long long)my_rc) : (unsigned long long)chunks.size();
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt + 2 * 64, &word, 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllGather(d, d->d_cnt + 2 * 64, d->d_cnt, 1, ncclUint64, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(d->h_cnt, d->d_cnt, (size_t)d->world * 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    u64 rounds = 0;
    int bad = -1, malformed = -1;
    for (int p = 0; p < d->world; p++) {
        const unsigned long long w = d->h_cnt[p];
        if (!(w & BAD)) { rounds = std::max<u64>(rounds, w); continue; }
        if (bad < 0) bad = p;
        if (malformed < 0 && -(long long)(w & ~BAD) == GK_E_FORMAT) malformed = p;
    }
    if (malformed >= 0)
        return my_rc == GK_E_FORMAT ? fail(ctx, GK_E_FORMAT, my_err)
                                    : fail(ctx, GK_E_FORMAT, "the .bin stream of rank " + std::to_string(malformed) + " is malformed: no rank counted anything");
    if (my_rc) return fail(ctx, my_rc, my_err);
    if (bad >= 0) return fail(ctx, GK_E_COMM, "rank " + std::to_string(bad) + " could not start its count: no rank counted anything");
    // ---- 3. the rounds
    const int k = local->k;
    int failed = GK_OK;
    std::string failed_err;
    auto grow = [&](void **buf, u64 *have, u64 want) -> int {
        if (*have >= want && *buf) return GK_OK;
        if (*buf) GK_HIP(ctx, pool_free(ctx, *buf));
        *buf = nullptr; *have = 0;
        GK_HIP(ctx, pool_malloc(ctx, buf, want));
        *have = want;
        return GK_OK;
    };
    auto begin = [&](u64 i) -> int {
        const int s = (int)(i % NR);      // (batch i - 3 used this area: it was counted, its route has finished)
        if (failed || i >= chunks.size()) return route_begin_impl(d, k, nullptr, nullptr, 0, 0, 0, failed, failed_err);
        const BinChunk &c = chunks[i];
        const bool ragged = !c.offs.empty();
        int rc = grow((void **)&d->d_stage[s], &d->stage_bytes[s], c.bytes + 64);
        if (!rc && ragged) rc = grow((void **)&d->d_stage_offs[s], &d->stage_offs_bytes[s], c.offs.size() * sizeof(u32));
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(d->d_stage[s], bin + c.begin, c.bytes, hipMemcpyHostToDevice, ctx->copy_stream);
        if (!rc && ragged && e == hipSuccess) e = hipMemcpyAsync(d->d_stage_offs[s], c.offs.data(), c.offs.size() * sizeof(u32), hipMemcpyHostToDevice, ctx->copy_stream);
        if (!rc && e != hipSuccess) rc = hip_fail(ctx, e, "gk_dist_count_reads: staging upload");
        if (rc) return route_begin_impl(d, k, nullptr, nullptr, 0, 0, 0, rc, ctx->err);
        if (!ragged) return route_begin_impl(d, k, d->d_stage[s], nullptr, c.reads, c.first_len, 0);
        return route_begin_impl(d, k, d->d_stage[s], d->d_stage_offs[s], c.reads, 255, c.occ);
    };
    u64 begun = 0, sent = 0, owned = 0;
    for (; begun < std::min<u64>(rounds, NR); begun++) { if (int rc = begin(begun)) return rc; }
    for (u64 i = 0; i < rounds; i++) {
        uint64_t s1 = 0, o1 = 0;
        const int rc = gk_dist_count_routed(d, local, &s1, &o1);
        if (rc && !failed) { failed = rc; failed_err = ctx->err; }
        sent += s1; owned += o1;
        if (begun < rounds) { if (int rc2 = begin(begun++)) return rc2; }
    }
    if (failed) return fail(ctx, failed, failed_err + " (gk_dist_count_reads: the local map holds an unspecified part of the counts)");
    if (occurrences_sent) *occurrences_sent = sent;
    if (occurrences_owned) *occurrences_owned = owned;
    return GK_OK;
}

int gk_dist_last_ms(gk_dist *d, float *ms4) {
    if (!d || !ms4) return fail(nullptr, GK_E_INVALID, "gk_dist_last_ms: null argument");
    for (int i = 0; i < 4; i++) ms4[i] = d->last_ms[i];
    return GK_OK;
}

// The whole k-mer set on every rank.  CHUNKED: every rank exports the live (key, count) of 2^25 of its slots at a time, the
// chunk's sizes go round (one word per rank — ~0 = "I failed": then EVERY rank gives up together, nobody is left waiting in a
// receive), the parts are exchanged and inserted, and the staging is reused: 0.67 GB to send and P x that to receive whatever
// the table's size (until round 3 the whole set was staged at 20 B per key — 62 GB at C5 — beside the table being built).
// The new table is sized the way the graph phase wants it (graph_table_load).
//
// CLASSIFIED form (gk_dist_gather_classified_map; SURVEY.md 8(e) "beyond counting", Graph.scala:320-329 through
// PartitionedDNAMap.mapReduce :55-58): before a chunk's keys travel, their owner classifies them — neighbours it owns itself
// are looked up in its own partition, the others are asked of THEIR owners (one all-to-all of canonical keys, one of answer
// bytes: k_dc_* in gk_graph.hip) — and the 8-bit (incoming, outcoming) mask travels with each key into the replica's annotation
// word.  gk_graph_build on the gathered table then derives terminal / secondary from the masks in one streaming pass instead of
// eight random lookups per key on EVERY rank: the classify's work is divided by the number of ranks.  A partition that holds
// verbatim non-canonical keys (dirty) on any rank turns the form off for everybody (plain gather).
static int dist_gather(gk_dist *d, gk_map *local, gk_map **full, bool classify) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (!local || !full || local->ctx != ctx) return fail(ctx, GK_E_INVALID, "gk_dist_gather_map: bad argument");
    *full = nullptr;
    if (int rc = dist_quiesce(d)) return rc;
    if (int rc = map_materialize(local)) return rc;
    const int P = d->world, W = local->W;
    // (the masks live in the annotation word: a partition that still counts in 12-byte slots is rebuilt first — a local step,
    //  whose failure is announced with the first chunk's word like any other)
    int pre_rc = GK_OK;
    std::string pre_err;
    if (classify) { pre_rc = map_to_graph_layout(local); if (pre_rc) pre_err = ctx->err; }
    constexpr u64 CHS = 1ull << 25;
    // live keys of every rank, and the number of chunks of the rank with the largest table
    // (one maximum over all ranks carries both: the chunk count of SOME rank in its low 40 bits and, above them, "some partition holds verbatim
    //  non-canonical keys" — the replica holds every partition's keys, so it is dirty if ANY of them is; the chunk count itself is a second maximum)
    unsigned long long mine[2] = {local->size, ((local->capacity + CHS - 1) / CHS) | (local->dirty ? 1ull << 40 : 0ull)};
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt + 2 * 64, mine, 16, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllGather(d, d->d_cnt + 2 * 64, d->d_cnt, 1, ncclUint64, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt + 2 * 64 + 1, d->d_cnt + 64, 1, ncclUint64, ncclMax, ctx->stream));
    unsigned long long chunks_only = (local->capacity + CHS - 1) / CHS;
    GK_HIP(ctx, hipMemcpyAsync(d->d_cnt + 2 * 64 + 2, &chunks_only, 8, hipMemcpyHostToDevice, ctx->stream));
    GK_NCCL(ctx, xAllReduce(d, d->d_cnt + 2 * 64 + 2, d->d_cnt + 65, 1, ncclUint64, ncclMax, ctx->stream));
    GK_HIP(ctx, hipMemcpyAsync(d->h_cnt, d->d_cnt, (64 + 2) * 8, hipMemcpyDeviceToHost, ctx->stream));
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    u64 total = 0;
    const u64 nchunks = d->h_cnt[65];
    const bool any_dirty = (d->h_cnt[64] >> 40) != 0;
    classify = classify && !any_dirty;                 // (every rank takes the same decision: the word is a maximum over all of them)
    for (int p = 0; p < P; p++) total += d->h_cnt[p];
    if (d->h_cnt[d->rank] != mine[0]) return fail(ctx, GK_E_COMM, "gk_dist_gather_map: size exchange is inconsistent");
    gk_map *m = nullptr;
    u64 *d_send_k = nullptr, *d_recv_k = nullptr;
    i32 *d_send_c = nullptr, *d_recv_c = nullptr;
    unsigned long long *d_cur = nullptr;
    uint8_t *d_send_m = nullptr, *d_recv_m = nullptr;                  // classified form: the masks beside the keys
    unsigned long long *d_dc = nullptr;                                // [5][64]: counts to send | counts received | remote counts | region offsets | cursors
    u64 *d_qk = nullptr, *d_qref = nullptr, *d_rk = nullptr;           // queries out (keys, who asked), queries in
    uint8_t *d_ans_in = nullptr, *d_ans_out = nullptr;                 // answers to my queries, my answers to the others'
    u64 q_out_cap = 0, q_in_cap = 0;
    // every rank's chunk holds at most CHS keys: the receive staging is allocated ONCE, before anything is agreed — no allocation,
    // hence no local failure, between a chunk's size exchange and its sends and receives
    const u64 recv_cap = std::max<u64>(std::min<u64>(total, (u64)P * CHS), 1);
    DevScratch tmp(ctx);
    auto done = [&](int code) {          // a failed gather leaves no table behind
        if (code != GK_OK && m) { gk_map_destroy(m); m = nullptr; }
        return code;
    };
    // a local failure must not leave the peers in a receive: it is announced in the chunk's size word and everybody stops
    int my_rc = pre_rc;
    std::string my_err = pre_err;
    if (!my_rc) { my_rc = map_create_for_graph(ctx, local->k, total, &m); if (my_rc) my_err = ctx->err; }
    const u64 send_cap = std::min<u64>(CHS, local->capacity);
    if (!my_rc) {
        hipError_t e = tmp.get(&d_send_k, std::max<u64>(send_cap, 1) * W);
        if (e == hipSuccess) e = tmp.get(&d_send_c, send_cap);
        if (e == hipSuccess) e = tmp.get(&d_cur, 1);
        if (e == hipSuccess) e = tmp.get(&d_recv_k, recv_cap * W);
        if (e == hipSuccess) e = tmp.get(&d_recv_c, recv_cap);
        if (e == hipSuccess && classify) e = tmp.get(&d_send_m, send_cap);
        if (e == hipSuccess && classify) e = tmp.get(&d_recv_m, recv_cap);
        if (e == hipSuccess && classify) e = tmp.get(&d_dc, 5 * 64);
        if (e != hipSuccess) { my_rc = hip_fail(ctx, e, "gk_dist_gather_map: staging"); my_err = ctx->err; }
    }
#define HIPD(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return done(hip_fail(ctx, e__, #call)); } while (0)
    for (u64 c = 0; c < nchunks; c++) {
        uint64_t n_mine = 0;
        if (classify && P > 1) {
            // ---- the owners' classify of this chunk's slots: count -> sizes round -> queries -> answers -> masks --------------
            unsigned long long h_send[64] = {0}, h_recv[64] = {0}, h_off[64] = {0};
            if (!my_rc) {
                my_rc = dclass_count(local, d->rank, P, c * CHS, (c + 1) * CHS, d_dc + 2 * 64);
                if (!my_rc) {
                    const hipError_t e = read_back(ctx, h_send, d_dc + 2 * 64, P);
                    if (e != hipSuccess) my_rc = hip_fail(ctx, e, "gk_dist_gather_map: classify counts");
                }
                if (my_rc) my_err = ctx->err;
            }
            // what I will ask of every peer (or ~0: I failed, nobody goes on), against what every peer will ask of me
            unsigned long long words[64];
            for (int p = 0; p < P; p++) words[p] = my_rc ? ~0ull : h_send[p];
            unsigned long long *d_w_out = d->d_cnt + 4 * 64, *d_w_in = d->d_cnt + 5 * 64;      // (the handle's own words: they exist whatever failed above)
            HIPD(hipMemcpyAsync(d_w_out, words, P * 8, hipMemcpyHostToDevice, ctx->stream));
            {
                int grc = xGroupStart(d);
                for (int p = 0; p < P; p++) {
                    if (p == d->rank) continue;
                    if (grc == ncclSuccess) grc = xSend(d, d_w_out + p, 1, ncclUint64, p, ctx->stream);
                    if (grc == ncclSuccess) grc = xRecv(d, d_w_in + p, 1, ncclUint64, p, ctx->stream);
                }
                const int gend = xGroupEnd(d);
                if (grc == ncclSuccess) grc = gend;
                if (grc != ncclSuccess) return done(fail(ctx, GK_E_COMM, std::string("gk_dist_gather_map: ") + comm_error_text(grc)));
            }
            HIPD(hipMemcpyAsync(h_recv, d_w_in, P * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPD(hipStreamSynchronize(ctx->stream));
            h_recv[d->rank] = 0;
            bool peer_failed = false;
            for (int p = 0; p < P; p++) if (p != d->rank && h_recv[p] == ~0ull) peer_failed = true;
            // (a rank that failed told EVERY peer so: all of them are here, none has posted a payload receive)
            if (my_rc || peer_failed) return done(my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, "gk_dist_gather_map: another rank failed; the gather was abandoned on every rank"));
            u64 nq_out = 0, nq_in = 0;
            unsigned long long r_off[64] = {0};
            for (int p = 0; p < P; p++) { h_off[p] = nq_out; nq_out += h_send[p]; r_off[p] = nq_in; nq_in += h_recv[p]; }
            // room for both directions; a failure here is agreed on before anybody posts a receive
            if (ctx->hook_dist_fail_classify) {       // test hook: this rank alone cannot stage its queries
                ctx->hook_dist_fail_classify = 0;
                my_rc = fail(ctx, GK_E_CAPACITY, "injected failure (test_dist_fail_classify)");
                my_err = ctx->err;
            }
            if (!my_rc && nq_out > q_out_cap) {
                tmp.release(d_qk); tmp.release(d_qref); tmp.release(d_ans_in);
                q_out_cap = 0;
                hipError_t e = tmp.get(&d_qk, nq_out * W);
                if (e == hipSuccess) e = tmp.get(&d_qref, nq_out);
                if (e == hipSuccess) e = tmp.get(&d_ans_in, nq_out);
                if (e != hipSuccess) { my_rc = hip_fail(ctx, e, "gk_dist_gather_map: query staging"); my_err = ctx->err; } else q_out_cap = nq_out;
            }
            if (!my_rc && nq_in > q_in_cap) {
                tmp.release(d_rk); tmp.release(d_ans_out);
                q_in_cap = 0;
                hipError_t e = tmp.get(&d_rk, nq_in * W);
                if (e == hipSuccess) e = tmp.get(&d_ans_out, nq_in);
                if (e != hipSuccess) { my_rc = hip_fail(ctx, e, "gk_dist_gather_map: query staging"); my_err = ctx->err; } else q_in_cap = nq_in;
            }
            {
                unsigned long long word = my_rc ? 1ull : 0ull;
                HIPD(hipMemcpyAsync(d->d_cnt + 2 * 64, &word, 8, hipMemcpyHostToDevice, ctx->stream));
                const int g = xAllReduce(d, d->d_cnt + 2 * 64, d->d_cnt + 2 * 64, 1, ncclUint64, ncclMax, ctx->stream);
                if (g != ncclSuccess) return done(fail(ctx, GK_E_COMM, "gk_dist_gather_map: " + comm_error_text(g)));
                HIPD(hipMemcpyAsync(&word, d->d_cnt + 2 * 64, 8, hipMemcpyDeviceToHost, ctx->stream));
                HIPD(hipStreamSynchronize(ctx->stream));
                if (my_rc) return done(fail(ctx, my_rc, my_err));
                if (word) return done(fail(ctx, GK_E_COMM, "gk_dist_gather_map: another rank failed; the gather was abandoned on every rank"));
            }
            HIPD(hipMemcpyAsync(d_dc + 3 * 64, h_off, P * 8, hipMemcpyHostToDevice, ctx->stream));
            if (nq_out) { if (int rc = dclass_fill(local, d->rank, P, c * CHS, (c + 1) * CHS, d_dc + 3 * 64, d_dc + 4 * 64, d_qk, d_qref)) return done(rc); }
            {
                int grc = xGroupStart(d);
                for (int p = 0; p < P; p++) {
                    if (p == d->rank) continue;
                    if (h_send[p] && grc == ncclSuccess) grc = xSend(d, d_qk + h_off[p] * W, (size_t)h_send[p] * W, ncclUint64, p, ctx->stream);
                    if (h_recv[p] && grc == ncclSuccess) grc = xRecv(d, d_rk + r_off[p] * W, (size_t)h_recv[p] * W, ncclUint64, p, ctx->stream);
                }
                const int gend = xGroupEnd(d);
                if (grc == ncclSuccess) grc = gend;
                if (grc != ncclSuccess) return done(fail(ctx, GK_E_COMM, std::string("gk_dist_gather_map: ") + comm_error_text(grc)));
            }
            if (int rc = dclass_answer(local, d_rk, nq_in, d_ans_out)) return done(rc);
            {
                int grc = xGroupStart(d);
                for (int p = 0; p < P; p++) {
                    if (p == d->rank) continue;
                    if (h_recv[p] && grc == ncclSuccess) grc = xSend(d, d_ans_out + r_off[p], (size_t)h_recv[p], ncclUint8, p, ctx->stream);
                    if (h_send[p] && grc == ncclSuccess) grc = xRecv(d, d_ans_in + h_off[p], (size_t)h_send[p], ncclUint8, p, ctx->stream);
                }
                const int gend = xGroupEnd(d);
                if (grc == ncclSuccess) grc = gend;
                if (grc != ncclSuccess) return done(fail(ctx, GK_E_COMM, std::string("gk_dist_gather_map: ") + comm_error_text(grc)));
            }
            if (int rc = dclass_apply(local, d_qref, d_ans_in, nq_out)) return done(rc);
            d->classify_queries += nq_out;
        } else if (classify && !my_rc) {
            my_rc = dclass_count(local, d->rank, P, c * CHS, (c + 1) * CHS, d_dc + 2 * 64);       // one rank: every neighbour is local
            if (my_rc) my_err = ctx->err;
        }
        if (!my_rc && c * CHS < local->capacity) {
            my_rc = map_export_range_dev(local, c * CHS, (c + 1) * CHS, d_send_k, d_send_c, d_cur, &n_mine, classify ? d_send_m : nullptr);
            if (my_rc) my_err = ctx->err;
        }
        unsigned long long word = my_rc ? ~0ull : n_mine;
        HIPD(hipMemcpyAsync(d->d_cnt + 2 * 64, &word, 8, hipMemcpyHostToDevice, ctx->stream));
        { const int g = xAllGather(d, d->d_cnt + 2 * 64, d->d_cnt, 1, ncclUint64, ctx->stream); if (g != ncclSuccess) return done(fail(ctx, GK_E_COMM, "gk_dist_gather_map: " + comm_error_text(g))); }
        HIPD(hipMemcpyAsync(d->h_cnt, d->d_cnt, P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPD(hipStreamSynchronize(ctx->stream));
        u64 tot_c = 0, my_off = 0;
        bool peer_failed = false;
        for (int p = 0; p < P; p++) {
            if (d->h_cnt[p] == ~0ull) { peer_failed = true; continue; }
            if (p == d->rank) my_off = tot_c;
            tot_c += d->h_cnt[p];
        }
        if (peer_failed) return done(my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, "gk_dist_gather_map: another rank failed; the gather was abandoned on every rank"));
        if (tot_c == 0) continue;
        if (tot_c > recv_cap) return done(fail(ctx, GK_E_STATE, "gk_dist_gather_map: a chunk holds more keys than its slots"));   // (cannot happen: <= CHS per rank)
        if (n_mine) {
            HIPD(hipMemcpyAsync(d_recv_k + my_off * W, d_send_k, n_mine * 8 * W, hipMemcpyDeviceToDevice, ctx->stream));
            HIPD(hipMemcpyAsync(d_recv_c + my_off, d_send_c, n_mine * 4, hipMemcpyDeviceToDevice, ctx->stream));
            if (classify) HIPD(hipMemcpyAsync(d_recv_m + my_off, d_send_m, n_mine, hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (P > 1) {
            int grc = xGroupStart(d);
            u64 off = 0;
            for (int p = 0; p < P; p++) {
                const u64 n = d->h_cnt[p];
                if (p != d->rank) {
                    if (n_mine && grc == ncclSuccess) grc = xSend(d, d_send_k, (size_t)n_mine * W, ncclUint64, p, ctx->stream);
                    if (n_mine && grc == ncclSuccess) grc = xSend(d, d_send_c, (size_t)n_mine * 4, ncclUint8, p, ctx->stream);
                    if (classify && n_mine && grc == ncclSuccess) grc = xSend(d, d_send_m, (size_t)n_mine, ncclUint8, p, ctx->stream);
                    if (n && grc == ncclSuccess) grc = xRecv(d, d_recv_k + off * W, (size_t)n * W, ncclUint64, p, ctx->stream);
                    if (n && grc == ncclSuccess) grc = xRecv(d, d_recv_c + off, (size_t)n * 4, ncclUint8, p, ctx->stream);
                    if (classify && n && grc == ncclSuccess) grc = xRecv(d, d_recv_m + off, (size_t)n, ncclUint8, p, ctx->stream);
                }
                off += n;
            }
            const int gend = xGroupEnd(d);                 // (the group is always closed, whatever was posted)
            if (grc == ncclSuccess) grc = gend;
            if (grc != ncclSuccess) return done(fail(ctx, GK_E_COMM, std::string("gk_dist_gather_map: ") + comm_error_text(grc)));
        }
        // one table holding every partition's keys (each key has exactly one owner: nothing merges)
        // (each key has exactly one owner and the table was created for all of them: one CAS per key, count and mask beside it)
        my_rc = map_add_unique_keys_dev(m, d_recv_k, d_recv_c, classify ? d_recv_m : nullptr, tot_c);
        if (my_rc) my_err = ctx->err;
    }
    // the last chunk's insert may have failed after its word went out: agree on the outcome once more
    {
        unsigned long long word = my_rc ? ~0ull : 0ull;
        HIPD(hipMemcpyAsync(d->d_cnt + 2 * 64, &word, 8, hipMemcpyHostToDevice, ctx->stream));
        const int g = xAllReduce(d, d->d_cnt + 2 * 64, d->d_cnt + 2 * 64, 1, ncclUint64, ncclMax, ctx->stream);
        if (g != ncclSuccess) return done(fail(ctx, GK_E_COMM, "gk_dist_gather_map: " + comm_error_text(g)));
        HIPD(hipMemcpyAsync(&word, d->d_cnt + 2 * 64, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPD(hipStreamSynchronize(ctx->stream));
        if (my_rc) return done(fail(ctx, my_rc, my_err));
        if (word) return done(fail(ctx, GK_E_COMM, "gk_dist_gather_map: another rank failed; the gathered table is void on every rank"));
    }
    if (int rc = map_sync_counters(m)) return done(rc);
    if (m->size != total) return done(fail(ctx, GK_E_STATE, "gk_dist_gather_map: gathered " + std::to_string(m->size) + " keys, the partitions hold " + std::to_string(total)));
    m->dirty = any_dirty;
    m->masks_valid = classify;           // (set after the last map_sync_counters of this table: any later change of its contents clears it)
    *full = m;
    return done(GK_OK);
}
#undef HIPD
int gk_dist_gather_map(gk_dist *d, gk_map *local, gk_map **full) { return dist_gather(d, local, full, false); }
int gk_dist_gather_classified_map(gk_dist *d, gk_map *local, gk_map **full) { return dist_gather(d, local, full, true); }
int gk_dist_classify_queries(gk_dist *d, uint64_t *n) {
    if (!d || !n) return fail(nullptr, GK_E_INVALID, "gk_dist_classify_queries: null argument");
    *n = d->classify_queries;
    return GK_OK;
}
#define HIPD(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(ctx, e__, #call); } while (0)
#undef HIPD

}  // extern "C"

// ---- the paired-end support over the ranks (gk_dist_reduce_support) -----------------------------------------------------------
// Reference: every storage node's WalkingActor counts the (inEdge, outEdge) pairs of the walks it did and the driver sums them
// into one pathsMap (S/scripts/GraphSimplifier.scala:172-186, 209-248).  Here the sum is sharded: a pair's OWNER (a hash of
// the key, not the slot hash) merges every rank's count of it, and the owners' shards — disjoint — then go to every rank,
// which builds its table from their concatenation.  Steps, every rank taking the same ones whatever happens to it locally:
//   1. the replica's canonical edge numbering (graph_edge_canon); all-gather (status | distinct pairs) and the replica's CONTENT
//      fingerprint: any failure or a content mismatch -> everybody stops
//   2. bucket by owner, the keys translated to the canonical numbering; all-to-all of region sizes (~0 = failed)
//   3. room for the arrivals and the owner's shard table; max-reduction of "no room"
//   4. records (12 bytes) to their owners; the owner merge (overflow-checked); the shard compacted back into the arrival buffer
//   5. all-gather of shard sizes (~0 failed, ~0 - 1 a count passed 2^32-1): -> everybody stops
//   6. room for every shard and the new table; max-reduction of "no room"
//   7. every shard to every rank; the keys back to this replica's ids; the rebuild; one sum-reduction of {bad pairs, walked, failures}: the table is swapped in only
//      where, and when, every rank has its own
// Every allocation is made in front of the agreement that covers it, and nothing is allocated between an agreement and the
// payload it guards.
namespace {
struct SupHandle {        // a temporary support table on the handle's context
    gk_support *s = nullptr;
    ~SupHandle() { if (s) gk_support_destroy(s); }
};
}  // namespace

extern "C" int gk_dist_reduce_support(gk_dist *d, gk_graph *g, gk_support *sup) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (int rc = dist_quiesce(d)) return rc;
    const int P = d->world, me = d->rank;
    const char *who = "gk_dist_reduce_support: ";
    // A local failure is not returned at once: the peers are about to wait for this rank's words.  It is announced, and every
    // rank returns from the same step.
    int my_rc = GK_OK;
    std::string my_err;
    auto local = [&](int rc) { if (rc != GK_OK && my_rc == GK_OK) { my_rc = rc; my_err = ctx->err; } };
    auto comm_fail = [&](int grc) { return fail(ctx, GK_E_COMM, who + comm_error_text(grc)); };
    auto give_up = [&](const std::string &why) { return my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, who + why); };
#define HIPR(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(ctx, e__, #call); } while (0)
#define XPR(call) do { const int g__ = (call); if (g__ != XP_SUCCESS) return comm_fail(g__); } while (0)
    unsigned long long *d_w = d->d_cnt;                           // the handle's own words: they exist whatever fails here
    // grouped exchange of one word with every rank (itself included): out[p] -> rank p, in[p] <- rank p
    auto words_all_to_all = [&](const unsigned long long *out, unsigned long long *in) -> int {
        HIPR(hipMemcpyAsync(d_w + 4 * 64, out, P * 8, hipMemcpyHostToDevice, ctx->stream));
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            grc = xSend(d, d_w + 4 * 64 + p, 1, XP_UINT64, p, ctx->stream);
            if (grc == XP_SUCCESS) grc = xRecv(d, d_w + 5 * 64 + p, 1, XP_UINT64, p, ctx->stream);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        if (grc != XP_SUCCESS) return comm_fail(grc);
        HIPR(hipMemcpyAsync(in, d_w + 5 * 64, P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        return GK_OK;
    };
    // one word of every rank, in rank order
    auto word_all_gather = [&](unsigned long long mine, unsigned long long *all) -> int {
        HIPR(hipMemcpyAsync(d_w + 2 * 64, &mine, 8, hipMemcpyHostToDevice, ctx->stream));
        XPR(xAllGather(d, d_w + 2 * 64, d_w, 1, XP_UINT64, ctx->stream));
        HIPR(hipMemcpyAsync(all, d_w, P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        return GK_OK;
    };
    // max over the ranks of "this rank cannot go on"
    auto any_rank = [&](bool mine, bool *any) -> int {
        unsigned long long w = mine ? 1ull : 0ull;
        HIPR(hipMemcpyAsync(d_w + 2 * 64, &w, 8, hipMemcpyHostToDevice, ctx->stream));
        XPR(xAllReduce(d, d_w + 2 * 64, d_w + 2 * 64 + 1, 1, XP_UINT64, XP_MAX, ctx->stream));
        HIPR(hipMemcpyAsync(&w, d_w + 2 * 64 + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        *any = w != 0;
        return GK_OK;
    };
    // ---- 1. status and the replicas' content.  The replicas need not number their edges alike (a build numbers in table slot
    //      order, with atomic output cursors): the pairs travel in the CANONICAL numbering of graph_edge_canon — live edges
    //      ordered by (start k-mer, first base) — which is the same on every replica that holds the same edges.
    DevScratch buf(ctx);
    u64 fp = 0, nlive = 0;
    u32 *d_canon = nullptr, *d_inv = nullptr;
    unsigned long long ctr[4] = {0, 0, 0, 0};
    if (!g || !sup) local(fail(ctx, GK_E_INVALID, std::string(who) + "null graph or support"));
    else if (check_graph(g) != GK_OK) local(GK_E_INVALID);
    else if (g->ctx != ctx || sup->ctx != ctx) local(fail(ctx, GK_E_INVALID, std::string(who) + "the graph and the support must live on the handle's context"));
    if (!my_rc) {
        local(graph_edge_canon(g, buf, &d_canon, &d_inv, &nlive, &fp));
    }
    if (!my_rc) local(support_counters(sup, ctr));
    std::vector<unsigned long long> st(P), fps(P);
    if (int rc = word_all_gather(my_rc ? ~0ull : ctr[0], st.data())) return rc;
    if (int rc = word_all_gather(fp, fps.data())) return rc;
    for (int p = 0; p < P; p++)
        if (st[p] == ~0ull) return give_up("rank " + std::to_string(p) + " could not take part; every rank gave up, nothing was changed");
    for (int p = 0; p < P; p++)
        if (fps[p] != fps[me])
            return fail(ctx, GK_E_STATE, std::string(who) + "the graph replicas differ (content fingerprint of rank " + std::to_string(p) + ": " + std::to_string(fps[p]) +
                                             ", of this rank: " + std::to_string(fps[me]) + "): they do not hold the same edges, nothing was added up");
    if (P == 1) return GK_OK;
    // ---- 2. this rank's pairs by owner, in the canonical numbering; region sizes to every owner
    SupHandle shard, fresh;
    u64 *d_sk = nullptr, *d_rk = nullptr, *d_ak = nullptr;       // by owner (send) | arrivals, then this rank's shard | every shard
    u32 *d_sc = nullptr, *d_rc = nullptr, *d_ac = nullptr;
    std::vector<u64> region(P + 1, 0);
    const u64 mine = ctr[0];
    if (buf.get(&d_sk, mine) != hipSuccess || buf.get(&d_sc, mine) != hipSuccess) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(mine) + " pairs"));
    if (!my_rc) local(support_bucket(sup, P, d_sk, d_sc, mine, region.data(), d_canon, g->v.n_edges));
    std::vector<unsigned long long> out(P), in(P);
    for (int p = 0; p < P; p++) out[p] = my_rc ? ~0ull : region[p + 1] - region[p];
    if (int rc = words_all_to_all(out.data(), in.data())) return rc;
    u64 nin = 0;
    std::vector<u64> roff(P + 1, 0);
    for (int p = 0; p < P; p++) {
        if (in[p] == ~0ull) return give_up("rank " + std::to_string(p) + " could not bucket its pairs; every rank gave up, nothing was changed");
        roff[p] = nin;
        nin += in[p];
    }
    if (my_rc) return give_up("");                                // (unreachable: this rank sent ~0 to itself)
    // ---- 3. room for the arrivals and the shard table
    if (buf.get(&d_rk, nin) != hipSuccess || buf.get(&d_rc, nin) != hipSuccess) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(nin) + " arriving pairs"));
    if (!my_rc) local(gk_support_create(ctx, &shard.s));
    if (!my_rc) local(support_reserve(shard.s, nin));
    {
        bool any = false;
        if (int rc = any_rank(my_rc != GK_OK, &any)) return rc;
        if (any) return give_up("a rank had no room for the pairs it owns; every rank gave up, nothing was changed");
    }
    // ---- 4. the records to their owners, the owner merge
    {
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            const u64 n = region[p + 1] - region[p];
            if (n) grc = xSend(d, d_sk + region[p], (size_t)n, XP_UINT64, p, ctx->stream);
            if (n && grc == XP_SUCCESS) grc = xSend(d, d_sc + region[p], (size_t)n * 4, XP_UINT8, p, ctx->stream);
            if (in[p] && grc == XP_SUCCESS) grc = xRecv(d, d_rk + roff[p], (size_t)in[p], XP_UINT64, p, ctx->stream);
            if (in[p] && grc == XP_SUCCESS) grc = xRecv(d, d_rc + roff[p], (size_t)in[p] * 4, XP_UINT8, p, ctx->stream);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        if (grc != XP_SUCCESS) return comm_fail(grc);
    }
    bool wrapped = false;
    local(support_insert(shard.s, d_rk, d_rc, nin, true, &wrapped));
    if (ctx->hook_dist_fail_reduce) {         // test hook: this rank alone fails its owner merge, after the payload has moved
        ctx->hook_dist_fail_reduce = 0;
        local(fail(ctx, GK_E_STATE, std::string(who) + "injected failure (test_dist_fail_reduce)"));
    }
    std::vector<u64> sreg(2, 0);
    if (!my_rc && !wrapped) local(support_bucket(shard.s, 1, d_rk, d_rc, nin, sreg.data()));       // the shard, compacted where the arrivals were
    // ---- 5. shard sizes: the owners' verdicts
    std::vector<unsigned long long> ssz(P);
    if (int rc = word_all_gather(my_rc ? ~0ull : wrapped ? ~0ull - 1 : sreg[1], ssz.data())) return rc;
    bool over = false;
    for (int p = 0; p < P; p++) {
        if (ssz[p] == ~0ull) return give_up("rank " + std::to_string(p) + " failed its owner merge; every rank gave up, nothing was changed");
        over |= ssz[p] == ~0ull - 1;
    }
    if (over) return fail(ctx, GK_E_CAPACITY, std::string(who) + "a pair's count summed over the ranks would pass 2^32-1; nothing was changed");
    u64 total = 0;
    std::vector<u64> soff(P + 1, 0);
    for (int p = 0; p < P; p++) { soff[p] = total; total += ssz[p]; }
    // ---- 6. room for every shard and the new table
    if (buf.get(&d_ak, total) != hipSuccess || buf.get(&d_ac, total) != hipSuccess) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(total) + " pairs"));
    if (!my_rc) local(gk_support_create(ctx, &fresh.s));
    if (!my_rc) local(support_reserve(fresh.s, total));
    {
        bool any = false;
        if (int rc = any_rank(my_rc != GK_OK, &any)) return rc;
        if (any) return give_up("a rank had no room for the summed support; every rank gave up, nothing was changed");
    }
    // ---- 7. every shard to every rank, the rebuild, the last agreement
    {
        const u64 n = ssz[me];
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            if (n) grc = xSend(d, d_rk, (size_t)n, XP_UINT64, p, ctx->stream);
            if (n && grc == XP_SUCCESS) grc = xSend(d, d_rc, (size_t)n * 4, XP_UINT8, p, ctx->stream);
            if (ssz[p] && grc == XP_SUCCESS) grc = xRecv(d, d_ak + soff[p], (size_t)ssz[p], XP_UINT64, p, ctx->stream);
            if (ssz[p] && grc == XP_SUCCESS) grc = xRecv(d, d_ac + soff[p], (size_t)ssz[p] * 4, XP_UINT8, p, ctx->stream);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        if (grc != XP_SUCCESS) return comm_fail(grc);
    }
    local(support_keys_uncanon(ctx, d_ak, total, d_inv, nlive));          // back to this replica's own edge ids
    if (!my_rc) local(support_insert(fresh.s, d_ak, d_ac, total, false, nullptr));      // (the shards are disjoint: every record is a new key)
    unsigned long long got[4] = {0, 0, 0, 0};
    if (!my_rc) local(support_counters(fresh.s, got));
    if (!my_rc && got[0] != total) local(fail(ctx, GK_E_STATE, std::string(who) + "rebuilt " + std::to_string(got[0]) + " pairs from " + std::to_string(total) + " shard records"));
    unsigned long long sums[3] = {ctr[1], ctr[2], my_rc ? 1ull : 0ull};
    HIPR(hipMemcpyAsync(d_w + 2 * 64, sums, 24, hipMemcpyHostToDevice, ctx->stream));
    XPR(xAllReduce(d, d_w + 2 * 64, d_w + 3 * 64, 3, XP_UINT64, XP_SUM, ctx->stream));
    HIPR(hipMemcpyAsync(sums, d_w + 3 * 64, 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPR(hipStreamSynchronize(ctx->stream));
    if (sums[2]) return give_up("a rank could not rebuild the summed support; every rank gave up, nothing was changed");
    return support_adopt(sup, fresh.s, sums[0], sums[1]);
#undef XPR
#undef HIPR
}

// ---- link and span tables over the ranks (gk_dist_reduce_links, gk_dist_reduce_spans) --------------------------------------------
// gk_dist_reduce_support's seven steps, written once for a table type T whose records travel as the three planes of gk_links.h
// (key u64, count u32, extra u64: 20 bytes a record).  Two things differ from the support's reduce.  These tables are taken on the
// FINAL graph, whose node splits and edge copies share k-mers, so the canonical numbering is the one by path content
// (graph_edge_pathkeys) and a record that names a dead edge, or one of two edges with the same path, is GK_E_STATE on its rank
// (hence everywhere).  And a record's owner is a hash of its key plane alone: the at most four out-edges behind a span's (e, m)
// meet at one owner, whose insert is the table's own.  world == 1: the checks of steps 1 and 2 and nothing else.
namespace {
template <class T> struct RecHandle {       // a temporary table on the handle's context
    T *t = nullptr;
    ~RecHandle() { if (t) rec_free(t); }
};

// The one-word agreements of a collective, over the handle's own device words (d->d_cnt: they exist whatever fails in the
// caller): out[p] -> rank p and in[p] <- rank p; one word of every rank in rank order; "some rank cannot go on".  (Compiled once:
// the exchange below is a template, these are not.  gk_dist_reduce_support keeps its own copies as lambdas.)
struct RankWords {
    gk_dist *d;
    const char *who;
#define HIPR(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return hip_fail(ctx, e__, #call); } while (0)
#define XPR(call) do { const int g__ = (call); if (g__ != XP_SUCCESS) return fail(ctx, GK_E_COMM, who + comm_error_text(g__)); } while (0)
    int all_to_all(const unsigned long long *out, unsigned long long *in) const {
        gk_ctx *ctx = d->ctx;
        unsigned long long *d_w = d->d_cnt;
        const int P = d->world;
        HIPR(hipMemcpyAsync(d_w + 4 * 64, out, P * 8, hipMemcpyHostToDevice, ctx->stream));
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            grc = xSend(d, d_w + 4 * 64 + p, 1, XP_UINT64, p, ctx->stream);
            if (grc == XP_SUCCESS) grc = xRecv(d, d_w + 5 * 64 + p, 1, XP_UINT64, p, ctx->stream);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        XPR(grc);
        HIPR(hipMemcpyAsync(in, d_w + 5 * 64, P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        return GK_OK;
    }
    int all_gather(unsigned long long mine, unsigned long long *all) const {
        gk_ctx *ctx = d->ctx;
        unsigned long long *d_w = d->d_cnt;
        HIPR(hipMemcpyAsync(d_w + 2 * 64, &mine, 8, hipMemcpyHostToDevice, ctx->stream));
        XPR(xAllGather(d, d_w + 2 * 64, d_w, 1, XP_UINT64, ctx->stream));
        HIPR(hipMemcpyAsync(all, d_w, d->world * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        return GK_OK;
    }
    int any(bool mine, bool *any_of) const {
        gk_ctx *ctx = d->ctx;
        unsigned long long *d_w = d->d_cnt, w = mine ? 1ull : 0ull;
        HIPR(hipMemcpyAsync(d_w + 2 * 64, &w, 8, hipMemcpyHostToDevice, ctx->stream));
        XPR(xAllReduce(d, d_w + 2 * 64, d_w + 2 * 64 + 1, 1, XP_UINT64, XP_MAX, ctx->stream));
        HIPR(hipMemcpyAsync(&w, d_w + 2 * 64 + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPR(hipStreamSynchronize(ctx->stream));
        *any_of = w != 0;
        return GK_OK;
    }
#undef XPR
#undef HIPR
};

template <class T> int dist_reduce_records(gk_dist *d, gk_graph *g, T *tab, const char *who, const char *what) {
    if (int rc = dist_check(d)) return rc;
    gk_ctx *ctx = d->ctx;
    if (int rc = dist_quiesce(d)) return rc;
    const int P = d->world, me = d->rank;
    int my_rc = GK_OK;
    std::string my_err;
    auto local = [&](int rc) { if (rc != GK_OK && my_rc == GK_OK) { my_rc = rc; my_err = ctx->err; } };
    auto comm_fail = [&](int grc) { return fail(ctx, GK_E_COMM, who + comm_error_text(grc)); };
    auto give_up = [&](const std::string &why) { return my_rc ? fail(ctx, my_rc, my_err) : fail(ctx, GK_E_COMM, who + why); };
    RankWords rw{d, who};
    auto words_all_to_all = [&](const unsigned long long *out, unsigned long long *in) { return rw.all_to_all(out, in); };
    auto word_all_gather = [&](unsigned long long mine, unsigned long long *all) { return rw.all_gather(mine, all); };
    auto any_rank = [&](bool mine, bool *any) { return rw.any(mine, any); };
    // the three planes of n records, and one region of them to or from a peer
    DevScratch buf(ctx);
    auto planes = [&](RecPlanes *p, u64 n) { return buf.get(&p->key, n) == hipSuccess && buf.get(&p->cnt, n) == hipSuccess && buf.get(&p->x, n) == hipSuccess; };
    auto send_planes = [&](const RecPlanes &p, u64 at, u64 n, int peer) {
        int grc = xSend(d, p.key + at, (size_t)n, XP_UINT64, peer, ctx->stream);
        if (grc == XP_SUCCESS) grc = xSend(d, p.cnt + at, (size_t)n * 4, XP_UINT8, peer, ctx->stream);
        if (grc == XP_SUCCESS) grc = xSend(d, p.x + at, (size_t)n, XP_UINT64, peer, ctx->stream);
        return grc;
    };
    auto recv_planes = [&](const RecPlanes &p, u64 at, u64 n, int peer) {
        int grc = xRecv(d, p.key + at, (size_t)n, XP_UINT64, peer, ctx->stream);
        if (grc == XP_SUCCESS) grc = xRecv(d, p.cnt + at, (size_t)n * 4, XP_UINT8, peer, ctx->stream);
        if (grc == XP_SUCCESS) grc = xRecv(d, p.x + at, (size_t)n, XP_UINT64, peer, ctx->stream);
        return grc;
    };
    // ---- 1. status and the replicas' content
    u64 fp = 0, nlive = 0, mine = 0;
    u32 *d_canon = nullptr, *d_inv = nullptr;
    uint8_t *d_dup = nullptr;
    if (!g || !tab) local(fail(ctx, GK_E_INVALID, std::string(who) + "null graph or table"));
    else if (check_graph(g) != GK_OK) local(GK_E_INVALID);
    else if (g->ctx != ctx || rec_ctx(tab) != ctx) local(fail(ctx, GK_E_INVALID, std::string(who) + "the graph and the table must live on the handle's context"));
    if (!my_rc) local(graph_edge_pathkeys(g, buf, &d_canon, &d_inv, &d_dup, &nlive, &fp));
    if (!my_rc) local(rec_distinct(tab, &mine));
    std::vector<unsigned long long> st(P), fps(P);
    if (int rc = word_all_gather(my_rc ? ~0ull : mine, st.data())) return rc;
    if (int rc = word_all_gather(fp, fps.data())) return rc;
    for (int p = 0; p < P; p++)
        if (st[p] == ~0ull) return give_up("rank " + std::to_string(p) + " could not take part; every rank gave up, nothing was changed");
    for (int p = 0; p < P; p++)
        if (fps[p] != fps[me])
            return fail(ctx, GK_E_STATE, std::string(who) + "the graph replicas differ (path fingerprint of rank " + std::to_string(p) + ": " + std::to_string(fps[p]) +
                                             ", of this rank: " + std::to_string(fps[me]) + "): they do not hold the same edge paths, nothing was added up");
    // ---- 2. this rank's records by owner, in the canonical numbering; region sizes to every owner
    RecHandle<T> shard, fresh;
    RecPlanes snd, rcv, all;                                      // by owner (send) | arrivals, then this rank's shard | every shard
    std::vector<u64> region(P + 1, 0);
    if (!planes(&snd, mine)) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(mine) + " records"));
    if (!my_rc) local(rec_bucket(tab, P, snd, mine, region.data(), d_canon, d_dup, g->v.n_edges));
    if (P == 1) return my_rc ? fail(ctx, my_rc, my_err) : GK_OK;
    std::vector<unsigned long long> out(P), in(P);
    for (int p = 0; p < P; p++) out[p] = my_rc ? ~0ull : region[p + 1] - region[p];
    if (int rc = words_all_to_all(out.data(), in.data())) return rc;
    u64 nin = 0;
    std::vector<u64> roff(P + 1, 0);
    for (int p = 0; p < P; p++) {
        if (in[p] == ~0ull) return give_up("rank " + std::to_string(p) + " could not bucket " + what + "; every rank gave up, nothing was changed");
        roff[p] = nin;
        nin += in[p];
    }
    if (my_rc) return give_up("");                                // (unreachable: this rank sent ~0 to itself)
    // ---- 3. room for the arrivals and the shard table
    if (!planes(&rcv, nin)) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(nin) + " arriving records"));
    if (!my_rc) local(rec_new(ctx, nin, (u64)nlive, &shard.t));
    {
        bool any = false;
        if (int rc = any_rank(my_rc != GK_OK, &any)) return rc;
        if (any) return give_up(std::string("a rank had no room for ") + what + " it owns; every rank gave up, nothing was changed");
    }
    // ---- 4. the records to their owners, the owner merge
    {
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            const u64 n = region[p + 1] - region[p];
            if (n) grc = send_planes(snd, region[p], n, p);
            if (in[p] && grc == XP_SUCCESS) grc = recv_planes(rcv, roff[p], in[p], p);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        if (grc != XP_SUCCESS) return comm_fail(grc);
    }
    bool wrapped = false;
    local(rec_insert(shard.t, rcv, nin, &wrapped));
    if (ctx->hook_dist_fail_reduce) {         // test hook: this rank alone fails its owner merge, after the payload has moved
        ctx->hook_dist_fail_reduce = 0;
        local(fail(ctx, GK_E_STATE, std::string(who) + "injected failure (test_dist_fail_reduce)"));
    }
    std::vector<u64> sreg(2, 0);
    if (!my_rc && !wrapped) local(rec_bucket(shard.t, 1, rcv, nin, sreg.data(), nullptr, nullptr, 0));     // the shard, compacted where the arrivals were
    // ---- 5. shard sizes: the owners' verdicts
    std::vector<unsigned long long> ssz(P);
    if (int rc = word_all_gather(my_rc ? ~0ull : wrapped ? ~0ull - 1 : sreg[1], ssz.data())) return rc;
    bool over = false;
    for (int p = 0; p < P; p++) {
        if (ssz[p] == ~0ull) return give_up("rank " + std::to_string(p) + " failed its owner merge; every rank gave up, nothing was changed");
        over |= ssz[p] == ~0ull - 1;
    }
    if (over) return fail(ctx, GK_E_CAPACITY, std::string(who) + "a count summed over the ranks would pass 2^32-1; nothing was changed");
    u64 total = 0;
    std::vector<u64> soff(P + 1, 0);
    for (int p = 0; p < P; p++) { soff[p] = total; total += ssz[p]; }
    // ---- 6. room for every shard and the new table
    if (!planes(&all, total)) local(fail(ctx, GK_E_HIP, std::string(who) + "staging of " + std::to_string(total) + " records"));
    if (!my_rc) local(rec_new(ctx, total, g->v.n_edges, &fresh.t));
    {
        bool any = false;
        if (int rc = any_rank(my_rc != GK_OK, &any)) return rc;
        if (any) return give_up(std::string("a rank had no room for the summed ") + what + "; every rank gave up, nothing was changed");
    }
    // ---- 7. every shard to every rank, the rebuild, the last agreement
    {
        const u64 n = ssz[me];
        int grc = xGroupStart(d);
        for (int p = 0; p < P && grc == XP_SUCCESS; p++) {
            if (n) grc = send_planes(rcv, 0, n, p);
            if (ssz[p] && grc == XP_SUCCESS) grc = recv_planes(all, soff[p], ssz[p], p);
        }
        { const int gend = xGroupEnd(d); if (grc == XP_SUCCESS) grc = gend; }
        if (grc != XP_SUCCESS) return comm_fail(grc);
    }
    local(rec_uncanon<T>(ctx, all, total, d_inv, nlive));             // back to this replica's own edge ids
    bool never = false;
    if (!my_rc) local(rec_insert(fresh.t, all, total, &never));       // (the shards are disjoint: every record is a new one)
    u64 got = 0;
    if (!my_rc) local(rec_distinct(fresh.t, &got));
    if (!my_rc && (got != total || never)) local(fail(ctx, GK_E_STATE, std::string(who) + "rebuilt " + std::to_string(got) + " records from " + std::to_string(total) + " shard records"));
    {
        bool any = false;
        if (int rc = any_rank(my_rc != GK_OK, &any)) return rc;
        if (any) return give_up(std::string("a rank could not rebuild the summed ") + what + "; every rank gave up, nothing was changed");
    }
    return rec_adopt(tab, fresh.t);
}
}  // namespace

extern "C" int gk_dist_reduce_links(gk_dist *d, gk_graph *g, gk_links *links) { return dist_reduce_records(d, g, links, "gk_dist_reduce_links: ", "the links"); }
extern "C" int gk_dist_reduce_spans(gk_dist *d, gk_graph *g, gk_spans *spans) { return dist_reduce_records(d, g, spans, "gk_dist_reduce_spans: ", "the spans"); }
