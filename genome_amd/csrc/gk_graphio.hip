// gk_graphio.hip — the graph file between GraphBuilder and GraphSimplifier (version 1; layout in include/genome_amd.h).
//
// Reference path replaced (S/ = the reference's src/main/scala/ru/ifmo/genome/):
//   MapGraph.write                 S/data/graph/Graph.scala:232-261     gk_graph_save: live flags -> scans (gk_scan.h) ->
//                                                                       k_gio_save_nodes / k_gio_save_edges (id order),
//                                                                       k_gio_save_pool (one wave per edge) -> chunked
//                                                                       download through two pinned buffers beside the writes
//   Graph(file)                    Graph.scala:384-390                  gk_graph_load: chunked read into two pinned buffers beside
//                                                                       the uploads (records to scratch, pool in place)
//   the loaded graph's checks      S/scripts/GraphSimplifier.scala:157-169   k_gio_load_nodes / _edges / _link / _orders
//                                                                       (flag words), then the checksum and id fingerprint
//
// The records of the file are compact (live only, ascending id) and the graph's arrays are indexed by id, so the records land in
// a scratch buffer and a scatter puts them in place.  The pool is already in edge-file order: it is read straight into the
// graph's pool, and e_off is the exclusive scan of ceil(len/4) in that order — offsets never come from the file.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "gk_graph.h"
#include "gk_scan.h"
#include "gk_tile.h"

namespace {

constexpr char GIO_MAGIC[8] = {'G', 'K', 'G', 'R', 'A', 'P', 'H', '\0'};
constexpr u32 GIO_VERSION = 1;
constexpr u64 GIO_HEADER = 128;
constexpr u64 GIO_STAGE = 64ull << 20;            // bytes per pinned staging buffer (two of them)
constexpr u64 GIO_MAX_LEN = 4ull * 0xFFFFFFFFull;  // ceil(len / 4) goes through the u32 scan

// load flag bits: which check failed (gio_flag_text)
enum : u32 {
    GF_NODE_ID = 1, GF_EDGE_ID = 2, GF_ENDPOINT = 4, GF_LENGTH = 8, GF_DUP_OUT = 16, GF_ORDER = 32, GF_PAD_BITS = 64,
    GF_END_KMER = 128, GF_SECTION_PAD = 256
};

std::string gio_flag_text(u32 f) {
    static const char *names[] = {"node ids not ascending or out of bounds", "edge ids not ascending or out of bounds",
                                  "an edge's start or end is not a live node", "an edge of length 0",
                                  "two edges leave one node with the same first base", "a node's out-order disagrees with its edges",
                                  "nonzero padding bits after an edge's last base", "an edge's last k bases are not its end node's k-mer",
                                  "nonzero padding between sections"};
    std::string s;
    for (int i = 0; i < 9; i++) if (f & (1u << i)) s += (s.empty() ? "" : "; ") + std::string(names[i]);
    return s;
}

u64 al8(u64 v) { return (v + 7) & ~7ull; }

// byte offsets in the file of every array (version 1)
struct Layout {
    u64 ids, lo, hi, order, eid, est, een, elen, pool, end;
};
Layout gio_layout(int k, u64 nn, u64 ne, u64 pool_bytes) {
    Layout L{};
    u64 o = GIO_HEADER;
    L.ids = o; o = al8(o + 4 * nn);
    L.lo = o; o += 8 * nn;
    L.hi = 0; if (k >= 34) { L.hi = o; o += 8 * nn; }
    L.order = o; o = al8(o + 4 * nn);
    L.eid = o; o = al8(o + 4 * ne);
    L.est = o; o = al8(o + 4 * ne);
    L.een = o; o = al8(o + 4 * ne);
    L.elen = o; o += 8 * ne;
    L.pool = o;
    L.end = o + pool_bytes;
    return L;
}

struct Header {
    u32 k = 0;
    u64 node_bound = 0, edge_bound = 0, nodes = 0, edges = 0, pool_bytes = 0, cs_nodes = 0, cs_edges = 0, fp = 0;
};
void put32(uint8_t *p, u32 v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
void put64(uint8_t *p, u64 v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
u32 get32(const uint8_t *p) { u32 v = 0; for (int i = 0; i < 4; i++) v |= (u32)p[i] << (8 * i); return v; }
u64 get64(const uint8_t *p) { u64 v = 0; for (int i = 0; i < 8; i++) v |= (u64)p[i] << (8 * i); return v; }

void header_encode(const Header &h, uint8_t *b) {
    std::memset(b, 0, GIO_HEADER);
    std::memcpy(b, GIO_MAGIC, 8);
    put32(b + 8, GIO_VERSION);
    put32(b + 12, h.k);
    put64(b + 16, h.node_bound); put64(b + 24, h.edge_bound);
    put64(b + 32, h.nodes); put64(b + 40, h.edges); put64(b + 48, h.pool_bytes);
    put64(b + 56, h.cs_nodes); put64(b + 64, h.cs_edges); put64(b + 72, h.fp);
}

// two pinned staging buffers and their "copy done" events
struct Stage {
    gk_ctx *ctx;
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    u64 bytes = 0;
    explicit Stage(gk_ctx *c) : ctx(c) {}
    int init(u64 total) {
        bytes = std::max<u64>(1, std::min(total, GIO_STAGE));
        for (int i = 0; i < 2; i++) {
            if (int rc = gk_host_alloc(ctx, bytes, &buf[i])) return rc;
            GK_HIP(ctx, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        return GK_OK;
    }
    ~Stage() {
        for (int i = 0; i < 2; i++) {
            if (ev[i]) { (void)hipEventSynchronize(ev[i]); (void)hipEventDestroy(ev[i]); }
            if (buf[i]) (void)gk_host_free(ctx, buf[i]);
        }
    }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

// ---- save kernels -----------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(BLOCK) void k_gio_save_flags(GraphView g, u32 *__restrict__ nlive, u32 *__restrict__ elive, u32 *__restrict__ ebytes) {
    const u64 tid = (u64)blockIdx.x * BLOCK + threadIdx.x, stride = (u64)gridDim.x * BLOCK;
    for (u64 n = tid; n < g.n_nodes; n += stride) nlive[n] = g.node_alive[n] ? 1u : 0u;
    for (u64 e = tid; e < g.n_edges; e += stride) {
        const bool a = g.e_alive[e];
        elive[e] = a ? 1u : 0u;
        ebytes[e] = a ? (u32)((g.e_len[e] + 3) / 4) : 0u;
    }
}
// the live node / edge records in ascending id order (an id's rank among the live ones = the exclusive scan of the live flags)
static __global__ __launch_bounds__(BLOCK) void k_gio_save_nodes(GraphView g, const unsigned long long *__restrict__ rank, u32 *ids, u64 *lo, u64 *hi,
                                                          u32 *order) {
    for (u64 n = (u64)blockIdx.x * BLOCK + threadIdx.x; n < g.n_nodes; n += (u64)gridDim.x * BLOCK) {
        if (!g.node_alive[n]) continue;
        const u64 j = rank[n];
        ids[j] = (u32)n;
        lo[j] = g.node_lo[n];
        if (hi) hi[j] = g.node_hi[n];
        order[j] = g.out_order[n];
    }
}
static __global__ __launch_bounds__(BLOCK) void k_gio_save_edges(GraphView g, const unsigned long long *__restrict__ rank, u32 *ids, u32 *st, u32 *en,
                                                          u64 *len) {
    for (u64 e = (u64)blockIdx.x * BLOCK + threadIdx.x; e < g.n_edges; e += (u64)gridDim.x * BLOCK) {
        if (!g.e_alive[e]) continue;
        const u64 j = rank[e];
        ids[j] = (u32)e;
        st[j] = g.e_start[e];
        en[j] = g.e_end[e];
        len[j] = g.e_len[e];
    }
}
// the live edges' bytes into the contiguous pool: one wave per edge, the 64 lanes copy consecutive bytes (coalesced on both
// sides); the unused high bits of an edge's last byte are cleared (the in-memory pool may hold bits there after a merge)
static __global__ __launch_bounds__(BLOCK) void k_gio_save_pool(GraphView g, const unsigned long long *__restrict__ dst_off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const u64 wave = ((u64)blockIdx.x * BLOCK + threadIdx.x) >> 6, nwaves = ((u64)gridDim.x * BLOCK) >> 6;
    for (u64 e = wave; e < g.n_edges; e += nwaves) {
        if (!g.e_alive[e]) continue;
        const u64 len = g.e_len[e], nb = (len + 3) / 4, src = g.e_off[e], dst = dst_off[e];
        for (u64 i = lane; i < nb; i += 64) {
            u32 b = g.pool[src + i];
            if (i == nb - 1 && (len & 3)) b &= (1u << ((len & 3) * 2)) - 1u;
            out[dst + i] = (uint8_t)b;
        }
    }
}

// ---- load kernels (GraphSimplifier.scala:157-169) ---------------------------------------------------------------------------
// node records -> their ids' slots; ids must ascend and stay below the bound (an out-of-bounds id is never written)
static __global__ __launch_bounds__(BLOCK) void k_gio_load_nodes(GraphView g, const u32 *__restrict__ ids, const u64 *__restrict__ lo, const u64 *__restrict__ hi,
                                                          const u32 *__restrict__ order, u64 nn, u32 *flags) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nn; j += (u64)gridDim.x * BLOCK) {
        const u32 id = ids[j];
        if ((u64)id >= g.n_nodes || (j > 0 && ids[j - 1] >= id)) { atomicOr(flags, GF_NODE_ID); continue; }
        g.node_lo[id] = lo[j];
        g.node_hi[id] = hi ? hi[j] : 0ull;
        g.out_order[id] = order[j];
        g.node_alive[id] = 1;
    }
    // (zero padding after an odd number of u32 records)
    if (blockIdx.x == 0 && threadIdx.x == 0 && (nn & 1) && (ids[nn] | order[nn])) atomicOr(flags, GF_SECTION_PAD);
}
// edge records -> their ids' slots (not alive yet); nbytes[j] = ceil(len / 4) in file order for the pool scan
static __global__ __launch_bounds__(BLOCK) void k_gio_load_edges(GraphView g, const u32 *__restrict__ ids, const u32 *__restrict__ st, const u32 *__restrict__ en,
                                                          const u64 *__restrict__ len, u64 ne, u32 *__restrict__ nbytes, u32 *flags) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < ne; j += (u64)gridDim.x * BLOCK) {
        const u32 id = ids[j], s = st[j], t = en[j];
        const u64 ln = len[j];
        nbytes[j] = 0;
        u32 bad = 0;
        if ((u64)id >= g.n_edges || (j > 0 && ids[j - 1] >= id)) bad |= GF_EDGE_ID;
        if ((u64)s >= g.n_nodes || (u64)t >= g.n_nodes) bad |= GF_ENDPOINT;
        if (ln == 0 || ln > GIO_MAX_LEN) bad |= GF_LENGTH;
        if (bad) { atomicOr(flags, bad); continue; }
        g.e_start[id] = s;
        g.e_end[id] = t;
        g.e_len[id] = ln;
        nbytes[j] = (u32)((ln + 3) / 4);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (ne & 1) && (ids[ne] | st[ne] | en[ne])) atomicOr(flags, GF_SECTION_PAD);
}
static __device__ __forceinline__ int gio_kmer_base(const GraphView &g, u32 n, int i) {
    return (int)(((i < 32 ? g.node_lo[n] : g.node_hi[n]) >> (2 * (i & 31))) & 3);
}
// runs only when every id, endpoint and length passed and the pool is exactly sum ceil(len / 4) bytes: e_off, e_first, alive,
// the out-edge table (claimed once per (start, first base)), in-degrees, the padding bits and the end k-mer:
// base i of the end node = base len + i of (start k-mer ++ sequence), O(k) per edge
static __global__ __launch_bounds__(BLOCK) void k_gio_load_link(GraphView g, int k, const u32 *__restrict__ ids, const unsigned long long *__restrict__ poff,
                                                         u64 ne, u32 *flags) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < ne; j += (u64)gridDim.x * BLOCK) {
        const u32 e = ids[j], s = g.e_start[e], t = g.e_end[e];
        const u64 off = poff[j], len = g.e_len[e], nb = (len + 3) / 4;
        g.e_off[e] = off;
        if (!g.node_alive[s] || !g.node_alive[t]) { atomicOr(flags, GF_ENDPOINT); continue; }
        u32 bad = 0;
        if ((len & 3) && (g.pool[off + nb - 1] >> ((len & 3) * 2))) bad |= GF_PAD_BITS;
        for (int i = 0; i < k; i++) {
            const u64 p = len + (u64)i;
            const int b = p < (u64)k ? gio_kmer_base(g, s, (int)p) : pool_get(g.pool, off, p - (u64)k);
            if (b != gio_kmer_base(g, t, i)) { bad |= GF_END_KMER; break; }
        }
        const int first = pool_get(g.pool, off, 0);
        g.e_first[e] = (uint8_t)first;
        g.e_alive[e] = 1;
        if (atomicCAS(&g.out_edge[(u64)s * 4 + first], NONE, e) != NONE) bad |= GF_DUP_OUT;
        atomicAdd(&g.in_deg[t], 1u);
        if (bad) atomicOr(flags, bad);
    }
}
// every live node's out-order lists exactly the bases that have an out-edge, each once
static __global__ __launch_bounds__(BLOCK) void k_gio_load_orders(GraphView g, const u32 *__restrict__ ids, u64 nn, u32 *flags) {
    for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nn; j += (u64)gridDim.x * BLOCK) {
        const u32 n = ids[j], o = g.out_order[n];
        const int c = order_count(o);
        u32 listed = 0, present = 0;
        bool bad = c > 4;
        for (int i = 0; i < c && !bad; i++) {
            const u32 bit = 1u << order_base(o, i);
            bad = (listed & bit) != 0;
            listed |= bit;
        }
        for (int b = 0; b < 4; b++) if (g.out_edge[(u64)n * 4 + b] != NONE) present |= 1u << b;
        if (bad || listed != present) atomicOr(flags, GF_ORDER);
    }
}

namespace {

// ---- host side ----------------------------------------------------------------------------------------------------------------
int sys_fail(gk_ctx *ctx, const std::string &what, const std::string &path) {
    return fail(ctx, GK_E_INVALID, what + " " + path + ": " + std::strerror(errno));
}

// write all of [p, p + n) to fd
bool write_all(int fd, const void *p, u64 n) {
    const char *c = (const char *)p;
    while (n) {
        const ssize_t w = ::write(fd, c, std::min<u64>(n, 1ull << 30));
        if (w < 0) { if (errno == EINTR) continue; return false; }
        c += w; n -= (u64)w;
    }
    return true;
}
// read n bytes; false on an error or an early end (errno = 0 then)
bool read_all(int fd, void *p, u64 n) {
    char *c = (char *)p;
    while (n) {
        const ssize_t r = ::read(fd, c, std::min<u64>(n, 1ull << 30));
        if (r < 0) { if (errno == EINTR) continue; return false; }
        if (r == 0) { errno = 0; return false; }
        c += r; n -= (u64)r;
    }
    return true;
}

int graph_save_impl(gk_graph *g, const std::string &path, const std::string &tmp, float *ms) {
    gk_ctx *ctx = g->ctx;
    const GraphView &v = g->v;
    const double t0 = now_ms();
    double t_io = 0, t_copy = 0;
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (v.n_nodes >= NONE || v.n_edges >= NONE) return fail(ctx, GK_E_CAPACITY, "gk_graph_save: id bounds beyond the format's 2^32-2");
    Header h;
    h.k = (u32)g->k;
    h.node_bound = v.n_nodes;
    h.edge_bound = v.n_edges;
    const double t_k0 = now_ms();
    if (int rc = gk_graph_checksum(g, &h.cs_nodes, &h.cs_edges)) return rc;
    if (int rc = gk_graph_id_fingerprint(g, &h.fp)) return rc;
    // live flags -> ranks (record slots) and pool offsets
    DevScratch tmp_(ctx);
    const u64 nn = v.n_nodes, ne = v.n_edges;
    u32 *nlive = nullptr, *elive = nullptr, *ebytes = nullptr;
    unsigned long long *nrank = nullptr, *erank = nullptr, *poff = nullptr;
    GK_HIP(ctx, tmp_.get(&nlive, nn));
    GK_HIP(ctx, tmp_.get(&elive, ne));
    GK_HIP(ctx, tmp_.get(&ebytes, ne));
    GK_HIP(ctx, tmp_.get(&nrank, nn + 1));
    GK_HIP(ctx, tmp_.get(&erank, ne + 1));
    GK_HIP(ctx, tmp_.get(&poff, ne + 1));
    if (nn || ne) {
        hipLaunchKernelGGL(k_gio_save_flags, dim3(ggrid(ctx, std::max(nn, ne))), dim3(BLOCK), 0, ctx->stream, v, nlive, elive, ebytes);
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, scan_counts(ctx, tmp_, nlive, nn, nrank));      // (each scan holds its own few KB of scratch until this call returns)
    GK_HIP(ctx, scan_counts(ctx, tmp_, elive, ne, erank));
    GK_HIP(ctx, scan_counts(ctx, tmp_, ebytes, ne, poff));
    unsigned long long tot[3] = {0, 0, 0};
    GK_HIP(ctx, read_back(ctx, {{&tot[0], nrank + nn, 8}, {&tot[1], erank + ne, 8}, {&tot[2], poff + ne, 8}}));
    h.nodes = tot[0]; h.edges = tot[1]; h.pool_bytes = tot[2];
    if (h.nodes != g->live_nodes || h.edges != g->live_edges) return fail(ctx, GK_E_STATE, "gk_graph_save: live counts disagree with the graph's");
    const Layout L = gio_layout(g->k, h.nodes, h.edges, h.pool_bytes);
    const u64 body = L.end - GIO_HEADER;
    uint8_t *d_body = nullptr;
    GK_HIP(ctx, tmp_.get(&d_body, body));
    if (body) {
        GK_HIP(ctx, hipMemsetAsync(d_body, 0, body, ctx->stream));     // (the padding between sections)
        auto at = [&](u64 off) { return d_body + (off - GIO_HEADER); };
        if (nn) {
            hipLaunchKernelGGL(k_gio_save_nodes, dim3(ggrid(ctx, nn)), dim3(BLOCK), 0, ctx->stream, v, nrank, (u32 *)at(L.ids), (u64 *)at(L.lo),
                               L.hi ? (u64 *)at(L.hi) : nullptr, (u32 *)at(L.order));
            GK_HIP(ctx, hipGetLastError());
        }
        if (ne) {
            hipLaunchKernelGGL(k_gio_save_edges, dim3(ggrid(ctx, ne)), dim3(BLOCK), 0, ctx->stream, v, erank, (u32 *)at(L.eid), (u32 *)at(L.est),
                               (u32 *)at(L.een), (u64 *)at(L.elen));
            GK_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_gio_save_pool, dim3(ggrid(ctx, ne * 64)), dim3(BLOCK), 0, ctx->stream, v, poff, at(L.pool));
            GK_HIP(ctx, hipGetLastError());
        }
    }
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double t_k = now_ms() - t_k0;
    // the file: header, then the body in chunks — chunk c + 1 downloads while chunk c is written
    uint8_t hb[GIO_HEADER];
    header_encode(h, hb);
    Stage st(ctx);
    if (int rc = st.init(body)) return rc;
    double t = now_ms();
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) return sys_fail(ctx, "gk_graph_save: cannot open", tmp);
    bool ok = write_all(fd, hb, GIO_HEADER);
    t_io += now_ms() - t;
    const u64 nch = (body + st.bytes - 1) / st.bytes;
    auto issue = [&](u64 c) -> hipError_t {
        const u64 o = c * st.bytes, n = std::min(st.bytes, body - o);
        hipError_t e = hipMemcpyAsync(st.buf[c & 1], d_body + o, n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(st.ev[c & 1], ctx->stream);
        return e;
    };
    hipError_t he = nch ? issue(0) : hipSuccess;
    for (u64 c = 0; c < nch && ok && he == hipSuccess; c++) {
        if (c + 1 < nch) he = issue(c + 1);
        if (he != hipSuccess) break;
        t = now_ms();
        he = hipEventSynchronize(st.ev[c & 1]);
        t_copy += now_ms() - t;
        if (he != hipSuccess) break;
        t = now_ms();
        ok = write_all(fd, st.buf[c & 1], std::min(st.bytes, body - c * st.bytes));
        t_io += now_ms() - t;
    }
    t = now_ms();
    if (::close(fd) != 0) ok = false;
    t_io += now_ms() - t;
    if (he != hipSuccess) { ::unlink(tmp.c_str()); return hip_fail(ctx, he, "gk_graph_save: download"); }
    if (!ok) { const int en = errno; ::unlink(tmp.c_str()); errno = en; return sys_fail(ctx, "gk_graph_save: cannot write", tmp); }
    if (std::rename(tmp.c_str(), path.c_str()) != 0) { const int en = errno; ::unlink(tmp.c_str()); errno = en; return sys_fail(ctx, "gk_graph_save: cannot rename to", path); }
    ms[0] = (float)t_io; ms[1] = (float)t_copy; ms[2] = (float)t_k; ms[3] = (float)(now_ms() - t0);
    return GK_OK;
}

int graph_load_impl(gk_ctx *ctx, const std::string &path, gk_graph *g, float *ms) {
    const double t0 = now_ms();
    double t_io = 0, t_copy = 0, t_k = 0;
    double t = now_ms();
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) return sys_fail(ctx, "gk_graph_load: cannot open", path);
    struct FdGuard { int fd; ~FdGuard() { ::close(fd); } } guard{fd};
    struct stat sb{};
    if (::fstat(fd, &sb) != 0) return sys_fail(ctx, "gk_graph_load: cannot stat", path);
    const u64 fsize = (u64)sb.st_size;
    uint8_t hb[GIO_HEADER];
    if (fsize < GIO_HEADER) return fail(ctx, GK_E_FORMAT, "gk_graph_load: " + path + ": shorter than the 128-byte header");
    if (!read_all(fd, hb, GIO_HEADER)) return sys_fail(ctx, "gk_graph_load: cannot read", path);
    t_io += now_ms() - t;
    auto bad = [&](const std::string &why) { return fail(ctx, GK_E_FORMAT, "gk_graph_load: " + path + ": " + why); };
    if (std::memcmp(hb, GIO_MAGIC, 8) != 0) return bad("not a graph file (magic)");
    if (get32(hb + 8) != GIO_VERSION) return bad("version " + std::to_string(get32(hb + 8)) + " (this library reads version 1)");
    Header h;
    h.k = get32(hb + 12);
    h.node_bound = get64(hb + 16); h.edge_bound = get64(hb + 24);
    h.nodes = get64(hb + 32); h.edges = get64(hb + 40); h.pool_bytes = get64(hb + 48);
    h.cs_nodes = get64(hb + 56); h.cs_edges = get64(hb + 64); h.fp = get64(hb + 72);
    for (u64 i = 80; i < GIO_HEADER; i++) if (hb[i]) return bad("nonzero reserved header bytes");
    if (h.k > 64 || !k_supported((int)h.k)) return bad("k = " + std::to_string(h.k));
    if (h.node_bound >= NONE || h.edge_bound >= NONE) return bad("id bounds beyond 2^32-2");
    if (h.nodes > h.node_bound || h.edges > h.edge_bound) return bad("more records than ids");
    if (h.pool_bytes > fsize) return bad("pool larger than the file");
    const Layout L = gio_layout((int)h.k, h.nodes, h.edges, h.pool_bytes);
    if (fsize < L.end) return bad("truncated (" + std::to_string(fsize) + " bytes, the header needs " + std::to_string(L.end) + ")");
    if (fsize > L.end) return bad("trailing bytes (" + std::to_string(fsize) + " bytes, the header needs " + std::to_string(L.end) + ")");
    g->ctx = ctx;
    g->k = (int)h.k;
    g->v.k = (int)h.k;           // (the kernels that take the view alone read k from it: edge coverage, the contigs)
    g->W = words_for_k((int)h.k);
    if (int rc = graph_alloc_nodes(g, h.node_bound)) return rc;
    if (int rc = graph_alloc_edges(g, h.edge_bound)) return rc;
    GraphView &v = g->v;
    // dead ids read back as zeros
    GK_HIP(ctx, hipMemsetAsync(v.node_lo, 0, g->node_cap * 8, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.node_hi, 0, g->node_cap * 8, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.e_start, 0, g->edge_cap * 4, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.e_end, 0, g->edge_cap * 4, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.e_len, 0, g->edge_cap * 8, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.e_off, 0, g->edge_cap * 8, ctx->stream));
    GK_HIP(ctx, hipMemsetAsync(v.e_first, 0, g->edge_cap, ctx->stream));
    // the pool: whole 32-bit words and 8 bytes of slack (k_copy_long / k_pj_emit OR whole words), zeroed
    g->pool_used = h.pool_bytes;
    g->pool_cap = (h.pool_bytes + 8 + 3) / 4 * 4;
    GK_HIP(ctx, pool_malloc(ctx, &v.pool, g->pool_cap));
    GK_HIP(ctx, hipMemsetAsync(v.pool, 0, g->pool_cap, ctx->stream));
    // records -> scratch, pool -> v.pool: chunk c + 1 is read while chunk c uploads
    DevScratch tmp_(ctx);
    const u64 rec_bytes = L.pool - GIO_HEADER, body = L.end - GIO_HEADER;
    uint8_t *d_rec = nullptr;
    GK_HIP(ctx, tmp_.get(&d_rec, rec_bytes + 8));
    GK_HIP(ctx, hipMemsetAsync(d_rec, 0, rec_bytes + 8, ctx->stream));
    Stage st(ctx);
    if (int rc = st.init(body)) return rc;
    for (u64 o = 0, c = 0; o < body; o += st.bytes, c++) {
        const int b = (int)(c & 1);
        const u64 n = std::min(st.bytes, body - o);
        if (st.pending[b]) {
            t = now_ms();
            GK_HIP(ctx, hipEventSynchronize(st.ev[b]));
            t_copy += now_ms() - t;
        }
        t = now_ms();
        if (!read_all(fd, st.buf[b], n)) {
            if (errno == 0) return bad("the file changed while it was read");
            return sys_fail(ctx, "gk_graph_load: cannot read", path);
        }
        t_io += now_ms() - t;
        const uint8_t *src = (const uint8_t *)st.buf[b];
        if (o < rec_bytes) GK_HIP(ctx, hipMemcpyAsync(d_rec + o, src, std::min(n, rec_bytes - o), hipMemcpyHostToDevice, ctx->stream));
        if (o + n > rec_bytes) {
            const u64 s0 = std::max(o, rec_bytes);
            GK_HIP(ctx, hipMemcpyAsync(v.pool + (s0 - rec_bytes), src + (s0 - o), o + n - s0, hipMemcpyHostToDevice, ctx->stream));
        }
        GK_HIP(ctx, hipEventRecord(st.ev[b], ctx->stream));
        st.pending[b] = true;
    }
    t = now_ms();
    GK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    t_copy += now_ms() - t;
    // the checks
    const double t_k0 = now_ms();
    auto at = [&](u64 off) { return d_rec + (off - GIO_HEADER); };
    const u32 *ids = (const u32 *)at(L.ids), *eid = (const u32 *)at(L.eid);
    u32 *flags = nullptr, *nbytes = nullptr;
    unsigned long long *poff = nullptr;
    GK_HIP(ctx, tmp_.get(&flags, 1));
    GK_HIP(ctx, tmp_.get(&nbytes, h.edges));
    GK_HIP(ctx, tmp_.get(&poff, h.edges + 1));
    GK_HIP(ctx, hipMemsetAsync(flags, 0, 4, ctx->stream));
    if (h.nodes) {
        hipLaunchKernelGGL(k_gio_load_nodes, dim3(ggrid(ctx, h.nodes)), dim3(BLOCK), 0, ctx->stream, v, ids, (const u64 *)at(L.lo),
                           L.hi ? (const u64 *)at(L.hi) : nullptr, (const u32 *)at(L.order), h.nodes, flags);
        GK_HIP(ctx, hipGetLastError());
    }
    if (h.edges) {
        hipLaunchKernelGGL(k_gio_load_edges, dim3(ggrid(ctx, h.edges)), dim3(BLOCK), 0, ctx->stream, v, eid, (const u32 *)at(L.est),
                           (const u32 *)at(L.een), (const u64 *)at(L.elen), h.edges, nbytes, flags);
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, scan_counts(ctx, tmp_, nbytes, h.edges, poff));
    u32 hflags = 0;
    unsigned long long pool_sum = 0;
    GK_HIP(ctx, read_back(ctx, {{&hflags, flags, 4}, {&pool_sum, poff + h.edges, 8}}));
    if (hflags) return bad(gio_flag_text(hflags));
    if (pool_sum != h.pool_bytes)
        return bad("pool of " + std::to_string(h.pool_bytes) + " bytes, the edge lengths need " + std::to_string(pool_sum));
    if (h.edges) {
        hipLaunchKernelGGL(k_gio_load_link, dim3(ggrid(ctx, h.edges)), dim3(BLOCK), 0, ctx->stream, v, g->k, eid, poff, h.edges, flags);
        GK_HIP(ctx, hipGetLastError());
    }
    if (h.nodes) {
        hipLaunchKernelGGL(k_gio_load_orders, dim3(ggrid(ctx, h.nodes)), dim3(BLOCK), 0, ctx->stream, v, ids, h.nodes, flags);
        GK_HIP(ctx, hipGetLastError());
    }
    GK_HIP(ctx, read_back(ctx, &hflags, flags));
    if (hflags) return bad(gio_flag_text(hflags));
    if (int rc = graph_refresh_counts(g)) return rc;
    g->index_ready = false;                   // (built on the first point query, as after a build)
    u64 cn = 0, ce = 0, fp = 0;
    if (int rc = gk_graph_checksum(g, &cn, &ce)) return rc;
    if (int rc = gk_graph_id_fingerprint(g, &fp)) return rc;
    t_k += now_ms() - t_k0;
    if (g->live_nodes != h.nodes || g->live_edges != h.edges) return bad("live counts disagree with the header");
    if (cn != h.cs_nodes || ce != h.cs_edges) return bad("content checksum mismatch");
    if (fp != h.fp) return bad("id fingerprint mismatch");
    ms[0] = (float)t_io; ms[1] = (float)t_copy; ms[2] = (float)t_k; ms[3] = (float)(now_ms() - t0);
    return GK_OK;
}

}  // namespace

extern "C" {

int gk_graph_save(gk_graph *g, const char *path) {
    if (int rc = check_graph(g)) return rc;
    gk_ctx *ctx = g->ctx;
    if (!path || !*path) return fail(ctx, GK_E_INVALID, "gk_graph_save: null path");
    const std::string p(path), tmp = p + ".tmp";
    float ms[4] = {0, 0, 0, 0};
    const int rc = graph_save_impl(g, p, tmp, ms);
    if (rc != GK_OK) {
        (void)::unlink(tmp.c_str());
        return rc;
    }
    std::memcpy(ctx->graph_io_ms, ms, sizeof(ms));
    return GK_OK;
}

int gk_graph_load(gk_ctx *ctx, const char *path, gk_graph **out) {
    if (!ctx) return fail(nullptr, GK_E_INVALID, "gk_graph_load: null context");
    if (!out) return fail(ctx, GK_E_INVALID, "gk_graph_load: out is NULL");
    *out = nullptr;
    if (!path || !*path) return fail(ctx, GK_E_INVALID, "gk_graph_load: null path");
    GK_HIP(ctx, hipSetDevice(ctx->device));
    gk_graph *g = new gk_graph();
    g->ctx = ctx;
    float ms[4] = {0, 0, 0, 0};
    const int rc = graph_load_impl(ctx, path, g, ms);
    if (rc != GK_OK) {
        const std::string msg = ctx->err;     // (keep the load's message past the cleanup)
        gk_graph_destroy(g);
        set_error(ctx, msg);
        return rc;
    }
    std::memcpy(ctx->graph_io_ms, ms, sizeof(ms));
    *out = g;
    return GK_OK;
}

int gk_graph_k(const gk_graph *g) {
    if (int rc = check_graph(g)) return rc;
    return g->k;
}

int gk_graph_io_stats(gk_ctx *ctx, float *ms4) {
    if (!ctx || !ms4) return fail(ctx, GK_E_INVALID, "gk_graph_io_stats: null argument");
    std::memcpy(ms4, ctx->graph_io_ms, sizeof(ctx->graph_io_ms));
    return GK_OK;
}

}  // extern "C"
