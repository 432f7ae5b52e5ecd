// scratch_check.hip — host-only checks of DevScratch (gk_internal.h) and of the `.bin` framing helpers (gk_binstream.h).
// A program of its own: the pool is malloc / free with counters and a switch that fails the n-th allocation, gk::fail records
// its message.  Nothing here needs a device: allocations that succeed are only asked for with get(), and a DevScratch whose
// error has stuck does not reach the runtime.  Built with -fsanitize=address,undefined (tests/test_scratch_cpu.py): every
// stream lives in a heap block of exactly its size, so a read past it is a report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../genome_amd/csrc/gk_binstream.h"
#include "../../genome_amd/csrc/gk_internal.h"

static int g_allocs = 0, g_alloc_calls = 0, g_frees = 0, g_fail_at = -1;     // g_fail_at: the allocator call that fails (0-based)
static std::string g_msg;
static int g_code = 0;
static int g_failed = 0;

namespace gk {
hipError_t pool_malloc(gk_ctx *, void **p, size_t bytes) {
    if (g_alloc_calls++ == g_fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    g_allocs++;
    return hipSuccess;
}
hipError_t pool_free(gk_ctx *, void *p) {
    if (p) { std::free(p); g_frees++; }
    return hipSuccess;
}
int fail(const gk_ctx *, int code, const std::string &msg) { g_code = code; g_msg = msg; return code; }
}  // namespace gk

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

using gk::DevScratch;

// call number `i` of the sequence of five: before the failing position only get(); from it on every form in turn
static hipError_t scratch_call(DevScratch &tmp, int i, int fail_at, uint32_t **p) {
    static const uint32_t host[4] = {1, 2, 3, 4};
    if (i < fail_at) return tmp.get(p, 4);
    switch ((i - fail_at) % 3) {
        case 0: return tmp.get(p, 4);
        case 1: return tmp.zeroed(p, 4);
        default: return tmp.upload(p, host, 4);
    }
}

static void check_scratch(gk_ctx *ctx) {
    for (int fail_at = 0; fail_at <= 5; fail_at++) {             // 5: nothing fails
        g_allocs = g_alloc_calls = g_frees = 0;
        g_fail_at = fail_at < 5 ? fail_at : -1;
        {
            DevScratch tmp(ctx);
            std::set<void *> seen;
            for (int i = 0; i < 5; i++) {
                uint32_t *p = (uint32_t *)0x1;
                const int calls_before = g_alloc_calls;
                const hipError_t e = scratch_call(tmp, i, fail_at, &p);
                if (i < fail_at) {
                    CHECK(e == hipSuccess && p != nullptr && seen.insert(p).second);
                    CHECK(tmp.error() == hipSuccess);
                } else {
                    CHECK(e == hipErrorOutOfMemory && p == nullptr);
                    CHECK(tmp.error() == hipErrorOutOfMemory);
                    CHECK(g_alloc_calls == calls_before + (i == fail_at ? 1 : 0));       // no allocator call once the error has stuck
                }
            }
            CHECK(tmp.note(hipErrorInvalidValue) == (fail_at < 5 ? hipErrorOutOfMemory : hipErrorInvalidValue));   // the FIRST error stays
            CHECK(g_allocs == std::min(fail_at, 5) && g_frees == 0);
        }
        CHECK(g_frees == g_allocs);
    }
    // note() alone makes the error stick too
    g_allocs = g_alloc_calls = g_frees = 0; g_fail_at = -1;
    {
        DevScratch tmp(ctx);
        uint32_t *p = nullptr;
        CHECK(tmp.note(hipSuccess) == hipSuccess && tmp.error() == hipSuccess);
        CHECK(tmp.note(hipErrorInvalidValue) == hipErrorInvalidValue);
        CHECK(tmp.get(&p, 1) == hipErrorInvalidValue && p == nullptr && g_alloc_calls == 0);
    }
    // take() hands a buffer over, release() frees one early and once
    g_allocs = g_alloc_calls = g_frees = 0;
    uint32_t *kept = nullptr;
    {
        DevScratch tmp(ctx);
        uint32_t *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(tmp.get(&a, 3) == hipSuccess && tmp.get(&b, 0) == hipSuccess && tmp.get(&c, 7) == hipSuccess);
        kept = tmp.take(a);
        CHECK(kept == a && g_frees == 0);
        tmp.release(b);
        CHECK(b == nullptr && g_frees == 1);
    }
    CHECK(g_allocs == 3 && g_frees == 2);                        // c went with the scope, b was not freed again, a is ours
    (void)gk::pool_free(ctx, kept);
    CHECK(g_frees == 3);
}

// a stream of the given record lengths in a heap block of exactly nbytes bytes (the records, cut or followed by `extra` bytes)
struct Stream {
    uint8_t *bin = nullptr;
    size_t nbytes = 0;
    std::vector<size_t> off;                                     // record offsets and the end
    Stream(const std::vector<int> &lens, long extra) {
        std::vector<uint8_t> all;
        for (int len : lens) {
            off.push_back(all.size());
            all.push_back((uint8_t)len);
            for (int j = 0; j < (len + 3) / 4; j++) all.push_back((uint8_t)(0xA5 ^ j ^ len));
        }
        off.push_back(all.size());
        for (long j = 0; j < extra; j++) all.push_back(0xff);    // (a length byte of 255 if it were ever read as one)
        nbytes = (size_t)((long)all.size() + std::min(extra, 0L));
        bin = (uint8_t *)std::malloc(nbytes ? nbytes : 1);
        if (nbytes) std::memcpy(bin, all.data(), nbytes);
    }
    ~Stream() { std::free(bin); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
};

static const std::vector<std::vector<int>> ORDERS = {
    {0, 1, 4, 5, 255}, {255, 5, 4, 1, 0}, {4, 0, 255, 0, 1, 5}, {5, 255, 255, 1}, {0}, {255}, {0, 0, 0}, {1, 4, 5, 0},
};

static void check_walk(gk_ctx *ctx) {
    CHECK(gk::bin_record_bytes(0) == 1 && gk::bin_record_bytes(1) == 2 && gk::bin_record_bytes(4) == 2 && gk::bin_record_bytes(5) == 3 &&
          gk::bin_record_bytes(255) == 65);
    for (const auto &lens : ORDERS) {
        const uint64_t n = lens.size();
        for (long extra : {0L, 3L}) {                            // nbytes == end, and bytes behind the last record
            Stream s(lens, extra);
            size_t end = ~(size_t)0;
            CHECK(gk::bin_walk(ctx, s.bin, s.nbytes, n, &end) == GK_OK && end == s.off[n]);
            CHECK(gk::bin_walk(ctx, s.bin, s.nbytes, 0, &end) == GK_OK && end == 0);
        }
        // the stream ends one byte short of the end of record r: inside r — or, where r is a single byte, before it starts
        for (uint64_t r = 0; r < n; r++) {
            std::vector<int> head(lens.begin(), lens.begin() + r + 1);
            Stream s(head, -1);
            size_t end = 12345;
            g_msg.clear();
            CHECK(gk::bin_walk(ctx, s.bin, s.nbytes, r + 1, &end) == GK_E_FORMAT && g_code == GK_E_FORMAT && end == 12345);
            const std::string want = lens[r] == 0 ? "truncated .bin stream: record " + std::to_string(r) + " starts past the end"
                                                  : "truncated .bin stream inside record " + std::to_string(r);
            CHECK(g_msg == want);
        }
        {   // one record more than the stream holds
            Stream s(lens, 0);
            size_t end = 0;
            g_msg.clear();
            CHECK(gk::bin_walk(ctx, s.bin, s.nbytes, n + 1, &end) == GK_E_FORMAT);
            CHECK(g_msg == "truncated .bin stream: record " + std::to_string(n) + " starts past the end");
        }
    }
}

static void check_cut() {
    for (const auto &lens : ORDERS) {
        Stream s(lens, 0);
        const size_t end = s.off.back();
        std::set<size_t> caps = {1, end};
        for (int len : lens) {
            const size_t rb = gk::bin_record_bytes((unsigned)len);
            caps.insert(rb); caps.insert(rb + 1);
            if (rb > 1) caps.insert(rb - 1);
        }
        for (size_t cap : caps) {
            size_t pos = 0, rec = 0;
            while (pos < end) {
                const gk::BinPiece p = gk::bin_cut(s.bin, end, pos, cap);
                CHECK(p.begin == pos);                           // the pieces tile [0, end) in order
                CHECK(p.offs.size() >= 2);                       // at least one record
                CHECK(p.offs.front() == 0 && p.offs.back() == p.bytes);
                const size_t nrec = p.offs.size() - 1;
                for (size_t j = 0; j < nrec; j++) {
                    CHECK(p.offs[j] < p.offs[j + 1]);            // strictly increasing, by the record's own size (1 for an empty record)
                    CHECK(pos + p.offs[j] == s.off[rec + j] && p.offs[j + 1] - p.offs[j] == gk::bin_record_bytes(s.bin[pos + p.offs[j]]));
                }
                CHECK(p.bytes <= cap || nrec == 1);              // only a record that alone exceeds the cap may pass it
                if (pos + p.bytes < end) CHECK(p.bytes + gk::bin_record_bytes(s.bin[pos + p.bytes]) > cap);   // it stopped because the next would not fit
                if (p.offs.size() < 2 || p.bytes == 0) break;    // (reported above; do not spin)
                pos += p.bytes; rec += nrec;
            }
            CHECK(pos == end && rec == lens.size());
        }
        const gk::BinPiece none = gk::bin_cut(s.bin, end, end, 1);                    // nothing left: the empty piece the feeder stops at
        CHECK(none.bytes == 0 && none.offs.size() == 1);
    }
}

int main() {
    gk_ctx ctx;
    check_scratch(&ctx);
    check_walk(&ctx);
    check_cut();
    // the small helpers that go with them
    const gk::ReadSrc f = gk::ReadSrc::fixed((const void *)0x1000, 7, 101);
    CHECK(f.rec == (const uint8_t *)0x1000 && f.nreads == 7 && f.off == nullptr && f.stride == gk::bin_record_bytes(101) && f.max_len == 101);
    const gk::ReadSrc r = gk::ReadSrc::framed((const uint8_t *)0x1000, (const uint32_t *)0x2000, 9);
    CHECK(r.nreads == 9 && r.off == (const uint32_t *)0x2000 && r.stride == 0 && r.max_len == 255);
    CHECK(gk::check_read_len(&ctx, 0) == GK_OK && gk::check_read_len(&ctx, 255) == GK_OK);
    CHECK(gk::check_read_len(&ctx, -1) == GK_E_FORMAT && gk::check_read_len(&ctx, 256) == GK_E_FORMAT);
    CHECK(g_msg == "read_len must be 0..255 (one length byte per record)");
    if (g_failed) { std::fprintf(stderr, "scratch_check: %d checks failed\n", g_failed); return 1; }
    std::puts("scratch_check ok");
    return 0;
}
