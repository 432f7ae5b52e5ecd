// gk_binstream.h — a `.bin` read stream in HOST memory (PairedEndData.scala:20-36: one length byte, then the bases four to a
// byte): its framing, and the double-buffered feed of whole records through two device staging areas.  Host code only.
//
// Who feeds from here: gk_reads_correct and gk_graph_thread_reads.  Who does not, on purpose: gk_map_count_reads /
// gk_dist_count_reads (map_cut_chunk: chunks bounded by windows too, possibly unwalked, prefetched) and the pre-filter
// (pf_for_each_host_chunk, gk_prefilter.hip: chunks bounded in bytes by "test_max_stage" and, in pass 2, in windows by
// "test_prefilter_chunk_windows"; gk_test_prefilter_chunks echoes what it staged — include/genome_amd_test.h).
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "gk_internal.h"

namespace gk {

inline size_t bin_record_bytes(unsigned len) { return 1 + (size_t)(len + 3) / 4; }

// what a framing walk can find (the values map_cut_chunk reports in *err), and the GK_E_FORMAT message that goes with each
enum { BIN_PAST_END = 1, BIN_INSIDE = 2 };
inline int bin_truncated(const gk_ctx *ctx, int kind, uint64_t record) {
    return fail(ctx, GK_E_FORMAT, kind == BIN_PAST_END ? "truncated .bin stream: record " + std::to_string(record) + " starts past the end"
                                                       : "truncated .bin stream inside record " + std::to_string(record));
}

// The framing of nreads records, walked before anything is written or launched.  *end = the byte after the last record.
inline int bin_walk(const gk_ctx *ctx, const uint8_t *bin, size_t nbytes, uint64_t nreads, size_t *end) {
    size_t pos = 0;
    for (uint64_t r = 0; r < nreads; r++) {
        if (pos >= nbytes) return bin_truncated(ctx, BIN_PAST_END, r);
        pos += bin_record_bytes(bin[pos]);
        if (pos > nbytes) return bin_truncated(ctx, BIN_INSIDE, r);
    }
    *end = pos;
    return GK_OK;
}

// Whole records of a walked stream from `pos` on: at least one, and no further one that would take the piece past byte_cap.
// offs = the record offsets from `begin`, and the end.
struct BinPiece {
    size_t begin = 0, bytes = 0;
    std::vector<uint32_t> offs;
};
inline BinPiece bin_cut(const uint8_t *bin, size_t end, size_t pos, size_t byte_cap) {
    BinPiece c;
    c.begin = pos;
    while (pos < end) {
        const size_t rb = bin_record_bytes(bin[pos]);
        if (!c.offs.empty() && pos + rb - c.begin > byte_cap) break;
        c.offs.push_back((uint32_t)(pos - c.begin));
        pos += rb;
    }
    c.offs.push_back((uint32_t)(pos - c.begin));
    c.bytes = pos - c.begin;
    return c;
}

// Feed bin[0, end) through the device in pieces of whole records, bounded by the staging area; two areas, so that the next
// piece's upload (copy stream, announced by cev[0]) runs beside this piece's kernels.  per_chunk(src, d_area, piece, &back) queues
// the piece's launches on ctx->stream and may name a way back: read_back does it after the next upload has been issued, and with
// no destination it is the plain check-and-wait.  The end of every piece waits for the main stream, so the offset table and the
// other area are free when the next piece needs them.  The areas and the table belong to `tmp`.
template <class PerChunk> int bin_feed(gk_ctx *ctx, DevScratch &tmp, const uint8_t *bin, size_t end, PerChunk per_chunk) {
    if (end == 0) return GK_OK;
    const size_t cap = ctx->hook_max_stage > 0 ? (size_t)ctx->hook_max_stage : (size_t)704 << 20;
    const size_t area = std::min(cap + 260, end) + 64;
    uint8_t *d_area[2] = {nullptr, nullptr};
    uint32_t *d_off = nullptr;
    size_t off_cap = 0;
    auto run = [&]() -> int {
        GK_HIP(ctx, tmp.get(&d_area[0], area));
        BinPiece cur = bin_cut(bin, end, 0, cap);
        GK_HIP(ctx, hipMemcpyAsync(d_area[0], bin, cur.bytes, hipMemcpyHostToDevice, ctx->stream));
        for (int i = 0; cur.bytes; i ^= 1) {
            BinPiece nxt;
            if (cur.begin + cur.bytes < end) nxt = bin_cut(bin, end, cur.begin + cur.bytes, cap);
            if (cur.offs.size() > off_cap) {
                if (d_off) tmp.release(d_off);
                GK_HIP(ctx, tmp.get(&d_off, cur.offs.size()));
                off_cap = cur.offs.size();
            }
            GK_HIP(ctx, hipMemcpyAsync(d_off, cur.offs.data(), cur.offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            // (the host has walked this framing: every length byte is what the offsets say)
            D2H back{nullptr, nullptr, 0};
            if (int rc = per_chunk(ReadSrc::framed(d_area[i], d_off, cur.offs.size() - 1), d_area[i], cur, &back)) return rc;
            if (nxt.bytes) {
                if (!d_area[i ^ 1]) GK_HIP(ctx, tmp.get(&d_area[i ^ 1], area));
                GK_HIP(ctx, hipMemcpyAsync(d_area[i ^ 1], bin + nxt.begin, nxt.bytes, hipMemcpyHostToDevice, ctx->copy_stream));
                GK_HIP(ctx, hipEventRecord(ctx->cev[0], ctx->copy_stream));
            }
            GK_HIP(ctx, read_back(ctx, {back}));
            if (nxt.bytes) GK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->cev[0], 0));
            cur = std::move(nxt);
        }
        return GK_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->copy_stream);            // (the areas go back to the pool, which does not wait for uploads)
    return rc;
}

}  // namespace gk
