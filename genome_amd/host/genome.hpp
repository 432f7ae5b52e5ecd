// genome.hpp — C++ host side above the C-ABI (include/genome_amd.h), mirroring the reference's
// Scala interface for the hot path name for name (the image has no JVM, so the host side is C++;
// the JNI stub + Scala adapter a maintainer would add are in INTEGRATION.md).
//
//   trait DNAMap[T]                       S/ds/ArrayDNAMap.scala:49-60      -> genome::DNAMap (T = Int)
//   FreqFilter.extractFilteredKmers       S/data/FreqFilter.scala:25-58     -> genome::FreqFilter::extractFilteredKmers
//   Graph.buildGraph / trait Graph        S/data/graph/Graph.scala:23-150,269-382 -> genome::Graph
//   PairedEndData                         S/data/PairedEndData.scala:11-36  -> genome::PairedEndData
//   PartitionedDNAMap                     S/ds/PartitionedDNAMap.scala:15-64 -> genome::PartitionedDNAMap (one rank per GPU, RCCL)
//
// Header-only, C++17, links against libgenome_amd.so.  Errors are exceptions (GkError) carrying the
// C-ABI status and message; a wrong key length throws KeyLengthError, the analogue of the
// reference's AssertionError (ArrayDNAMap.scala:182).  No CPU fallback: without a GPU the
// Context constructor throws.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <optional>
#include <ostream>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/genome_amd.h"

namespace genome {

struct GkError : std::runtime_error {
    int code;
    GkError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct KeyLengthError : GkError {
    using GkError::GkError;
};

inline void check(int rc, const gk_ctx *ctx) {
    if (rc == GK_OK) return;
    std::string msg = gk_last_error(ctx);
    if (rc == GK_E_KLEN) throw KeyLengthError(rc, msg);
    throw GkError(rc, msg);
}

// S/dna/Base.scala:13-19 + S/dna/DNASeq.scala:74-215: a sequence of <= 64 bases, base i at bits 2i.
struct DNASeq {
    uint64_t lo = 0, hi = 0;
    int len = 0;
    static int code(char c) {
        switch (c) { case 'A': return 0; case 'G': return 1; case 'C': return 2; case 'T': return 3; }
        throw std::invalid_argument(std::string("not a base: ") + c);
    }
    static DNASeq fromString(const std::string &s) {
        if (s.size() > 64) throw std::invalid_argument("DNASeq longer than 64 bases");
        DNASeq r;
        r.len = (int)s.size();
        for (int i = 0; i < r.len; i++) (i < 32 ? r.lo : r.hi) |= (uint64_t)code(s[i]) << (2 * (i % 32));
        return r;
    }
    int apply(int i) const { return (int)(((i < 32 ? lo : hi) >> (2 * (i % 32))) & 3); }
    std::string toString() const {
        std::string s(len, 'A');
        for (int i = 0; i < len; i++) s[i] = "AGCT"[apply(i)];
        return s;
    }
    DNASeq revComplement() const {     // DNASeq.scala:27-28
        std::string s = toString(), r(s.rbegin(), s.rend());
        for (auto &c : r) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'G' ? 'C' : 'G';
        return fromString(r);
    }
    bool operator==(const DNASeq &o) const { return len == o.len && lo == o.lo && hi == o.hi; }
    bool operator<(const DNASeq &o) const { return std::tie(hi, lo) < std::tie(o.hi, o.lo); }
};

// replaces ActorsHome.system (S/scripts/ActorsHome.scala:20-30)
class Context {
  public:
    explicit Context(int device = 0) { check(gk_ctx_create(device, &h_), nullptr); }
    ~Context() { gk_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    gk_ctx *handle() const { return h_; }
    void trim() { check(gk_ctx_trim(h_), h_); }        // device buffers parked in the context's pool go back to the device

  private:
    gk_ctx *h_ = nullptr;
};

// S/data/PairedEndData.scala:11-36: `count` pairs in a `.bin` record stream, two records per pair.
struct PairedEndData {
    uint64_t count = 0;
    int insert = 0;
    std::vector<uint8_t> bin;
    // Convert2bin (S/scripts/Convert2bin.scala) on the GPU straight into memory: the `.bin` stream and the pair count of a FASTQ
    // file (plain text; splitAt = Convert2bin's n, 0 = interleaved).  Defined after FastqReader.
    static PairedEndData fromFastq(Context &ctx, const std::string &path, int splitAt = 36);
};

// gk_fastq: FASTQ text -> `.bin` records on the GPU, fed in pieces of any size (the rules: include/genome_amd.h, "FASTQ")
class FastqReader {
  public:
    struct Stats { uint64_t pairs = 0, shortPairs = 0, kmers = 0, textBytes = 0, carriedBytes = 0; };
    explicit FastqReader(Context &ctx, int splitAt = 36, int kStats = 23, uint64_t maxPairs = 0) : ctx_(ctx.handle()) {
        check(gk_fastq_create(ctx_, splitAt, kStats, maxPairs, &h_), ctx_);
    }
    ~FastqReader() { gk_fastq_destroy(h_); }
    FastqReader(const FastqReader &) = delete;
    FastqReader &operator=(const FastqReader &) = delete;
    // appends the records of every pair this piece completes to `out` (last: the input ends with this piece)
    void convert(const char *text, size_t n, bool last, std::vector<uint8_t> &out) {
        const size_t old = out.size(), cap = stats().carriedBytes + n;
        out.resize(old + cap);
        size_t w = 0;
        const int rc = gk_fastq_convert(h_, text, n, last ? 1 : 0, out.data() + old, cap, &w);
        out.resize(old + w);
        check(rc, ctx_);
    }
    Stats stats() const {
        Stats s;
        check(gk_fastq_stats(h_, &s.pairs, &s.shortPairs, &s.kmers, &s.textBytes, &s.carriedBytes), ctx_);
        return s;
    }
    gk_fastq *handle() const { return h_; }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_fastq *h_ = nullptr;
};

// the file's bytes in pieces of `piece` bytes, each handed to f(data, n, last)
template <class F>
inline void forEachPiece(const std::string &path, size_t piece, F f) {
    FILE *fp = std::fopen(path.c_str(), "rb");
    if (!fp) throw GkError(GK_E_INVALID, "cannot open " + path);
    std::vector<char> a(piece), b(piece);
    size_t na = std::fread(a.data(), 1, piece, fp);
    for (;;) {
        const size_t nb = na == piece ? std::fread(b.data(), 1, piece, fp) : 0;
        if (std::ferror(fp)) { std::fclose(fp); throw GkError(GK_E_INVALID, "cannot read " + path); }
        try { f(a.data(), na, nb == 0); } catch (...) { std::fclose(fp); throw; }
        if (nb == 0) break;
        a.swap(b);
        na = nb;
    }
    std::fclose(fp);
}

inline PairedEndData PairedEndData::fromFastq(Context &ctx, const std::string &path, int splitAt) {
    PairedEndData d;
    FastqReader rd(ctx, splitAt);
    forEachPiece(path, 64u << 20, [&](const char *p, size_t n, bool last) { rd.convert(p, n, last, d.bin); });
    d.count = rd.stats().pairs;
    return d;
}

// Sharing the pairs out over N ranks: rank `rank` of `world` takes the pairs [n * rank / world, n * (rank + 1) / world) of the
// first n = min(takeFirst, count) — the same range for the count and for the walks.
inline std::pair<uint64_t, uint64_t> pairShare(uint64_t count, uint64_t takeFirst, int rank, int world) {
    if (world < 1 || rank < 0 || rank >= world) throw GkError(GK_E_INVALID, "pairShare: need 0 <= rank < world");
    const unsigned __int128 n = std::min(count, takeFirst);
    return {(uint64_t)(n * (unsigned)rank / (unsigned)world), (uint64_t)(n * (unsigned)(rank + 1) / (unsigned)world)};
}
// byte range [first, end) of pairs [firstPair, endPair) of a `.bin` stream of mate records (two per pair), by walking its framing
inline std::pair<size_t, size_t> pairBytes(const PairedEndData &data, uint64_t firstPair, uint64_t endPair) {
    if (firstPair > endPair) throw GkError(GK_E_INVALID, "pairBytes: firstPair > endPair");
    size_t pos = 0, first = 0;
    for (uint64_t rec = 0; rec < 2 * endPair; rec++) {
        if (rec == 2 * firstPair) first = pos;
        if (pos >= data.bin.size()) throw GkError(GK_E_FORMAT, "the stream ends before pair " + std::to_string(rec / 2));
        pos += 1 + ((size_t)data.bin[pos] + 3) / 4;
        if (pos > data.bin.size()) throw GkError(GK_E_FORMAT, "the stream ends inside pair " + std::to_string(rec / 2));
    }
    return {firstPair == endPair ? pos : first, pos};
}

// the two closures the hot path passes to DNAMap
struct PlusOne {};                 // `_ + 1`            FreqFilter.scala:33
struct ValueLessThan { int rounds; };   // `(k, v) => v < rounds`   FreqFilter.scala:55

// A k-mer count spectrum (gk_map_spectrum / gk_dist_spectrum) and the deleteAll cutoff it suggests (gk_spectrum_cutoff: pure host
// code).  valley == 0: the spectrum has no valley — callers fall back to the reference's rounds = 3 (GraphBuilder.scala:30).
struct Spectrum {
    std::vector<uint64_t> hist;
    uint64_t distinct = 0, occurrences = 0;
    uint32_t maxCount = 0;
};
struct SpectrumCutoff { uint32_t valley = 0, peak = 0; uint64_t genomeSize = 0; };
// minCount: 1 normally; 2 for a table counted through the singleton pre-filter, whose bin 1 is incomplete by construction
inline SpectrumCutoff spectrumCutoff(const std::vector<uint64_t> &hist, uint32_t minCount = 1) {
    SpectrumCutoff c;
    check(gk_spectrum_cutoff(hist.data(), (uint32_t)hist.size(), minCount, &c.valley, &c.peak, &c.genomeSize), nullptr);
    return c;
}

class Graph;
// trait DNAMap[Int] over one HBM-resident partition (ArrayDNAMap.scala:49-60, 62-243)
class DNAMap {
  public:
    DNAMap(Context &ctx, int k, uint64_t capacityHint = 0) : ctx_(ctx), k_(k) { check(gk_map_create(ctx.handle(), k, capacityHint, &h_), ctx.handle()); }
    ~DNAMap() { gk_map_destroy(h_); }
    DNAMap(const DNAMap &) = delete;
    DNAMap &operator=(const DNAMap &) = delete;
    DNAMap(DNAMap &&o) noexcept : ctx_(o.ctx_), k_(o.k_), h_(o.h_) { o.h_ = nullptr; }
    // adopt a handle the library created (gk_dist_gather_map)
    DNAMap(Context &ctx, int k, gk_map *adopted) : ctx_(ctx), k_(k), h_(adopted) {}

    int k() const { return k_; }
    gk_map *handle() const { return h_; }
    Context &context() const { return ctx_; }

    uint64_t size() const {                                        // :50
        uint64_t n = 0;
        check(gk_map_size(h_, &n), ctx_.handle());
        return n;
    }
    std::optional<int32_t> apply(const DNASeq &key) const {        // :51
        requireLen(key);
        int32_t v = -1;
        check(gk_map_get_batch(h_, &key.lo, &key.hi, 1, &v, nullptr), ctx_.handle());
        return v < 0 ? std::nullopt : std::optional<int32_t>(v);
    }
    bool contains(const DNASeq &key) const { return apply(key).has_value(); }   // :57
    void update(const DNASeq &key, int32_t v0, PlusOne) {          // :54 update(key, 1, _ + 1)
        requireLen(key);
        if (v0 != 1) throw GkError(GK_E_INVALID, "only update(key, 1, _ + 1) is a fused GPU form");
        check(gk_map_update_inc(h_, &key.lo, &key.hi, 1), ctx_.handle());
    }
    void updateAll(const std::vector<DNASeq> &keys, int32_t v0, PlusOne p) {   // batched form of the above
        (void)p;
        if (v0 != 1) throw GkError(GK_E_INVALID, "only update(key, 1, _ + 1) is a fused GPU form");
        std::vector<uint64_t> lo(keys.size()), hi(keys.size());
        for (size_t i = 0; i < keys.size(); i++) { requireLen(keys[i]); lo[i] = keys[i].lo; hi[i] = keys[i].hi; }
        check(gk_map_update_inc(h_, lo.data(), hi.data(), keys.size()), ctx_.handle());
    }
    void deleteAll(ValueLessThan p) { check(gk_map_filter_lt(h_, p.rounds), ctx_.handle()); }   // :56
    // :58-59 mapReduce / foreach: the table comes back to the host and `f` runs there
    void foreach(const std::function<void(const DNASeq &, int32_t)> &f) const {
        uint64_t n = size(), got = 0;
        std::vector<uint64_t> lo(n), hi(n);
        std::vector<int32_t> cnt(n);
        check(gk_map_export(h_, lo.data(), hi.data(), cnt.data(), n, &got), ctx_.handle());
        for (uint64_t i = 0; i < got; i++) f(DNASeq{lo[i], hi[i], k_}, cnt[i]);
    }
    // FreqFilter.add over a record stream (FreqFilter.scala:28-36, 44-48)
    uint64_t countReads(const uint8_t *bin, size_t nbytes, uint64_t nreads) {
        uint64_t occ = 0;
        check(gk_map_count_reads(h_, bin, nbytes, nreads, &occ), ctx_.handle());
        return occ;
    }
    // the count spectrum, taken on the device (gk_map_spectrum): hist[c] = keys seen exactly c times, the last bin = keys seen
    // bins - 1 times and more; the table is not changed
    Spectrum spectrum(uint32_t bins = 4096) const {
        Spectrum s;
        s.hist.assign(bins, 0);
        check(gk_map_spectrum(h_, s.hist.data(), bins, &s.distinct, &s.occurrences, &s.maxCount), ctx_.handle());
        return s;
    }
    // spectral read correction (gk_reads_correct: this project's own rule, include/genome_amd.h): the bases of `bin` under a run of
    // weak k-mers (count < solid in this table) are replaced where exactly one replacement makes the run solid.  `out` holds
    // nbytes and may be `bin`.  The table is not changed.
    struct CorrectStats {
        uint64_t v[GK_CORRECT_NSTATS] = {};
        uint64_t operator[](int i) const { return v[i]; }
        // {"reads": .., "short": .., ...} in the order of the GK_CORRECT_* indices
        std::string json() const {
            static const char *names[GK_CORRECT_NSTATS] = {"reads", "short", "windows", "weak_windows", "weak_runs", "corrected", "ambiguous", "unresolved",
                                                           "skipped", "reads_changed"};
            std::string s = "{";
            for (int i = 0; i < GK_CORRECT_NSTATS; i++) s += std::string(i ? ", \"" : "\"") + names[i] + "\": " + std::to_string(v[i]);
            return s + "}";
        }
    };
    CorrectStats correctReads(const uint8_t *bin, size_t nbytes, uint64_t nreads, uint32_t solid, uint8_t *out) const {
        CorrectStats st;
        check(gk_reads_correct(h_, bin, nbytes, nreads, solid, out, st.v), ctx_.handle());
        return st;
    }
    void clear() { check(gk_map_clear(h_), ctx_.handle()); }       // back to an empty table of the same capacity
    // multi-k seeding (gk_map_add_graph_paths; include/genome_amd.h, "multi-k"): every window of this map's k of every contig of
    // `graph` (a smaller k; one strand per contig) is added `weight` times, oriented as a read's window is; the graph is not changed
    struct GraphPathStats { uint64_t v[6] = {}; };            // gk_map_add_graph_paths' stats6
    static constexpr const char *graphPathStatNames[6] = {"live_edges", "short", "forward", "self_twin", "reverse", "windows"};
    GraphPathStats addGraphPaths(const Graph &graph, uint32_t weight);      // (defined behind Graph)
    // the table's invariants and an order-independent content checksum (gk_map_verify)
    struct Verify { uint64_t live, bad, sumCounts, checksum; };
    Verify verify() const {
        Verify v{};
        check(gk_map_verify(h_, &v.live, &v.bad, &v.sumCounts, &v.checksum), ctx_.handle());
        return v;
    }

  private:
    void requireLen(const DNASeq &key) const {                     // assert(key.length == k)  :182
        if (key.len != k_) throw KeyLengthError(GK_E_KLEN, "key length " + std::to_string(key.len) + " != k=" + std::to_string(k_));
    }
    Context &ctx_;
    int k_;
    gk_map *h_ = nullptr;
};

// One rank's view of a PartitionedDNAMap[Int] spread over the GPUs of a node (PartitionedDNAMap.scala:15-64): this rank's
// partition (an ordinary DNAMap on this rank's device) + the RCCL communicator.  One process per GPU; rank 0 obtains the id
// with PartitionedDNAMap::uniqueId() and hands it to the others through whatever channel the host program has.
// Every member that moves data is COLLECTIVE.  Owner of a k-mer = strand-symmetric minimizer hash mod world (gk_owner_of),
// not `hashCode mod P` (:60-63): the partition function is unobservable in results and keeps x and rc(x) together.
class Graph;
class Support;
class Links;
class Spans;
class PartitionedDNAMap {
  public:
    static std::vector<uint8_t> uniqueId() {
        std::vector<uint8_t> id(128);
        check(gk_dist_unique_id(id.data()), nullptr);
        return id;
    }
    PartitionedDNAMap(Context &ctx, int k, int rank, int world, const std::vector<uint8_t> &id128, uint64_t capacityHintPerRank = 0)
        : ctx_(ctx), local_(ctx, k, capacityHintPerRank) {
        if (id128.size() != 128) throw GkError(GK_E_INVALID, "the RCCL id is 128 bytes");
        check(gk_dist_create(ctx.handle(), rank, world, id128.data(), &d_), ctx.handle());
    }
    ~PartitionedDNAMap() { gk_dist_destroy(d_); }
    PartitionedDNAMap(const PartitionedDNAMap &) = delete;
    PartitionedDNAMap &operator=(const PartitionedDNAMap &) = delete;

    int rank() const { return gk_dist_rank(d_); }
    int world() const { return gk_dist_world(d_); }
    DNAMap &local() { return local_; }
    // FreqFilter.add over THIS rank's device-resident reads: update(key, 1, _ + 1) sent to each key's owner (:41-43)
    std::pair<uint64_t, uint64_t> countReadsDev(const void *devRecords, uint64_t nreads, int readLen) {
        uint64_t sent = 0, owned = 0;
        check(gk_dist_count_reads_dev(d_, local_.handle(), devRecords, nreads, readLen, &sent, &owned), ctx_.handle());
        return {sent, owned};
    }
    // FreqFilter.add over pairs [firstPair, endPair) of a host `.bin` stream (ragged mates allowed): chunked, uploaded and routed
    // inside the library (gk_dist_count_reads).  A malformed stream on any rank throws GK_E_FORMAT on every rank, nothing counted.
    std::pair<uint64_t, uint64_t> countReads(const PairedEndData &data, uint64_t firstPair, uint64_t endPair) {
        const auto [b0, b1] = pairBytes(data, firstPair, endPair);
        uint64_t sent = 0, owned = 0;
        check(gk_dist_count_reads(d_, local_.handle(), data.bin.data() + b0, b1 - b0, 2 * (endPair - firstPair), &sent, &owned), ctx_.handle());
        return {sent, owned};
    }
    // the same in two halves for a streaming loop: routeBegin(batch i+1), and routeBegin(batch i+2) for the exchange to run
    // ahead as well, before countRouted() of batch i (at most three begun)
    void routeBegin(const void *devRecords, uint64_t nreads, int readLen) {
        check(gk_dist_route_begin(d_, local_.k(), devRecords, nreads, readLen), ctx_.handle());
    }
    std::pair<uint64_t, uint64_t> countRouted() {
        uint64_t sent = 0, owned = 0;
        check(gk_dist_count_routed(d_, local_.handle(), &sent, &owned), ctx_.handle());
        return {sent, owned};
    }
    uint64_t size() {                                              // :31
        uint64_t n = 0;
        check(gk_dist_size(d_, local_.handle(), &n), ctx_.handle());
        return n;
    }
    // the count spectrum of the WHOLE map on every rank (gk_dist_spectrum): collective
    Spectrum spectrum(uint32_t bins = 4096) {
        Spectrum s;
        s.hist.assign(bins, 0);
        check(gk_dist_spectrum(d_, local_.handle(), s.hist.data(), bins, &s.distinct, &s.occurrences, &s.maxCount), ctx_.handle());
        return s;
    }
    void deleteAll(ValueLessThan p) { local_.deleteAll(p); }      // :49-51 — every partition filters its own keys
    // every partition's keys in one table on this rank: what Graph.buildGraph needs.  classified: the keys' owners
    // classify them first (Graph.scala:320-329 on every partition, :55-58) and the degree masks travel with the keys
    DNAMap gathered(bool classified = false) {
        gk_map *full = nullptr;
        check(classified ? gk_dist_gather_classified_map(d_, local_.handle(), &full) : gk_dist_gather_map(d_, local_.handle(), &full), ctx_.handle());
        return DNAMap(ctx_, local_.k(), full);
    }
    void barrier() { check(gk_dist_barrier(d_), ctx_.handle()); }
    // every rank's support (its share of the pairs walked on its replica) becomes the sum over all ranks (gk_dist_reduce_support)
    void reduceSupport(Graph &graph, Support &support);
    // every rank's link table (pairLinks of its share of the pairs on its replica) / span table (threadSpans of its share of the
    // reads) becomes the sum over all ranks, keyed by this rank's edge ids (gk_dist_reduce_links / gk_dist_reduce_spans).  The graph
    // may be an edited one: the records travel in a numbering of the edges by path content.  COLLECTIVE; on any failure every rank
    // throws and every table is unchanged.
    void reduceLinks(Graph &graph, Links &links);
    void reduceSpans(Graph &graph, Spans &spans);
    gk_dist *distHandle() const { return d_; }

  private:
    Context &ctx_;
    DNAMap local_;
    gk_dist *d_ = nullptr;
};

namespace FreqFilter {
// Asking extractFilteredKmers for more than a number: autoRounds = take the cutoff from the count spectrum of the counted table
// (its valley; 3 when there is none) instead of `rounds`; wantSpectrum = take the spectrum although `rounds` is used.  Filled
// in on return: the spectrum before deleteAll, the cutoff it suggests, the rounds used, and autoFound (asked for auto and the
// spectrum had a valley).  Without a Chosen, or with both flags false, nothing changes and no spectrum is taken.
struct Chosen {
    bool autoRounds = false, wantSpectrum = false;
    Spectrum spectrum;
    SpectrumCutoff cutoff;
    bool autoFound = false;
    int rounds = 0;
};
template <class Map> inline int chooseRounds(Map &kmersFreq, int rounds, uint32_t minCount, Chosen *chosen) {
    if (!chosen || !(chosen->autoRounds || chosen->wantSpectrum)) return rounds;
    chosen->spectrum = kmersFreq.spectrum();
    chosen->cutoff = spectrumCutoff(chosen->spectrum.hist, minCount);
    chosen->autoFound = chosen->autoRounds && chosen->cutoff.valley != 0;
    if (chosen->autoRounds) rounds = chosen->autoFound ? (int)chosen->cutoff.valley : 3;
    chosen->rounds = rounds;
    return rounds;
}
// FreqFilter.extractFilteredKmers(data, k, rounds) (FreqFilter.scala:25-58); `takeFirst` is
// genome.takeFirst (:40, :44)
// prefilterDistinct > 0 (rounds >= 2 only): the exact two-pass singleton pre-filter sized for that many
// distinct k-mers runs first (include/genome_amd.h); same result, k-mers seen once take no table slot
// chosen->autoRounds: the cutoff is the valley of the table's count spectrum (chooseRounds; min_count = 2 behind the pre-filter)
// beforeFilter(table, rounds): called between the count and deleteAll, with the rounds that will be used
inline DNAMap extractFilteredKmers(Context &ctx, const PairedEndData &data, int k, int rounds,
                                   uint64_t takeFirst = UINT64_MAX, uint64_t capacityHint = 0, uint64_t prefilterDistinct = 0,
                                   Chosen *chosen = nullptr, const std::function<void(DNAMap &, int)> &beforeFilter = {}) {
    DNAMap kmersFreq(ctx, k, capacityHint);
    const uint64_t pairs = std::min<uint64_t>(data.count, takeFirst);
    if (prefilterDistinct) {
        if (rounds < 2 && !(chosen && chosen->autoRounds)) throw GkError(GK_E_INVALID, "the singleton pre-filter needs rounds >= 2");
        gk_prefilter *pf = nullptr;
        check(gk_prefilter_create(ctx.handle(), k, prefilterDistinct, &pf), ctx.handle());
        int rc = gk_prefilter_add_reads(pf, data.bin.data(), data.bin.size(), 2 * pairs);
        if (rc == GK_OK) rc = gk_map_count_reads_prefiltered(kmersFreq.handle(), pf, data.bin.data(), data.bin.size(), 2 * pairs, nullptr, nullptr);
        gk_prefilter_destroy(pf);
        check(rc, ctx.handle());
    } else {
        kmersFreq.countReads(data.bin.data(), data.bin.size(), 2 * pairs);
    }
    rounds = chooseRounds(kmersFreq, rounds, prefilterDistinct ? 2 : 1, chosen);
    if (prefilterDistinct && rounds < 2) rounds = 2;       // (auto only: a number below 2 was refused above)
    if (beforeFilter) beforeFilter(kmersFreq, rounds);     // (multi-k: the seeds go in behind the choice of rounds — they would move the valley)
    kmersFreq.deleteAll(ValueLessThan{rounds});
    return kmersFreq;
}
// the same over N ranks: this rank counts its share of the first min(takeFirst, count) pairs (pairShare) into its partition and
// filters it; every partition then holds its owned k-mers seen at least `rounds` times -> (windows sent, windows counted as owner)
// (chosen->autoRounds: the valley of the REDUCED spectrum, so that every rank filters alike)
inline std::pair<uint64_t, uint64_t> extractFilteredKmers(PartitionedDNAMap &kmersFreq, const PairedEndData &data, int rounds,
                                                          uint64_t takeFirst = UINT64_MAX, Chosen *chosen = nullptr) {
    const auto [a, b] = pairShare(data.count, takeFirst, kmersFreq.rank(), kmersFreq.world());
    const auto occ = kmersFreq.countReads(data, a, b);
    rounds = chooseRounds(kmersFreq, rounds, 1, chosen);
    kmersFreq.deleteAll(ValueLessThan{rounds});
    return occ;
}
}  // namespace FreqFilter

// DNAMap[GraphPosition] — the multimap Graph.getGraphMap fills (Graph.scala:90-119); values are GK_POS_* encoded
class PositionMap {
  public:
    PositionMap(Context &ctx, int k, uint64_t capacityHint = 0) : ctx_(ctx) { check(gk_vmap_create(ctx.handle(), k, capacityHint, &h_), ctx.handle()); }
    ~PositionMap() { gk_vmap_destroy(h_); }
    PositionMap(PositionMap &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    PositionMap(const PositionMap &) = delete;
    gk_vmap *handle() const { return h_; }
    uint64_t size() const { uint64_t n = 0; check(gk_vmap_size(h_, &n), ctx_.handle()); return n; }

  private:
    Context &ctx_;
    gk_vmap *h_ = nullptr;
};

// gk_fasta_check: every k-window of a FASTA text looked up in a position map, fed in pieces of any size (the rules:
// include/genome_amd.h, "FASTA check")
class FastaCheck {
  public:
    struct Stats { uint64_t lines = 0, records = 0, bases = 0, validBases = 0, windows = 0, found = 0, missing = 0, coveredBases = 0, shortLines = 0; };
    struct Missing { uint64_t offset, line, column, lo, hi; };
    FastaCheck(Context &ctx, PositionMap &positions, bool perLine = false, uint64_t maxMissing = 0) : ctx_(ctx.handle()) {
        check(gk_fasta_check_create(ctx_, positions.handle(), perLine ? 1 : 0, maxMissing, &h_), ctx_);
    }
    ~FastaCheck() { gk_fasta_check_destroy(h_); }
    FastaCheck(const FastaCheck &) = delete;
    FastaCheck &operator=(const FastaCheck &) = delete;
    void feed(const char *text, size_t n, bool last) { check(gk_fasta_check_feed(h_, text, n, last ? 1 : 0), ctx_); }
    Stats stats() const {
        Stats s;
        check(gk_fasta_check_stats(h_, &s.lines, &s.records, &s.bases, &s.validBases, &s.windows, &s.found, &s.missing, &s.coveredBases, &s.shortLines), ctx_);
        return s;
    }
    std::vector<Missing> missing() const {                                          // the first maxMissing not-found windows, in stream order
        uint64_t n = 0;
        check(gk_fasta_check_missing(h_, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n), ctx_);
        std::vector<uint64_t> a(5 * n);
        if (n) check(gk_fasta_check_missing(h_, a.data(), a.data() + n, a.data() + 2 * n, a.data() + 3 * n, a.data() + 4 * n, n, &n), ctx_);
        std::vector<Missing> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = Missing{a[i], a[n + i], a[2 * n + i], a[3 * n + i], a[4 * n + i]};
        return out;
    }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_fasta_check *h_ = nullptr;
};

// pathsMap + badPairs of GraphSimplifier.scala:209-211
class Support {
  public:
    explicit Support(Context &ctx) : ctx_(ctx) { check(gk_support_create(ctx.handle(), &h_), ctx.handle()); }
    ~Support() { gk_support_destroy(h_); }
    Support(const Support &) = delete;
    gk_support *handle() const { return h_; }
    // -> (supported edge pairs, bad pairs, pair orientations walked)
    std::tuple<uint64_t, uint64_t, uint64_t> sizes() const {
        uint64_t a = 0, b = 0, c = 0;
        check(gk_support_size(h_, &a, &b, &c), ctx_.handle());
        return {a, b, c};
    }
    // add (e1, e2, count) triples (duplicates add up) and the two counters; throws (nothing added) if a count would pass 2^32-1
    void add(const std::vector<uint32_t> &e1, const std::vector<uint32_t> &e2, const std::vector<uint32_t> &count, uint64_t badPairs = 0,
             uint64_t walked = 0) {
        if (e1.size() != e2.size() || e1.size() != count.size()) throw GkError(GK_E_INVALID, "Support::add: the three lists differ in length");
        check(gk_support_add(h_, e1.data(), e2.data(), count.data(), e1.size(), badPairs, walked), ctx_.handle());
    }
    // *this += other on the device (the supports of two walks on one GPU); other is unchanged
    void merge(const Support &other) { check(gk_support_merge(h_, other.h_), ctx_.handle()); }

  private:
    Context &ctx_;
    gk_support *h_ = nullptr;
};

// gk_links: scaffold links (include/genome_amd.h, "scaffold links"): (edge id, edge id) -> the pair orientations whose mates lie on
// the two edges and the sum of the bases those fragments need on them.  Filled by Graph::pairLinks; meaningless after a graph edit.
class Links {
  public:
    struct Records { std::vector<uint32_t> e1, e2, count; std::vector<uint64_t> sumU; };
    struct JoinStats { uint64_t v[5] = {}; };     // links, supported, joins, forks, merges
    static constexpr const char *joinStatNames[5] = {"links", "supported", "joins", "forks", "merges"};
    explicit Links(Context &ctx) : ctx_(ctx) { check(gk_links_create(ctx.handle(), &h_), ctx.handle()); }
    ~Links() { gk_links_destroy(h_); }
    Links(const Links &) = delete;
    gk_links *handle() const { return h_; }
    // -> (distinct links, the sum of their counts)
    std::pair<uint64_t, uint64_t> size() const {
        uint64_t a = 0, b = 0;
        check(gk_links_size(h_, &a, &b), ctx_.handle());
        return {a, b};
    }
    // every link, unordered
    Records exportAll() const {
        Records r;
        uint64_t n = size().first;
        r.e1.resize(n); r.e2.resize(n); r.count.resize(n); r.sumU.resize(n);
        check(gk_links_export(h_, r.e1.data(), r.e2.data(), r.count.data(), r.sumU.data(), n, &n), ctx_.handle());
        return r;
    }
    // add records (duplicates add up); throws (nothing added) if a count would pass 2^32-1
    void add(const Records &r) {
        if (r.e1.size() != r.e2.size() || r.e1.size() != r.count.size() || r.e1.size() != r.sumU.size())
            throw GkError(GK_E_INVALID, "Links::add: the four lists differ in length");
        check(gk_links_add(h_, r.e1.data(), r.e2.data(), r.count.data(), r.sumU.data(), r.e1.size()), ctx_.handle());
    }
    // the links that are the only supported one (count >= minSupport) out of their first edge and into their second, ascending e1
    Records joins(uint32_t minSupport, JoinStats *stats = nullptr) const {
        Records r;
        uint64_t n = 0;
        const int rc = gk_links_joins(h_, minSupport, nullptr, nullptr, nullptr, nullptr, 0, &n, nullptr);
        if (rc != GK_OK && rc != GK_E_CAPACITY) check(rc, ctx_.handle());
        r.e1.resize(n); r.e2.resize(n); r.count.resize(n); r.sumU.resize(n);
        check(gk_links_joins(h_, minSupport, r.e1.data(), r.e2.data(), r.count.data(), r.sumU.data(), n, &n, stats ? stats->v : nullptr), ctx_.handle());
        return r;
    }

  private:
    Context &ctx_;
    gk_links *h_ = nullptr;
};

// gk_spans: reads followed across a whole edge (include/genome_amd.h, "spans"): (in-edge, edge, out-edge) -> how often a read crossed
// the edge from end to end by those two.  Filled by Graph::threadSpans, read by Graph::splitEdgesBySpans; the ids are the graph's
// at the time of the call.
class Spans {
  public:
    struct Records { std::vector<uint32_t> e, m, f, count; };
    explicit Spans(Context &ctx) : ctx_(ctx) { check(gk_spans_create(ctx.handle(), &h_), ctx.handle()); }
    ~Spans() { gk_spans_destroy(h_); }
    Spans(const Spans &) = delete;
    gk_spans *handle() const { return h_; }
    // -> (distinct triples, the sum of their counts)
    std::pair<uint64_t, uint64_t> size() const {
        uint64_t a = 0, b = 0;
        check(gk_spans_size(h_, &a, &b), ctx_.handle());
        return {a, b};
    }
    // every triple, unordered
    Records exportAll() const {
        Records r;
        uint64_t n = 0;
        check(gk_spans_size(h_, &n, nullptr), ctx_.handle());                       // the triples alone: a counter, no table pass
        r.e.resize(n); r.m.resize(n); r.f.resize(n); r.count.resize(n);
        check(gk_spans_export(h_, r.e.data(), r.m.data(), r.f.data(), r.count.data(), n, &n), ctx_.handle());
        return r;
    }
    // add records (duplicates add up); throws (nothing added) if a count would pass 2^32-1
    void add(const Records &r) {
        if (r.e.size() != r.m.size() || r.e.size() != r.f.size() || r.e.size() != r.count.size())
            throw GkError(GK_E_INVALID, "Spans::add: the four lists differ in length");
        check(gk_spans_add(h_, r.e.data(), r.m.data(), r.f.data(), r.count.data(), r.e.size()), ctx_.handle());
    }

  private:
    Context &ctx_;
    gk_spans *h_ = nullptr;
};

// gk_scaffold_chains over a join list: the chains as lists of edge ids in ascending order of first member; *cycles = how many of
// them are cycles (a cycle starts at its smallest id).  Host code: no context, no GPU.
inline std::vector<std::vector<uint32_t>> scaffoldChains(const std::vector<uint32_t> &e1, const std::vector<uint32_t> &e2, uint64_t *cycles = nullptr) {
    if (e1.size() != e2.size()) throw GkError(GK_E_INVALID, "scaffoldChains: the two lists differ in length");
    const uint64_t n = e1.size();
    std::vector<uint32_t> members(2 * n + 1);
    std::vector<uint64_t> off(n + 1);
    uint64_t nch = 0, ncy = 0;
    check(gk_scaffold_chains(e1.data(), e2.data(), n, members.data(), 2 * n, off.data(), n, &nch, &ncy), nullptr);
    std::vector<std::vector<uint32_t>> out(nch);
    for (uint64_t i = 0; i < nch; i++) out[i].assign(members.begin() + off[i], members.begin() + off[i + 1]);
    if (cycles) *cycles = ncy;
    return out;
}

// gk_contigs: a plan of the FASTA text of a graph's contigs (Graph::contigs; the rule: include/genome_amd.h, "contigs").  The text
// is emitted by the device when it is read or written.  The graph must outlive the plan; after any edit of the graph read / text
// / write throw GK_E_STATE and stats() still answers.
class Contigs {
  public:
    struct Stats {
        uint64_t liveEdges = 0, shortEdges = 0, forward = 0, selfTwin = 0, reverse = 0, records = 0, bases = 0, textBytes = 0, missingWindows = 0;
        std::string json() const {                           // the names of gk_contigs_stats' stats9
            const uint64_t v[9] = {liveEdges, shortEdges, forward, selfTwin, reverse, records, bases, textBytes, missingWindows};
            const char *names[9] = {"live_edges", "short", "forward", "self_twin", "reverse", "records", "bases", "text_bytes", "missing_windows"};
            std::string s = "{";
            for (int i = 0; i < 9; i++) s += std::string(i ? ",\"" : "\"") + names[i] + "\":" + std::to_string(v[i]);
            return s + "}";
        }
    };
    Contigs(gk_ctx *ctx, gk_contigs *h) : ctx_(ctx), h_(h) {}
    ~Contigs() { close(); }
    void close() { gk_contigs_destroy(h_); h_ = nullptr; }
    Contigs(Contigs &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Contigs(const Contigs &) = delete;
    Contigs &operator=(const Contigs &) = delete;
    Stats stats() const {
        uint64_t v[9] = {};
        check(gk_contigs_stats(h_, v), ctx_);
        return Stats{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
    }
    // bytes [offset, offset + n) of the text, fewer at its end
    std::string read(uint64_t offset, uint64_t n) {
        std::string out((size_t)n, '\0');
        uint64_t got = 0;
        check(gk_contigs_read(h_, offset, out.data(), n, &got), ctx_);
        out.resize((size_t)got);
        return out;
    }
    std::string text() { return read(0, stats().textBytes); }
    // the whole text to path, written aside and renamed onto it
    void write(const std::string &path) { check(gk_contigs_write(h_, path.c_str()), ctx_); }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_contigs *h_ = nullptr;
};

// gk_gfa: a plan of the GFA 1.0 text of a graph (Graph::gfa; the rule: include/genome_amd.h, "the graph as GFA").  As Contigs: the
// device emits the text when it is read or written, and an edit of the graph makes the plan stale.
class Gfa {
  public:
    struct Stats {
        uint64_t liveEdges = 0, segments = 0, folded = 0, pairs = 0, links = 0, mirrored = 0, bases = 0, textBytes = 0, missingWindows = 0;
        std::string json() const {                           // the names of gk_gfa_stats' stats9
            const uint64_t v[9] = {liveEdges, segments, folded, pairs, links, mirrored, bases, textBytes, missingWindows};
            const char *names[9] = {"live_edges", "segments", "folded", "pairs", "links", "mirrored", "bases", "text_bytes", "missing_windows"};
            std::string s = "{";
            for (int i = 0; i < 9; i++) s += std::string(i ? ",\"" : "\"") + names[i] + "\":" + std::to_string(v[i]);
            return s + "}";
        }
    };
    Gfa(gk_ctx *ctx, gk_gfa *h) : ctx_(ctx), h_(h) {}
    ~Gfa() { close(); }
    void close() { gk_gfa_destroy(h_); h_ = nullptr; }
    Gfa(Gfa &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Gfa(const Gfa &) = delete;
    Gfa &operator=(const Gfa &) = delete;
    Stats stats() const {
        uint64_t v[9] = {};
        check(gk_gfa_stats(h_, v), ctx_);
        return Stats{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
    }
    // bytes [offset, offset + n) of the text, fewer at its end
    std::string read(uint64_t offset, uint64_t n) {
        std::string out((size_t)n, '\0');
        uint64_t got = 0;
        check(gk_gfa_read(h_, offset, out.data(), n, &got), ctx_);
        out.resize((size_t)got);
        return out;
    }
    std::string text() { return read(0, stats().textBytes); }
    // the whole text to path, written aside and renamed onto it
    void write(const std::string &path) { check(gk_gfa_write(h_, path.c_str()), ctx_); }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_gfa *h_ = nullptr;
};

// gk_placements: where every edge of a graph lies on a reference genome (Graph::place; the rule: include/genome_amd.h,
// "placements").  Holds neither the graph nor the position map: both must outlive it, and an edit of the graph makes it stale.
class Placements {
  public:
    static constexpr const char *statNames[GK_PLACE_NSTATS] = {"records", "bases", "valid_bases", "windows", "fwd_absent", "fwd_repetitive", "fwd_at_node", "fwd_edge",
                                                               "rev_absent", "rev_repetitive", "rev_at_node", "rev_edge", "unplaced", "both_strands", "scattered",
                                                               "forward", "reverse", "forward_bases", "reverse_bases", "saturated"};
    struct Stats { uint64_t v[GK_PLACE_NSTATS] = {}; };
    struct Edges { std::vector<uint8_t> cls; std::vector<uint32_t> record; std::vector<int64_t> pos; std::vector<uint32_t> windowsFwd, windowsRev; };
    Placements(gk_ctx *ctx, gk_graph *g, gk_vmap *positions) : ctx_(ctx) { check(gk_placements_create(g, positions, &h_), ctx_); }
    ~Placements() { close(); }
    void close() { gk_placements_destroy(h_); h_ = nullptr; }
    Placements(Placements &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Placements(const Placements &) = delete;
    Placements &operator=(const Placements &) = delete;
    gk_placements *handle() const { return h_; }
    // the next reference record: its joined sequence characters
    void add(const std::string &record) { check(gk_placements_add_record(h_, record.data(), record.size()), ctx_); }
    Stats stats() const {
        Stats st;
        check(gk_placements_stats(h_, st.v), ctx_);
        return st;
    }
    Edges edges(const std::vector<uint32_t> &ids) const {
        Edges e;
        const size_t n = ids.size();
        e.cls.resize(n); e.record.resize(n); e.pos.resize(n); e.windowsFwd.resize(n); e.windowsRev.resize(n);
        check(gk_placements_edges(h_, ids.data(), n, e.cls.data(), e.record.data(), e.pos.data(), e.windowsFwd.data(), e.windowsRev.data()), ctx_);
        return e;
    }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_placements *h_ = nullptr;
};

// gk_blocks: every edge of a graph aligned to a reference genome as exact runs, and the breakpoints between them (Graph::alignBlocks;
// the rules: include/genome_amd.h, "alignment blocks" and "breakpoints").  Feed the records, finish(tol) once or several times,
// then read.  Holds neither the graph nor the position map: both must outlive it, and an edit of the graph makes it stale.
class Blocks {
  public:
    static constexpr const char *statNames[GK_BLOCKS_NSTATS] = {"records", "bases", "valid_bases", "windows", "covered", "rows", "brk_overlap", "brk_translocation",
                                                                "brk_inversion", "brk_relocation", "brk_indel", "brk_colinear", "edges_unaligned", "edges_repeat",
                                                                "edges_misassembled", "edges_indel", "edges_colinear", "edges_exact", "full_edges", "aligned_kmers",
                                                                "pieces", "piece_bases", "indel_shift_sum", "indel_shift_max"};
    struct Stats { uint64_t v[GK_BLOCKS_NSTATS] = {}; };
    struct Rows { std::vector<uint32_t> edge; std::vector<uint8_t> strand; std::vector<uint32_t> record; std::vector<int64_t> pos; std::vector<uint32_t> dlo, dhi;
                  std::vector<uint8_t> brk; std::vector<int64_t> shift; };
    struct Edges { std::vector<uint8_t> cls, full; std::vector<uint32_t> firstRow, nrows; };
    struct Pieces { std::vector<uint64_t> len; std::vector<uint32_t> edge; };
    Blocks(gk_ctx *ctx, gk_graph *g, gk_vmap *positions) : ctx_(ctx) { check(gk_blocks_create(g, positions, &h_), ctx_); }
    ~Blocks() { close(); }
    void close() { gk_blocks_destroy(h_); h_ = nullptr; }
    Blocks(Blocks &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Blocks(const Blocks &) = delete;
    Blocks &operator=(const Blocks &) = delete;
    gk_blocks *handle() const { return h_; }
    // the next reference record: its joined sequence characters
    void addRecord(const std::string &record) { check(gk_blocks_add_record(h_, record.data(), record.size()), ctx_); }
    // order the rows, class every breakpoint and edge, cut the pieces; again with another tol without feeding again
    void finish(uint64_t tol) { check(gk_blocks_finish(h_, tol), ctx_); }
    Stats stats() const {
        Stats st;
        check(gk_blocks_stats(h_, st.v), ctx_);
        return st;
    }
    Rows rows() const {
        Rows r;
        const size_t n = (size_t)stats().v[5];
        uint64_t got = 0;
        r.edge.resize(n); r.strand.resize(n); r.record.resize(n); r.pos.resize(n); r.dlo.resize(n); r.dhi.resize(n); r.brk.resize(n); r.shift.resize(n);
        check(gk_blocks_rows(h_, r.edge.data(), r.strand.data(), r.record.data(), r.pos.data(), r.dlo.data(), r.dhi.data(), r.brk.data(), r.shift.data(), n, &got), ctx_);
        return r;
    }
    Edges edges(const std::vector<uint32_t> &ids) const {
        Edges e;
        const size_t n = ids.size();
        e.cls.resize(n); e.full.resize(n); e.firstRow.resize(n); e.nrows.resize(n);
        check(gk_blocks_edges(h_, ids.data(), n, e.cls.data(), e.full.data(), e.firstRow.data(), e.nrows.data()), ctx_);
        return e;
    }
    Pieces pieces() const {
        Pieces p;
        const size_t n = (size_t)stats().v[20];
        uint64_t got = 0;
        p.len.resize(n); p.edge.resize(n);
        check(gk_blocks_pieces(h_, p.len.data(), p.edge.data(), n, &got), ctx_);
        return p;
    }
    // lengths descending, the first at which twice the running sum reaches `total`; 0 for none
    static uint64_t nx50(std::vector<uint64_t> lengths, uint64_t total) {
        std::sort(lengths.rbegin(), lengths.rend());
        uint64_t run = 0;
        for (const uint64_t x : lengths) {
            run += x;
            if (2 * run >= total) return x;
        }
        return 0;
    }
    // NA50 against the piece bases, NGA50 against the valid bases of the reference
    std::pair<uint64_t, uint64_t> na50() const {
        const Stats st = stats();
        const Pieces p = pieces();
        return {nx50(p.len, st.v[21]), nx50(p.len, st.v[2])};
    }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_blocks *h_ = nullptr;
};

// gk_scaffolds: a plan of the FASTA text of a graph's scaffolds (Graph::scaffolds; the rule: include/genome_amd.h, "scaffolds").
// As Contigs: the device emits the text when it is read or written, and an edit of the graph makes the plan stale.
class Scaffolds {
  public:
    struct Stats {
        uint64_t v[13] = {};                                     // gk_scaffolds_stats' stats13, under these names
        std::string json() const {
            const char *names[13] = {"chains", "chain_forward", "chain_self_twin", "chain_reverse", "singletons", "records", "members", "adjacent", "gapped",
                                     "clamped", "n_bases", "bases", "text_bytes"};
            std::string s = "{";
            for (int i = 0; i < 13; i++) s += std::string(i ? ",\"" : "\"") + names[i] + "\":" + std::to_string(v[i]);
            return s + "}";
        }
        uint64_t textBytes() const { return v[12]; }
    };
    // one piece of an edge in a record: the record's index in the text, the first base in its sequence, bases written, bases skipped
    struct Segment { uint64_t record; uint32_t edge; uint64_t first, bases; uint32_t skipped; };
    Scaffolds(gk_ctx *ctx, gk_scaffolds *h) : ctx_(ctx), h_(h) {}
    ~Scaffolds() { close(); }
    void close() { gk_scaffolds_destroy(h_); h_ = nullptr; }
    Scaffolds(Scaffolds &&o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    Scaffolds(const Scaffolds &) = delete;
    Scaffolds &operator=(const Scaffolds &) = delete;
    Stats stats() const {
        Stats st;
        check(gk_scaffolds_stats(h_, st.v), ctx_);
        return st;
    }
    std::string read(uint64_t offset, uint64_t n) {
        std::string out((size_t)n, '\0');
        uint64_t got = 0;
        check(gk_scaffolds_read(h_, offset, out.data(), n, &got), ctx_);
        out.resize((size_t)got);
        return out;
    }
    // {junctions joined on an overlap, bases they left out} over the chain records written (Graph::scaffolds with overlaps)
    std::pair<uint64_t, uint64_t> overlapStats() const {
        uint64_t v[2] = {};
        check(gk_scaffolds_overlap_stats(h_, v), ctx_);
        return {v[0], v[1]};
    }
    std::string text() { return read(0, stats().textBytes()); }
    void write(const std::string &path) { check(gk_scaffolds_write(h_, path.c_str()), ctx_); }
    std::vector<Segment> segments() const {
        const Stats st = stats();
        const uint64_t n = st.v[6] + st.v[4];
        std::vector<uint64_t> rec(n), first(n), bases(n);
        std::vector<uint32_t> edge(n), skip(n);
        uint64_t got = 0;
        check(gk_scaffolds_segments(h_, rec.data(), edge.data(), first.data(), bases.data(), skip.data(), n, &got), ctx_);
        std::vector<Segment> out(n);
        for (uint64_t i = 0; i < n; i++) out[i] = Segment{rec[i], edge[i], first[i], bases[i], skip[i]};
        return out;
    }
    // Every junction of the plan (two consecutive rows of segments() in one record) held against the placements of its two edges
    // (include/genome_amd.h, "the judge"): the GK_JUDGE_* class and err per junction in row order, and the stats under these names.
    // tol is a choice, not a measurement.
    static constexpr const char *judgeStatNames[GK_JUDGE_NSTATS] = {
        "junctions", "unjudged", "other_record", "strand", "order", "distance", "correct",
        "adjacent_unjudged", "adjacent_other_record", "adjacent_strand", "adjacent_order", "adjacent_distance", "adjacent_correct",
        "gapped_unjudged", "gapped_other_record", "gapped_strand", "gapped_order", "gapped_distance", "gapped_correct",
        "overlapped_unjudged", "overlapped_other_record", "overlapped_strand", "overlapped_order", "overlapped_distance", "overlapped_correct",
        "gapped_correct_abs_err_sum", "gapped_correct_abs_err_max", "records_judged", "records_clean"};
    struct Judged {
        std::vector<uint8_t> classes;
        std::vector<int64_t> err;
        uint64_t v[GK_JUDGE_NSTATS] = {};
        static bool misjoin(uint8_t c) { return c >= GK_JUDGE_OTHER_RECORD && c <= GK_JUDGE_DISTANCE; }
    };
    Judged judge(const Placements &placements, uint64_t tol) const {
        const Stats st = stats();
        const uint64_t cap = st.v[6] + st.v[4] - st.v[5];          // rows - records
        Judged j;
        j.classes.resize(cap); j.err.resize(cap);
        uint64_t n = 0;
        check(gk_scaffolds_judge(h_, placements.handle(), tol, j.classes.data(), j.err.data(), cap, &n, j.v), ctx_);
        return j;
    }

  private:
    gk_ctx *ctx_ = nullptr;
    gk_scaffolds *h_ = nullptr;
};

struct Edge {                 // S/data/graph/Edge.scala:11 (ids are not part of the observable result)
    DNASeq start, end;
    std::string seq;
};

// trait Graph / MapGraph (Graph.scala:23-262), HBM resident
class Graph {
  public:
    // Graph.buildGraph(k, kmersFreq) :269-382
    // keepCycles: perfect cycles, which the reference ignores (:375), become self-loops at their anchors (gk_graph_build_cycles;
    // include/genome_amd.h, "perfect cycles"); cycleStats() holds the six statistics then, and every simplifyGraph() of this
    // object keeps cycles too (keepCycles(false) turns that off again).
    static Graph buildGraph(int k, DNAMap &kmersFreq, bool keepCycles = false) {
        if (kmersFreq.k() != k) throw KeyLengthError(GK_E_KLEN, "map k != k");
        Graph g(kmersFreq.context(), k);
        if (keepCycles) check(gk_graph_build_cycles(kmersFreq.handle(), &g.h_, g.cycleStats_.v), kmersFreq.context().handle());
        else check(gk_graph_build(kmersFreq.handle(), &g.h_), kmersFreq.context().handle());
        g.keepCycles_ = keepCycles;
        return g;
    }
    static Graph build(int k, DNAMap &kmersFreq, bool keepCycles = false) { return buildGraph(k, kmersFreq, keepCycles); }
    struct CycleStats { uint64_t v[6] = {}; };              // gk_graph_build_cycles' stats6
    static constexpr const char *cycleStatNames[6] = {"cycle_kmers", "cycles", "anchors", "self_complementary", "longest", "rounds"};
    struct KeepStats { uint64_t v[4] = {}; };               // gk_graph_simplify_keep_cycles' stats4
    static constexpr const char *keepStatNames[4] = {"kept_self_loops", "cycles_merged", "anchors_kept", "nodes_removed"};
    const CycleStats &cycleStats() const { return cycleStats_; }
    const KeepStats &keptTotal() const { return keptTotal_; }   // summed over this object's keeping simplifyGraph calls
    void keepCycles(bool on) { keepCycles_ = on; }
    bool keepsCycles() const { return keepCycles_; }
    // Graph(file) (Graph.scala:384-390) with GraphSimplifier's checks of the loaded graph (GraphSimplifier.scala:157-169); k comes
    // from the file (:153).  A malformed or corrupt file throws GK_E_FORMAT.
    static Graph load(Context &ctx, const std::string &path) {
        Graph g(ctx, 0);
        check(gk_graph_load(ctx.handle(), path.c_str(), &g.h_), ctx.handle());
        g.k_ = gk_graph_k(g.h_);
        return g;
    }
    // MapGraph.write (Graph.scala:232-261): the live nodes and edges with their ids, written aside and renamed onto path
    void save(const std::string &path) const { check(gk_graph_save(h_, path.c_str()), ctx_.handle()); }
    int k() const { return k_; }
    ~Graph() { gk_graph_destroy(h_); }
    Graph(Graph &&o) noexcept : ctx_(o.ctx_), k_(o.k_), h_(o.h_), keepCycles_(o.keepCycles_), cycleStats_(o.cycleStats_), keptTotal_(o.keptTotal_) { o.h_ = nullptr; }
    Graph(const Graph &) = delete;

    void simplifyGraph() { simplifyGraph(keepCycles_); }                            // :211-230
    // keepCycles: self-loop nodes stay and every cycle of merge-away nodes keeps its anchors -> the four statistics (zeros otherwise)
    KeepStats simplifyGraph(bool keepCycles) {
        KeepStats st;
        if (!keepCycles) { check(gk_graph_simplify(h_), ctx_.handle()); return st; }
        check(gk_graph_simplify_keep_cycles(h_, st.v), ctx_.handle());
        for (int i = 0; i < 4; i++) keptTotal_.v[i] += st.v[i];
        return st;
    }
    void removeBubbles() { check(gk_graph_remove_bubbles(h_), ctx_.handle()); }     // :125-149
    bool removeEdge(const DNASeq &start, char firstBase) {                          // :191-195
        uint8_t b = (uint8_t)DNASeq::code(firstBase);
        uint64_t removed = 0;
        check(gk_graph_remove_edges(h_, &start.lo, &start.hi, &b, 1, &removed), ctx_.handle());
        return removed == 1;
    }
    // components.maxBy(_.size) + retain (:54-72, :161-165; GraphBuilder.scala:52-54)
    std::pair<uint64_t, uint64_t> retainLargestComponent() {
        uint64_t kept = 0, comps = 0;
        check(gk_graph_retain_largest(h_, &kept, &comps), ctx_.handle());
        return {kept, comps};
    }
    // GraphBuilder.scala:41-47: `hist` = components grouped by node count, `hist2` = grouped by the summed length of their
    // nodes' out-edges; each as value -> number of components, ascending
    std::pair<std::map<uint64_t, uint64_t>, std::map<uint64_t, uint64_t>> componentHistograms() const {
        uint64_t n = 0;
        int rc = gk_graph_component_stats(h_, nullptr, nullptr, 0, &n);
        if (rc != GK_OK && rc != GK_E_CAPACITY) check(rc, ctx_.handle());
        std::vector<uint32_t> nodes(n);
        std::vector<uint64_t> len(n);
        if (n) check(gk_graph_component_stats(h_, nodes.data(), len.data(), n, &n), ctx_.handle());
        std::map<uint64_t, uint64_t> h1, h2;
        for (uint64_t i = 0; i < n; i++) { h1[nodes[i]]++; h2[len[i]]++; }
        return {h1, h2};
    }
    // Graph.getGraphMap :90-119
    PositionMap getGraphMap() {
        auto [n, e, l] = counts();
        PositionMap pm(ctx_, k_, l + n);
        uint64_t entries = 0;
        check(gk_graph_position_map(h_, pm.handle(), &entries), ctx_.handle());
        return pm;
    }
    // Every edge placed on a reference genome (include/genome_amd.h, "placements"): `records` = the joined sequence of every reference
    // record, `positions` = getGraphMap of the graph as it is now.  Scaffolds::judge takes the result.
    Placements place(PositionMap &positions, const std::vector<std::string> &records) const {
        Placements p(ctx_.handle(), h_, positions.handle());
        for (const std::string &r : records) p.add(r);
        return p;
    }
    // Every edge aligned to a reference genome in blocks (include/genome_amd.h, "alignment blocks" and "breakpoints"): the records
    // are fed and the result finished at `tol`; Blocks::finish may be called again with another.
    Blocks alignBlocks(PositionMap &positions, const std::vector<std::string> &records, uint64_t tol) const {
        Blocks b(ctx_.handle(), h_, positions.handle());
        for (const std::string &r : records) b.addRecord(r);
        b.finish(tol);
        return b;
    }
    // GraphSimplifier.scala:213-247: the pairs' positions, annotate, the bounded walks -> support counts
    void walkPairs(PositionMap &positions, Support &support, const PairedEndData &data, uint64_t takeFirst, int rangeLo = 180, int rangeHi = 250) {
        check(gk_graph_walk_pairs(h_, positions.handle(), support.handle(), data.bin.data(), data.bin.size(), std::min<uint64_t>(data.count, takeFirst),
                                  rangeLo, rangeHi), ctx_.handle());
    }
    // the same over pairs [firstPair, endPair) only (one rank's share)
    void walkPairs(PositionMap &positions, Support &support, const PairedEndData &data, uint64_t firstPair, uint64_t endPair, int rangeLo, int rangeHi) {
        if (endPair <= firstPair) return;
        const auto [b0, b1] = pairBytes(data, firstPair, endPair);
        check(gk_graph_walk_pairs(h_, positions.handle(), support.handle(), data.bin.data() + b0, b1 - b0, endPair - firstPair, rangeLo, rangeHi),
              ctx_.handle());
    }
    // Reads threaded through the graph (this project's own rule, include/genome_amd.h: gk_graph_thread_reads): every window of both
    // mates of the first `takeFirst` pairs, as single reads; a window that is a node's k-mer adds one to the support of the
    // (in-edge, out-edge) the read crossed it by.  -> {records threaded, inner windows, off_graph, repeated, on_edge, broken,
    // crossings}.  On an error the support is unchanged.
    struct ThreadStats { uint64_t v[7] = {}; };
    static constexpr const char *threadStatNames[7] = {"records", "inner_windows", "off_graph", "repeated", "on_edge", "broken", "crossings"};
    ThreadStats threadReads(PositionMap &positions, Support &support, const PairedEndData &data, uint64_t takeFirst) {
        ThreadStats st;
        check(gk_graph_thread_reads(h_, positions.handle(), support.handle(), data.bin.data(), data.bin.size(), 2 * std::min<uint64_t>(data.count, takeFirst),
                                    st.v), ctx_.handle());
        return st;
    }
    // the same over pairs [firstPair, endPair) only (one rank's share)
    ThreadStats threadReads(PositionMap &positions, Support &support, const PairedEndData &data, uint64_t firstPair, uint64_t endPair) {
        ThreadStats st;
        if (endPair <= firstPair) return st;
        const auto [b0, b1] = pairBytes(data, firstPair, endPair);
        check(gk_graph_thread_reads(h_, positions.handle(), support.handle(), data.bin.data() + b0, b1 - b0, 2 * (endPair - firstPair), st.v), ctx_.handle());
        return st;
    }
    // Reads followed across a whole edge (this project's own rule, include/genome_amd.h: gk_graph_thread_spans): both mates of the
    // first `takeFirst` pairs, as single reads; every edge a read crosses from end to end adds one to spans[(the edge it came by,
    // the edge, the edge it left by)].  -> {records threaded, crossings, spans, interrupted, open}.  On an error `spans` is
    // unchanged.  Over N ranks every rank threads its share and PartitionedDNAMap::reduceSpans sums the tables.
    struct SpanStats { uint64_t v[5] = {}; };
    static constexpr const char *spanStatNames[5] = {"records", "crossings", "spans", "interrupted", "open"};
    SpanStats threadSpans(PositionMap &positions, Spans &spans, const PairedEndData &data, uint64_t takeFirst) {
        SpanStats st;
        check(gk_graph_thread_spans(h_, positions.handle(), spans.handle(), data.bin.data(), data.bin.size(), 2 * std::min<uint64_t>(data.count, takeFirst),
                                    st.v), ctx_.handle());
        return st;
    }
    // gk_graph_split_edges_by_spans: every one-to-one pairing (at least `cutoff` spans each) of the in- and out-edges of a repeat
    // edge gets its own copy of the edge -> {candidates, resolved, unequal, ambiguous, unsupported, new edges, new nodes};
    // simplifyGraph() is the next call.
    struct SplitEdgeStats { uint64_t v[7] = {}; };
    static constexpr const char *splitEdgeStatNames[7] = {"candidates", "resolved", "unequal", "ambiguous", "unsupported", "new_edges", "new_nodes"};
    SplitEdgeStats splitEdgesBySpans(const Spans &spans, uint32_t cutoff) {
        SplitEdgeStats st;
        check(gk_graph_split_edges_by_spans(h_, spans.handle(), cutoff, st.v), ctx_.handle());
        return st;
    }
    // The fragment lengths of the pairs whose mates' first k-mers lie on one edge (include/genome_amd.h, "the insert range"):
    // hist[D] over bins = maxInsert + 1 lengths and the nine classes {orientations, unplaced, repetitive, apart, ambiguous,
    // reversed, beyond, near_end, counted}.  pm != nullptr: pairs [firstPair, endPair) are this rank's share and the result is
    // the sum over the ranks (COLLECTIVE).
    struct PairDistances { std::vector<uint64_t> hist; uint64_t classes[9] = {}; };
    static constexpr const char *pairClassNames[9] = {"orientations", "unplaced", "repetitive", "apart", "ambiguous", "reversed", "beyond", "near_end", "counted"};
    PairDistances pairDistances(PositionMap &positions, const PairedEndData &data, uint64_t takeFirst, uint32_t bins = 4096) {
        PairDistances r;
        r.hist.resize(bins >= 1 ? bins : 1);
        check(gk_graph_pair_distances(h_, positions.handle(), data.bin.data(), data.bin.size(), std::min<uint64_t>(data.count, takeFirst), bins,
                                      r.hist.data(), r.classes), ctx_.handle());
        return r;
    }
    PairDistances pairDistances(PartitionedDNAMap &pm, PositionMap &positions, const PairedEndData &data, uint64_t firstPair, uint64_t endPair, uint32_t bins = 4096);
    // The pairs whose mates' first k-mers lie on two different edges (include/genome_amd.h, "scaffold links"), added to `links`
    // -> the eight classes.  On an error `links` is unchanged.
    struct LinkClasses { uint64_t v[8] = {}; };
    static constexpr const char *linkClassNames[8] = {"orientations", "unplaced", "repetitive", "at_node", "same_edge", "short_edge", "too_far", "linked"};
    LinkClasses pairLinks(PositionMap &positions, Links &links, const PairedEndData &data, uint64_t takeFirst, uint64_t minLen, uint64_t maxSpan) {
        LinkClasses c;
        check(gk_graph_pair_links(h_, positions.handle(), links.handle(), data.bin.data(), data.bin.size(), std::min<uint64_t>(data.count, takeFirst), minLen,
                                  maxSpan, c.v), ctx_.handle());
        return c;
    }
    gk_graph *handle() const { return h_; }
    // :272-316 -> (edges removed, nodes added); simplifyGraph() is the next call (:318)
    std::pair<uint64_t, uint64_t> splitBySupport(const Support &support, int cutoff) {
        uint64_t rm = 0, nn = 0;
        check(gk_graph_split_by_support(h_, support.handle(), cutoff, &rm, &nn), ctx_.handle());
        return {rm, nn};
    }
    // Edge coverage (this project's own rule, include/genome_amd.h): per id the number of k-mers (len + 1 windows), the sum, minimum
    // and maximum of their counts in `counts`; zeros for a dead or out-of-range id.  Default: every id below the edge id bound.
    struct EdgeCoverage { std::vector<uint32_t> ids; std::vector<uint64_t> kmers, sum; std::vector<uint32_t> min, max; uint64_t missing = 0; };
    EdgeCoverage edgeCoverage(const DNAMap &counts) const {
        uint64_t nodeIds = 0, edgeIds = 0;
        check(gk_graph_id_bounds(h_, &nodeIds, &edgeIds), ctx_.handle());
        std::vector<uint32_t> ids(edgeIds);
        for (uint64_t i = 0; i < edgeIds; i++) ids[i] = (uint32_t)i;
        return edgeCoverage(counts, ids);
    }
    EdgeCoverage edgeCoverage(const DNAMap &counts, const std::vector<uint32_t> &ids) const {
        EdgeCoverage c;
        c.ids = ids;
        const size_t n = ids.size();
        c.kmers.resize(n); c.sum.resize(n); c.min.resize(n); c.max.resize(n);
        check(gk_graph_edge_coverage(h_, counts.handle(), ids.data(), n, c.kmers.data(), c.sum.data(), c.min.data(), c.max.data(), &c.missing), ctx_.handle());
        return c;
    }
    // One round of tip removal (include/genome_amd.h): dead-end edges of at most maxLen bases (0 = the default, 2k) beside an edge
    // of strictly higher mean coverage -> edges removed; simplifyGraph() is the next call.  GK_E_STATE if `counts` is not this graph's.
    uint64_t clipTips(const DNAMap &counts, uint64_t maxLen = 0) {
        uint64_t removed = 0;
        check(gk_graph_clip_tips(h_, counts.handle(), maxLen ? maxLen : 2 * (uint64_t)k_, &removed), ctx_.handle());
        return removed;
    }
    // Per pair of edge ids min(Levenshtein distance of the two edges' sequences, maxDiff + 1); 0xffffffff for a dead or
    // out-of-range id; maxDiff <= 31 (include/genome_amd.h)
    std::vector<uint32_t> edgeDistance(const std::vector<uint32_t> &e1, const std::vector<uint32_t> &e2, uint32_t maxDiff) const {
        if (e1.size() != e2.size()) throw GkError(GK_E_INVALID, "edgeDistance: the id lists differ in length");
        std::vector<uint32_t> dist(e1.size());
        check(gk_graph_edge_distance(h_, e1.data(), e2.data(), e1.size(), maxDiff, dist.data()), ctx_.handle());
        return dist;
    }
    // One round of bubble removal (include/genome_amd.h): of two parallel edges of at most maxLen bases (0 = the default, 2k)
    // within edit distance maxDiff (default 3, the reference's commented-out maxerrors) the one of strictly lower mean coverage
    // goes -> (edges removed, pairs compared); simplifyGraph() is the next call.  GK_E_STATE if `counts` is not this graph's.
    std::pair<uint64_t, uint64_t> popBubbles(const DNAMap &counts, uint64_t maxLen = 0, uint32_t maxDiff = 3) {
        uint64_t removed = 0, pairs = 0;
        check(gk_graph_pop_bubbles(h_, counts.handle(), maxLen ? maxLen : 2 * (uint64_t)k_, maxDiff, &removed, &pairs), ctx_.handle());
        return {removed, pairs};
    }
    // One round of weak-connection removal (include/genome_amd.h): an edge of at most maxLen bases (0 = the default, 2k) with another
    // way out of its start node and another way into its end node goes if at each end one of those has more than `ratio` times its
    // mean coverage (0: off; at most 65535), and so does any edge whose mean is below `floor` (0: off); simplifyGraph() is the next
    // call.  ratio 5 and 2k are choices, not measurements.  GK_E_STATE if `counts` is not this graph's.
    struct WeakStats { uint64_t candidates = 0, removedRatio = 0, removedFloorOnly = 0, removed = 0; };
    WeakStats removeWeakEdges(const DNAMap &counts, uint64_t maxLen = 0, uint32_t ratio = 5, uint32_t floor = 0) {
        uint64_t st[4] = {0, 0, 0, 0};
        check(gk_graph_remove_weak_edges(h_, counts.handle(), maxLen ? maxLen : 2 * (uint64_t)k_, ratio, floor, st), ctx_.handle());
        return {st[0], st[1], st[2], st[3]};
    }
    // CheckGraph.scala:37-41 over the live edges longer than longerThan: count, summed length, median (sorted[count / 2], the
    // reference's "N50"), the real N50, the maximum; computed on the device
    struct ContigStats { uint64_t count = 0, sum = 0, median = 0, n50 = 0, max = 0; };
    ContigStats contigStats(uint64_t longerThan = 200) const {
        ContigStats c;
        check(gk_graph_contig_stats(h_, longerThan, &c.count, &c.sum, &c.median, &c.n50, &c.max), ctx_.handle());
        return c;
    }
    std::tuple<uint64_t, uint64_t, uint64_t> counts() const {
        uint64_t n = 0, e = 0, l = 0;
        check(gk_graph_counts(h_, &n, &e, &l), ctx_.handle());
        return {n, e, l};
    }
    std::vector<DNASeq> getNodes() const {                                          // sorted by k-mer
        auto [n, e, l] = counts();
        (void)e; (void)l;
        std::vector<uint64_t> lo(n), hi(n);
        uint64_t got = 0;
        check(gk_graph_export_nodes(h_, lo.data(), hi.data(), n, &got), ctx_.handle());
        std::vector<DNASeq> out(got);
        for (uint64_t i = 0; i < got; i++) out[i] = DNASeq{lo[i], hi[i], k_};
        std::sort(out.begin(), out.end());
        return out;
    }
    std::vector<Edge> getEdges() const {                                            // sorted by (start, first base)
        auto [n, ne, ln] = counts();
        (void)n;
        std::vector<uint64_t> slo(ne), shi(ne), elo(ne), ehi(ne);
        std::vector<int64_t> len(ne), off(ne);
        std::vector<uint8_t> seq((ln + 3 * ne) / 4 + 1);
        uint64_t got = 0, used = 0;
        check(gk_graph_export_edges(h_, slo.data(), shi.data(), elo.data(), ehi.data(), len.data(), off.data(), ne, &got,
                                    seq.data(), seq.size(), &used), ctx_.handle());
        std::vector<Edge> out(got);
        for (uint64_t i = 0; i < got; i++) {
            out[i].start = DNASeq{slo[i], shi[i], k_};
            out[i].end = DNASeq{elo[i], ehi[i], k_};
            out[i].seq.resize((size_t)len[i]);
            for (int64_t j = 0; j < len[i]; j++) out[i].seq[(size_t)j] = "AGCT"[(seq[(size_t)(off[i] + j / 4)] >> ((j % 4) * 2)) & 3];
        }
        std::sort(out.begin(), out.end(), [](const Edge &a, const Edge &b) {
            if (!(a.start == b.start)) return a.start < b.start;
            return DNASeq::code(a.seq[0]) < DNASeq::code(b.seq[0]);
        });
        return out;
    }

    // The twin of every edge asked for, by content (include/genome_amd.h, "edge twins"): twin[i] (0xffffffff: none), cls[i]
    // (GK_TWIN_*) and the six stats over all live edges, named as gk_graph_edge_twins' stats6
    struct EdgeTwins {
        std::vector<uint32_t> twin;
        std::vector<uint8_t> cls;
        uint64_t liveEdges = 0, paired = 0, self = 0, missing = 0, ambiguous = 0, keyCollisions = 0;
        std::string json() const {
            return "{\"live_edges\":" + std::to_string(liveEdges) + ",\"paired\":" + std::to_string(paired) + ",\"self\":" + std::to_string(self) +
                   ",\"missing\":" + std::to_string(missing) + ",\"ambiguous\":" + std::to_string(ambiguous) + ",\"key_collisions\":" + std::to_string(keyCollisions) + "}";
        }
    };
    EdgeTwins edgeTwins(const std::vector<uint32_t> &ids = {}) const {
        EdgeTwins t;
        t.twin.resize(ids.size());
        t.cls.resize(ids.size());
        uint64_t st[6] = {};
        check(gk_graph_edge_twins(h_, ids.data(), ids.size(), t.twin.data(), t.cls.data(), st), ctx_.handle());
        t.liveEdges = st[0]; t.paired = st[1]; t.self = st[2]; t.missing = st[3]; t.ambiguous = st[4]; t.keyCollisions = st[5];
        return t;
    }
    // The graph as GFA 1.0, planned on the device (include/genome_amd.h, "the graph as GFA"): counts (may be null) adds KC:i:
    Gfa gfa(const DNAMap *counts = nullptr) const {
        gk_gfa *c = nullptr;
        check(gk_graph_gfa_plan(h_, counts ? counts->handle() : nullptr, &c), ctx_.handle());
        return Gfa(ctx_.handle(), c);
    }
    // The assembly as FASTA, planned on the device (include/genome_amd.h, "contigs"): one record `>e<id> len=<n>[ cov=<mean>]` per
    // live edge whose path (start k-mer ++ seq) is not above its reverse complement (bothStrands: every live edge), n >= minLen, in
    // ascending edge id, wrapped at lineWidth (0: one line); `counts` (may be null) adds the cov= field.
    Contigs contigs(const DNAMap *counts = nullptr, uint64_t minLen = 0, uint32_t lineWidth = 60, bool bothStrands = false) const {
        gk_contigs *c = nullptr;
        check(gk_graph_contigs_plan(h_, counts ? counts->handle() : nullptr, minLen, lineWidth, bothStrands ? 2 : 1, &c), ctx_.handle());
        return Contigs(ctx_.handle(), c);
    }
    // The chains (scaffoldChains') as scaffold FASTA, planned on the device (include/genome_amd.h, "scaffolds"): gaps[c][i] = the gap
    // after member i of chain c (an entry for the last member may be left out).  minGap = 10 is a choice, not a measurement.
    Scaffolds scaffolds(const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<int64_t>> &gaps, int64_t minGap = 10, uint64_t minLen = 0,
                        uint32_t lineWidth = 60, bool bothStrands = false, bool singletons = true) const {
        return scaffoldsPlan(chains, gaps, nullptr, minGap, minLen, lineWidth, bothStrands, singletons);
    }
    // The same with overlapGaps' overlaps (include/genome_amd.h, "overlap detection"): where overlaps[c][i] = o > 0 nothing goes between
    // the two members and the next one contributes its path from base o.  The plan checks every o against the paths.
    Scaffolds scaffolds(const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<int64_t>> &gaps,
                        const std::vector<std::vector<uint32_t>> &overlaps, int64_t minGap = 10, uint64_t minLen = 0, uint32_t lineWidth = 60, bool bothStrands = false,
                        bool singletons = true) const {
        return scaffoldsPlan(chains, gaps, &overlaps, minGap, minLen, lineWidth, bothStrands, singletons);
    }
    // Overlap detection between fillGaps (or scaffoldChains) and scaffolds (include/genome_amd.h, "overlap detection"): where the last o
    // bases of a member's path equal the first o of the next member's, exactly, for exactly one o in minOverlap .. maxOverlap within tol
    // of -gap, overlaps[c][i] = o, else 0.  classes[c][i]: the GK_OVL_* class of the junction after member i of chain c.  maxOverlap 0
    // means k.  minOverlap = 10 and maxOverlap = k are choices, not measurements (a chance match of 10 bases: about 1e-6 per candidate).
    struct Overlapped {
        std::vector<std::vector<uint32_t>> overlaps;
        std::vector<std::vector<uint8_t>> classes;
        uint64_t v[7] = {};                                      // gk_graph_overlap_gaps' stats7, under these names
        std::string json() const {
            const char *names[7] = {"junctions", "adjacent", "out_of_range", "none", "ambiguous", "overlap", "overlap_bases"};
            std::string s = "{";
            for (int i = 0; i < 7; i++) s += std::string(i ? ",\"" : "\"") + names[i] + "\":" + std::to_string(v[i]);
            return s + "}";
        }
    };
    Overlapped overlapGaps(const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<int64_t>> &gaps, uint64_t tol, uint32_t minOverlap = 10,
                           uint32_t maxOverlap = 0) const {
        std::vector<uint32_t> members;
        std::vector<int64_t> gap;
        std::vector<uint64_t> off;
        flatten("overlapGaps", "gap", chains, gaps, gap, &members, &off);
        std::vector<uint32_t> ovl(members.size() + 1);
        std::vector<uint8_t> jclass(members.size() + 1);
        Overlapped r;
        check(gk_graph_overlap_gaps(h_, members.data(), off.data(), chains.size(), gap.data(), tol, minOverlap, maxOverlap ? maxOverlap : (uint32_t)k_, ovl.data(),
                                    jclass.data(), r.v), ctx_.handle());
        for (size_t c = 0; c < chains.size(); c++) {
            r.overlaps.emplace_back(ovl.begin() + off[c], ovl.begin() + off[c + 1] - 1);
            r.classes.emplace_back(jclass.begin() + off[c], jclass.begin() + off[c + 1] - 1);
        }
        return r;
    }
    // Gap filling between scaffoldChains and scaffolds (include/genome_amd.h, "gap filling"): where the graph holds exactly one path
    // of at most maxEdges edges between two consecutive members whose length is within tol bases of the gap, and no edge of it is
    // contested, its edges become members.  chains / gaps feed scaffolds() unchanged (a new junction's gap is -k).  classes[c][i] /
    // lengths[c][i]: the GK_FILL_* class of the junction after member i of input chain c, and the path's L where it is shared or
    // filled.  maxEdges = 16 and maxPaths = 256 are choices, not measurements.
    struct Filled {
        std::vector<std::vector<uint32_t>> chains;
        std::vector<std::vector<int64_t>> gaps, lengths;
        std::vector<std::vector<uint8_t>> classes;
        uint64_t v[10] = {};                                     // gk_graph_fill_gaps' stats10, under these names
        std::string json() const {
            const char *names[10] = {"junctions", "adjacent", "overflow", "none", "ambiguous", "shared", "filled", "filler_edges", "filler_bases",
                                     "searched_backward"};
            std::string s = "{";
            for (int i = 0; i < 10; i++) s += std::string(i ? ",\"" : "\"") + names[i] + "\":" + std::to_string(v[i]);
            return s + "}";
        }
    };
    Filled fillGaps(const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<int64_t>> &gaps, uint64_t tol, uint32_t maxEdges = 16,
                    uint32_t maxPaths = 256) const {
        std::vector<uint32_t> members;
        std::vector<int64_t> gap;
        std::vector<uint64_t> off;
        flatten("fillGaps", "gap", chains, gaps, gap, &members, &off);
        uint64_t nodeBound = 0, cap = 0, n = 0;
        check(gk_graph_id_bounds(h_, &nodeBound, &cap), ctx_.handle());      // (no edge is written twice: the filled chains fit the edge ids)
        std::vector<uint32_t> outMembers(cap + 1);
        std::vector<int64_t> outGap(cap + 1), jlen(members.size() + 1);
        std::vector<uint64_t> outOff(chains.size() + 1);
        std::vector<uint8_t> jclass(members.size() + 1);
        Filled r;
        check(gk_graph_fill_gaps(h_, members.data(), off.data(), chains.size(), gap.data(), tol, maxEdges, maxPaths, outMembers.data(), outGap.data(), cap,
                                 outOff.data(), jclass.data(), jlen.data(), &n, r.v), ctx_.handle());
        for (size_t c = 0; c < chains.size(); c++) {
            r.chains.emplace_back(outMembers.begin() + outOff[c], outMembers.begin() + outOff[c + 1]);
            r.gaps.emplace_back(outGap.begin() + outOff[c], outGap.begin() + outOff[c + 1] - 1);
            r.classes.emplace_back(jclass.begin() + off[c], jclass.begin() + off[c + 1] - 1);
            r.lengths.emplace_back(jlen.begin() + off[c], jlen.begin() + off[c + 1] - 1);
        }
        return r;
    }
    // the `contigs` file of GraphSimplifier.scala:338-347: per edge its sequence, then ">abacaba<i>"
    // (edge order: canonical, since the reference's is ConcurrentHashMap order)
    void writeContigs(std::ostream &out) const {
        size_t i = 0;
        for (const auto &e : getEdges()) out << e.seq << "\n>abacaba" << i++ << "\n";
    }
    // Graph.writeDot (Graph.scala:74-88): `start -> end [label=seq|length]`, ids = rank of the node's k-mer
    void writeDot(std::ostream &out) const {
        const auto nodes = getNodes();
        auto id = [&](const DNASeq &s) { return (size_t)(std::lower_bound(nodes.begin(), nodes.end(), s) - nodes.begin()) + 1; };
        out << "digraph G {\n";
        for (const auto &e : getEdges())
            out << id(e.start) << " -> " << id(e.end) << " [label=" << (e.seq.size() <= 50 ? e.seq : std::to_string(e.seq.size())) << "]\n";
        out << "}\n";
    }

  private:
    // per-junction lists of chains (`what`: "gap", "overlap") as the C calls take them: an entry per member (0 at a chain's last);
    // with them, where asked for, the members and chain_off
    template <class T>
    static void flatten(const char *who, const std::string &what, const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<T>> &lists,
                        std::vector<T> &flat, std::vector<uint32_t> *members = nullptr, std::vector<uint64_t> *off = nullptr) {
        if (chains.size() != lists.size()) throw GkError(GK_E_INVALID, std::string(who) + ": as many " + what + " lists as chains");
        if (off) off->assign(1, 0);
        for (size_t c = 0; c < chains.size(); c++) {
            if (lists[c].size() + 1 < chains[c].size()) throw GkError(GK_E_INVALID, std::string(who) + ": a chain with fewer " + what + "s than junctions");
            for (size_t j = 0; j < chains[c].size(); j++) flat.push_back(j + 1 < chains[c].size() ? lists[c][j] : 0);
            if (members) members->insert(members->end(), chains[c].begin(), chains[c].end());
            if (off) off->push_back(off->back() + chains[c].size());
        }
    }
    Scaffolds scaffoldsPlan(const std::vector<std::vector<uint32_t>> &chains, const std::vector<std::vector<int64_t>> &gaps,
                            const std::vector<std::vector<uint32_t>> *overlaps, int64_t minGap, uint64_t minLen, uint32_t lineWidth, bool bothStrands,
                            bool singletons) const {
        std::vector<uint32_t> members, ovl;
        std::vector<int64_t> gap;
        std::vector<uint64_t> off;
        flatten("scaffolds", "gap", chains, gaps, gap, &members, &off);
        gk_scaffolds *s = nullptr;
        if (!overlaps) {
            check(gk_graph_scaffolds_plan(h_, members.data(), off.data(), chains.size(), gap.data(), minGap, minLen, lineWidth, bothStrands ? 2 : 1, singletons ? 1 : 0,
                                          &s), ctx_.handle());
            return Scaffolds(ctx_.handle(), s);
        }
        flatten("scaffolds", "overlap", chains, *overlaps, ovl);
        check(gk_graph_scaffolds_plan_overlaps(h_, members.data(), off.data(), chains.size(), gap.data(), ovl.data(), minGap, minLen, lineWidth, bothStrands ? 2 : 1,
                                               singletons ? 1 : 0, &s), ctx_.handle());
        return Scaffolds(ctx_.handle(), s);
    }
    Graph(Context &ctx, int k) : ctx_(ctx), k_(k) {}
    Context &ctx_;
    int k_;
    gk_graph *h_ = nullptr;
    bool keepCycles_ = false;
    CycleStats cycleStats_;
    KeepStats keptTotal_;
};

inline Graph::PairDistances Graph::pairDistances(PartitionedDNAMap &pm, PositionMap &positions, const PairedEndData &data, uint64_t firstPair, uint64_t endPair,
                                                 uint32_t bins) {
    PairDistances r;
    r.hist.resize(bins >= 1 ? bins : 1);
    size_t b0 = 0, b1 = 0;
    if (endPair > firstPair) std::tie(b0, b1) = pairBytes(data, firstPair, endPair);
    check(gk_dist_pair_distances(pm.distHandle(), h_, positions.handle(), data.bin.data() + b0, b1 - b0, endPair > firstPair ? endPair - firstPair : 0, bins,
                                 r.hist.data(), r.classes), ctx_.handle());
    return r;
}

inline DNAMap::GraphPathStats DNAMap::addGraphPaths(const Graph &graph, uint32_t weight) {
    GraphPathStats st;
    check(gk_map_add_graph_paths(h_, graph.handle(), weight, st.v), ctx_.handle());
    return st;
}

// gk_insert_range over a pairDistances histogram: lo / hi cut trimPermille thousandths off either tail, median; estimated =
// false ("no estimate", fewer than max(minObservations, 1) observations): lo / hi are then the reference's 180 / 250
// (GraphSimplifier.scala:146).  The two defaults are choices, not measurements.  Host code: no context, no GPU.
struct InsertRange { uint32_t lo = 180, hi = 250, median = 0; bool estimated = false; uint64_t observations = 0; };
inline InsertRange insertRange(const std::vector<uint64_t> &hist, uint32_t trimPermille = 25, uint64_t minObservations = 1000) {
    InsertRange r;
    uint32_t lo = 0, hi = 0, med = 0;
    check(gk_insert_range(hist.data(), (uint32_t)hist.size(), trimPermille, minObservations, &lo, &hi, &med), nullptr);
    for (uint64_t c : hist) r.observations += c;
    if (r.observations >= std::max<uint64_t>(minObservations, 1)) { r.lo = lo; r.hi = hi; r.median = med; r.estimated = true; }
    return r;
}

inline void PartitionedDNAMap::reduceSupport(Graph &graph, Support &support) {
    check(gk_dist_reduce_support(d_, graph.handle(), support.handle()), ctx_.handle());
}
inline void PartitionedDNAMap::reduceLinks(Graph &graph, Links &links) {
    check(gk_dist_reduce_links(d_, graph.handle(), links.handle()), ctx_.handle());
}
inline void PartitionedDNAMap::reduceSpans(Graph &graph, Spans &spans) {
    check(gk_dist_reduce_spans(d_, graph.handle(), spans.handle()), ctx_.handle());
}

}  // namespace genome
