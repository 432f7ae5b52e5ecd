// tool_common.hpp — what the command-line tools in this directory share: a cursor over argv, the option groups and input forms
// that more than one tool takes, the paired-end stage of graph_builder --walk-pairs and graph_simplifier, and the writers of
// their text files and JSON fragments.  One header, no library; genome.hpp stays the twin of the reference's API and knows no
// command line.  (tests/host/tool_common_check.cpp runs the parts that need no device, links nothing, under sanitizers.)
#pragma once

#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <type_traits>

#include "genome.hpp"
#include "rank_id.hpp"

// A cursor over argv: `for (Args a(argc, argv, first); a.more(); a.next())` with one `if (a.…) … else if (a.…) …` chain per
// argument.  Every method answers for the argument under the cursor and consumes the values it takes.  An option whose values
// are missing matches nothing, so it ends in the chain's `else` (unknown argument).
struct Args {
    int argc;
    char **argv;
    int i;
    Args(int argc_, char **argv_, int first) : argc(argc_), argv(argv_), i(first) {}
    bool more() const { return i < argc; }
    void next() { i++; }
    const char *cur() const { return argv[i]; }
    bool flag(const char *name) const { return !std::strcmp(argv[i], name); }
    // `name` with at least n more tokens behind it
    bool has(const char *name, int n) const { return flag(name) && i + n < argc; }
    // `name` whose at-th token behind it is the word w (--range auto: at 1; --walk-pairs CUTOFF auto: at 2); consumes nothing
    bool word(const char *name, int at, const char *w) const { return has(name, at) && !std::strcmp(argv[i + at], w); }
    void skip(int n = 1) { i += n; }
    // --x V, --x LO HI, …: one target per value — std::string, or a signed or unsigned integer
    template <class... T> bool value(const char *name, T &...out) {
        if (!has(name, (int)sizeof...(T))) return false;
        (convert(name, argv[++i], out), ...);
        return true;
    }
    // --x [N|auto]: takes the next token if it is `auto` (out stays as it is) or starts with a digit
    template <class T> bool optional(const char *name, T &out) {
        if (!flag(name)) return false;
        const char *n = i + 1 < argc ? argv[i + 1] : nullptr;
        if (n && !std::strcmp(n, "auto")) i++;
        else if (n && n[0] >= '0' && n[0] <= '9') convert(name, argv[++i], out);
        return true;
    }
    // the one place numbers are read: the whole of s is a number that T holds, or false (out untouched)
    template <class T> static bool number(const char *s, T &out) {
        const char *end = s + std::strlen(s);
        T v{};
        const auto r = std::from_chars(s, end, v);
        if (r.ec != std::errc() || r.ptr != end) return false;
        out = v;
        return true;
    }
    static void convert(const char *, const char *s, std::string &out) { out = s; }
    // anything else is a usage error: one line that names the option (or the positional argument), exit 2
    template <class T> static void convert(const char *name, const char *s, T &out) {
        if (number(s, out)) return;
        std::fprintf(stderr, "%s needs %s, not '%s'\n", name, std::is_signed<T>::value ? "an integer" : "a non-negative integer", s);
        std::exit(2);
    }
};

// The --fastq forms: where argv[at] is "--fastq", take the FASTQ path and the split options out of argv and put the `.bin`
// form's argv in their place (the reads file and pair count are filled in after the conversion).  path stays empty otherwise.
struct FastqForm {
    std::string path;
    int split = 36;                               // Convert2bin's n; 0 = interleaved
    std::vector<char *> args;
    // -> false for a usage error
    bool parse(int &argc, char **&argv, int at) {
        static char empty[] = "", zero[] = "0";
        if (argc <= at || std::strcmp(argv[at], "--fastq")) return true;
        if (at + 1 >= argc) return false;
        path = argv[at + 1];
        for (Args a(argc, argv, 0); a.more(); a.next()) {
            if (a.i == at) { args.push_back(empty); args.push_back(zero); a.skip(); }
            else if (a.value("--split", split)) { if (split < 1) return false; }
            else if (a.flag("--interleaved")) split = 0;
            else if (a.flag("--world")) return false;        // N-rank ingestion of FASTQ is not supported: convert first
            else args.push_back(argv[a.i]);
        }
        args.push_back(nullptr);
        argc = (int)args.size() - 1;
        argv = args.data();
        return true;
    }
};

// --contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]
struct ContigOpts {
    std::string path;
    uint64_t minLen = 0;
    uint32_t width = 60;
    bool both = false;
    bool parse(Args &a) {
        if (a.flag("--contig-both-strands")) { both = true; return true; }
        return a.value("--contigs", path) || a.value("--contig-min-len", minLen) || a.value("--contig-width", width);
    }
};

// --gfa PATH: the final graph as GFA 1.0 (gk_graph_gfa_plan / gk_gfa_write); one GPU only, as --links is
struct GfaOpts {
    std::string path;
    bool parse(Args &a) { return a.value("--gfa", path); }
    bool check(int world) const {
        if (path.empty() || !world) return true;
        std::fprintf(stderr, "--gfa runs on one GPU only (not with --world): write it from the saved graph\n");
        return false;
    }
    // writes the text; -> the nine stats as JSON ("" if --gfa was not given)
    std::string run(const genome::Graph &graph, const genome::DNAMap *counts) const {
        if (path.empty()) return "";
        auto gfa = graph.gfa(counts);
        gfa.write(path);
        return gfa.stats().json();
    }
};

// --world W --rank R --id-file PATH; world 0: one GPU, no communicator
struct RankOpts {
    int world = 0, rank = 0;
    std::string idFile;
    bool parse(Args &a) { return a.value("--world", world) || a.value("--rank", rank) || a.value("--id-file", idFile); }
    bool check() const {
        if (!world || (world >= 1 && rank >= 0 && rank < world && !idFile.empty())) return true;
        std::fprintf(stderr, "--world W needs --rank R (0 <= R < W) and --id-file PATH\n");
        return false;
    }
    int device() const {
        if (!world) return 0;
        const int ndev = gk_device_count();
        if (ndev < 1) throw genome::GkError(GK_E_NODEVICE, "no GPU");
        return rank % ndev;
    }
};

inline std::vector<uint8_t> readBin(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// JSON fragments.  No nesting state and no escaping: the callers open and close their objects themselves.
// [[a,b],…]
inline std::string jsonPairs(const std::map<uint64_t, uint64_t> &h) {
    std::string s = "[";
    for (const auto &p : h) s += (s.size() > 1 ? ",[" : "[") + std::to_string(p.first) + "," + std::to_string(p.second) + "]";
    return s + "]";
}
// [a,b,…]
template <class T> inline std::string jsonList(const std::vector<T> &v) {
    std::string s = "[";
    for (const T &x : v) s += (s.size() > 1 ? "," : "") + std::to_string(x);
    return s + "]";
}
// "a":1,"b":2 (no braces)
template <class T> inline std::string jsonNamed(const char *const *names, const T *values, int n) {
    std::string s;
    for (int c = 0; c < n; c++) s += std::string(c ? ",\"" : "\"") + names[c] + "\":" + std::to_string(values[c]);
    return s;
}
// appends "key":value for each (key, value) given, with a comma before it unless it opens an object.  A value is an integer of
// any width (no cast at the call site), a bool, or text that is already rendered: null, an array, an object
inline void jsonPut(std::string &) {}
template <class V, class... Rest> inline void jsonPut(std::string &s, const char *key, const V &v, const Rest &...rest) {
    if (!s.empty() && s.back() != '{') s += ',';
    s += std::string("\"") + key + "\":";
    if constexpr (std::is_same<V, bool>::value) s += v ? "true" : "false";
    else if constexpr (std::is_integral<V>::value) s += std::to_string(v);
    else s += v;
    jsonPut(s, rest...);
}
// {"key":value,…}
template <class... KV> inline std::string jsonObject(const KV &...kv) {
    std::string s = "{";
    jsonPut(s, kv...);
    return s + "}";
}

// --spectrum PATH: one `count<TAB>keys` line per non-empty bin, the overflow bin as `>=N`
inline void writeSpectrum(const std::string &path, const std::vector<uint64_t> &h) {
    std::ofstream sf(path);
    for (size_t c = 1; c + 1 < h.size(); c++) if (h[c]) sf << c << "\t" << h[c] << "\n";
    if (h.back()) sf << ">=" << h.size() - 1 << "\t" << h.back() << "\n";
    if (!sf) throw std::runtime_error("cannot write " + path);
}

// --out prefix: <prefix>.nodes.txt, .edges.txt, .contigs (GraphSimplifier.scala:338-347) and .dot (Graph.scala:74-88)
inline void writeGraphText(genome::Graph &graph, const std::string &prefix) {
    std::ofstream nf(prefix + ".nodes.txt"), ef(prefix + ".edges.txt");
    for (const auto &n : graph.getNodes()) nf << n.toString() << "\n";
    for (const auto &e : graph.getEdges()) ef << e.start.toString() << " " << e.end.toString() << " " << e.seq << "\n";
    std::ofstream cf(prefix + ".contigs"), df(prefix + ".dot");
    graph.writeContigs(cf);
    graph.writeDot(df);
}

// --keep-cycles: perfect cycles are kept (include/genome_amd.h, "perfect cycles": this project's own rule; the reference ignores
// them, Graph.scala:375, :220-221).  graph_builder builds with gk_graph_build_cycles; every simplifyGraph either tool runs —
// the clip / pop rounds, --simplify, after the split by support, after each --resolve-repeats round — becomes
// gk_graph_simplify_keep_cycles (genome::Graph::keepCycles).  The JSON gains "cycles":{["build":{the six stats},] "simplify":{the
// four stats, summed over the calls}} and stderr one line.  One GPU only: there is no collective over ranks.
struct CycleOpts {
    bool keep = false;
    bool parse(Args &a) {
        if (!a.flag("--keep-cycles")) return false;
        keep = true;
        return true;
    }
    bool check(int world) const {
        if (keep && world) { std::fprintf(stderr, "--keep-cycles runs on one GPU only (not with --world): perfect cycles have no collective\n"); return false; }
        return true;
    }
    // after the last graph stage: the "cycles" object (empty text without the option), and the line on stderr
    std::string report(const genome::Graph &graph, bool built) const {
        if (!keep) return "";
        const std::string b = "{" + jsonNamed(genome::Graph::cycleStatNames, graph.cycleStats().v, 6) + "}";
        const std::string s = "{" + jsonNamed(genome::Graph::keepStatNames, graph.keptTotal().v, 4) + "}";
        std::fprintf(stderr, "keep-cycles:%s%s simplify %s\n", built ? " build " : "", built ? b.c_str() : "", s.c_str());
        return built ? jsonObject("build", b, "simplify", s) : jsonObject("simplify", s);
    }
};

// --seed-k K1[,K2,...]: multi-k assembly (include/genome_amd.h, "multi-k": this project's own rule).  The listed ks are seed stages,
// run before the count at the positional <k>: count the reads at K, add the contigs of the stage before at weight = rounds
// (genome::DNAMap::addGraphPaths), deleteAll(< rounds), buildGraph, the tool's clip / pop rounds, simplifyGraph; no retain (that would
// drop replicons).  The last seed stage's contigs go into the <k> table between its count and its deleteAll, and everything behind the
// count is unchanged.  The ks must be strictly increasing, below <k> and supported.  The JSON gains "seed_stages":[one object per
// stage: k, rounds, distinct k-mers before and after seeding, the six stats, nodes, edges] — the stage at <k> last — and stderr one
// line per stage.  One GPU only, and not with --prefilter (the seeds' k-mers are not in the reads' census).
struct SeedOpts {
    std::vector<int> ks;
    bool given = false;
    std::vector<std::string> stages;              // the per-stage JSON objects
    bool parse(Args &a) {
        std::string list;
        if (!a.value("--seed-k", list)) return false;
        given = true;
        ks.clear();
        size_t at = 0;
        while (at <= list.size()) {
            const size_t comma = std::min(list.find(',', at), list.size());
            int k = 0;
            if (!Args::number(list.substr(at, comma - at).c_str(), k)) { ks.assign(1, -1); break; }      // (refused by check)
            ks.push_back(k);
            at = comma + 1;
        }
        return true;
    }
    static bool supported(int k) { return (k >= 2 && k <= 31) || (k >= 34 && k <= 64); }
    bool check(int world, bool prefilter, int k) const {
        if (!given) return true;
        if (world) { std::fprintf(stderr, "--seed-k runs on one GPU only (not with --world): the seeding has no collective\n"); return false; }
        if (prefilter) { std::fprintf(stderr, "--seed-k does not run with --prefilter\n"); return false; }
        for (size_t i = 0; i < ks.size(); i++)
            if (!supported(ks[i]) || ks[i] >= k || (i && ks[i] <= ks[i - 1])) {
                std::fprintf(stderr, "usage: --seed-k K1[,K2,...] takes supported ks (2..31, 34..64), strictly increasing and below <k> = %d\n", k);
                return false;
            }
        return true;
    }
    // one stage's record: the JSON object and the line on stderr
    void report(int k, int rounds, uint64_t before, uint64_t after, const genome::DNAMap::GraphPathStats &st, uint64_t nodes, uint64_t edges) {
        const std::string paths = jsonNamed(genome::DNAMap::graphPathStatNames, st.v, 6);
        std::string js = "{";
        jsonPut(js, "k", k, "rounds", rounds, "distinct_before_seed", before, "distinct_after_seed", after);
        js += "," + paths;
        jsonPut(js, "nodes", nodes, "edges", edges);
        stages.push_back(js + "}");
        std::fprintf(stderr, "seed-k: k %d rounds %d distinct %llu -> %llu {%s} nodes %llu edges %llu\n", k, rounds, (unsigned long long)before,
                     (unsigned long long)after, paths.c_str(), (unsigned long long)nodes, (unsigned long long)edges);
    }
    std::string json() const {
        std::string s = "[";
        for (size_t i = 0; i < stages.size(); i++) s += (i ? "," : "") + stages[i];
        return s + "]";
    }
};

// GraphSimplifier.startup's paired-end stage (GraphSimplifier.scala:188-318) on a graph: position map, the pairs' walks, node
// split by their support, simplifyGraph — and this project's additions to it: the measured insert range, the threaded reads and,
// after the reference's stage, the repeats longer than k that single reads span.
// --resolve-repeats [CUTOFF] [--resolve-rounds N]: after the split and simplifyGraph, up to N rounds (default 1) of: a position map
// of the graph as it is now, gk_graph_thread_spans over both mates of the same pairs, gk_graph_split_edges_by_spans at CUTOFF,
// simplifyGraph (include/genome_amd.h, "spans": this project's own rule).  A round that resolves nothing is the last.  CUTOFF
// defaults to the stage's support cutoff (at least 1): a choice, not a measurement.  One GPU only: the spans have no collective.
struct PairedOpts {
    int cutoff = -1;                              // genome.cutoff
    int lo = 180, hi = 250;                       // GraphSimplifier.scala:146
    bool rangeAuto = false;                       // measure the range from the pairs instead
    long maxInsert = 4095;
    bool threadReads = false, walk = true;
    bool resolve = false;
    int64_t resolveCutoff = -1;                   // -1: the support cutoff
    uint32_t resolveRounds = 1;
    bool maxInsertOk() const { return maxInsert >= 1 && maxInsert <= 65535; }
    bool parseResolve(Args &a) {
        if (a.optional("--resolve-repeats", resolveCutoff)) { resolve = true; return true; }
        return a.value("--resolve-rounds", resolveRounds);
    }
    bool checkResolve(int world) const {
        if (resolve && (resolveCutoff == 0 || resolveCutoff > UINT32_MAX)) { std::fprintf(stderr, "--resolve-repeats CUTOFF is 1..4294967295\n"); return false; }
        if (!resolveRounds) { std::fprintf(stderr, "--resolve-rounds N needs N >= 1\n"); return false; }
        if (!resolve && resolveRounds != 1) { std::fprintf(stderr, "--resolve-rounds N goes with --resolve-repeats\n"); return false; }
        if (resolve && world) { std::fprintf(stderr, "--resolve-repeats runs on one GPU only (not with --world): the spans have no collective\n"); return false; }
        return true;
    }
    uint32_t spanCutoff() const { return resolveCutoff > 0 ? (uint32_t)resolveCutoff : (uint32_t)std::max(cutoff, 1); }
};
struct PairedResult {
    genome::InsertRange range;                    // rangeAuto only
    genome::Graph::PairDistances dist;            // rangeAuto only
    uint64_t supPairs = 0, badPairs = 0, walked = 0, removedEdges = 0, newNodes = 0;
    genome::Graph::ThreadStats threaded;          // summed over the ranks
    struct ResolveRound { genome::Graph::SpanStats spans; genome::Graph::SplitEdgeStats split; };
    std::vector<ResolveRound> resolved;           // --resolve-repeats: one entry per round run
    // the "walk_pairs" object both tools print
    std::string walkJson() const {
        return jsonObject("supported_edge_pairs", supPairs, "bad_pairs", badPairs, "orientations_walked", walked, "removed_edges", removedEdges,
                          "new_nodes", newNodes);
    }
    // the "resolve_repeats" object both tools print: the cutoff and, per round, the five and the seven counters
    std::string resolveJson(uint32_t cutoff) const {
        std::string rounds = "[";
        for (const ResolveRound &x : resolved)
            rounds += std::string(rounds.size() > 1 ? "," : "") + "{\"thread_spans\":{" + jsonNamed(genome::Graph::spanStatNames, x.spans.v, 5) + "},\"split_edges\":{" +
                      jsonNamed(genome::Graph::splitEdgeStatNames, x.split.v, 7) + "}}";
        return jsonObject("cutoff", cutoff, "rounds", rounds + "]");
    }
};
// pm = null and world = 0: one GPU, the first takeFirst pairs; else this rank's share of them, and the sums over the ranks
inline PairedResult pairedStage(genome::Graph &graph, genome::Context &ctx, genome::PartitionedDNAMap *pm, const genome::PairedEndData &data,
                                uint64_t takeFirst, int rank, int world, const PairedOpts &o) {
    PairedResult r;
    int lo = o.lo, hi = o.hi;
    uint64_t a = 0, b = 0;
    if (world) std::tie(a, b) = genome::pairShare(data.count, takeFirst, rank, world);
    auto graphMap = graph.getGraphMap();                                                             // :188
    if (o.rangeAuto) {                                                                               // the same pairs, before walking; over the ranks one histogram
        r.dist = world ? graph.pairDistances(*pm, graphMap, data, a, b, (uint32_t)o.maxInsert + 1)
                       : graph.pairDistances(graphMap, data, takeFirst, (uint32_t)o.maxInsert + 1);
        r.range = genome::insertRange(r.dist.hist);
        lo = (int)r.range.lo; hi = (int)r.range.hi;
        if (rank == 0 && r.range.estimated)
            std::fprintf(stderr, "insert range %u to %u, median %u, from %llu observations\n", r.range.lo, r.range.hi, r.range.median,
                         (unsigned long long)r.range.observations);
        else if (rank == 0)
            std::fprintf(stderr, "no estimate of the insert range (%llu observations): falling back to the reference's %u to %u\n",
                         (unsigned long long)r.range.observations, r.range.lo, r.range.hi);
    }
    genome::Support support(ctx);
    if (world) {                                                                                     // this rank's pairs, then the sum over the ranks
        if (o.walk) graph.walkPairs(graphMap, support, data, a, b, lo, hi);
        if (o.threadReads) {
            r.threaded = graph.threadReads(graphMap, support, data, a, b);
            double v[7];
            for (int i = 0; i < 7; i++) v[i] = (double)r.threaded.v[i];
            genome::check(gk_dist_allreduce_f64(pm->distHandle(), v, 7, 0), ctx.handle());
            for (int i = 0; i < 7; i++) r.threaded.v[i] = (uint64_t)v[i];
        }
        pm->reduceSupport(graph, support);                                                           // (before any node split)
    } else {
        if (o.walk) graph.walkPairs(graphMap, support, data, takeFirst, lo, hi);                     // :213-263
        if (o.threadReads) r.threaded = graph.threadReads(graphMap, support, data, takeFirst);
    }
    std::tie(r.supPairs, r.badPairs, r.walked) = support.sizes();                                    // :266 "Bad pairs"
    // (--no-pairs --resolve-repeats without --thread-reads gathered no support: the split would remove every edge at a branching
    // node for want of evidence, so it does not run and the spans alone edit the graph)
    if (o.walk || o.threadReads) std::tie(r.removedEdges, r.newNodes) = graph.splitBySupport(support, o.cutoff);   // :272-316
    graph.simplifyGraph();                                                                           // :318
    for (uint32_t round = 0; o.resolve && round < o.resolveRounds; round++) {                        // this project's own: repeats longer than k
        auto positions = graph.getGraphMap();                                                        // of the graph as it is NOW
        genome::Spans spans(ctx);
        PairedResult::ResolveRound x;
        x.spans = graph.threadSpans(positions, spans, data, takeFirst);
        x.split = graph.splitEdgesBySpans(spans, o.spanCutoff());
        r.resolved.push_back(x);
        std::fprintf(stderr, "resolve-repeats round %u (cutoff %u): thread_spans %s; split_edges %s\n", round + 1, o.spanCutoff(),
                     jsonNamed(genome::Graph::spanStatNames, x.spans.v, 5).c_str(), jsonNamed(genome::Graph::splitEdgeStatNames, x.split.v, 7).c_str());
        if (!x.split.v[1]) break;                                                                    // nothing resolved: the graph is as it was
        graph.simplifyGraph();
    }
    return r;
}

// --links PATH [--link-min-support N] [--link-min-len N] [--scaffolds PATH]: scaffold links of the FINAL graph (include/genome_amd.h,
// "scaffold links"; this project's own rule), after the paired-end stage.  One GPU.
// --scaffold-fasta PATH [--scaffold-min-gap N] [--scaffold-width N] [--scaffold-both-strands]: the chains of those links as FASTA
// (include/genome_amd.h, "scaffolds"), the edges in no chain after them; --link-min-len is the singletons' length filter too.
// --fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N] (with --scaffolds or --scaffold-fasta): the chains go through
// gk_graph_fill_gaps first (include/genome_amd.h, "gap filling"), and both files are written from the filled chains.
// --overlap-gaps [TOL] [--overlap-min N] [--overlap-max N] (with --scaffolds or --scaffold-fasta): the chains, after --fill-gaps when
// both are given (a graph path is the stronger evidence, and the junctions it leaves are the ones searched), go through
// gk_graph_overlap_gaps (include/genome_amd.h, "overlap detection"); the FASTA joins an overlapped junction on its o bases, and
// the id list shows -o as its gap.
// --judge GENOME.fasta [--judge-tol N] (with --scaffold-fasta): the edges of the final graph are placed on the reference (plain FASTA
// text) with the links' position map, and every junction of the plan that was written is judged (include/genome_amd.h,
// "placements" and "the judge").  N defaults to the fill / overlap TOL, half the width of the insert range: a choice, not a
// measurement.
// --blocks [--block-tol N] [--block-rows PATH]: the edges of the graph aligned to the reference in blocks and every breakpoint classed
// (include/genome_amd.h, "alignment blocks" and "breakpoints").  N defaults to 1000: a choice, not a measurement.  PATH gets one
// text line per row.  check_graph takes them beside its FASTA; graph_simplifier and graph_builder --walk-pairs beside --judge, whose
// FASTA they read.
struct BlockOpts {
    bool blocks = false;
    int64_t tol = -1;                             // -1: 1000; a choice, not a measurement
    std::string rows;
    bool parse(Args &a) {
        if (a.flag("--blocks")) { blocks = true; return true; }
        return a.value("--block-tol", tol) || a.value("--block-rows", rows);
    }
    bool check() const {
        if (!blocks && tol != -1) { std::fprintf(stderr, "--block-tol N goes with --blocks\n"); return false; }
        if (!blocks && !rows.empty()) { std::fprintf(stderr, "--block-rows PATH goes with --blocks\n"); return false; }
        if (tol < -1) { std::fprintf(stderr, "--block-tol N needs N >= 0\n"); return false; }
        return true;
    }
    uint64_t tolerance() const { return tol >= 0 ? (uint64_t)tol : 1000; }
};
struct LinkOpts {
    std::string path, scaffolds, scaffoldFasta;
    uint32_t minSupport = 3;
    uint64_t minLen = 0;
    int64_t scaffoldMinGap = 10;                  // a choice, not a measurement
    uint32_t scaffoldWidth = 60;
    bool scaffoldBoth = false;
    bool fillGaps = false;
    int64_t fillTol = -1;                         // -1: half the width of the insert range the stage used; a choice, not a measurement
    uint32_t fillMaxEdges = 16, fillMaxPaths = 256;   // choices, not measurements
    bool overlapGaps = false;
    int64_t overlapTol = -1;                      // -1: as fillTol
    uint32_t overlapMin = 10, overlapMax = 0;     // 0: k.  Choices, not measurements: a chance match of 10 bases is about 1e-6 per candidate
    std::string judge;                            // --judge: the reference FASTA
    int64_t judgeTol = -1;                        // -1: as fillTol; a choice, not a measurement
    BlockOpts block;                              // --blocks [--block-tol N] [--block-rows PATH], beside --judge
    bool parse(Args &a) {
        if (block.parse(a)) return true;
        if (a.flag("--scaffold-both-strands")) { scaffoldBoth = true; return true; }
        if (a.optional("--fill-gaps", fillTol)) { fillGaps = true; return true; }
        if (a.value("--fill-max-edges", fillMaxEdges) || a.value("--fill-max-paths", fillMaxPaths)) return true;
        if (a.optional("--overlap-gaps", overlapTol)) { overlapGaps = true; return true; }
        if (a.value("--overlap-min", overlapMin) || a.value("--overlap-max", overlapMax)) return true;
        if (a.value("--judge", judge) || a.value("--judge-tol", judgeTol)) return true;
        return a.value("--links", path) || a.value("--link-min-support", minSupport) || a.value("--link-min-len", minLen) || a.value("--scaffolds", scaffolds) ||
               a.value("--scaffold-fasta", scaffoldFasta) || a.value("--scaffold-min-gap", scaffoldMinGap) || a.value("--scaffold-width", scaffoldWidth);
    }
    bool wanted() const { return !path.empty(); }
    bool check(int world) const {
        if (path.empty() && !scaffolds.empty()) { std::fprintf(stderr, "--scaffolds PATH goes with --links PATH\n"); return false; }
        if (path.empty() && !scaffoldFasta.empty()) { std::fprintf(stderr, "--scaffold-fasta PATH goes with --links PATH\n"); return false; }
        if (fillGaps && scaffolds.empty() && scaffoldFasta.empty()) { std::fprintf(stderr, "--fill-gaps goes with --scaffolds PATH or --scaffold-fasta PATH\n"); return false; }
        if (overlapGaps && scaffolds.empty() && scaffoldFasta.empty()) { std::fprintf(stderr, "--overlap-gaps goes with --scaffolds PATH or --scaffold-fasta PATH\n"); return false; }
        if (!judge.empty() && scaffoldFasta.empty()) { std::fprintf(stderr, "--judge GENOME.fasta goes with --scaffold-fasta PATH\n"); return false; }
        if (judge.empty() && judgeTol != -1) { std::fprintf(stderr, "--judge-tol N goes with --judge GENOME.fasta\n"); return false; }
        if (judgeTol < -1) { std::fprintf(stderr, "--judge-tol N needs N >= 0\n"); return false; }
        if (!block.check()) return false;
        if (block.blocks && judge.empty()) { std::fprintf(stderr, "--blocks goes with --judge GENOME.fasta\n"); return false; }
        if (wanted() && world) { std::fprintf(stderr, "--links runs on one GPU only (not with --world): export per rank and add the tables\n"); return false; }
        return true;
    }
};
struct LinkResult {
    genome::Graph::LinkClasses classes;
    genome::Links::JoinStats joins;
    uint64_t mid = 0, maxSpan = 0, chains = 0, cycles = 0;
    std::string scaffoldsJson;                    // the stats of --scaffold-fasta's text; empty without the flag
    std::string fillJson;                         // --fill-gaps: tol, the two limits and the ten stats; empty without the flag
    std::string overlapJson;                      // --overlap-gaps: tol, the two bounds and the seven stats; empty without the flag
    std::string judgeJson;                        // --judge: tol, both stats arrays by name, n50 and n50_broken; empty without the flag
    std::string blocksJson;                       // --blocks: blocksStage's object; empty without the flag
    std::string json() const {
        return "{" + jsonNamed(genome::Graph::linkClassNames, classes.v, 8) + "," + jsonNamed(genome::Links::joinStatNames, joins.v, 5) + ",\"mid\":" +
               std::to_string(mid) + ",\"max_span\":" + std::to_string(maxSpan) + ",\"chains\":" + std::to_string(chains) + ",\"cycles\":" + std::to_string(cycles) + "}";
    }
};
// The records of a FASTA text as joined sequence characters, by the record rule of the FASTA check with per_line == 0
// (include/genome_amd.h): a line ends at "\n", "\r" or "\r\n"; a line that starts with '>' is a header and starts a record; sequence
// characters before the first header are record 0; terminators are dropped, every other character is kept as it is.
inline std::vector<std::string> fastaRecords(const std::string &text) {
    std::vector<std::string> records;
    std::string cur;
    bool seenHeader = false;
    size_t i = 0;
    const size_t n = text.size();
    while (i < n) {
        size_t e = i;
        while (e < n && text[e] != '\n' && text[e] != '\r') e++;
        if (e > i && text[i] == '>') {
            if (seenHeader || !cur.empty()) records.push_back(cur);
            cur.clear();
            seenHeader = true;
        } else cur.append(text, i, e - i);
        i = e < n ? e + ((text[e] == '\r' && e + 1 < n && text[e + 1] == '\n') ? 2 : 1) : e;
    }
    if (seenHeader || !cur.empty()) records.push_back(cur);
    return records;
}
// --blocks: the records aligned at o's tol with `positions` (of the graph as it is now); one line to stderr, the rows to o.rows if
// given -> {"tol", "stats": the 24 by name, "genome_fraction": covered / windows, "na50", "nga50"}
inline std::string blocksStage(const genome::Graph &graph, genome::PositionMap &positions, const std::vector<std::string> &records, const BlockOpts &o) {
    const uint64_t tol = o.tolerance();
    const auto b = graph.alignBlocks(positions, records, tol);
    const auto st = b.stats();
    const auto n = b.na50();
    const double fraction = st.v[3] ? (double)st.v[4] / (double)st.v[3] : 0.0;
    typedef unsigned long long ull;
    std::fprintf(stderr, "blocks: tol %llu (%s), %llu rows on %llu edges: %llu exact, %llu colinear, %llu indel, %llu misassembled, %llu repeat, %llu unaligned; "
                         "genome fraction %.6f, NA50 %llu, NGA50 %llu\n", (ull)tol, o.tol >= 0 ? "given" : "the default, a choice", (ull)st.v[5],
                 (ull)(st.v[13] + st.v[14] + st.v[15] + st.v[16] + st.v[17]), (ull)st.v[17], (ull)st.v[16], (ull)st.v[15], (ull)st.v[14], (ull)st.v[13], (ull)st.v[12],
                 fraction, (ull)n.first, (ull)n.second);
    if (!o.rows.empty()) {
        const auto r = b.rows();
        std::ofstream rf(o.rows);
        rf << "# alignment blocks of the graph's edges on the reference, in the rule's order (include/genome_amd.h); tol " << tol << "\n"
           << "# brk: 0 first, 1 overlap, 2 translocation, 3 inversion, 4 relocation, 5 indel, 6 colinear\n"
           << "# edge\tstrand\trecord\tpos\tdlo\tdhi\tbrk\tshift\n";
        for (size_t i = 0; i < r.edge.size(); i++)
            rf << r.edge[i] << "\t" << (int)r.strand[i] << "\t" << r.record[i] << "\t" << r.pos[i] << "\t" << r.dlo[i] << "\t" << r.dhi[i] << "\t" << (int)r.brk[i] << "\t"
               << r.shift[i] << "\n";
        if (!rf) throw std::runtime_error("cannot write " + o.rows);
    }
    char frac[40];
    std::snprintf(frac, sizeof frac, "%.17g", fraction);
    return jsonObject("tol", tol, "stats", "{" + jsonNamed(genome::Blocks::statNames, st.v, GK_BLOCKS_NSTATS) + "}", "genome_fraction", std::string(frac), "na50", n.first,
                      "nga50", n.second);
}
// lengths descending, the first at which twice the running sum reaches the total (gk_graph_contig_stats' n50); 0 for none
inline uint64_t n50Of(std::vector<uint64_t> lengths) {
    std::sort(lengths.rbegin(), lengths.rend());
    uint64_t total = 0, run = 0;
    for (const uint64_t x : lengths) total += x;
    for (const uint64_t x : lengths) {
        run += x;
        if (2 * run >= total) return x;
    }
    return 0;
}
// From the segment rows and the junction classes: the N50 of the records as written, and the N50 after every record is broken at
// each misjoin (the N run of a broken junction belongs to neither piece).
inline std::pair<uint64_t, uint64_t> scaffoldN50s(const std::vector<genome::Scaffolds::Segment> &rows, const std::vector<uint8_t> &classes) {
    std::vector<uint64_t> whole, broken;
    uint64_t start = 0, piece = 0;
    size_t j = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        if (i == 0 || rows[i - 1].record != rows[i].record) start = piece = rows[i].first;
        else if (genome::Scaffolds::Judged::misjoin(classes[j - 1])) {
            broken.push_back(rows[i - 1].first + rows[i - 1].bases - piece);
            piece = rows[i].first;
        }
        if (i + 1 == rows.size() || rows[i + 1].record != rows[i].record) {
            whole.push_back(rows[i].first + rows[i].bases - start);
            broken.push_back(rows[i].first + rows[i].bases - piece);
        } else j++;
    }
    return {n50Of(whole), n50Of(broken)};
}
// gap of a link = mid - floor(sum_u / count), signed
inline long long linkGap(uint64_t mid, uint32_t count, uint64_t sumU) { return (long long)mid - (long long)(sumU / (count ? count : 1)); }
// `walked`: what the paired-end stage measured (null: no such stage ran, the range is o's as given).  max_span = range_hi + k;
// mid = the median of an estimated range, else (lo + hi) div 2 of the range in force (the fallback 180..250 included).
inline LinkResult linksStage(genome::Graph &graph, genome::Context &ctx, const genome::PairedEndData &data, uint64_t takeFirst, const LinkOpts &lo,
                             const PairedOpts &o, const PairedResult *walked) {
    LinkResult r;
    const bool measured = walked && o.rangeAuto;
    const uint64_t rlo = measured ? walked->range.lo : (uint64_t)o.lo, rhi = measured ? walked->range.hi : (uint64_t)o.hi;
    const bool median = measured && walked->range.estimated;
    r.mid = median ? walked->range.median : (rlo + rhi) / 2;
    r.maxSpan = rhi + (uint64_t)graph.k();
    std::fprintf(stderr, "links: max_span %llu = %llu + k, gap = %llu - floor(sum_u / count): %s\n", (unsigned long long)r.maxSpan, (unsigned long long)rhi,
                 (unsigned long long)r.mid, median ? "the median of the estimated insert range" :
                 measured ? "the middle of the fallback range (no estimate)" : "the middle of the given range");
    auto positions = graph.getGraphMap();                                                            // of the graph as it is NOW
    genome::Links links(ctx);
    r.classes = graph.pairLinks(positions, links, data, takeFirst, lo.minLen, r.maxSpan);
    auto all = links.exportAll();
    std::vector<size_t> order(all.e1.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::make_pair(all.e1[a], all.e2[a]) < std::make_pair(all.e1[b], all.e2[b]); });
    std::ofstream lf(lo.path);
    lf << "# scaffold links: pair orientations whose mates lie on two different edges of the final graph (ids as in --contigs / --save-graph)\n"
       << "# min_len " << lo.minLen << " max_span " << r.maxSpan << " mid " << r.mid << "; gap = mid - floor(sum_u / count), negative: the contigs overlap\n"
       << "# e1\te2\tcount\tsum_u\tgap\n";
    for (const size_t i : order)
        lf << all.e1[i] << "\t" << all.e2[i] << "\t" << all.count[i] << "\t" << all.sumU[i] << "\t" << linkGap(r.mid, all.count[i], all.sumU[i]) << "\n";
    if (!lf) throw std::runtime_error("cannot write " + lo.path);
    const auto joins = links.joins(lo.minSupport, &r.joins);
    uint64_t cycles = 0;
    const auto chains = genome::scaffoldChains(joins.e1, joins.e2, &cycles);
    r.chains = chains.size(); r.cycles = cycles;
    // the gap after every member that joins the next (the closing gap of a cycle stays with the joins: `closing` below)
    std::map<std::pair<uint32_t, uint32_t>, int64_t> gapOf;
    for (size_t i = 0; i < joins.e1.size(); i++) gapOf[{joins.e1[i], joins.e2[i]}] = linkGap(r.mid, joins.count[i], joins.sumU[i]);
    std::vector<std::vector<uint32_t>> members = chains;
    std::vector<std::vector<int64_t>> gaps(chains.size());
    for (size_t c = 0; c < chains.size(); c++)
        for (size_t j = 0; j + 1 < chains[c].size(); j++) gaps[c].push_back(gapOf.at({chains[c][j], chains[c][j + 1]}));
    if (lo.fillGaps) {                                                                               // both files come from the filled chains
        const uint64_t tol = lo.fillTol >= 0 ? (uint64_t)lo.fillTol : (rhi - rlo) / 2;
        auto f = graph.fillGaps(members, gaps, tol, lo.fillMaxEdges, lo.fillMaxPaths);
        std::fprintf(stderr, "fill-gaps: tol %llu (%s), %llu of %llu junctions filled with %llu edges\n", (unsigned long long)tol,
                     lo.fillTol >= 0 ? "given" : "half the width of the insert range", (unsigned long long)f.v[6], (unsigned long long)f.v[0], (unsigned long long)f.v[7]);
        r.fillJson = "{\"tol\":" + std::to_string(tol) + ",\"max_edges\":" + std::to_string(lo.fillMaxEdges) + ",\"max_paths\":" + std::to_string(lo.fillMaxPaths) + "," +
                     f.json().substr(1);
        members = std::move(f.chains); gaps = std::move(f.gaps);
    }
    std::vector<std::vector<uint32_t>> overlaps;
    if (lo.overlapGaps) {                                                                            // after --fill-gaps: the junctions it left
        const uint64_t tol = lo.overlapTol >= 0 ? (uint64_t)lo.overlapTol : (rhi - rlo) / 2;
        const uint32_t omax = lo.overlapMax ? lo.overlapMax : (uint32_t)graph.k();
        auto ov = graph.overlapGaps(members, gaps, tol, lo.overlapMin, omax);
        std::fprintf(stderr, "overlap-gaps: tol %llu (%s), overlaps of %u to %u bases: %llu of %llu junctions overlap by %llu bases together\n", (unsigned long long)tol,
                     lo.overlapTol >= 0 ? "given" : "half the width of the insert range", lo.overlapMin, omax, (unsigned long long)ov.v[5], (unsigned long long)ov.v[0],
                     (unsigned long long)ov.v[6]);
        r.overlapJson = "{\"tol\":" + std::to_string(tol) + ",\"min_overlap\":" + std::to_string(lo.overlapMin) + ",\"max_overlap\":" + std::to_string(omax) + "," +
                        ov.json().substr(1);
        overlaps = std::move(ov.overlaps);
    }
    if (!lo.scaffolds.empty()) {
        std::ofstream sf(lo.scaffolds);
        sf << "# scaffold chains: maximal paths of joins (the only link of at least " << lo.minSupport << " observations out of one edge and into the next)\n"
           << "# both strands' chains appear, as --contigs --contig-both-strands shows the edges: a chain and the chain of its twins are the same scaffold\n"
           << "# s<i>\t<members>\te<id>\t<gap>\te<id>...; a cycle starts at its smallest id and ends with the closing gap and the word cycle\n";
        if (lo.fillGaps) sf << "# --fill-gaps: members between two joined edges are the one path the graph holds there; the gap at such a junction is -k\n";
        if (lo.overlapGaps) sf << "# --overlap-gaps: where the end of a member and the start of the next spell the same o bases, the gap at that junction is -o\n";
        for (size_t i = 0; i < members.size(); i++) {
            const auto &c = members[i];
            sf << "s" << i << "\t" << c.size();
            for (size_t j = 0; j < c.size(); j++) {
                sf << "\te" << c[j];
                if (j + 1 < c.size()) sf << "\t" << (lo.overlapGaps && overlaps[i][j] ? -(int64_t)overlaps[i][j] : gaps[i][j]);
            }
            const auto closing = gapOf.find({c.back(), c.front()});                                  // the last member of a path joins nothing
            if (closing != gapOf.end()) sf << "\t" << closing->second << "\tcycle";
            sf << "\n";
        }
        if (!sf) throw std::runtime_error("cannot write " + lo.scaffolds);
    }
    if (!lo.scaffoldFasta.empty()) {
        auto sc = lo.overlapGaps ? graph.scaffolds(members, gaps, overlaps, lo.scaffoldMinGap, lo.minLen, lo.scaffoldWidth, lo.scaffoldBoth, true)
                                 : graph.scaffolds(members, gaps, lo.scaffoldMinGap, lo.minLen, lo.scaffoldWidth, lo.scaffoldBoth, true);
        sc.write(lo.scaffoldFasta);
        r.scaffoldsJson = sc.stats().json();
        if (!lo.judge.empty()) {                                                                     // the plan that was written, on the final graph
            const uint64_t tol = lo.judgeTol >= 0 ? (uint64_t)lo.judgeTol : (rhi - rlo) / 2;
            const std::vector<uint8_t> text = readBin(lo.judge);
            const std::vector<std::string> records = fastaRecords(std::string(text.begin(), text.end()));
            const auto placements = graph.place(positions, records);
            const auto pst = placements.stats();
            const auto jd = sc.judge(placements, tol);
            const auto n50 = scaffoldN50s(sc.segments(), jd.classes);
            std::fprintf(stderr, "judge: tol %llu (%s), %llu junctions: %llu correct, %llu unjudged, %llu misjoins (other_record %llu, strand %llu, order %llu, distance %llu); "
                                 "N50 %llu, %llu broken at the misjoins\n", (unsigned long long)tol, lo.judgeTol >= 0 ? "given" : "half the width of the insert range",
                         (unsigned long long)jd.v[0], (unsigned long long)jd.v[6], (unsigned long long)jd.v[1], (unsigned long long)(jd.v[2] + jd.v[3] + jd.v[4] + jd.v[5]),
                         (unsigned long long)jd.v[2], (unsigned long long)jd.v[3], (unsigned long long)jd.v[4], (unsigned long long)jd.v[5], (unsigned long long)n50.first,
                         (unsigned long long)n50.second);
            r.judgeJson = jsonObject("tol", tol, "placements", "{" + jsonNamed(genome::Placements::statNames, pst.v, GK_PLACE_NSTATS) + "}", "stats",
                                     "{" + jsonNamed(genome::Scaffolds::judgeStatNames, jd.v, GK_JUDGE_NSTATS) + "}", "classes", jsonList(std::vector<uint32_t>(jd.classes.begin(), jd.classes.end())),
                                     "err", jsonList(jd.err), "n50", n50.first, "n50_broken", n50.second);
            if (lo.block.blocks) r.blocksJson = blocksStage(graph, positions, records, lo.block);
        }
    }
    return r;
}
