// check_graph.cpp — C++ twin of CheckGraph.startup (S/scripts/CheckGraph.scala:17-56) over genome.hpp: loads a graph file, computes
// the contig statistics (:37-41) and looks every k-window of a reference FASTA up in the graph's position map (:43-55).  The
// reference logs its figures; here they are one JSON object, with the keys of genome_amd.check.check_graph.
//
//   check_graph <graph.gkg> <genome.fasta> [--longer-than N] [--per-line] [--missing N] [--blocks [--block-tol N] [--block-rows PATH]]
//   --longer-than N: contigs are the edges longer than N (the reference: 200).  --per-line: windows never cross a line end (the
//   reference's literal rule); otherwise the sequence lines of a record are joined.  --missing N: list the first N windows that
//   are not found.  The rules of the check: include/genome_amd.h, "FASTA check".
//   --blocks [--block-tol N] [--block-rows PATH]: the graph's edges aligned to the reference in blocks, every breakpoint classed
//   (include/genome_amd.h, "alignment blocks" and "breakpoints"; plain FASTA text, records joined whatever --per-line says).  N
//   defaults to 1000: a choice, not a measurement.  stderr gets one line; the JSON gains "blocks":{tol, "stats":{the twenty-four
//   stats}, genome_fraction, na50, nga50}; PATH gets one text line per row.
//   --twins: the twin census of the graph's edges (include/genome_amd.h, "edge twins"): stderr gets the six stats on one line, the
//   JSON gains "twins":{live_edges, paired, self, missing, ambiguous, key_collisions}.  missing == 0: the graph is strand-closed.
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/check_graph.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/check_graph
#include "tool_common.hpp"

int main(int argc, char **argv) {
    const char *usage = "usage: %s <graph.gkg> <genome.fasta> [--longer-than N] [--per-line] [--missing N]\n";
    const char *blockUsage = "usage: %s <graph.gkg> <genome.fasta> --blocks [--block-tol N] [--block-rows PATH]   (N defaults to 1000: a choice, not a measurement)\n";
    if (argc < 3) { std::fprintf(stderr, usage, argv[0]); return 2; }
    const std::string graphFile = argv[1], fasta = argv[2];
    uint64_t longerThan = 200, maxMissing = 0;
    bool perLine = false, twins = false;
    BlockOpts block;
    for (Args a(argc, argv, 3); a.more(); a.next()) {
        if (a.value("--longer-than", longerThan) || a.value("--missing", maxMissing)) {}
        else if (a.flag("--per-line")) perLine = true;
        else if (a.flag("--twins")) twins = true;
        else if (block.parse(a)) {}
        else { std::fprintf(stderr, "unknown argument %s\n", a.cur()); std::fprintf(stderr, usage, argv[0]); return 2; }
    }
    if (!block.check()) { std::fprintf(stderr, blockUsage, argv[0]); return 2; }
    try {
        genome::Context ctx(0);
        auto graph = genome::Graph::load(ctx, graphFile);                                   // :30
        const auto contigs = graph.contigStats(longerThan);                                 // :37-41
        auto graphMap = graph.getGraphMap();                                                // :43
        genome::FastaCheck fc(ctx, graphMap, perLine, maxMissing);
        genome::forEachPiece(fasta, 64u << 20, [&](const char *p, size_t n, bool last) { fc.feed(p, n, last); });   // :48-55
        const auto st = fc.stats();
        typedef unsigned long long ull;
        std::printf("{\"k\":%d,\"longer_than\":%llu,\"per_line\":%s,"
                    "\"contigs\":{\"count\":%llu,\"sum\":%llu,\"median\":%llu,\"n50\":%llu,\"max\":%llu},"
                    "\"lines\":%llu,\"records\":%llu,\"bases\":%llu,\"valid_bases\":%llu,\"windows\":%llu,\"found\":%llu,\"missing\":%llu,"
                    "\"covered_bases\":%llu,\"short_lines\":%llu,\"coverage\":%.17g,\"missing_list\":[",
                    graph.k(), (ull)longerThan, perLine ? "true" : "false", (ull)contigs.count, (ull)contigs.sum, (ull)contigs.median, (ull)contigs.n50,
                    (ull)contigs.max, (ull)st.lines, (ull)st.records, (ull)st.bases, (ull)st.validBases, (ull)st.windows, (ull)st.found, (ull)st.missing,
                    (ull)st.coveredBases, (ull)st.shortLines, st.validBases ? (double)st.coveredBases / (double)st.validBases : 0.0);
        bool first = true;
        for (const auto &m : fc.missing()) {
            std::printf("%s{\"offset\":%llu,\"line\":%llu,\"column\":%llu,\"lo\":%llu,\"hi\":%llu}", first ? "" : ",", (ull)m.offset, (ull)m.line, (ull)m.column,
                        (ull)m.lo, (ull)m.hi);
            first = false;
        }
        std::printf("]");
        if (block.blocks) {
            const std::vector<uint8_t> text = readBin(fasta);
            std::printf(",\"blocks\":%s", blocksStage(graph, graphMap, fastaRecords(std::string(text.begin(), text.end())), block).c_str());
        }
        if (twins) {
            const auto t = graph.edgeTwins();
            std::fprintf(stderr, "twins: live_edges %llu paired %llu self %llu missing %llu ambiguous %llu key_collisions %llu\n", (ull)t.liveEdges, (ull)t.paired,
                         (ull)t.self, (ull)t.missing, (ull)t.ambiguous, (ull)t.keyCollisions);
            std::printf(",\"twins\":%s", t.json().c_str());
        }
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "check_graph: %s\n", e.what());
        return 1;
    }
    return 0;
}
