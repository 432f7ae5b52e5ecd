// graph_builder.cpp — C++ twin of GraphBuilder.startup (S/scripts/GraphBuilder.scala:18-59) over
// genome.hpp: counts k-mers of a `.bin` read stream on the GPU, drops k-mers seen < rounds times,
// builds the de Bruijn graph, keeps the largest component, and writes the graph as text.
// The reference logs its counters through akka Logging (:34-53); here they are one JSON object.
//
//   graph_builder <reads.bin> <pairs> <k> [--rounds 3 | --rounds auto] [--spectrum PATH] [--take-first N] [--prefilter DISTINCT] [--no-retain] [--simplify]
//                 [--clip-tips [MAXLEN|auto]] [--pop-bubbles [MAXDIFF|auto]] [--bubble-max-len N] [--edge-coverage] [--walk-pairs CUTOFF LO HI | --walk-pairs CUTOFF auto [--max-insert N]]
//                 [--out prefix] [--save-graph PATH] [--correct N|auto]
//                 [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]]
//   graph_builder --fastq <reads.fastq> <k> [--split N | --interleaved] [the options above]
//   --fastq converts the FASTQ file on the GPU first (Convert2bin, gk_fastq; --split N = its n, default 36) and takes the pair
//   count from the conversion; the flow is then the same.  Not with --world (exit 2): convert2bin the file first.
//   --rounds auto takes the k-mer count spectrum of the counted table on the GPU (gk_map_spectrum; over --world the spectrum reduced
//   over the ranks, so that every rank filters alike) and uses its valley as the cutoff (gk_spectrum_cutoff; behind --prefilter
//   with min_count = 2); a spectrum without a valley falls back to the reference's 3 and the JSON says "rounds_auto":false.
//   --spectrum PATH writes that spectrum as one `count<TAB>keys` line per non-empty bin, the overflow bin as `>=N` (rank 0).
//   With either flag the JSON gains "rounds_auto", "valley", "peak" and "genome_size_estimate"; "rounds" is the number used.
//   --clip-tips removes dead-end tips by edge coverage (gk_graph_clip_tips: this project's own rule, the reference has none) after
//   the retain and before --simplify's two steps: clip, then simplifyGraph, repeated until a round removes nothing, 8 rounds at
//   most; MAXLEN = the longest edge a tip may be (auto, the default: 2k).  The JSON gains "clip_tips":{"max_len","removed":[per round]}.
//   --edge-coverage, with --out, writes <prefix>.coverage.txt: per live edge of the final graph, ascending ids, one line
//   `edge id, len, kmers, sum, min, max` (gk_graph_edge_coverage).  Neither runs with --world (exit 2).
//   --pop-bubbles removes the weaker of two similar parallel edges (gk_graph_pop_bubbles: this project's own rule; --simplify's
//   removeBubbles is the reference's and stays) in the same rounds: clip if asked, pop if asked, then simplifyGraph, until a
//   round removes nothing, 8 rounds at most.  MAXDIFF = the edit distance two branches may be apart (auto, the default: 3, at most
//   31); --bubble-max-len N = the longest edge a branch may be (default 2k).  The JSON gains
//   "pop_bubbles":{"max_len","max_diff","removed":[per round],"pairs":[per round]}.  Not with --world (exit 2).
//   --correct N|auto corrects the reads before they are counted (gk_reads_correct: this project's own rule, the reference has none):
//   count, correct the stream in host memory against that count (solid = N, or the valley of its spectrum; 3 when it has none),
//   then count the corrected stream and go on as without the flag — --rounds auto sees the second spectrum, and --walk-pairs walks
//   the corrected mates.  The JSON gains "correct":{"solid","solid_auto",the ten statistics}.  Not with --world (exit 2).
//   --simplify runs removeBubbles + simplifyGraph (GraphSimplifier.scala:317-318) before writing;
//   --walk-pairs runs GraphSimplifier.startup's paired-end stage on the graph GraphBuilder hands over (:188-318): position
//   map, the pairs' walks with range LO to HI (the reference: 180 to 250, :146), node split at genome.cutoff = CUTOFF,
//   removeEdge, simplifyGraph; its counters join the JSON;
//   --out writes <prefix>.nodes.txt, .edges.txt, .contigs (GraphSimplifier.scala:338-347) and .dot (Graph.scala:74-88)
//   --contigs PATH writes the final graph's contigs as FASTA on the device (gk_graph_contigs_plan / gk_contigs_write: this project's
//   own rule, beside --out's .contigs, which stays the reference's): one record `>e<id> len=<n> cov=<mean>` per live edge whose path
//   is not above its reverse complement (--contig-both-strands: every live edge), n >= --contig-min-len (default 0), lines of
//   --contig-width bases (default 60, 0 = one line); the coverage comes from the table the graph was built from.  The JSON gains
//   "contigs_fasta":{the nine stats}.  Over --world rank 0 writes.  (Where the two strands of the genome are separate components,
//   the retain keeps one of them and its edges may be the reverse ones, which one strand per contig leaves to their dead twins:
//   "forward" != "reverse" in the stats says so; --contig-both-strands or --no-retain writes them.)
//   --save-graph writes the same graph as a graph file (gk_graph_save; GraphBuilder.scala:55-56) for graph_simplifier
//   --world W --rank R --id-file PATH: one rank of W (one process per rank, on device R % gk_device_count()).  Rank 0 writes the
//   communicator id to PATH (a file that must not exist yet: written aside, then renamed), the others wait for it (2 minutes at
//   most).  Each rank counts its contiguous share of the pairs into its partition (gk_dist_count_reads), the partitions are
//   filtered and gathered into a replica of the graph on every rank, and with --walk-pairs each rank walks its share of the
//   pairs and the supports are summed over the ranks before the split.  Rank 0 alone prints the JSON (plus occurrences_sent,
//   occurrences_owned — rank 0's — and world) and writes --out.  (RCCL may print a banner line to stdout before the JSON line.)
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/graph_builder.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/graph_builder
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include <thread>

#include "genome.hpp"
#include "rank_id.hpp"

// The --fastq forms: take the FASTQ path and the split options out of argv, and leave the `.bin` form's argv in `args`
// (the reads file and pair count are filled in after the conversion).  at = argv index of "--fastq"; -> 0, or 2 for a usage error.
static int fastqArgs(int argc, char **argv, int at, std::string *fastq, int *split, std::vector<char *> *args) {
    static char empty[] = "", zero[] = "0";
    if (at + 1 >= argc) return 2;
    *fastq = argv[at + 1];
    for (int i = 0; i < argc; i++) {
        if (i == at) { args->push_back(empty); args->push_back(zero); i++; continue; }
        if (!std::strcmp(argv[i], "--split") && i + 1 < argc) { *split = std::stoi(argv[++i]); if (*split < 1) return 2; continue; }
        if (!std::strcmp(argv[i], "--interleaved")) { *split = 0; continue; }
        if (!std::strcmp(argv[i], "--world")) return 2;      // N-rank ingestion of FASTQ is not supported: convert first
        args->push_back(argv[i]);
    }
    args->push_back(nullptr);
    return 0;
}

int main(int argc, char **argv) {
    std::string fastq;
    int split = 36;
    std::vector<char *> fargs;
    const int fastq_at = argc >= 2 && !std::strcmp(argv[1], "--fastq") ? 1 : 0;
    if (fastq_at) {
        if (fastqArgs(argc, argv, fastq_at, &fastq, &split, &fargs)) {
            std::fprintf(stderr, "usage: %s --fastq <reads.fastq> <k> [--split N | --interleaved] [options of the .bin form]\n"
                                 "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n", argv[0]);
            return 2;
        }
        argc = (int)fargs.size() - 1;
        argv = fargs.data();
    }
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <reads.bin> <pairs> <k> [--rounds 3|auto] [--spectrum PATH] [--take-first N] [--prefilter DISTINCT] [--no-retain] [--simplify] "
                             "[--clip-tips [MAXLEN|auto]] [--pop-bubbles [MAXDIFF|auto]] [--bubble-max-len N] [--edge-coverage] [--walk-pairs CUTOFF LO HI | --walk-pairs CUTOFF auto [--max-insert N]] [--out prefix] [--save-graph PATH] "
                             "[--correct N|auto] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]] [--world W --rank R --id-file PATH]\n", argv[0]);
        return 2;
    }
    const std::string infile = argv[1];
    genome::PairedEndData data;
    data.count = std::stoull(argv[2]);
    const int k = std::stoi(argv[3]);
    int rounds = 3;                               // GraphBuilder.scala:30
    bool autoRounds = false;                      // --rounds auto
    uint64_t takeFirst = UINT64_MAX;              // genome.takeFirst
    uint64_t prefilter = 0;                       // expected distinct k-mers; 0 = no singleton pre-filter
    bool retain = true, simplify = false;
    bool clipTips = false, edgeCoverage = false;
    uint64_t tipMaxLen = 0;                       // 0 = auto: 2k
    bool popBubbles = false;
    uint32_t bubbleMaxDiff = 3;                   // auto: the reference's commented-out maxerrors (Graph.scala:121-123)
    uint64_t bubbleMaxLen = 0;                    // 0 = auto: 2k
    bool correct = false;                         // --correct
    uint32_t solid = 0;                           // 0 = auto: the valley of the first count's spectrum
    int walkCutoff = -1, walkLo = 180, walkHi = 250;
    bool walkAuto = false;                                   // --walk-pairs CUTOFF auto: the range is measured from the pairs (graph_simplifier --range auto)
    long maxInsert = 4095;
    std::string out, idFile, saveGraph, spectrumPath, contigsPath;
    uint64_t contigMinLen = 0;
    uint32_t contigWidth = 60;
    bool contigBoth = false;
    int world = 0, rank = 0;                      // world 0: one GPU, no communicator
    for (int i = 4; i < argc; i++) {
        if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) {
            if (!std::strcmp(argv[++i], "auto")) autoRounds = true;   // chosen from the spectrum
            else { autoRounds = false; rounds = std::stoi(argv[i]); }
        }
        else if (!std::strcmp(argv[i], "--spectrum") && i + 1 < argc) spectrumPath = argv[++i];
        else if (!std::strcmp(argv[i], "--take-first") && i + 1 < argc) takeFirst = std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--prefilter") && i + 1 < argc) prefilter = std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--no-retain")) retain = false;
        else if (!std::strcmp(argv[i], "--simplify")) simplify = true;
        else if (!std::strcmp(argv[i], "--clip-tips")) {
            clipTips = true;
            if (i + 1 < argc && !std::strcmp(argv[i + 1], "auto")) i++;
            else if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') tipMaxLen = std::stoull(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--pop-bubbles")) {
            popBubbles = true;
            if (i + 1 < argc && !std::strcmp(argv[i + 1], "auto")) i++;
            else if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') bubbleMaxDiff = (uint32_t)std::stoul(argv[++i]);
        }
        else if (!std::strcmp(argv[i], "--bubble-max-len") && i + 1 < argc) bubbleMaxLen = std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--edge-coverage")) edgeCoverage = true;
        else if (!std::strcmp(argv[i], "--correct") && i + 1 < argc) {
            correct = true;
            if (!std::strcmp(argv[++i], "auto")) solid = 0;
            else if ((solid = (uint32_t)std::stoul(argv[i])) == 0) { std::fprintf(stderr, "--correct N needs N >= 1 (or auto)\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--walk-pairs") && i + 2 < argc && !std::strcmp(argv[i + 2], "auto")) { walkCutoff = std::stoi(argv[++i]); walkAuto = true; i++; }
        else if (!std::strcmp(argv[i], "--max-insert") && i + 1 < argc) { maxInsert = std::stol(argv[++i]); if (maxInsert < 1 || maxInsert > 65535) { std::fprintf(stderr, "--max-insert N is 1..65535\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--walk-pairs") && i + 3 < argc) { walkCutoff = std::stoi(argv[++i]); walkLo = std::stoi(argv[++i]); walkHi = std::stoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
        else if (!std::strcmp(argv[i], "--save-graph") && i + 1 < argc) saveGraph = argv[++i];
        else if (!std::strcmp(argv[i], "--contigs") && i + 1 < argc) contigsPath = argv[++i];
        else if (!std::strcmp(argv[i], "--contig-min-len") && i + 1 < argc) contigMinLen = std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--contig-width") && i + 1 < argc) contigWidth = (uint32_t)std::stoul(argv[++i]);
        else if (!std::strcmp(argv[i], "--contig-both-strands")) contigBoth = true;
        else if (!std::strcmp(argv[i], "--world") && i + 1 < argc) world = std::stoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--rank") && i + 1 < argc) rank = std::stoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--id-file") && i + 1 < argc) idFile = argv[++i];
        else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if (world && (world < 1 || rank < 0 || rank >= world || idFile.empty())) {
        std::fprintf(stderr, "--world W needs --rank R (0 <= R < W) and --id-file PATH\n");
        return 2;
    }
    if (world && prefilter) {
        std::fprintf(stderr, "--prefilter runs on one GPU only (not with --world)\n");
        return 2;
    }
    if (world && (clipTips || edgeCoverage)) {
        std::fprintf(stderr, "--clip-tips and --edge-coverage run on one GPU only (not with --world)\n");
        return 2;
    }
    if (world && correct) {
        std::fprintf(stderr, "--correct runs on one GPU only (not with --world)\n");
        return 2;
    }
    if (world && popBubbles) {
        std::fprintf(stderr, "--pop-bubbles runs on one GPU only (not with --world)\n");
        return 2;
    }
    if (popBubbles && bubbleMaxDiff > 31) {
        std::fprintf(stderr, "--pop-bubbles MAXDIFF is at most 31\n");
        return 2;
    }
    if (clipTips && !tipMaxLen) tipMaxLen = 2 * (uint64_t)k;
    if (popBubbles && !bubbleMaxLen) bubbleMaxLen = 2 * (uint64_t)k;
    try {
        if (fastq.empty()) {
            std::ifstream f(infile, std::ios::binary);
            if (!f) throw std::runtime_error("cannot open " + infile);
            data.bin.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        }
        int device = 0;
        if (world) {
            const int ndev = gk_device_count();
            if (ndev < 1) throw genome::GkError(GK_E_NODEVICE, "no GPU");
            device = rank % ndev;
        }
        genome::Context ctx(device);
        if (!fastq.empty()) data = genome::PairedEndData::fromFastq(ctx, fastq, split);     // the pair count comes from the conversion
        // --correct: a count of the reads as they are, the stream corrected against it in place, and the flow below starts over
        genome::DNAMap::CorrectStats corrected;
        bool solidAuto = false;
        if (correct) {
            const uint64_t pairs = std::min<uint64_t>(data.count, takeFirst);
            const size_t nbytes = genome::pairBytes(data, 0, pairs).second;
            genome::DNAMap raw(ctx, k);
            raw.countReads(data.bin.data(), nbytes, 2 * pairs);
            if (!solid) {
                const uint32_t valley = genome::spectrumCutoff(raw.spectrum().hist).valley;
                solidAuto = valley != 0;
                solid = solidAuto ? valley : 3;
            }
            corrected = raw.correctReads(data.bin.data(), nbytes, 2 * pairs, solid, data.bin.data());
        }
        std::unique_ptr<genome::PartitionedDNAMap> pm;
        uint64_t sent = 0, owned = 0, good = 0;
        std::unique_ptr<genome::DNAMap> kmersFreq;
        genome::FreqFilter::Chosen chosen;
        chosen.autoRounds = autoRounds;
        chosen.wantSpectrum = !spectrumPath.empty();
        const bool withSpectrum = chosen.autoRounds || chosen.wantSpectrum;
        if (world) {
            pm = std::make_unique<genome::PartitionedDNAMap>(ctx, k, rank, world, shareId(rank, idFile));
            std::tie(sent, owned) = genome::FreqFilter::extractFilteredKmers(*pm, data, rounds, takeFirst, &chosen);  // :32 over N ranks
            good = pm->size();                                                                                          // :34
            kmersFreq = std::make_unique<genome::DNAMap>(pm->gathered(true));
        } else {
            kmersFreq = std::make_unique<genome::DNAMap>(genome::FreqFilter::extractFilteredKmers(ctx, data, k, rounds, takeFirst, 0, prefilter, &chosen));   // :32
            good = kmersFreq->size();                                                                                  // :34
        }
        if (withSpectrum) rounds = chosen.rounds;
        if (rank == 0 && !spectrumPath.empty()) {
            std::ofstream sf(spectrumPath);
            const auto &h = chosen.spectrum.hist;
            for (size_t c = 1; c + 1 < h.size(); c++) if (h[c]) sf << c << "\t" << h[c] << "\n";
            if (h.back()) sf << ">=" << h.size() - 1 << "\t" << h.back() << "\n";
            if (!sf) throw std::runtime_error("cannot write " + spectrumPath);
        }
        auto graph = genome::Graph::buildGraph(k, *kmersFreq);                                           // :36
        auto [nodes, edges, totalLen] = graph.counts();                                                  // :39
        // :41-47 the two component histograms, on the graph as built (the reference computes them before retain)
        auto [hist, hist2] = graph.componentHistograms();
        uint64_t kept = nodes, comps = 0;
        if (retain) std::tie(kept, comps) = graph.retainLargestComponent();                              // :52-54
        // --clip-tips / --pop-bubbles: clip, pop, then simplifyGraph, until a round removes nothing (the counts are the table the
        // graph was built from)
        std::vector<uint64_t> tipsRemoved, bubblesRemoved, bubblePairs;
        for (int round = 0; (clipTips || popBubbles) && round < 8; round++) {
            uint64_t gone = 0;
            if (clipTips) { tipsRemoved.push_back(graph.clipTips(*kmersFreq, tipMaxLen)); gone += tipsRemoved.back(); }
            if (popBubbles) {
                const auto [removed, pairs] = graph.popBubbles(*kmersFreq, bubbleMaxLen, bubbleMaxDiff);
                bubblesRemoved.push_back(removed); bubblePairs.push_back(pairs);
                gone += removed;
            }
            if (!gone) break;
            graph.simplifyGraph();
        }
        // --simplify = GraphSimplifier.scala:317-318, applied to the graph GraphBuilder hands over (i.e. after retain)
        if (simplify) { graph.removeBubbles(); graph.simplifyGraph(); }
        uint64_t supPairs = 0, badPairs = 0, walked = 0, removedEdges = 0, newNodes = 0;
        genome::InsertRange insertEst;
        if (walkCutoff >= 0) {
            auto graphMap = graph.getGraphMap();                                                         // GraphSimplifier.scala:188
            if (walkAuto) {                                                                              // the same pairs, before walking; over the ranks one histogram
                genome::Graph::PairDistances dist;
                if (world) {
                    const auto [a, b] = genome::pairShare(data.count, takeFirst, rank, world);
                    dist = graph.pairDistances(*pm, graphMap, data, a, b, (uint32_t)maxInsert + 1);
                } else {
                    dist = graph.pairDistances(graphMap, data, takeFirst, (uint32_t)maxInsert + 1);
                }
                insertEst = genome::insertRange(dist.hist);
                walkLo = (int)insertEst.lo; walkHi = (int)insertEst.hi;
                if (rank == 0 && insertEst.estimated)
                    std::fprintf(stderr, "insert range %u to %u, median %u, from %llu observations\n", insertEst.lo, insertEst.hi, insertEst.median, (unsigned long long)insertEst.observations);
                else if (rank == 0)
                    std::fprintf(stderr, "no estimate of the insert range (%llu observations): falling back to the reference's %u to %u\n",
                                 (unsigned long long)insertEst.observations, insertEst.lo, insertEst.hi);
            }
            genome::Support support(ctx);
            if (world) {                                                                                 // this rank's pairs, then the sum over the ranks
                const auto [a, b] = genome::pairShare(data.count, takeFirst, rank, world);
                graph.walkPairs(graphMap, support, data, a, b, walkLo, walkHi);
                pm->reduceSupport(graph, support);                                                       // (before any node split)
            } else {
                graph.walkPairs(graphMap, support, data, takeFirst, walkLo, walkHi);                     // :213-263
            }
            std::tie(supPairs, badPairs, walked) = support.sizes();                                      // :266 "Bad pairs"
            std::tie(removedEdges, newNodes) = graph.splitBySupport(support, walkCutoff);                // :272-316
            graph.simplifyGraph();                                                                       // :318
        }
        auto [n2, e2, l2] = graph.counts();
        if (pm) pm->barrier();
        if (rank != 0) return 0;
        // --contigs: the text is written after the last graph stage, with the coverage of the table the graph was built from
        genome::Contigs::Stats fasta;
        if (!contigsPath.empty()) {
            auto contigs = graph.contigs(kmersFreq.get(), contigMinLen, contigWidth, contigBoth);
            contigs.write(contigsPath);
            fasta = contigs.stats();
        }
        std::printf("{\"k\":%d,\"rounds\":%d,\"good_kmers\":%llu,\"graph_nodes\":%llu,\"graph_edges\":%llu,"
                    "\"total_edges_length\":%llu,\"components\":%llu,\"max_component_size\":%llu,"
                    "\"retained_nodes\":%llu,\"retained_edges\":%llu,\"retained_edges_length\":%llu,",
                    k, rounds, (unsigned long long)good, (unsigned long long)nodes, (unsigned long long)edges,
                    (unsigned long long)totalLen, (unsigned long long)comps, (unsigned long long)kept,
                    (unsigned long long)n2, (unsigned long long)e2, (unsigned long long)l2);
        if (withSpectrum)
            std::printf("\"rounds_auto\":%s,\"valley\":%u,\"peak\":%u,\"genome_size_estimate\":%llu,", chosen.autoFound ? "true" : "false",
                        chosen.cutoff.valley, chosen.cutoff.peak, (unsigned long long)chosen.cutoff.genomeSize);
        if (correct) {
            std::string st = corrected.json();
            std::printf("\"correct\":{\"solid\":%u,\"solid_auto\":%s,%s,", solid, solidAuto ? "true" : "false", st.c_str() + 1);
        }
        if (clipTips) {
            std::printf("\"clip_tips\":{\"max_len\":%llu,\"removed\":[", (unsigned long long)tipMaxLen);
            for (size_t i = 0; i < tipsRemoved.size(); i++) std::printf("%s%llu", i ? "," : "", (unsigned long long)tipsRemoved[i]);
            std::printf("]},");
        }
        if (popBubbles) {
            std::printf("\"pop_bubbles\":{\"max_len\":%llu,\"max_diff\":%u,\"removed\":[", (unsigned long long)bubbleMaxLen, bubbleMaxDiff);
            for (size_t i = 0; i < bubblesRemoved.size(); i++) std::printf("%s%llu", i ? "," : "", (unsigned long long)bubblesRemoved[i]);
            std::printf("],\"pairs\":[");
            for (size_t i = 0; i < bubblePairs.size(); i++) std::printf("%s%llu", i ? "," : "", (unsigned long long)bubblePairs[i]);
            std::printf("]},");
        }
        if (walkCutoff >= 0 && walkAuto)
            std::printf("\"insert_range\":{\"lo\":%u,\"hi\":%u,\"estimated\":%s,\"observations\":%llu},", insertEst.lo, insertEst.hi, insertEst.estimated ? "true" : "false",
                        (unsigned long long)insertEst.observations);
        if (walkCutoff >= 0)
            std::printf("\"walk_pairs\":{\"supported_edge_pairs\":%llu,\"bad_pairs\":%llu,\"orientations_walked\":%llu,\"removed_edges\":%llu,\"new_nodes\":%llu},",
                        (unsigned long long)supPairs, (unsigned long long)badPairs, (unsigned long long)walked, (unsigned long long)removedEdges,
                        (unsigned long long)newNodes);
        if (!contigsPath.empty()) std::printf("\"contigs_fasta\":%s,", fasta.json().c_str());
        auto dump = [](const char *name, const std::map<uint64_t, uint64_t> &h, const char *tail) {
            std::printf("\"%s\":[", name);
            bool first = true;
            for (const auto &p : h) { std::printf("%s[%llu,%llu]", first ? "" : ",", (unsigned long long)p.first, (unsigned long long)p.second); first = false; }
            std::printf("]%s", tail);
        };
        dump("components_histogram", hist, ",");          // GraphBuilder.scala:42 "Components histogram"
        dump("components_histogram_2", hist2, world ? "," : "}\n");     // :47 "Components histogram 2"
        if (world) std::printf("\"occurrences_sent\":%llu,\"occurrences_owned\":%llu,\"world\":%d}\n", (unsigned long long)sent, (unsigned long long)owned, world);
        if (!saveGraph.empty()) graph.save(saveGraph);                                                   // :55-56 (a Kryo file there)
        if (!out.empty()) {
            std::ofstream nf(out + ".nodes.txt"), ef(out + ".edges.txt");
            for (const auto &n : graph.getNodes()) nf << n.toString() << "\n";
            for (const auto &e : graph.getEdges()) ef << e.start.toString() << " " << e.end.toString() << " " << e.seq << "\n";
            std::ofstream cf(out + ".contigs"), df(out + ".dot");
            graph.writeContigs(cf);
            graph.writeDot(df);
            if (edgeCoverage) {
                std::ofstream vf(out + ".coverage.txt");
                const auto c = graph.edgeCoverage(*kmersFreq);
                for (size_t i = 0; i < c.ids.size(); i++)
                    if (c.kmers[i]) vf << c.ids[i] << " " << c.kmers[i] - 1 << " " << c.kmers[i] << " " << c.sum[i] << " " << c.min[i] << " " << c.max[i] << "\n";
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "graph_builder: %s\n", e.what());
        return 1;
    }
    return 0;
}
