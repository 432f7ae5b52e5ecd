// graph_builder.cpp — C++ twin of GraphBuilder.startup (S/scripts/GraphBuilder.scala:18-59) over
// genome.hpp: counts k-mers of a `.bin` read stream on the GPU, drops k-mers seen < rounds times,
// builds the de Bruijn graph, keeps the largest component, and writes the graph as text.
// The reference logs its counters through akka Logging (:34-53); here they are one JSON object.
//
//   graph_builder <reads.bin> <pairs> <k> [--rounds 3 | --rounds auto] [--spectrum PATH] [--take-first N] [--prefilter DISTINCT] [--no-retain] [--simplify]
//                 [--clip-tips [MAXLEN|auto]] [--pop-bubbles [MAXDIFF|auto]] [--bubble-max-len N] [--remove-weak [RATIO] [--weak-max-len N] [--min-coverage N]] [--edge-coverage] [--walk-pairs CUTOFF LO HI | --walk-pairs CUTOFF auto [--max-insert N]] [--resolve-repeats [CUTOFF] [--resolve-rounds N]]
//                 [--links PATH [--link-min-support N] [--link-min-len N] [--scaffolds PATH] [--scaffold-fasta PATH [--scaffold-min-gap N] [--scaffold-width N] [--scaffold-both-strands]] [--fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N]] [--overlap-gaps [TOL] [--overlap-min N] [--overlap-max N]] [--judge GENOME.fasta [--judge-tol N] [--blocks [--block-tol N] [--block-rows PATH]]]]   (with --walk-pairs: graph_simplifier.cpp says what they write)
//                 [--out prefix] [--save-graph PATH] [--correct N|auto]
//                 [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]] [--seed-k K1[,K2,...]]
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
//   --remove-weak [RATIO] removes weak connections (gk_graph_remove_weak_edges: this project's own rule) in the same rounds, after
//   the clip and the pop and before the round's simplifyGraph: an edge whose start node has another way out and whose end node
//   another way in goes if at each end one of those others has more than RATIO times its mean coverage (auto, the default: 5; at
//   most 65535).  --weak-max-len N = the longest edge that may go (default 2k); --min-coverage N (only with --remove-weak) also
//   removes every edge within that length whose mean coverage is below N (default 0: off).  RATIO 5 and 2k are choices, not
//   measurements.  A round that removes anything keeps the loop going; 8 rounds at most.  The JSON gains
//   "remove_weak":{"max_len","ratio","floor","candidates":[per round],"removed_ratio":[per round],"removed_floor":[per round]},
//   stderr one line.  Not with --world (exit 2).
//   --correct N|auto corrects the reads before they are counted (gk_reads_correct: this project's own rule, the reference has none):
//   count, correct the stream in host memory against that count (solid = N, or the valley of its spectrum; 3 when it has none),
//   then count the corrected stream and go on as without the flag — --rounds auto sees the second spectrum, and --walk-pairs walks
//   the corrected mates.  The JSON gains "correct":{"solid","solid_auto",the ten statistics}.  Not with --world (exit 2).
//   --simplify runs removeBubbles + simplifyGraph (GraphSimplifier.scala:317-318) before writing;
//   --walk-pairs runs GraphSimplifier.startup's paired-end stage on the graph GraphBuilder hands over (:188-318): position
//   map, the pairs' walks with range LO to HI (the reference: 180 to 250, :146), node split at genome.cutoff = CUTOFF,
//   removeEdge, simplifyGraph; its counters join the JSON;
//   --resolve-repeats [CUTOFF] [--resolve-rounds N] (with --walk-pairs) adds graph_simplifier's rounds of gk_graph_thread_spans,
//   gk_graph_split_edges_by_spans and simplifyGraph behind that stage (graph_simplifier.cpp says what they do and print; CUTOFF
//   defaults to --walk-pairs' CUTOFF, at least 1: a choice, not a measurement).  Not with --world (exit 2).
//   --out writes <prefix>.nodes.txt, .edges.txt, .contigs (GraphSimplifier.scala:338-347) and .dot (Graph.scala:74-88)
//   --contigs PATH writes the final graph's contigs as FASTA on the device (gk_graph_contigs_plan / gk_contigs_write: this project's
//   own rule, beside --out's .contigs, which stays the reference's): one record `>e<id> len=<n> cov=<mean>` per live edge whose path
//   is not above its reverse complement (--contig-both-strands: every live edge), n >= --contig-min-len (default 0), lines of
//   --contig-width bases (default 60, 0 = one line); the coverage comes from the table the graph was built from.  The JSON gains
//   "contigs_fasta":{the nine stats}.  Over --world rank 0 writes.  (Where the two strands of the genome are separate components,
//   the retain keeps one of them and its edges may be the reverse ones, which one strand per contig leaves to their dead twins:
//   "forward" != "reverse" in the stats says so; --contig-both-strands or --no-retain writes them.)
//   --save-graph writes the same graph as a graph file (gk_graph_save; GraphBuilder.scala:55-56) for graph_simplifier
//   --gfa PATH writes the final graph as GFA 1.0 on the device (gk_graph_gfa_plan / gk_gfa_write; include/genome_amd.h, "the graph
//   as GFA"), after all edits, with KC:i: from the table the graph was built from.  The JSON gains "gfa":{the nine stats}.  Not
//   with --world (exit 2).
//   --keep-cycles keeps perfect cycles (include/genome_amd.h, "perfect cycles": this project's own rule): the build is
//   gk_graph_build_cycles and every simplifyGraph this tool runs (the clip / pop rounds, --simplify, the paired-end stage,
//   --resolve-repeats) keeps self-loop nodes and the anchors of all-interior cycles.  The JSON gains "cycles":{"build":{the six
//   stats},"simplify":{the four stats, summed}}, stderr one line.  Not with --world (exit 2).
//   --seed-k K1[,K2,...] assembles at the listed smaller ks first, each stage seeding the next one's count table with its contigs
//   (tool_common.hpp: SeedOpts; include/genome_amd.h, "multi-k"); the positional <k> stays the final stage.  The JSON gains
//   "seed_stages".  Not with --world or --prefilter (exit 2).
//   --world W --rank R --id-file PATH: one rank of W (one process per rank, on device R % gk_device_count()).  Rank 0 writes the
//   communicator id to PATH (a file that must not exist yet: written aside, then renamed), the others wait for it (2 minutes at
//   most).  Each rank counts its contiguous share of the pairs into its partition (gk_dist_count_reads), the partitions are
//   filtered and gathered into a replica of the graph on every rank, and with --walk-pairs each rank walks its share of the
//   pairs and the supports are summed over the ranks before the split.  Rank 0 alone prints the JSON (plus occurrences_sent,
//   occurrences_owned — rank 0's — and world) and writes --out.  (RCCL may print a banner line to stdout before the JSON line.)
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/graph_builder.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/graph_builder
#include "tool_common.hpp"

int main(int argc, char **argv) {
    FastqForm fastq;
    if (!fastq.parse(argc, argv, 1)) {
        std::fprintf(stderr, "usage: %s --fastq <reads.fastq> <k> [--split N | --interleaved] [options of the .bin form]\n"
                             "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n", argv[0]);
        return 2;
    }
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <reads.bin> <pairs> <k> [--rounds 3|auto] [--spectrum PATH] [--take-first N] [--prefilter DISTINCT] [--no-retain] [--simplify] "
                             "[--clip-tips [MAXLEN|auto]] [--pop-bubbles [MAXDIFF|auto]] [--bubble-max-len N] [--remove-weak [RATIO (default 5: a choice, not a measurement)] [--weak-max-len N (default 2k: a choice too)] [--min-coverage N]] [--edge-coverage] [--walk-pairs CUTOFF LO HI | --walk-pairs CUTOFF auto [--max-insert N]] [--resolve-repeats [CUTOFF] [--resolve-rounds N]] [--links PATH [--link-min-support N] [--link-min-len N] [--scaffolds PATH] [--scaffold-fasta PATH [--scaffold-min-gap N] [--scaffold-width N] [--scaffold-both-strands]] [--fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N]] [--overlap-gaps [TOL] [--overlap-min N] [--overlap-max N]] [--judge GENOME.fasta [--judge-tol N] [--blocks [--block-tol N (default 1000: a choice, not a measurement)] [--block-rows PATH]]]] [--out prefix] [--save-graph PATH] "
                             "[--correct N|auto] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]] [--gfa PATH] [--keep-cycles] [--seed-k K1[,K2,...]] [--world W --rank R --id-file PATH]\n", argv[0]);
        return 2;
    }
    const std::string infile = argv[1];
    genome::PairedEndData data;
    int k = 0;
    Args::convert("<pairs>", argv[2], data.count);
    Args::convert("<k>", argv[3], k);
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
    bool removeWeak = false, minCoverageGiven = false;
    uint32_t weakRatio = 5, weakFloor = 0;        // auto: 5 (a choice, not a measurement); --min-coverage
    uint64_t weakMaxLen = 0;                      // 0 = auto: 2k
    bool correct = false;                         // --correct
    uint32_t solid = 0;                           // 0 = auto: the valley of the first count's spectrum
    PairedOpts walk;                              // --walk-pairs: cutoff < 0 = no such stage; rangeAuto = --walk-pairs CUTOFF auto
    std::string out, saveGraph, spectrumPath;
    ContigOpts contig;
    GfaOpts gfaOpt;
    LinkOpts link;                                // --links / --scaffolds: with --walk-pairs, on the graph that stage leaves
    RankOpts ranks;
    CycleOpts cyc;                                // --keep-cycles
    SeedOpts seed;                                // --seed-k
    for (Args a(argc, argv, 4); a.more(); a.next()) {
        if (a.word("--rounds", 1, "auto")) { autoRounds = true; a.skip(); }   // chosen from the spectrum
        else if (a.value("--rounds", rounds)) autoRounds = false;
        else if (a.value("--spectrum", spectrumPath) || a.value("--take-first", takeFirst) || a.value("--prefilter", prefilter)) {}
        else if (a.flag("--no-retain")) retain = false;
        else if (a.flag("--simplify")) simplify = true;
        else if (a.optional("--clip-tips", tipMaxLen)) clipTips = true;
        else if (a.optional("--pop-bubbles", bubbleMaxDiff)) popBubbles = true;
        else if (a.value("--bubble-max-len", bubbleMaxLen)) {}
        else if (a.optional("--remove-weak", weakRatio)) removeWeak = true;
        else if (a.value("--weak-max-len", weakMaxLen)) {}
        else if (a.value("--min-coverage", weakFloor)) minCoverageGiven = true;
        else if (a.flag("--edge-coverage")) edgeCoverage = true;
        else if (a.word("--correct", 1, "auto")) { correct = true; solid = 0; a.skip(); }
        else if (a.value("--correct", solid)) {
            correct = true;
            if (!solid) { std::fprintf(stderr, "--correct N needs N >= 1 (or auto)\n"); return 2; }
        }
        else if (a.word("--walk-pairs", 2, "auto")) { a.value("--walk-pairs", walk.cutoff); walk.rangeAuto = true; a.skip(); }
        else if (a.value("--max-insert", walk.maxInsert)) { if (!walk.maxInsertOk()) { std::fprintf(stderr, "--max-insert N is 1..65535\n"); return 2; } }
        else if (a.value("--walk-pairs", walk.cutoff, walk.lo, walk.hi)) {}
        else if (walk.parseResolve(a)) {}
        else if (a.value("--out", out) || a.value("--save-graph", saveGraph) || contig.parse(a) || gfaOpt.parse(a) || link.parse(a) || ranks.parse(a) || cyc.parse(a) || seed.parse(a)) {}
        else { std::fprintf(stderr, "unknown argument %s\n", a.cur()); return 2; }
    }
    if (!ranks.check() || !link.check(ranks.world) || !gfaOpt.check(ranks.world) || !walk.checkResolve(ranks.world) || !cyc.check(ranks.world) || !seed.check(ranks.world, prefilter != 0, k)) return 2;
    if (walk.resolve && walk.cutoff < 0) {
        std::fprintf(stderr, "--resolve-repeats goes with --walk-pairs (it runs behind the paired-end stage)\n");
        return 2;
    }
    if (link.wanted() && walk.cutoff < 0) {
        std::fprintf(stderr, "--links goes with --walk-pairs (the links are those of the graph the paired-end stage leaves)\n");
        return 2;
    }
    const int world = ranks.world, rank = ranks.rank;
    const char *oneGpu = prefilter ? "--prefilter runs" : clipTips || edgeCoverage ? "--clip-tips and --edge-coverage run" :
                         correct ? "--correct runs" : popBubbles ? "--pop-bubbles runs" : removeWeak ? "--remove-weak runs" : nullptr;
    if (world && oneGpu) {
        std::fprintf(stderr, "%s on one GPU only (not with --world)\n", oneGpu);
        return 2;
    }
    if (popBubbles && bubbleMaxDiff > 31) {
        std::fprintf(stderr, "--pop-bubbles MAXDIFF is at most 31\n");
        return 2;
    }
    if (removeWeak && weakRatio > 65535) {
        std::fprintf(stderr, "--remove-weak RATIO is at most 65535\n");
        return 2;
    }
    if (minCoverageGiven && !removeWeak) {
        std::fprintf(stderr, "--min-coverage goes with --remove-weak (it is that step's floor)\n");
        return 2;
    }
    const uint64_t tipGiven = tipMaxLen, bubbleGiven = bubbleMaxLen, weakGiven = weakMaxLen;      // (0 = auto: 2k of the stage that clips)
    if (clipTips && !tipMaxLen) tipMaxLen = 2 * (uint64_t)k;
    if (popBubbles && !bubbleMaxLen) bubbleMaxLen = 2 * (uint64_t)k;
    if (removeWeak && !weakMaxLen) weakMaxLen = 2 * (uint64_t)k;
    struct WeakRounds { std::vector<uint64_t> candidates, removedRatio, removedFloor; };
    // --clip-tips / --pop-bubbles / --remove-weak: clip, pop, remove weak connections, then simplifyGraph, until a round removes
    // nothing, 8 rounds at most (the counts are the table the graph was built from)
    auto cleanRounds = [&](genome::Graph &graph, genome::DNAMap &counts, uint64_t tipLen, uint64_t bubbleLen, uint64_t weakLen, std::vector<uint64_t> &tipsRemoved,
                           std::vector<uint64_t> &bubblesRemoved, std::vector<uint64_t> &bubblePairs, WeakRounds &weak) {
        for (int round = 0; (clipTips || popBubbles || removeWeak) && round < 8; round++) {
            uint64_t gone = 0;
            if (clipTips) { tipsRemoved.push_back(graph.clipTips(counts, tipLen)); gone += tipsRemoved.back(); }
            if (popBubbles) {
                const auto [removed, pairs] = graph.popBubbles(counts, bubbleLen, bubbleMaxDiff);
                bubblesRemoved.push_back(removed); bubblePairs.push_back(pairs);
                gone += removed;
            }
            if (removeWeak) {
                const auto w = graph.removeWeakEdges(counts, weakLen, weakRatio, weakFloor);
                weak.candidates.push_back(w.candidates); weak.removedRatio.push_back(w.removedRatio); weak.removedFloor.push_back(w.removedFloorOnly);
                gone += w.removed;
            }
            if (!gone) break;
            graph.simplifyGraph();
        }
    };
    try {
        if (fastq.path.empty()) data.bin = readBin(infile);
        genome::Context ctx(ranks.device());
        if (!fastq.path.empty()) data = genome::PairedEndData::fromFastq(ctx, fastq.path, fastq.split);     // the pair count comes from the conversion
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
        // --seed-k: the seed stages, each seeded by the graph the one before left; `seedInto` is what a stage's count calls between
        // its count and its deleteAll
        std::unique_ptr<genome::DNAMap> seedMap;
        std::unique_ptr<genome::Graph> seedGraph;
        int stageRounds = 0;
        uint64_t stageBefore = 0, stageAfter = 0;
        genome::DNAMap::GraphPathStats stageStats;
        const auto seedInto = [&](genome::DNAMap &table, int r) {
            stageRounds = r;
            stageStats = {};
            stageBefore = table.size();
            if (seedGraph) stageStats = table.addGraphPaths(*seedGraph, (uint32_t)r);
            seedGraph.reset();
            seedMap.reset();
            stageAfter = table.size();
        };
        for (const int sk : seed.ks) {
            genome::FreqFilter::Chosen ch;
            ch.autoRounds = autoRounds;
            auto m = std::make_unique<genome::DNAMap>(genome::FreqFilter::extractFilteredKmers(ctx, data, sk, rounds, takeFirst, 0, 0, &ch, seedInto));
            auto g = std::make_unique<genome::Graph>(genome::Graph::buildGraph(sk, *m, cyc.keep));
            std::vector<uint64_t> t, b, p;
            WeakRounds w;
            cleanRounds(*g, *m, tipGiven ? tipGiven : 2 * (uint64_t)sk, bubbleGiven ? bubbleGiven : 2 * (uint64_t)sk, weakGiven ? weakGiven : 2 * (uint64_t)sk, t, b, p, w);
            g->simplifyGraph();                               // (a seed stage always simplifies and never retains: that would drop replicons)
            const auto [sn, se, sl] = g->counts();
            (void)sl;
            seed.report(sk, stageRounds, stageBefore, stageAfter, stageStats, sn, se);
            seedMap = std::move(m);
            seedGraph = std::move(g);
        }
        std::unique_ptr<genome::PartitionedDNAMap> pm;
        uint64_t sent = 0, owned = 0, good = 0;
        std::unique_ptr<genome::DNAMap> kmersFreq;
        genome::FreqFilter::Chosen chosen;
        chosen.autoRounds = autoRounds;
        chosen.wantSpectrum = !spectrumPath.empty();
        const bool withSpectrum = chosen.autoRounds || chosen.wantSpectrum;
        if (world) {
            pm = std::make_unique<genome::PartitionedDNAMap>(ctx, k, rank, world, shareId(rank, ranks.idFile));
            std::tie(sent, owned) = genome::FreqFilter::extractFilteredKmers(*pm, data, rounds, takeFirst, &chosen);  // :32 over N ranks
            good = pm->size();                                                                                          // :34
            kmersFreq = std::make_unique<genome::DNAMap>(pm->gathered(true));
        } else {
            kmersFreq = std::make_unique<genome::DNAMap>(genome::FreqFilter::extractFilteredKmers(ctx, data, k, rounds, takeFirst, 0, prefilter, &chosen,
                                                                                                      seed.given ? std::function<void(genome::DNAMap &, int)>(seedInto) : nullptr));   // :32
            good = kmersFreq->size();                                                                                  // :34
        }
        if (withSpectrum) rounds = chosen.rounds;
        if (rank == 0 && !spectrumPath.empty()) writeSpectrum(spectrumPath, chosen.spectrum.hist);
        auto graph = genome::Graph::buildGraph(k, *kmersFreq, cyc.keep);                                          // :36
        auto [nodes, edges, totalLen] = graph.counts();                                                  // :39
        if (seed.given) seed.report(k, stageRounds, stageBefore, stageAfter, stageStats, nodes, edges);
        // :41-47 the two component histograms, on the graph as built (the reference computes them before retain)
        auto [hist, hist2] = graph.componentHistograms();
        uint64_t kept = nodes, comps = 0;
        if (retain) std::tie(kept, comps) = graph.retainLargestComponent();                              // :52-54
        std::vector<uint64_t> tipsRemoved, bubblesRemoved, bubblePairs;
        WeakRounds weak;
        cleanRounds(graph, *kmersFreq, tipMaxLen, bubbleMaxLen, weakMaxLen, tipsRemoved, bubblesRemoved, bubblePairs, weak);
        if (removeWeak && rank == 0) {
            uint64_t byRatio = 0, byFloor = 0;
            for (const uint64_t x : weak.removedRatio) byRatio += x;
            for (const uint64_t x : weak.removedFloor) byFloor += x;
            std::fprintf(stderr, "remove-weak: %llu edges by ratio %u, %llu more below coverage %u, in %zu rounds (max_len %llu)\n", (unsigned long long)byRatio,
                         weakRatio, (unsigned long long)byFloor, weakFloor, weak.candidates.size(), (unsigned long long)weakMaxLen);
        }
        // --simplify = GraphSimplifier.scala:317-318, applied to the graph GraphBuilder hands over (i.e. after retain)
        if (simplify) { graph.removeBubbles(); graph.simplifyGraph(); }
        PairedResult walked;
        if (walk.cutoff >= 0) walked = pairedStage(graph, ctx, pm.get(), data, takeFirst, rank, world, walk);
        auto [n2, e2, l2] = graph.counts();
        if (pm) pm->barrier();
        if (rank != 0) return 0;
        // --contigs: the text is written after the last graph stage, with the coverage of the table the graph was built from
        genome::Contigs::Stats fasta;
        if (!contig.path.empty()) {
            auto contigs = graph.contigs(kmersFreq.get(), contig.minLen, contig.width, contig.both);
            contigs.write(contig.path);
            fasta = contigs.stats();
        }
        std::string js = "{";
        jsonPut(js, "k", k, "rounds", rounds, "good_kmers", good, "graph_nodes", nodes, "graph_edges", edges, "total_edges_length", totalLen,
                "components", comps, "max_component_size", kept, "retained_nodes", n2, "retained_edges", e2, "retained_edges_length", l2);
        if (withSpectrum)
            jsonPut(js, "rounds_auto", chosen.autoFound, "valley", chosen.cutoff.valley, "peak", chosen.cutoff.peak, "genome_size_estimate", chosen.cutoff.genomeSize);
        if (correct) jsonPut(js, "correct", "{\"solid\":" + std::to_string(solid) + ",\"solid_auto\":" + (solidAuto ? "true," : "false,") + corrected.json().substr(1));
        if (clipTips) jsonPut(js, "clip_tips", jsonObject("max_len", tipMaxLen, "removed", jsonList(tipsRemoved)));
        if (popBubbles)
            jsonPut(js, "pop_bubbles", jsonObject("max_len", bubbleMaxLen, "max_diff", bubbleMaxDiff, "removed", jsonList(bubblesRemoved), "pairs", jsonList(bubblePairs)));
        if (removeWeak)
            jsonPut(js, "remove_weak", jsonObject("max_len", weakMaxLen, "ratio", weakRatio, "floor", weakFloor, "candidates", jsonList(weak.candidates),
                                                  "removed_ratio", jsonList(weak.removedRatio), "removed_floor", jsonList(weak.removedFloor)));
        if (walk.cutoff >= 0 && walk.rangeAuto)
            jsonPut(js, "insert_range", jsonObject("lo", walked.range.lo, "hi", walked.range.hi, "estimated", walked.range.estimated,
                                                   "observations", walked.range.observations));
        if (walk.cutoff >= 0) jsonPut(js, "walk_pairs", walked.walkJson());
        if (walk.resolve) jsonPut(js, "resolve_repeats", walked.resolveJson(walk.spanCutoff()));
        if (link.wanted()) {
            const LinkResult lr = linksStage(graph, ctx, data, takeFirst, link, walk, &walked);
            jsonPut(js, "links", lr.json());
            if (!lr.fillJson.empty()) jsonPut(js, "fill", lr.fillJson);
            if (!lr.overlapJson.empty()) jsonPut(js, "overlap", lr.overlapJson);
            if (!lr.scaffoldsJson.empty()) jsonPut(js, "scaffolds", lr.scaffoldsJson);
            if (!lr.judgeJson.empty()) jsonPut(js, "judge", lr.judgeJson);
            if (!lr.blocksJson.empty()) jsonPut(js, "blocks", lr.blocksJson);
        }
        if (const std::string cj = cyc.report(graph, true); !cj.empty()) jsonPut(js, "cycles", cj);
        if (seed.given) jsonPut(js, "seed_stages", seed.json());
        if (!contig.path.empty()) jsonPut(js, "contigs_fasta", fasta.json());
        // --gfa: after all edits (the links stage's included), with KC from the table the graph was built from
        if (const std::string gj = gfaOpt.run(graph, kmersFreq.get()); !gj.empty()) jsonPut(js, "gfa", gj);
        jsonPut(js, "components_histogram", jsonPairs(hist), "components_histogram_2", jsonPairs(hist2));   // GraphBuilder.scala:42, :47
        if (world) jsonPut(js, "occurrences_sent", sent, "occurrences_owned", owned, "world", world);
        std::printf("%s}\n", js.c_str());
        if (!saveGraph.empty()) graph.save(saveGraph);                                                   // :55-56 (a Kryo file there)
        if (!out.empty()) {
            writeGraphText(graph, out);
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
