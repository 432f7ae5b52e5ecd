// graph_simplifier.cpp — C++ twin of GraphSimplifier.startup (S/scripts/GraphSimplifier.scala:140-352) over genome.hpp: loads
// the graph file graph_builder --save-graph wrote (:152-153, with the checks of :157-169), walks the read pairs over it, splits
// its nodes by the pairs' support and simplifies it.  The reference logs its counters (:266, :320-331); here they are one JSON
// object.
//
//   graph_simplifier <graph.gkg> <reads.bin> <pairs> --cutoff C [--range LO HI | --range auto [--max-insert N] [--insert-hist PATH]]
//                    [--take-first N] [--thread-reads [--no-pairs]] [--resolve-repeats [CUTOFF] [--resolve-rounds N]]
//                    [--out prefix] [--save-graph PATH] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]]
//                    [--links PATH [--link-min-support N] [--link-min-len N] [--scaffolds PATH] [--scaffold-fasta PATH [--scaffold-min-gap N] [--scaffold-width N] [--scaffold-both-strands]] [--fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N]] [--overlap-gaps [TOL] [--overlap-min N] [--overlap-max N]] [--judge GENOME.fasta [--judge-tol N] [--blocks [--block-tol N] [--block-rows PATH]]]]
//                    [--world W --rank R --id-file PATH]
//   graph_simplifier <graph.gkg> --fastq <reads.fastq> --cutoff C [--split N | --interleaved] [the options above but --world]
//   --fastq converts the FASTQ file on the GPU (Convert2bin, gk_fastq) and takes the pair count from the conversion.
//   k comes from the graph (:153); the range defaults to the reference's 180 to 250 (:146), the cutoff is genome.cutoff.
//   --range auto measures the range instead (include/genome_amd.h, "the insert range"): the fragment lengths of the pairs whose
//   mates lie on one edge, from the same pairs in the same --take-first prefix, before walking; fragments up to --max-insert
//   bases are looked for (default 4095; part of the rule: an edge shorter than that counts nothing, so set it little above the
//   largest fragment expected), the range is the central 95 % of at least 1000 observations (both choices, not measurements).
//   The JSON then holds "insert_range": lo, hi, median, estimated, observations and the nine classes; without an estimate the
//   walks fall back to 180 to 250 and "estimated" is false.  --insert-hist writes the histogram as text lines "D count".
//   --thread-reads threads both mates of the same pairs through the graph as single reads (include/genome_amd.h,
//   gk_graph_thread_reads: this project's own rule) into the same support before the split; --no-pairs skips the walks, so
//   that the reads alone are the evidence.  The JSON then holds "thread_reads": the seven stats (summed over the ranks).
//   --resolve-repeats [CUTOFF] resolves repeats longer than k that single reads span (include/genome_amd.h, "spans": this project's
//   own rule), after the stage's split and simplifyGraph: a position map of the graph as it is then, gk_graph_thread_spans over
//   both mates of the same pairs, gk_graph_split_edges_by_spans at CUTOFF (default: --cutoff's value, at least 1; a choice, not a
//   measurement), simplifyGraph; up to --resolve-rounds N rounds (default 1) while a round resolves something.  It goes with
//   --no-pairs too (without --thread-reads no support was gathered, the split by support does not run and the spans alone edit
//   the graph).  stderr gets one line per round; the JSON gains
//   "resolve_repeats":{"cutoff","rounds":[{"thread_spans":{the five stats},"split_edges":{the seven stats}} per round]}.  One GPU only.
//   The stage: getGraphMap (:188), walkPairs over the first N pairs (:213-263), splitBySupport (:272-316), simplifyGraph (:318).
//   --out writes graph_builder's <prefix>.nodes.txt, .edges.txt, .contigs (:338-347) and .dot; --save-graph writes the final
//   graph as a graph file (the reference's graphFile, :352).
//   --contigs PATH writes the final graph's contigs as FASTA on the device (gk_graph_contigs_plan / gk_contigs_write: this project's
//   own rule, beside --out's .contigs, which stays the reference's): one record `>e<id> len=<n>` per live edge whose path is not
//   above its reverse complement (--contig-both-strands: every live edge), n >= --contig-min-len (default 0), lines of
//   --contig-width bases (default 60, 0 = one line).  No cov= field: this tool holds no count table.  The JSON gains
//   "contigs_fasta":{the nine stats}.  Over --world rank 0 writes.
//   --links PATH writes the scaffold links of the FINAL graph (include/genome_amd.h, "scaffold links": this project's own rule):
//   the pairs of the same --take-first prefix whose mates' first k-mers lie on two different edges, one line
//   `e1<TAB>e2<TAB>count<TAB>sum_u<TAB>gap` per link in ascending (e1, e2) behind three `#` lines.  Edges whose contig is shorter than
//   --link-min-len bases (default 0) link nothing; max_span = the range's upper end + k; gap = mid - floor(sum_u / count), where mid
//   is the median --range auto measured, or (lo + hi) div 2 of the given range or of the fallback 180..250 (stderr says which).
//   --scaffolds PATH writes the chains of the joins (the only link of at least --link-min-support observations, default 3, out of
//   one edge and into the next): `s<i><TAB>members<TAB>e<id><TAB>gap<TAB>e<id>...`, a cycle ending in its closing gap and `cycle`;
//   both strands' chains appear.  The JSON gains "links":{the eight classes, the five join stats, mid, max_span, chains, cycles}.
//   One GPU only.
//   --scaffold-fasta PATH (with --links) writes those chains as FASTA (include/genome_amd.h, "scaffolds": this project's own rule):
//   `>s<i> len=<n> contigs=<m> gaps=<N bases>` per chain, members that meet in a node joined on its k bases, max(gap,
//   --scaffold-min-gap) bases N between any others (default 10: a choice, not a measurement), one strand per chain
//   (--scaffold-both-strands: every chain), lines of --scaffold-width bases (default 60, 0 = one line); the edges in no chain
//   follow as --contigs would write them, --link-min-len being their length filter.  The JSON gains "scaffolds":{the thirteen stats}.
//   --fill-gaps [TOL] (with --scaffolds or --scaffold-fasta) sends the chains through gk_graph_fill_gaps first (include/genome_amd.h,
//   "gap filling": this project's own rule): where the graph holds exactly one path of at most --fill-max-edges edges (default 16)
//   between two joined edges whose length is within TOL bases of the gap, its edges become members, and both files are written
//   from the filled chains.  TOL defaults to half the width of the insert range the stage used; junctions with more than
//   --fill-max-paths bounded paths from both sides (default 256) stay as they are.  All three defaults are choices, not
//   measurements.  The JSON gains "fill":{tol, max_edges, max_paths, the ten stats} before "scaffolds".
//   --overlap-gaps [TOL] (with --scaffolds or --scaffold-fasta) sends the chains, after --fill-gaps when both are given, through
//   gk_graph_overlap_gaps (include/genome_amd.h, "overlap detection": this project's own rule): where the last o bases of a member
//   equal the first o of the next, exactly, for exactly one o of --overlap-min (default 10) to --overlap-max (default k) bases
//   within TOL of -gap, the FASTA writes those bases once and no N, and the id list shows -o as the gap.  TOL defaults as
//   --fill-gaps' does; the defaults are choices, not measurements.  The JSON gains "overlap":{tol, min_overlap, max_overlap, the
//   seven stats} beside "fill".
//   --judge GENOME.fasta [--judge-tol N] (with --scaffold-fasta) judges the scaffolds that were written against a reference genome
//   (include/genome_amd.h, "placements" and "the judge": this project's own rules): the edges of the final graph are placed on the
//   reference's records (plain FASTA text) with a position map of that graph, and every junction of the plan is classed unjudged,
//   other_record, strand, order, distance or correct.  N defaults to the fill / overlap TOL, half the width of the insert range: a
//   choice, not a measurement.  stderr gets one line; the JSON gains "judge":{tol, "placements":{the twenty stats}, "stats":{the
//   twenty-nine stats}, "classes", "err" per junction, n50, n50_broken: the scaffold N50 as written and after breaking every chain
//   record at each misjoin}.
//   --blocks [--block-tol N] [--block-rows PATH] (with --judge) aligns the edges of the final graph to the same reference in blocks
//   and classes every breakpoint (include/genome_amd.h, "alignment blocks" and "breakpoints").  N defaults to 1000: a choice, not a
//   measurement.  stderr gets one line; the JSON gains "blocks":{tol, "stats":{the twenty-four stats}, genome_fraction, na50, nga50};
//   PATH gets one text line per row.
//   --gfa PATH writes the final graph as GFA 1.0 on the device (gk_graph_gfa_plan / gk_gfa_write; include/genome_amd.h, "the graph
//   as GFA"), without KC tags: there is no count table after a load.  The JSON gains "gfa":{the nine stats}.  Not with --world.
//   --keep-cycles keeps perfect cycles (include/genome_amd.h, "perfect cycles": this project's own rule): every simplifyGraph of
//   the stage (after the split by support, after each --resolve-repeats round) keeps self-loop nodes and the anchors of
//   all-interior cycles.  The JSON gains "cycles":{"simplify":{the four stats, summed}}, stderr one line.  Not with --world (exit 2).
//   --world W --rank R --id-file PATH: one rank of W (one process per rank, on device R % gk_device_count()).  Every rank loads
//   the same file, so the replicas are identical, ids included; each walks its contiguous share of the pairs and the supports
//   are summed over the ranks before the split.  Rank 0 alone prints the JSON (plus world) and writes --out / --save-graph.
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/graph_simplifier.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/graph_simplifier
#include "tool_common.hpp"

int main(int argc, char **argv) {
    FastqForm fastq;
    if (!fastq.parse(argc, argv, 2)) {
        std::fprintf(stderr, "usage: %s <graph.gkg> --fastq <reads.fastq> --cutoff C [--split N | --interleaved] [options of the .bin form]\n"
                             "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n", argv[0]);
        return 2;
    }
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <graph.gkg> <reads.bin> <pairs> --cutoff C [--range LO HI | --range auto [--max-insert N] [--insert-hist PATH]] [--take-first N] "
                             "[--thread-reads [--no-pairs]] [--resolve-repeats [CUTOFF] [--resolve-rounds N]] [--out prefix] [--save-graph PATH] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]] [--gfa PATH] "
                             "[--links PATH [--link-min-support N] [--link-min-len N] [--scaffolds PATH] [--scaffold-fasta PATH [--scaffold-min-gap N] [--scaffold-width N] [--scaffold-both-strands]] [--fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N]] [--overlap-gaps [TOL] [--overlap-min N] [--overlap-max N]] [--judge GENOME.fasta [--judge-tol N] [--blocks [--block-tol N (default 1000: a choice, not a measurement)] [--block-rows PATH]]]] [--keep-cycles] [--world W --rank R --id-file PATH]\n", argv[0]);
        return 2;
    }
    const std::string graphFile = argv[1], infile = argv[2];
    genome::PairedEndData data;
    Args::convert("<pairs>", argv[3], data.count);
    PairedOpts stage;                             // --cutoff, --range, --max-insert, --thread-reads, --no-pairs, --resolve-repeats
    uint64_t takeFirst = UINT64_MAX;
    std::string out, saveGraph, insertHist;
    ContigOpts contig;
    GfaOpts gfaOpt;
    LinkOpts link;
    RankOpts ranks;
    CycleOpts cyc;                                // --keep-cycles
    for (Args a(argc, argv, 4); a.more(); a.next()) {
        if (a.value("--cutoff", stage.cutoff)) {}
        else if (a.word("--range", 1, "auto")) { stage.rangeAuto = true; a.skip(); }
        else if (a.value("--max-insert", stage.maxInsert) || a.value("--insert-hist", insertHist)) {}
        else if (a.value("--range", stage.lo, stage.hi) || a.value("--take-first", takeFirst)) {}
        else if (a.flag("--thread-reads")) stage.threadReads = true;
        else if (a.flag("--no-pairs")) stage.walk = false;
        else if (stage.parseResolve(a)) {}
        else if (a.value("--out", out) || a.value("--save-graph", saveGraph) || contig.parse(a) || gfaOpt.parse(a) || link.parse(a) || ranks.parse(a) || cyc.parse(a)) {}
        else { std::fprintf(stderr, "unknown argument %s\n", a.cur()); return 2; }
    }
    if (stage.cutoff < 0) {
        std::fprintf(stderr, "--cutoff C is required\n");
        return 2;
    }
    if (!stage.maxInsertOk() || (!stage.rangeAuto && !insertHist.empty())) {
        std::fprintf(stderr, "--max-insert N is 1..65535; --insert-hist PATH goes with --range auto\n");
        return 2;
    }
    if (!stage.walk && ((!stage.threadReads && !stage.resolve) || stage.rangeAuto)) {
        std::fprintf(stderr, "--no-pairs goes with --thread-reads, and not with --range auto (no walk uses the range)\n");
        return 2;
    }
    if (!ranks.check() || !link.check(ranks.world) || !gfaOpt.check(ranks.world) || !stage.checkResolve(ranks.world) || !cyc.check(ranks.world)) return 2;
    const int world = ranks.world, rank = ranks.rank;
    try {
        if (fastq.path.empty()) data.bin = readBin(infile);
        genome::Context ctx(ranks.device());
        if (!fastq.path.empty()) data = genome::PairedEndData::fromFastq(ctx, fastq.path, fastq.split);     // the pair count comes from the conversion
        auto graph = genome::Graph::load(ctx, graphFile);                                                // :152-153, :157-169
        const int k = graph.k();
        graph.keepCycles(cyc.keep);
        std::unique_ptr<genome::PartitionedDNAMap> pm;
        if (world) pm = std::make_unique<genome::PartitionedDNAMap>(ctx, k, rank, world, shareId(rank, ranks.idFile));
        auto [n1, e1, l1] = graph.counts();
        const PairedResult res = pairedStage(graph, ctx, pm.get(), data, takeFirst, rank, world, stage);
        auto [n2, e2, l2] = graph.counts();
        auto [hist, hist2] = graph.componentHistograms();                                                // :320-331
        if (pm) pm->barrier();
        if (rank != 0) return 0;
        std::string js = "{";
        jsonPut(js, "k", k, "nodes", n1, "edges", e1, "edges_length", l1, "walk_pairs", res.walkJson());
        if (stage.rangeAuto) {
            if (!insertHist.empty()) {
                std::ofstream hf(insertHist);
                for (size_t d = 0; d < res.dist.hist.size(); d++) if (res.dist.hist[d]) hf << d << " " << res.dist.hist[d] << "\n";
                if (!hf) throw std::runtime_error("cannot write " + insertHist);
            }
            const genome::InsertRange &est = res.range;
            jsonPut(js, "insert_range", jsonObject("lo", est.lo, "hi", est.hi, "median", est.estimated ? std::to_string(est.median) : "null",
                                                   "estimated", est.estimated, "observations", est.observations, "max_insert", stage.maxInsert,
                                                   "classes", "{" + jsonNamed(genome::Graph::pairClassNames, res.dist.classes, 9) + "}"));
        }
        // --contigs: the text of the final graph (this tool holds no count table: no cov= field)
        if (!contig.path.empty()) {
            auto contigs = graph.contigs(nullptr, contig.minLen, contig.width, contig.both);
            contigs.write(contig.path);
            jsonPut(js, "contigs_fasta", contigs.stats().json());
        }
        // --links / --scaffolds: on the final graph, with a position map of its own
        if (link.wanted()) {
            const LinkResult lr = linksStage(graph, ctx, data, takeFirst, link, stage, &res);
            jsonPut(js, "links", lr.json());
            if (!lr.fillJson.empty()) jsonPut(js, "fill", lr.fillJson);
            if (!lr.overlapJson.empty()) jsonPut(js, "overlap", lr.overlapJson);
            if (!lr.scaffoldsJson.empty()) jsonPut(js, "scaffolds", lr.scaffoldsJson);
            if (!lr.judgeJson.empty()) jsonPut(js, "judge", lr.judgeJson);
            if (!lr.blocksJson.empty()) jsonPut(js, "blocks", lr.blocksJson);
        }
        // --gfa: the final graph as GFA 1.0 (this tool holds no count table: no KC tag)
        if (const std::string gj = gfaOpt.run(graph, nullptr); !gj.empty()) jsonPut(js, "gfa", gj);
        if (stage.threadReads) jsonPut(js, "thread_reads", "{" + jsonNamed(genome::Graph::threadStatNames, res.threaded.v, 7) + "}");
        if (stage.resolve) jsonPut(js, "resolve_repeats", res.resolveJson(stage.spanCutoff()));
        if (const std::string cj = cyc.report(graph, false); !cj.empty()) jsonPut(js, "cycles", cj);
        jsonPut(js, "simplified_nodes", n2, "simplified_edges", e2, "simplified_edges_length", l2, "components_histogram_2", jsonPairs(hist2),
                "max_component_size", hist.empty() ? 0 : hist.rbegin()->first);
        if (world) jsonPut(js, "world", world);
        std::printf("%s}\n", js.c_str());
        if (!saveGraph.empty()) graph.save(saveGraph);                                                   // :352 graphFile
        if (!out.empty()) writeGraphText(graph, out);                                                    // :338-347
    } catch (const std::exception &e) {
        std::fprintf(stderr, "graph_simplifier: %s\n", e.what());
        return 1;
    }
    return 0;
}
