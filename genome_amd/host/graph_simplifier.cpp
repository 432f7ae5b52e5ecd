// graph_simplifier.cpp — C++ twin of GraphSimplifier.startup (S/scripts/GraphSimplifier.scala:140-352) over genome.hpp: loads
// the graph file graph_builder --save-graph wrote (:152-153, with the checks of :157-169), walks the read pairs over it, splits
// its nodes by the pairs' support and simplifies it.  The reference logs its counters (:266, :320-331); here they are one JSON
// object.
//
//   graph_simplifier <graph.gkg> <reads.bin> <pairs> --cutoff C [--range LO HI | --range auto [--max-insert N] [--insert-hist PATH]]
//                    [--take-first N] [--thread-reads [--no-pairs]]
//                    [--out prefix] [--save-graph PATH] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]]
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
//   The stage: getGraphMap (:188), walkPairs over the first N pairs (:213-263), splitBySupport (:272-316), simplifyGraph (:318).
//   --out writes graph_builder's <prefix>.nodes.txt, .edges.txt, .contigs (:338-347) and .dot; --save-graph writes the final
//   graph as a graph file (the reference's graphFile, :352).
//   --contigs PATH writes the final graph's contigs as FASTA on the device (gk_graph_contigs_plan / gk_contigs_write: this project's
//   own rule, beside --out's .contigs, which stays the reference's): one record `>e<id> len=<n>` per live edge whose path is not
//   above its reverse complement (--contig-both-strands: every live edge), n >= --contig-min-len (default 0), lines of
//   --contig-width bases (default 60, 0 = one line).  No cov= field: this tool holds no count table.  The JSON gains
//   "contigs_fasta":{the nine stats}.  Over --world rank 0 writes.
//   --world W --rank R --id-file PATH: one rank of W (one process per rank, on device R % gk_device_count()).  Every rank loads
//   the same file, so the replicas are identical, ids included; each walks its contiguous share of the pairs and the supports
//   are summed over the ranks before the split.  Rank 0 alone prints the JSON (plus world) and writes --out / --save-graph.
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/graph_simplifier.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/graph_simplifier
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

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
    const int fastq_at = argc >= 3 && !std::strcmp(argv[2], "--fastq") ? 2 : 0;
    if (fastq_at) {
        if (fastqArgs(argc, argv, fastq_at, &fastq, &split, &fargs)) {
            std::fprintf(stderr, "usage: %s <graph.gkg> --fastq <reads.fastq> --cutoff C [--split N | --interleaved] [options of the .bin form]\n"
                                 "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n", argv[0]);
            return 2;
        }
        argc = (int)fargs.size() - 1;
        argv = fargs.data();
    }
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <graph.gkg> <reads.bin> <pairs> --cutoff C [--range LO HI | --range auto [--max-insert N] [--insert-hist PATH]] [--take-first N] "
                             "[--thread-reads [--no-pairs]] [--out prefix] [--save-graph PATH] [--contigs PATH [--contig-min-len N] [--contig-width W] [--contig-both-strands]] "
                             "[--world W --rank R --id-file PATH]\n", argv[0]);
        return 2;
    }
    const std::string graphFile = argv[1], infile = argv[2];
    genome::PairedEndData data;
    data.count = std::stoull(argv[3]);
    int cutoff = -1, rangeLo = 180, rangeHi = 250;          // GraphSimplifier.scala:146
    uint64_t takeFirst = UINT64_MAX;
    std::string out, saveGraph, idFile, insertHist, contigsPath;
    uint64_t contigMinLen = 0;
    uint32_t contigWidth = 60;
    bool contigBoth = false;
    int world = 0, rank = 0;
    bool rangeAuto = false, threadReads = false, noPairs = false;
    long maxInsert = 4095;
    for (int i = 4; i < argc; i++) {
        if (!std::strcmp(argv[i], "--cutoff") && i + 1 < argc) cutoff = std::stoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--range") && i + 1 < argc && !std::strcmp(argv[i + 1], "auto")) { rangeAuto = true; i++; }
        else if (!std::strcmp(argv[i], "--max-insert") && i + 1 < argc) maxInsert = std::stol(argv[++i]);
        else if (!std::strcmp(argv[i], "--insert-hist") && i + 1 < argc) insertHist = argv[++i];
        else if (!std::strcmp(argv[i], "--range") && i + 2 < argc) { rangeLo = std::stoi(argv[++i]); rangeHi = std::stoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--take-first") && i + 1 < argc) takeFirst = std::stoull(argv[++i]);
        else if (!std::strcmp(argv[i], "--thread-reads")) threadReads = true;
        else if (!std::strcmp(argv[i], "--no-pairs")) noPairs = true;
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
    if (cutoff < 0) {
        std::fprintf(stderr, "--cutoff C is required\n");
        return 2;
    }
    if (maxInsert < 1 || maxInsert > 65535 || (!rangeAuto && !insertHist.empty())) {
        std::fprintf(stderr, "--max-insert N is 1..65535; --insert-hist PATH goes with --range auto\n");
        return 2;
    }
    if (noPairs && (!threadReads || rangeAuto)) {
        std::fprintf(stderr, "--no-pairs goes with --thread-reads, and not with --range auto (no walk uses the range)\n");
        return 2;
    }
    if (world && (world < 1 || rank < 0 || rank >= world || idFile.empty())) {
        std::fprintf(stderr, "--world W needs --rank R (0 <= R < W) and --id-file PATH\n");
        return 2;
    }
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
        auto graph = genome::Graph::load(ctx, graphFile);                                                // :152-153, :157-169
        const int k = graph.k();
        std::unique_ptr<genome::PartitionedDNAMap> pm;
        if (world) pm = std::make_unique<genome::PartitionedDNAMap>(ctx, k, rank, world, shareId(rank, idFile));
        auto [n1, e1, l1] = graph.counts();
        auto graphMap = graph.getGraphMap();                                                             // :188
        genome::Graph::PairDistances dist;
        genome::InsertRange est;
        if (rangeAuto) {                                                                                 // the same pairs, before walking
            if (world) {
                const auto [a, b] = genome::pairShare(data.count, takeFirst, rank, world);
                dist = graph.pairDistances(*pm, graphMap, data, a, b, (uint32_t)maxInsert + 1);
            } else {
                dist = graph.pairDistances(graphMap, data, takeFirst, (uint32_t)maxInsert + 1);
            }
            est = genome::insertRange(dist.hist);
            rangeLo = (int)est.lo; rangeHi = (int)est.hi;
            if (rank == 0) {
                if (est.estimated) std::fprintf(stderr, "insert range %u to %u, median %u, from %llu observations\n", est.lo, est.hi, est.median, (unsigned long long)est.observations);
                else std::fprintf(stderr, "no estimate of the insert range (%llu observations): falling back to the reference's %u to %u\n",
                                  (unsigned long long)est.observations, est.lo, est.hi);
            }
            if (rank == 0 && !insertHist.empty()) {
                std::ofstream hf(insertHist);
                for (size_t d = 0; d < dist.hist.size(); d++) if (dist.hist[d]) hf << d << " " << dist.hist[d] << "\n";
                if (!hf) throw std::runtime_error("cannot write " + insertHist);
            }
        }
        genome::Support support(ctx);
        genome::Graph::ThreadStats threaded;
        if (world) {                                                                                     // this rank's pairs, then the sum over the ranks
            const auto [a, b] = genome::pairShare(data.count, takeFirst, rank, world);
            if (!noPairs) graph.walkPairs(graphMap, support, data, a, b, rangeLo, rangeHi);
            if (threadReads) {
                threaded = graph.threadReads(graphMap, support, data, a, b);
                double v[7];
                for (int i = 0; i < 7; i++) v[i] = (double)threaded.v[i];
                genome::check(gk_dist_allreduce_f64(pm->distHandle(), v, 7, 0), ctx.handle());
                for (int i = 0; i < 7; i++) threaded.v[i] = (uint64_t)v[i];
            }
            pm->reduceSupport(graph, support);                                                           // (before any node split)
        } else {
            if (!noPairs) graph.walkPairs(graphMap, support, data, takeFirst, rangeLo, rangeHi);         // :213-263
            if (threadReads) threaded = graph.threadReads(graphMap, support, data, takeFirst);
        }
        auto [supPairs, badPairs, walked] = support.sizes();                                             // :266 "Bad pairs"
        auto [removedEdges, newNodes] = graph.splitBySupport(support, cutoff);                           // :272-316
        graph.simplifyGraph();                                                                           // :318
        auto [n2, e2, l2] = graph.counts();
        auto [hist, hist2] = graph.componentHistograms();                                                // :320-331
        if (pm) pm->barrier();
        if (rank != 0) return 0;
        std::string autoJson;
        if (rangeAuto) {
            autoJson = "\"insert_range\":{\"lo\":" + std::to_string(est.lo) + ",\"hi\":" + std::to_string(est.hi) + ",\"median\":" +
                       (est.estimated ? std::to_string(est.median) : std::string("null")) + ",\"estimated\":" + (est.estimated ? "true" : "false") +
                       ",\"observations\":" + std::to_string(est.observations) + ",\"max_insert\":" + std::to_string(maxInsert) + ",\"classes\":{";
            for (int c = 0; c < 9; c++)
                autoJson += std::string(c ? "," : "") + "\"" + genome::Graph::pairClassNames[c] + "\":" + std::to_string(dist.classes[c]);
            autoJson += "}},";
        }
        // --contigs: the text of the final graph (this tool holds no count table: no cov= field)
        if (!contigsPath.empty()) {
            auto contigs = graph.contigs(nullptr, contigMinLen, contigWidth, contigBoth);
            contigs.write(contigsPath);
            autoJson += "\"contigs_fasta\":" + contigs.stats().json() + ",";
        }
        if (threadReads) {
            autoJson += "\"thread_reads\":{";
            for (int c = 0; c < 7; c++) autoJson += std::string(c ? "," : "") + "\"" + genome::Graph::threadStatNames[c] + "\":" + std::to_string(threaded.v[c]);
            autoJson += "},";
        }
        std::printf("{\"k\":%d,\"nodes\":%llu,\"edges\":%llu,\"edges_length\":%llu,"
                    "\"walk_pairs\":{\"supported_edge_pairs\":%llu,\"bad_pairs\":%llu,\"orientations_walked\":%llu,\"removed_edges\":%llu,\"new_nodes\":%llu},"
                    "%s\"simplified_nodes\":%llu,\"simplified_edges\":%llu,\"simplified_edges_length\":%llu,\"components_histogram_2\":[",
                    k, (unsigned long long)n1, (unsigned long long)e1, (unsigned long long)l1, (unsigned long long)supPairs,
                    (unsigned long long)badPairs, (unsigned long long)walked, (unsigned long long)removedEdges, (unsigned long long)newNodes, autoJson.c_str(),
                    (unsigned long long)n2, (unsigned long long)e2, (unsigned long long)l2);
        bool first = true;
        for (const auto &p : hist2) { std::printf("%s[%llu,%llu]", first ? "" : ",", (unsigned long long)p.first, (unsigned long long)p.second); first = false; }
        std::printf("],\"max_component_size\":%llu", (unsigned long long)(hist.empty() ? 0 : hist.rbegin()->first));
        if (world) std::printf(",\"world\":%d", world);
        std::printf("}\n");
        if (!saveGraph.empty()) graph.save(saveGraph);                                                   // :352 graphFile
        if (!out.empty()) {
            std::ofstream nf(out + ".nodes.txt"), ef(out + ".edges.txt");
            for (const auto &n : graph.getNodes()) nf << n.toString() << "\n";
            for (const auto &e : graph.getEdges()) ef << e.start.toString() << " " << e.end.toString() << " " << e.seq << "\n";
            std::ofstream cf(out + ".contigs"), df(out + ".dot");
            graph.writeContigs(cf);                                                                      // :338-347
            graph.writeDot(df);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "graph_simplifier: %s\n", e.what());
        return 1;
    }
    return 0;
}
