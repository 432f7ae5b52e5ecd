// convert2bin.cpp — twin of Convert2bin.main (S/scripts/Convert2bin.scala:25-87) over genome.hpp: FASTQ text to the `.bin` read
// stream, parsed on the GPU.  Writes <out-prefix>.bin (through <out-prefix>.bin.tmp and a rename) and prints one JSON object:
// pairs, kmers, short_pairs, bin_bytes, text_bytes.  The rules and the deliberate deviations are in include/genome_amd.h ("FASTQ").
//
//   convert2bin <in.fastq> <out-prefix> [--split N | --interleaved] [--k K]
//   --split N: Convert2bin's n (default 36, the reference's); --interleaved: records 2i and 2i+1 are the mates of pair i.
//   --k K: the k of the kmers / short_pairs statistics (default 23, the reference's).
//   The PairedEndData descriptor (:83) is not written: the tools take the pair count as an argument.
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/convert2bin.cpp -L genome_amd -lgenome_amd -Wl,-rpath,'$ORIGIN/..'
//        -o genome_amd/host/convert2bin
#include "tool_common.hpp"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <in.fastq> <out-prefix> [--split N | --interleaved] [--k K]\n", argv[0]);
        return 2;
    }
    const std::string in = argv[1], out = std::string(argv[2]) + ".bin", tmp = out + ".tmp";
    int split = 36, k = 23;
    for (Args a(argc, argv, 3); a.more(); a.next()) {
        if (a.value("--split", split) || a.value("--k", k)) {}
        else if (a.flag("--interleaved")) split = 0;
        else { std::fprintf(stderr, "unknown argument %s\n", a.cur()); return 2; }
    }
    if (split < 0 || k < 1 || k > 255) {
        std::fprintf(stderr, "--split N needs N >= 1 and --k K needs 1 <= K <= 255\n");
        return 2;
    }
    FILE *fo = nullptr;
    try {
        genome::Context ctx(0);
        genome::FastqReader rd(ctx, split, k);
        fo = std::fopen(tmp.c_str(), "wb");
        if (!fo) throw genome::GkError(GK_E_INVALID, "cannot write " + tmp);
        uint64_t bin_bytes = 0;
        std::vector<uint8_t> bin;
        genome::forEachPiece(in, 256u << 20, [&](const char *p, size_t n, bool last) {
            bin.clear();
            rd.convert(p, n, last, bin);
            if (!bin.empty() && std::fwrite(bin.data(), 1, bin.size(), fo) != bin.size()) throw genome::GkError(GK_E_INVALID, "cannot write " + tmp);
            bin_bytes += bin.size();
        });
        if (std::fclose(fo) != 0) { fo = nullptr; throw genome::GkError(GK_E_INVALID, "cannot write " + tmp); }
        fo = nullptr;
        if (std::rename(tmp.c_str(), out.c_str()) != 0) throw genome::GkError(GK_E_INVALID, "cannot rename " + tmp + " to " + out);
        const genome::FastqReader::Stats st = rd.stats();
        std::printf("{\"pairs\": %llu, \"kmers\": %llu, \"short_pairs\": %llu, \"bin_bytes\": %llu, \"text_bytes\": %llu}\n",
                    (unsigned long long)st.pairs, (unsigned long long)st.kmers, (unsigned long long)st.shortPairs,
                    (unsigned long long)bin_bytes, (unsigned long long)st.textBytes);
        return 0;
    } catch (const std::exception &e) {
        if (fo) std::fclose(fo);
        std::remove(tmp.c_str());
        std::fprintf(stderr, "convert2bin: %s\n", e.what());
        return 1;
    }
}
