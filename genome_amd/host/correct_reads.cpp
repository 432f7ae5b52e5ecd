// correct_reads.cpp — spectral correction of a `.bin` read stream on the GPU (gk_reads_correct: this project's own rule, stated in
// include/genome_amd.h; the reference has no corrector): counts the k-mers of the stream, takes the threshold below which a k-mer
// is weak, replaces the bases under runs of weak k-mers where exactly one replacement makes the run solid, and writes the stream
// back with the same framing.
//
//   correct_reads <reads.bin> <nreads> <k> --out <corrected.bin> [--solid N|auto] [--spectrum PATH]
//   <nreads> = records (two per pair).  --solid auto (the default) takes the valley of the count spectrum (gk_spectrum_cutoff);
//   a spectrum without one falls back to 3 and the JSON says "solid_auto":false.  --spectrum PATH writes the spectrum of the
//   count as graph_builder --spectrum does.  Stdout: one JSON object with k, solid and the ten statistics.
//
// Build: g++ -std=c++17 -O2 -I include genome_amd/host/correct_reads.cpp -L genome_amd -lgenome_amd
//        -Wl,-rpath,'$ORIGIN/..' -o genome_amd/host/correct_reads
#include "tool_common.hpp"

int main(int argc, char **argv) {
    std::string out, spectrumPath;
    uint32_t solid = 0;                           // 0 = auto
    bool ok = argc >= 4;
    for (Args a(argc, argv, 4); ok && a.more(); a.next()) {
        if (a.value("--out", out) || a.value("--spectrum", spectrumPath)) {}
        else if (a.word("--solid", 1, "auto")) { solid = 0; a.skip(); }
        else if (a.value("--solid", solid)) ok = solid >= 1;
        else ok = false;
    }
    if (!ok || out.empty()) {
        std::fprintf(stderr, "usage: %s <reads.bin> <nreads> <k> --out <corrected.bin> [--solid N|auto] [--spectrum PATH]\n", argv[0]);
        return 2;
    }
    try {
        const std::string infile = argv[1];
        const uint64_t nreads = std::stoull(argv[2]);
        const int k = std::stoi(argv[3]);
        std::vector<uint8_t> bin = readBin(infile);
        genome::Context ctx(0);
        genome::DNAMap counts(ctx, k);
        const uint64_t occ = counts.countReads(bin.data(), bin.size(), nreads);
        bool solidAuto = false;
        uint32_t valley = 0, peak = 0;
        if (!solid || !spectrumPath.empty()) {
            const genome::Spectrum sp = counts.spectrum();
            const genome::SpectrumCutoff c = genome::spectrumCutoff(sp.hist);
            valley = c.valley; peak = c.peak;
            if (!solid) { solidAuto = valley != 0; solid = solidAuto ? valley : 3; }
            if (!spectrumPath.empty()) writeSpectrum(spectrumPath, sp.hist);
        }
        const auto st = counts.correctReads(bin.data(), bin.size(), nreads, solid, bin.data());
        std::ofstream of(out, std::ios::binary);
        of.write(reinterpret_cast<const char *>(bin.data()), (std::streamsize)bin.size());
        of.close();
        if (!of) throw std::runtime_error("cannot write " + out);
        std::printf("{\"k\":%d,\"occurrences\":%llu,\"solid\":%u,\"solid_auto\":%s,\"valley\":%u,\"peak\":%u,%s\n", k, (unsigned long long)occ, solid,
                    solidAuto ? "true" : "false", valley, peak, st.json().c_str() + 1);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "correct_reads: %s\n", e.what());
        return 1;
    }
    return 0;
}
