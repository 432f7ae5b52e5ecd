// rank_id.hpp — the communicator id of an N-rank run (graph_builder / graph_simplifier --world W --rank R --id-file PATH):
// rank 0 writes it aside and renames it into place, the others wait for it (2 minutes at most).
#pragma once

#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <thread>
#include <vector>

#include "genome.hpp"

// the communicator id through a file: rank 0 writes it aside and renames it into place, the others wait for it
inline std::vector<uint8_t> shareId(int rank, const std::string &path) {
    if (rank == 0) {
        std::vector<uint8_t> id = genome::PartitionedDNAMap::uniqueId();
        const std::string tmp = path + ".tmp" + std::to_string(getpid());
        {
            std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
            f.write((const char *)id.data(), (std::streamsize)id.size());
            if (!f) throw std::runtime_error("cannot write " + tmp);
        }
        if (std::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot rename " + tmp + " to " + path);
        return id;
    }
    const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(120);
    for (;;) {
        std::ifstream f(path, std::ios::binary);
        if (f) {
            std::vector<uint8_t> id((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            if (id.size() == 128) return id;
        }
        if (std::chrono::steady_clock::now() > until) throw std::runtime_error("no communicator id in " + path + " after 120 s");
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
}

