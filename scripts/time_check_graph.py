"""Time CheckGraph's FASTA check on the device against the host-batched route, on the C3 genome (4.6 Mbp, gk_synth_reads_dev mode
G, config 3) and the graph of its own reads at k = 31.  Prints one JSON object (and writes it to --out):

  device       the genome as FASTA wrapped at 70, once through FastaCheck (the first run: gk_fasta_check_last_ms's split, wall ms)
  host_batched every k-window packed on the host (numpy) and pushed through HipValueMap.apply_batch in batches: wall ms with and
               without the packing
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genome_amd import synth  # noqa: E402
from genome_amd.check import FastaCheck  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import buildGraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    k, L, G = 31, 150, args.genome
    ctx = Context(0)
    d = ctx.alloc(args.reads * synth.record_stride(L) + 64)
    ctx.synth_reads(d, args.reads, L, "G", 3, 0, G, 0.005)
    m = HipDNAMap(ctx, k, 0)
    m.count_reads_dev(d, args.reads, L)
    m.deleteAll_lt(3)
    graph = buildGraph(k, m)
    vm = graph.getGraphMap()
    ctx.free(d)
    codes = synth.genome_bases(G, 3).astype(np.uint8)
    letters = np.frombuffer(b"AGCT", np.uint8)[codes]
    rows = (G + 69) // 70
    padded = np.full(rows * 70, ord("\n"), np.uint8)
    padded[:G] = letters
    body = np.concatenate([padded.reshape(rows, 70), np.full((rows, 1), ord("\n"), np.uint8)], axis=1).reshape(-1)
    tail = G - (rows - 1) * 70
    text = np.concatenate([np.frombuffer(b">genome\n", np.uint8), body[:(rows - 1) * 71 + tail], np.frombuffer(b"\n", np.uint8)])
    res = {"genome": G, "reads": args.reads, "k": k, "graph": graph.counts(), "position_map_entries": vm.size(), "text_bytes": int(text.size)}

    t0 = time.perf_counter()
    with FastaCheck(ctx, vm, False, 0) as fc:
        fc.feed(text, last=True)
        wall = (time.perf_counter() - t0) * 1e3
        st, split = fc.stats(), fc.last_ms()
    res["device"] = {"wall_ms": round(wall, 3), "last_ms": {a: round(b, 3) for a, b in split.items()}, "stats": st,
                     "lookups_per_s": round(st["windows"] / (wall * 1e-3))}

    t0 = time.perf_counter()
    lo = np.zeros(G - k + 1, np.uint64)
    c64 = codes.astype(np.uint64)
    for j in range(k):
        lo |= c64[j:G - k + 1 + j] << np.uint64(2 * j)
    hi = np.zeros_like(lo)
    pack_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    found = 0
    for a in range(0, len(lo), args.batch):
        _, f = vm.apply_batch((lo[a:a + args.batch], hi[a:a + args.batch]))
        found += int(f.sum())
    look_ms = (time.perf_counter() - t0) * 1e3
    assert found == st["found"] and len(lo) == st["windows"], (found, len(lo), st)
    res["host_batched"] = {"pack_ms": round(pack_ms, 3), "apply_batch_ms": round(look_ms, 3), "wall_ms": round(pack_ms + look_ms, 3),
                           "batch": args.batch, "lookups_per_s_apply_batch_alone": round(len(lo) / (look_ms * 1e-3))}
    res["device_over_host_batched"] = round(wall / (pack_ms + look_ms), 4)
    res["device_lookup_rate_over_apply_batch_alone"] = round(look_ms / wall, 4)
    vm.close(); graph.close(); m.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
