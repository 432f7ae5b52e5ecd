"""Save and load wall times of the graph file (gk_graph_save / gk_graph_load), split by gk_graph_io_stats into file I/O, waits
for host<->device copies and device kernels.  One JSON line per case.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats` (k_gio_*, k_scan_*, k_graph_checksum, k_graph_id_fingerprint, k_count_live).

  python scripts/time_graph_file.py c3  [reads=5000000] [genome=4600000]   C3 (k = 31, 150 bp, 0.5 % errors): the retained,
                                                                           simplified graph GraphBuilder hands over
  python scripts/time_graph_file.py big [reads=4000000] [genome=60000000]  error-free reads over a 6e7-base genome: >= 1e8 bases
                                                                           of edge sequence (both strands)
The file goes to a temporary directory (local disk) and is removed afterwards."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genome_amd import synth  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import buildGraph, graphIoStats, loadGraph  # noqa: E402


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "c3"
    arg = lambda i, d: int(float(sys.argv[i])) if len(sys.argv) > i else d
    if case == "c3":
        n, G, err, rounds = arg(2, 5_000_000), arg(3, 4_600_000), 0.005, 3
    else:
        n, G, err, rounds = arg(2, 4_000_000), arg(3, 60_000_000), 0.0, 1
    k, L = 31, 150
    ctx = Context(0)
    d = ctx.alloc(n * synth.record_stride(L) + 64)
    ctx.synth_reads(d, n, L, "G", 3, 0, G, err)
    m = HipDNAMap(ctx, k)
    m.count_reads_dev(d, n, L)
    ctx.free(d)
    m.deleteAll_lt(rounds)
    g = buildGraph(k, m)
    m.close()
    if case == "c3":
        g.removeBubbles(); g.simplifyGraph(); g.retainLargest()
    nodes, edges, bases = g.counts()
    out = {"case": case, "reads": n, "genome": G, "k": k, "nodes": nodes, "edges": edges, "edge_bases": bases, "id_bounds": list(g.idBounds())}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "g.gkg")
        for rep in range(3):
            t = time.perf_counter(); g.save(path); ws = (time.perf_counter() - t) * 1e3
            s = graphIoStats(ctx)
            c2 = Context(0)
            t = time.perf_counter(); h = loadGraph(c2, path); wl = (time.perf_counter() - t) * 1e3
            ls = graphIoStats(c2)
            assert h.checksum() == g.checksum() and h.idFingerprint() == g.idFingerprint()
            h.close(); c2.close()
            out["rep%d" % rep] = {"save_ms": round(ws, 2), "save": {x: round(v, 2) for x, v in s.items()},
                                  "load_ms": round(wl, 2), "load": {x: round(v, 2) for x, v in ls.items()}}
        out["file_bytes"] = os.path.getsize(path)
    g.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
