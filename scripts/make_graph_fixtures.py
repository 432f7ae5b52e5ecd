"""Write the committed version-1 graph files tests/golden/graph_v1_k11.gkg and graph_v1_k35.gkg: the graphs of the golden read
sets g_k11_p1 / g_k35_p2 right after buildGraph, saved by gk_graph_save (needs the GPU).  They pin the file format: the tests
load them (test_graph_file_gpu.py) and decode them without the library (test_graph_file_cpu.py).

    python scripts/make_graph_fixtures.py [OUT_DIR]        (default: tests/golden)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import buildGraph  # noqa: E402
from genome_amd.partitioned import PartitionedDNAMap  # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ctx = Context(0)
    for name in ("g_k11_p1", "g_k35_p2"):
        fx = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))
        k, P = fx["k"], fx["P"]
        m = PartitionedDNAMap(ctx, k, P) if P > 1 else HipDNAMap(ctx, k)
        m.count_reads(bytes.fromhex(fx["bin_hex"]), fx["nreads"])
        m.deleteAll_lt(fx["rounds"])
        g = buildGraph(k, m)
        path = os.path.join(out_dir, "graph_v1_k%d.gkg" % k)
        g.save(path)
        print(path, os.path.getsize(path), "bytes", g.counts())
        g.close(); m.close()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
