"""Time the contig FASTA writer on the C3 graph after simplify (4.6 Mbp genome, 5 x 10^6 reads of 150 bases at 0.5 % errors from
gk_synth_reads_dev mode G config 3, k = 31: count -> deleteAll(<3) -> buildGraph -> removeBubbles -> simplifyGraph, as
scripts/run_c3.py).  Run by hand on a GPU; not part of the suite.  Prints one JSON object (and writes it to --out):

  a  export_host   the only route there was: gk_graph_export_edges (HipGraph.getEdges + the start nodes by id) and the same
                   records formatted on the host (numpy: strand choice per edge, the 2-bit sequence to letters, line wrapping)
  b  plan_write    gk_graph_contigs_plan + gk_contigs_write to a file under --dir (default /dev/shm)
  c  emit          the emit kernels alone, from gk_contigs_last_ms of those writes (device events, summed over the chunks)

Each of a and b runs once to warm up (first launches load code objects, the pinned buffers are made) and then --reps times;
medians and the spread are reported.  a and b alternate in the same process.  (c)'s bytes per second stand beside the fill rate
gk_dev_stream_bench measures on the same card.  The host route's text is compared with the device's, byte for byte.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from genome_amd import _lib as L  # noqa: E402
from genome_amd import synth  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import buildGraph  # noqa: E402

CODES4 = ((np.arange(256, dtype=np.uint8)[:, None] >> np.array([0, 2, 4, 6], np.uint8)[None, :]) & 3).astype(np.uint8)   # a packed byte -> its 4 codes
COMPLEMENT = bytes([3, 2, 1, 0]) + bytes(range(4, 256))      # code -> 3 - code
TO_LETTERS = b"AGCT" + bytes(range(4, 256))


def host_route(g, k, width):
    """(a): the edges through gk_graph_export_edges, ids found by (start node, first base), the records formatted here"""
    ne = g.idBounds()[1]
    ids = np.arange(ne, dtype=np.uint32)
    by_id = g.edgesById(ids)
    e = g.getEdges()
    live = ids[by_id["alive"]]
    nodes = g.nodesById(by_id["start"][live])
    # name the exported edges: (start k-mer, first base) -> id
    first = (e["seq"][e["off"]] & 3).astype(np.uint64)
    key_exp = np.stack([e["shi"], e["slo"], first], axis=1)
    key_id = np.stack([nodes["hi"], nodes["lo"], by_id["first"][live].astype(np.uint64)], axis=1)
    oe, oi = np.lexsort(key_exp.T[::-1]), np.lexsort(key_id.T[::-1])
    eid = np.empty(len(live), np.uint32)
    eid[oe] = live[oi]
    j = np.arange(k, dtype=np.uint64)
    start_codes = (np.where(j < 32, e["slo"][:, None] >> (2 * (j % 32)), e["shi"][:, None] >> (2 * (j % 32))) & np.uint64(3)).astype(np.uint8)
    # per edge: the path as code bytes (one table lookup unpacks the 2-bit sequence), the strand choice and the letters as bytes
    # operations, the lines by slicing
    out = []
    lens, offs, seq, order = e["len"].tolist(), e["off"].tolist(), e["seq"], np.argsort(eid).tolist()
    eids = eid.tolist()
    for i in order:
        ln, off = lens[i], offs[i]
        codes = start_codes[i].tobytes() + CODES4[seq[off:off + (ln + 3) // 4]].tobytes()[:ln]
        if codes > codes[::-1].translate(COMPLEMENT):
            continue                                         # reverse: its twin is written
        n = k + ln
        text = codes.translate(TO_LETTERS)
        out.append(b">e%d len=%d\n" % (eids[i], n))
        out.extend(text[a:a + width] + b"\n" for a in range(0, n, width))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4_600_000)
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    k, rl = 31, 150
    ctx = Context(0)
    d = ctx.alloc(args.reads * synth.record_stride(rl) + 64)
    ctx.synth_reads(d, args.reads, rl, "G", 3, 0, args.genome, 0.005)
    m = HipDNAMap(ctx, k, 0)
    m.count_reads_dev(d, args.reads, rl)
    m.deleteAll_lt(3)
    g = buildGraph(k, m)
    ctx.free(d)
    g.removeBubbles()
    g.simplifyGraph()
    res = {"genome": args.genome, "reads": args.reads, "k": k, "line_width": args.width, "reps": args.reps, "graph": g.counts()}
    path = os.path.join(args.dir, "contigs_bench_%d.fa" % os.getpid())

    def plan_write(counts):
        t0 = time.perf_counter()
        c = g.contigs(counts, line_width=args.width)
        t1 = time.perf_counter()
        c.write(path)
        t2 = time.perf_counter()
        ms, st = c.last_ms(), c.stats()
        c.close()
        return {"plan_ms": (t1 - t0) * 1e3, "write_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3, "emit_ms": ms["emit_kernels"], "last_ms": ms}, st

    def host():
        t0 = time.perf_counter()
        text = host_route(g, k, args.width)
        with open(path + ".host", "wb") as f:
            f.write(text)
        return (time.perf_counter() - t0) * 1e3, text

    _, st = plan_write(None)                                 # warm-up of b, and the text to compare
    with open(path, "rb") as f:
        dev_text = f.read()
    _, host_text = host()                                    # warm-up of a
    assert host_text == dev_text, "the host route and the device disagree"
    a, b, bc = [], [], []
    for _ in range(args.reps):                               # alternating
        a.append(host()[0])
        b.append(plan_write(None)[0])
        bc.append(plan_write(m)[0])

    def med(xs):
        return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}

    emit = statistics.median(x["emit_ms"] for x in b)
    gbps = (C.c_double * 3)()
    L.check(L.lib().gk_dev_stream_bench(ctx.h, 256 << 20, 20, gbps), ctx.h)
    res.update({
        "stats": st, "text_bytes": st["text_bytes"],
        "a_export_host_ms": med(a),
        "b_plan_write_ms": {key: med([x[key] for x in b]) for key in ("plan_ms", "write_ms", "total_ms")},
        "b_with_cov_ms": {key: med([x[key] for x in bc]) for key in ("plan_ms", "write_ms", "total_ms")},
        "b_last_ms_of_the_median_run": sorted(b, key=lambda x: x["total_ms"])[len(b) // 2]["last_ms"],
        "c_emit_ms": med([x["emit_ms"] for x in b]),
        "c_emit_GBps_written": round(st["text_bytes"] / (emit * 1e-3) / 1e9, 3) if emit else None,
        "dev_stream_bench_GBps": {"copy": round(gbps[0], 1), "fill": round(gbps[1], 1), "sum": round(gbps[2], 1)},
        "b_over_a": round(statistics.median(x["total_ms"] for x in b) / statistics.median(a), 5),
    })
    for p in (path, path + ".host"):
        if os.path.exists(p):
            os.remove(p)
    g.close(); m.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
