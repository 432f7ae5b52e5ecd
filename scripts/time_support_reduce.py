"""Measurements of the paired-end support over N ranks (gk_dist_reduce_support, gk_support_add / _merge,
gk_graph_id_fingerprint).  Loads the TEST build of the library (the loopback transport: ranks as threads of one process on one
device), so what it times on one GPU is the device work of the reduce — bucket, owner merge, rebuild, fingerprint — with the
transport's device-to-device copies in place of xGMI.  Kernel times come from running it under `rocprofv3 --kernel-trace
--stats` (k_sup_bucket_count / k_sup_bucket_scatter, k_sup_add_list_checked = the owner merge, k_sup_add_list = the rebuild,
k_graph_id_fingerprint); the script itself prints wall times, one JSON line per case.

  python scripts/time_support_reduce.py reduce 1000000 [world]   two (or `world`) ranks, each holding that many distinct pairs
                                                                 of its replica's edges, half shared with the next rank
  python scripts/time_support_reduce.py walk 4000000              the pairs of scripts/time_walk_pairs.py at that genome length
                                                                 (4 Mbp: 4e5 pairs): distinct supported pairs, fingerprint
"""
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GK_LIB_PATH", os.path.join(ROOT, "genome_amd", "libgenome_amd_test.so"))

import numpy as np  # noqa: E402

from genome_amd import synth  # noqa: E402
from genome_amd.dist import HipDist  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import Support, buildGraph  # noqa: E402


def rank_graph(ctx, k=31):
    """the same graph content on every rank (reads with 2 % errors: tens of thousands of edges), counted on each rank's own context, so
    the replicas' ids may differ — the reduce moves the pairs in its canonical numbering.  -> (table, graph, this replica's
    live edge ids in one content order: (start k-mer, first base))"""
    rec = synth.reads_mode_g(100000, 100, 200000, 0.02, config_id=17)
    m = HipDNAMap(ctx, k)
    m.count_reads(rec.tobytes(), len(rec))
    m.deleteAll_lt(2)
    g = buildGraph(k, m)
    info = g.edgesById(np.arange(g.idBounds()[1]))
    live = np.flatnonzero(info["alive"]).astype(np.uint32)
    nodes = g.nodesById(info["start"][live])
    order = np.lexsort((info["first"][live], nodes["lo"], nodes["hi"]))
    return m, g, live[order]


def case_reduce(n, world):
    rng = np.random.default_rng(11)
    # rank r holds pairs [r * n / 2, r * n / 2 + n) of one random list of (edge, edge) pairs in content order: half shared with
    # the next rank; each rank translates them to its own replica's ids
    c0 = Context(0)
    m0, g0, order0 = rank_graph(c0)
    ne = len(order0)
    g0.close(); m0.close(); c0.close()
    total = n // 2 * (world + 1)
    assert ne * ne >= 2 * total, f"{ne} edges: too few for {total} distinct pairs"
    keys = np.unique(rng.integers(0, ne * ne, int(total * 1.2), dtype=np.uint64))[:total]
    assert len(keys) == total
    rng.shuffle(keys)
    id128 = bytes(random.Random(world).getrandbits(8) for _ in range(128))
    out, errors = [None] * world, []

    def run(rank):
        try:
            c = Context(0)
            hd = HipDist(c, rank, world, id128, loopback=True)
            m, g, order = rank_graph(c)
            mine = keys[rank * (n // 2): rank * (n // 2) + n]
            sup = Support(c)
            t0 = time.perf_counter()
            sup.add(order[mine // np.uint64(ne)], order[mine % np.uint64(ne)], np.ones(len(mine), np.uint32), 1, 2)
            t_add = time.perf_counter() - t0
            t0 = time.perf_counter()
            fp = g.idFingerprint()
            t_fp = time.perf_counter() - t0
            hd.barrier()
            t0 = time.perf_counter()
            hd.reduce_support(g, sup)
            t_red = time.perf_counter() - t0
            out[rank] = {"add_ms": t_add * 1e3, "fingerprint_ms": t_fp * 1e3, "reduce_ms": t_red * 1e3, "sizes": sup.sizes(), "fp": fp}
            hd.barrier()
            sup.close(); g.close(); m.close(); hd.close(); c.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise SystemExit(f"failed: {errors}")
    assert all(o["sizes"] == (total, world, 2 * world) for o in out), [o["sizes"] for o in out]
    print(json.dumps({"case": "reduce", "distinct_per_rank": n, "world": world, "distinct_total": total,
                      "reduce_ms_max": max(o["reduce_ms"] for o in out), "add_ms_max": max(o["add_ms"] for o in out),
                      "fingerprint_ms": out[0]["fingerprint_ms"],
                      "wire_bound_bytes_all_ranks": 12 * n * world + 12 * total * (world - 1)}))
    # one device, no transport: the merge of two supports of n distinct pairs each
    c = Context(0)
    a, b = Support(c), Support(c)
    for s, part in ((a, keys[:n]), (b, keys[n // 2: n // 2 + n])):
        s.add((part // np.uint64(ne)).astype(np.uint32), (part % np.uint64(ne)).astype(np.uint32), np.ones(len(part), np.uint32))
    c.sync()
    t0 = time.perf_counter()
    a.merge(b)
    print(json.dumps({"case": "merge", "distinct_each": n, "merge_ms": (time.perf_counter() - t0) * 1e3, "distinct_after": a.sizes()[0]}))
    a.close(); b.close(); c.close()


def case_walk(G):
    """the generator of scripts/time_walk_pairs.py: 30x of 150 bp mates, inserts 230..300, 0.5 % error, k = 31"""
    L, k, cov, err = 150, 31, 30, 0.005
    rng = np.random.default_rng(7)
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    npairs = G * cov // (2 * L)
    ins = rng.integers(230, 301, npairs)
    start = rng.integers(0, G - 300, npairs)
    flip = rng.random(npairs) < 0.5
    comp = np.array([3, 2, 1, 0], np.uint8)
    reads = np.empty((2 * npairs, L), np.uint8)
    idx = np.arange(L)
    for i in range(0, npairs, 100000):
        j = min(npairs, i + 100000)
        a = genome[start[i:j, None] + idx[None, :]]
        b = comp[genome[(start[i:j] + ins[i:j])[:, None] - 1 - idx[None, :]]]
        f = flip[i:j, None]
        reads[2 * i:2 * j:2] = np.where(f, b, a)
        reads[2 * i + 1:2 * j:2] = np.where(f, a, b)
    e = rng.random(reads.shape) < err
    reads = np.where(e, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
    pad = np.zeros((2 * npairs, 152), np.uint8)
    pad[:, :L] = reads
    packed = (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)
    binb = np.concatenate([np.full((2 * npairs, 1), L, np.uint8), packed], axis=1).tobytes()
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, 2 * npairs)
    m.deleteAll_lt(3)
    g = buildGraph(k, m)
    g2 = buildGraph(k, m)                              # a second build of the same table: do its ids agree?
    same_build = g.idFingerprint() == g2.idFingerprint()
    g2.close()
    g.retainLargest()
    vm = g.getGraphMap()
    sup = Support(ctx)
    g.walkPairs(vm, sup, binb, npairs, 180, 250)
    pairs, bad, walked = sup.sizes()
    g.idFingerprint()                                  # (first call: warm)
    t0 = time.perf_counter()
    for _ in range(10):
        g.idFingerprint()
    t_fp = (time.perf_counter() - t0) / 10
    n, ne, ln = g.counts()
    print(json.dumps({"case": "walk", "genome": G, "pairs": npairs, "distinct_supported_pairs": pairs, "bad_pairs": bad, "walked": walked,
                      "graph_nodes": n, "graph_edges": ne, "id_bounds": g.idBounds(), "fingerprint_ms": t_fp * 1e3, "two_builds_same_fingerprint": same_build,
                      "reduce_wire_bound_bytes_per_rank_at_P8": int(12 * pairs + 12 * pairs * 7 / 8)}))
    sup.close(); vm.close(); g.close(); m.close(); ctx.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "reduce"
    if what == "reduce":
        case_reduce(int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
    elif what == "walk":
        case_walk(int(sys.argv[2]) if len(sys.argv) > 2 else 4_000_000)
    else:
        raise SystemExit(__doc__)
