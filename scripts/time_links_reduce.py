"""Measurements of the link table over N ranks (gk_dist_reduce_links) and of the edge numbering by path content it rests on.
Loads the TEST build of the library (the loopback transport: ranks as threads of one process on one device; the hook
gk_test_edge_path_keys), so what it times on one GPU is the device work, with device-to-device copies in place of xGMI.

The library is scripts/time_pair_links.py's: a 4 Mbp genome by default, 30x of 150 bp mates = 4e5 pairs, inserts 230..300, 0.5 %
error, k = 31; count -> filter -> buildGraph -> retain.  One JSON line per case:

  numbering   on the graph as built: gk_dist_reduce_support at world 1 with an empty support, which is graph_edge_canon and the
              checks; then walkPairs, splitBySupport, simplifyGraph, and on that graph the path-key pass (the hook: the word
              count, the scan, k_pk_hash, k_pk_keys, two radix sorts, k_pk_canon and the read-back of four arrays) and
              gk_dist_reduce_links at world 1 with an empty table (the same pass without the read-back).  Beside them what the
              card copies, device to device, in buffers of the pool's live bytes (Context.stream_bench: bytes read + written per
              second) — the streaming bound of a pass that reads those bytes once.  Kernel times come from a run under
              `rocprofv3 --kernel-trace --stats`; this script prints wall times (median of REPS calls after one warm-up call).
  reduce      two loopback ranks, each linking half the pairs on its own replica: reduce_links, against the route it replaces —
              rank 1 exports, rank 0 takes the records with HipLinks.add (by id: the replicas here are built alike; between
              replicas that number differently that route does not even exist).

    python scripts/time_links_reduce.py [genome bases]
"""
import ctypes as C
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

from genome_amd import _lib as L  # noqa: E402
from genome_amd import dna  # noqa: E402
from genome_amd.dist import HipDist  # noqa: E402
from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.graph import HipLinks, Support, buildGraph  # noqa: E402

L_, K, COV, ERR, REPS = 150, 31, 30, 0.005, 7


def library(G):
    """time_pair_links.py's generator -> (`.bin` bytes, pairs)"""
    rng = np.random.default_rng(7)
    genome = rng.integers(0, 4, G, dtype=np.uint8)
    npairs = G * COV // (2 * L_)
    ins, start, flip = rng.integers(230, 301, npairs), rng.integers(0, G - 300, npairs), rng.random(npairs) < 0.5
    comp = np.array([3, 2, 1, 0], np.uint8)
    reads = np.empty((2 * npairs, L_), np.uint8)
    idx = np.arange(L_)
    for i in range(0, npairs, 100000):
        j = min(npairs, i + 100000)
        a = genome[start[i:j, None] + idx[None, :]]
        b = comp[genome[(start[i:j] + ins[i:j])[:, None] - 1 - idx[None, :]]]
        f = flip[i:j, None]
        reads[2 * i:2 * j:2] = np.where(f, b, a)
        reads[2 * i + 1:2 * j:2] = np.where(f, a, b)
    e = rng.random(reads.shape) < ERR
    reads = np.where(e, (reads + rng.integers(1, 4, reads.shape, dtype=np.uint8)) & 3, reads).astype(np.uint8)
    pad = np.zeros((2 * npairs, 152), np.uint8)
    pad[:, :L_] = reads
    packed = (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)
    return np.concatenate([np.full((2 * npairs, 1), L_, np.uint8), packed], axis=1).tobytes(), npairs


def built(ctx, binb, npairs):
    m = HipDNAMap(ctx, K)
    m.count_reads(binb, 2 * npairs)
    m.deleteAll_lt(3)
    g = buildGraph(K, m)
    g.retainLargest()
    return m, g


def edited(ctx, g, binb, npairs):
    vm, sup = g.getGraphMap(), Support(ctx)
    g.walkPairs(vm, sup, binb, npairs, 180, 250)
    split = g.splitBySupport(sup, 3)
    g.simplifyGraph()
    sup.close(); vm.close()
    return split


def median_ms(call):
    ms = []
    for rep in range(REPS + 1):                      # (the first call warms the block pool and the kernels' code up)
        t0 = time.perf_counter()
        call()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def path_keys(g):
    ne = g.idBounds()[1]
    h1, h2, canon, dup = np.zeros(ne, np.uint64), np.zeros(ne, np.uint64), np.zeros(ne, np.uint32), np.zeros(ne, np.uint8)
    n, fp = C.c_uint64(), C.c_uint64()
    L.check(L.test_hook("gk_test_edge_path_keys")(g.h, L.ptr(h1, C.c_uint64), L.ptr(h2, C.c_uint64), L.ptr(canon, C.c_uint32), L.ptr(dup, C.c_uint8),
                                                   C.byref(n), C.byref(fp)), g.ctx.h)
    return int(dup.sum())


def case_numbering(binb, npairs):
    ctx = Context(0)
    hd = HipDist(ctx, 0, 1, bytes(128), loopback=True)
    m, g = built(ctx, binb, npairs)
    sup, links = Support(ctx), HipLinks(ctx)
    before = g.counts()
    canon_ms = median_ms(lambda: hd.reduce_support(g, sup))
    split = edited(ctx, g, binb, npairs)
    nodes, edges, total_len = g.counts()
    live_bytes = max(total_len // 4, 1 << 20)
    dups = path_keys(g)
    hook_ms = median_ms(lambda: path_keys(g))
    pass_ms = median_ms(lambda: hd.reduce_links(g, links))
    copy = ctx.stream_bench(live_bytes, 20)
    copy_ms = 2 * live_bytes / (copy["copy_GBps"] * 1e9) * 1e3
    print(json.dumps({"case": "numbering", "graph_as_built": before, "split": split, "graph_edited": (nodes, edges, total_len), "duplicate_edges": dups,
                      "edge_canon_world1_ms": canon_ms, "path_keys_world1_ms": pass_ms, "path_keys_hook_ms": hook_ms,
                      "pool_live_bytes": total_len // 4, "copy_buffer_bytes": live_bytes, "copy_GBps": copy["copy_GBps"], "copy_of_live_bytes_ms": copy_ms,
                      "path_keys_over_edge_canon": pass_ms / canon_ms, "path_keys_over_copy": pass_ms / copy_ms}))
    sup.close(); links.close(); g.close(); m.close(); hd.close(); ctx.close()


def case_reduce(binb, npairs, world=2):
    id128 = bytes(random.Random(world).getrandbits(8) for _ in range(128))
    out, errors, handoff = [None] * world, [], {}
    ready = threading.Barrier(world)

    def run(rank):
        try:
            c = Context(0)
            hd = HipDist(c, rank, world, id128, loopback=True)
            m, g = built(c, binb, npairs)
            edited(c, g, binb, npairs)
            vm = g.getGraphMap()
            a, b = npairs * rank // world, npairs * (rank + 1) // world
            res = {"fp": g.idFingerprint()}
            red, old = [], []
            for rep in range(REPS + 1):
                lk = HipLinks(c)
                g.pairLinks(vm, (dna.bin_pairs(binb, a, b), b - a), lk, min_len=2 * K, max_span=300 + K)
                mine = lk.size()
                hd.barrier()
                t0 = time.perf_counter()
                hd.reduce_links(g, lk)
                if rep:
                    red.append((time.perf_counter() - t0) * 1e3)
                res["summed"], res["mine"] = lk.size(), mine
                lk.close()
                # the route it replaces: every other rank exports, rank 0 adds
                lk = HipLinks(c)
                g.pairLinks(vm, (dna.bin_pairs(binb, a, b), b - a), lk, min_len=2 * K, max_span=300 + K)
                hd.barrier()
                t0 = time.perf_counter()
                if rank:
                    handoff[rank] = lk.export()
                ready.wait()
                if rank == 0:
                    for r in range(1, world):
                        lk.add(*handoff[r])
                    res["added"] = lk.size()
                ready.wait()
                if rep:
                    old.append((time.perf_counter() - t0) * 1e3)
                lk.close()
            res["reduce_ms"], res["export_add_ms"] = float(np.median(red)), float(np.median(old))
            out[rank] = res
            hd.barrier()
            vm.close(); g.close(); m.close(); hd.close(); c.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            ready.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise SystemExit(f"failed: {errors}")
    same_ids = len({o["fp"] for o in out}) == 1
    red, old = max(o["reduce_ms"] for o in out), max(o["export_add_ms"] for o in out)
    print(json.dumps({"case": "reduce", "world": world, "links_per_rank": [o["mine"][0] for o in out], "links_summed": out[0]["summed"][0],
                      "replicas_number_alike": same_ids, "export_add_equals_reduce": same_ids and out[0]["added"] == out[0]["summed"],
                      "reduce_links_ms": red, "export_add_ms": old, "reduce_over_export_add": red / old,
                      "wire_bound_bytes_all_ranks": 20 * sum(o["mine"][0] for o in out) + 20 * out[0]["summed"][0] * (world - 1)}))


if __name__ == "__main__":
    binb, npairs = library(int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000)
    case_numbering(binb, npairs)
    case_reduce(binb, npairs)
