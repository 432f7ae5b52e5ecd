"""The canonical edge numbering by path content (-m gpu): gk_test_edge_path_keys, the function gk_dist_reduce_links and
gk_dist_reduce_spans number their records by, held bit-exact to tests/pathkey_ref.py — the keys, the places of the edges whose
key is theirs alone, the duplicate flags and the fingerprint — with the hash kernel's grid capped at 1 and 3 workgroups and free.

The device pass cuts the live words of the sequence pool into chunks of 64 words (2048 bases) whatever edge they fall in, so the
constructed paths put edges of 1 base, of 2047 / 2048 / 2049 and 4095 / 4096 / 4097 bases and one beyond 65 535 bases into one
graph, between edges whose byte counts are odd: they cannot all start on an 8-byte boundary of the pool (where the pool puts an edge
is not observable from here; the restatement, which every edge is compared with, knows no alignment)."""
import ctypes as C
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import pyref as R
from pathkey_ref import CHUNK_BASES, numbering, path_key
from test_spans_gpu import by_id, graph_of, pieces, spans_of
from thread_cases import tiling

pytestmark = pytest.mark.gpu
GRIDS = (1, 3, 0)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_option("test_max_grid", 0)
    c.close()


def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def device_keys(g):
    """the hook -> (h1, h2, canon, dup, nlive, fingerprint), the arrays by edge id"""
    ne = g.idBounds()[1]
    h1, h2 = np.zeros(ne, np.uint64), np.zeros(ne, np.uint64)
    canon, dup = np.zeros(ne, np.uint32), np.zeros(ne, np.uint8)
    n, fp = C.c_uint64(), C.c_uint64()
    L.check(L.test_hook("gk_test_edge_path_keys")(g.h, L.ptr(h1, C.c_uint64), L.ptr(h2, C.c_uint64), L.ptr(canon, C.c_uint32), L.ptr(dup, C.c_uint8),
                                                   C.byref(n), C.byref(fp)), g.ctx.h)
    return h1, h2, canon, dup, n.value, fp.value


def paths_by_id(g):
    nodes, edges = by_id(g)
    return {e: nodes[x[0]] + x[2] for e, x in enumerate(edges) if x is not None}


def grid_uses(c):
    n = C.c_uint64()
    L.check(L.test_hook("gk_test_grid_cap_uses")(c.h, C.byref(n)), c.h)
    return n.value


def check(g, paths=None, grids=GRIDS):
    """the hook against the restatement under every grid -> (paths by id, device keys by id, fingerprint)"""
    paths = paths_by_id(g) if paths is None else paths
    keys, canon, shared, dups, fp = numbering(g.k, paths)
    ne = g.idBounds()[1]
    for grid in grids:
        g.ctx.set_option("test_max_grid", grid)
        before = grid_uses(g.ctx)
        h1, h2, dcanon, ddup, nlive, dfp = device_keys(g)
        assert (grid_uses(g.ctx) > before) == (grid > 0)
        assert nlive == len(paths) and dfp == fp
        places = {}
        for e in range(ne):
            if e not in paths:
                assert (int(h1[e]), int(h2[e]), int(dcanon[e]), int(ddup[e])) == ((1 << 64) - 1, (1 << 64) - 1, 0xffffffff, 0), e
                continue
            assert (int(h1[e]), int(h2[e])) == keys[e], (grid, e, len(paths[e]))
            assert bool(ddup[e]) == (e in dups)
            if e in dups:
                places.setdefault(keys[e], []).append(int(dcanon[e]))
            else:
                assert int(dcanon[e]) == canon[e]
        assert {key: sorted(v) for key, v in places.items()} == shared          # duplicates share their places, in an order of their own
        assert sorted(int(dcanon[e]) for e in paths) == list(range(len(paths)))  # canon / inv: permutations of the live edges
    g.ctx.set_option("test_max_grid", 0)
    return paths, keys, fp


def graph_from(ctx, k, seqs, cap=0):
    reads = [r for s in seqs for r in (tiling(s, 200, 200 - k + 1) if len(s) > 200 else [s])]
    m = HipDNAMap(ctx, k, cap)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    g = buildGraph(k, m)
    m.close()
    return g


@pytest.mark.parametrize("k", [15, 31, 34, 41, 64])
def test_keys_match_the_restatement_and_replicas_agree(ctx, k):
    """A genome with repeats (a branching graph: edges of a few to a few hundred bases) built twice from tables of another
    capacity: every key bit-exact; equal fingerprints; the edge at every canonical place spells the same path on both; one
    edge less is another fingerprint."""
    rnd = random.Random(k)
    rep = rand_seq(rnd, 3 * k)
    genome = "".join(rand_seq(rnd, 400 + 37 * i) + rep for i in range(5)) + rand_seq(rnd, 301)
    a, b = graph_from(ctx, k, [genome], 1 << 14), graph_from(ctx, k, [genome], 3 << 15)
    pa, _, fpa = check(a)
    pb, _, fpb = check(b, grids=(0,))
    assert len(pa) >= 12 and len({len(p) for p in pa.values()}) >= 4
    assert fpa == fpb and sorted(pa.values()) == sorted(pb.values())
    ca, cb = device_keys(a)[2], device_keys(b)[2]
    inv_a, inv_b = {int(ca[e]): e for e in pa}, {int(cb[e]): e for e in pb}
    assert all(pa[inv_a[i]] == pb[inv_b[i]] for i in range(len(pa)))
    victim = sorted(pb)[len(pb) // 2]
    assert b.removeEdgesById([victim]) == 1
    pb2, _, fpb2 = check(b, grids=(0,))
    assert victim not in pb2 and fpb2 != fpa
    a.close(); b.close()


@pytest.mark.parametrize("k", [31, 64])
def test_constructed_paths(ctx, k):
    """k = 64: the start k-mer fills both words of the key"""
    rnd = random.Random(2049)
    lens = [1, CHUNK_BASES - 1, CHUNK_BASES, CHUNK_BASES + 1, 2 * CHUNK_BASES - 1, 2 * CHUNK_BASES, 2 * CHUNK_BASES + 1, 66001]
    base = [rand_seq(rnd, k + n) for n in lens]
    t_last, t_prefix, t_align = rand_seq(rnd, k + 3001), rand_seq(rnd, k + 3003), rand_seq(rnd, k + 5001)
    head, w = rand_seq(rnd, k), [rand_seq(rnd, 32) for _ in range(3)]
    t_words = head + w[0] + w[1] + w[2]
    set_a = base + [t_last, t_prefix, t_align, t_words]
    other_last = t_last[:-1] + ("A" if t_last[-1] != "A" else "C")
    set_b = [rand_seq(rnd, k + 5), other_last, t_prefix[:-40], rand_seq(rnd, k + 13), t_align, head + w[1] + w[0] + w[2]]
    strands = lambda seqs: sorted(list(seqs) + [R.rev_comp(s) for s in seqs])
    found = {}
    for name, seqs in (("a", set_a), ("b", set_b)):
        g = graph_from(ctx, k, seqs)
        paths, keys, _ = check(g)
        assert sorted(paths.values()) == strands(seqs)                    # every sequence is one edge per strand
        found[name] = {paths[e]: keys[e] for e in paths}
        g.close()
    a, b = found["a"], found["b"]
    assert max(len(p) for p in a) - k > 65535 and min(len(p) for p in a) - k == 1
    assert a[t_last] != b[other_last]                                      # the last base alone
    assert a[t_prefix] != b[t_prefix[:-40]]                                # a path and its own proper prefix
    assert a[t_words] != b[head + w[1] + w[0] + w[2]]                      # the same words in another order
    assert a[t_align] == b[t_align] == path_key(k, t_align)               # the same path wherever the pool put it
    assert len(set(a.values()) | set(b.values())) == len(a) + len(b) - 2  # (t_align and its twin are the only keys both graphs have)


def test_duplicates_after_an_edge_split(ctx):
    """A R B R C: splitEdgesBySpans leaves, until simplifyGraph merges them away, two live copies of the repeat's edge per strand:
    equal paths, hence equal keys, both flagged, neighbours in the order."""
    k = 35
    A, Rp, B, Cc = pieces(k, k, [300, k + 60, 280, 310], lambda A, Rp, B, Cc: [A + Rp + B + Rp + Cc])
    g, reads = graph_of(ctx, k, [A + Rp + B + Rp + Cc])
    assert not numbering(k, paths_by_id(g))[3]
    check(g)
    sp, _ = spans_of(g, reads)
    assert g.splitEdgesBySpans(sp, 3)["new_edges"] == 2
    paths = paths_by_id(g)
    dups = numbering(k, paths)[3]
    assert sorted(paths[e] for e in dups) == sorted([Rp, Rp, R.rev_comp(Rp), R.rev_comp(Rp)])
    check(g, paths)
    g.simplifyGraph()
    assert not numbering(k, paths_by_id(g))[3]
    check(g, grids=(0,))
    sp.close(); g.close()
