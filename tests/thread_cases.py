"""What the read-threading GPU tests share: genomes with planted k-long repeats, single reads cut from them, and the device
graph read back by id as the strings tests/thread_ref.py takes.  Seeds are chosen on the CPU (the convention of
insert_cases.py): the tests assert on the restatement alone that the classes a case is about are populated."""
import random
from collections import Counter

import numpy as np

from genome_amd import dna
from genome_amd.dnamap import HipDNAMap
from genome_amd.graph import buildGraph
from oracle import pyref as R
from thread_ref import thread_reads

GLEN = 2400


def genome(seed, k, glen=GLEN, nrep=3):
    """a random genome in which `nrep` k-mers occur twice in different contexts (pairs_ref.make_pairs' plant)"""
    rnd = random.Random(seed)
    g = [rnd.choice("AGCT") for _ in range(glen)]
    for _ in range(nrep):
        a = rnd.randrange(100, glen // 2 - 100)
        b = rnd.randrange(glen // 2 + 100, glen - 100)
        g[b:b + k] = g[a:a + k]
    return "".join(g)


def cut_reads(seed, g, lengths, err=0.0):
    """one read per entry of `lengths`, from a random place and strand of g, each base wrong with probability err"""
    rnd = random.Random(seed * 7919 + 1)
    reads = []
    for L in lengths:
        s = rnd.randrange(0, len(g) - L + 1)
        r = g[s:s + L]
        if rnd.random() < 0.5:
            r = R.rev_comp(r)
        if err:
            r = "".join(c if rnd.random() >= err else rnd.choice([x for x in "AGCT" if x != c]) for c in r)
        reads.append(r)
    return reads


def lengths_for(k, n, seed=0):
    """n read lengths that take every lane trip: k+1 (skipped), k+2, k+63, k+64, k+65 (one, two trips), 255, and lengths between"""
    rnd = random.Random(seed)
    special = [k + 1, k + 2, k + 63, k + 64, k + 65, 255]
    return [special[(i // 3) % len(special)] if i % 3 == 0 else rnd.randrange(k + 2, 256) for i in range(n)]


def tiling(g, L, step):
    """reads that cover g end to end (so that the graph of the reads is the graph of g)"""
    return [g[s:s + L] for s in range(0, len(g) - L + 1, step)] + [g[-L:]]


def build_graph(ctx, k, reads, min_count=1):
    binb = dna.reads_to_bin(reads)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    if min_count > 1:
        m.deleteAll_lt(min_count)
    g = buildGraph(k, m)
    m.close()
    return g


def device_graph(g):
    """the device graph's own live nodes and edges, by id -> (node k-mers, edges (start index, end index, sequence), the content
    key (start k-mer, first base code) of every edge): indices are ranks among the live ids.  The sequences come from the
    canonical export, matched by (start k-mer, first base), which stays unique after a split (out-edges partition among copies)."""
    k = g.k
    nn, ne = g.idBounds()
    ninfo, einfo = g.nodesById(np.arange(nn, dtype=np.uint32)), g.edgesById(np.arange(ne, dtype=np.uint32))
    nidx, nodes = {}, []
    for i in range(nn):
        if ninfo["alive"][i]:
            nidx[i] = len(nodes)
            nodes.append(dna.unpack(int(ninfo["lo"][i]), int(ninfo["hi"][i]), k))
    seqs = {}
    for s, _, q in g.canonical()[1]:
        assert (s, q[0]) not in seqs
        seqs[(s, q[0])] = q
    edges, keys = [], []
    for e in range(ne):
        if einfo["alive"][e]:
            s, t, b = int(einfo["start"][e]), int(einfo["end"][e]), int(einfo["first"][e])
            q = seqs[(nodes[nidx[s]], dna.BASES[b])]
            assert len(q) == int(einfo["len"][e]) and (nodes[nidx[s]] + q)[-k:] == nodes[nidx[t]]
            edges.append((nidx[s], nidx[t], q))
            keys.append((nodes[nidx[s]], b))
    return nodes, edges, keys


def restate(g, reads):
    """the restatement on the device graph as it is now -> (support by content as pairs_ref.gpu_support_by_content gives it, stats)"""
    nodes, edges, keys = device_graph(g)
    sup, st = thread_reads(g.k, nodes, edges, reads)
    return Counter({(keys[e], keys[f]): c for (e, f), c in sup.items()}), st
