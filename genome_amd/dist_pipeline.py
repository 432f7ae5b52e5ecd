"""GraphBuilder.startup (S/scripts/GraphBuilder.scala:18-59) and the paired-end stage of GraphSimplifier.startup
(S/scripts/GraphSimplifier.scala:188-318) over N ranks, one call per rank: the Python twin of
`graph_builder --world W --rank R` (genome_amd/host/graph_builder.cpp).

Every rank passes the same PairedEndData (the whole `.bin` stream) and takes its own contiguous share of the pairs, for the
count and for the walks alike:

  1. gk_dist_count_reads of its share (every k-mer counted by its owner rank);
  2. deleteAll(v < rounds) on its partition, gk_dist_size -> good_kmers;
  3. the gathered (classified) k-mer set, buildGraph on it: every rank holds a replica of the graph;
  4. component histograms, retainLargest, removeBubbles + simplifyGraph — on the replica, identical on every rank;
  5. walk_pairs = (cutoff, lo, hi): getGraphMap, walkPairs over its share, the supports summed over the ranks
     (gk_dist_reduce_support, which refuses replicas with split nodes: it comes before splitBySupport), splitBySupport,
     simplifyGraph.

Every step that moves data is collective: all ranks must call build_graph with the same arguments."""
from __future__ import annotations

import numpy as np

from . import dna
from .dist import DistDNAMap, HipDist
from .freqfilter import PairedEndData
from .graph import HipGraph, Support, buildGraph


def pair_share(npairs: int, world: int, rank: int, take_first: int | None = None) -> tuple[int, int]:
    """Rank `rank` of `world`: the pair range [n * rank // world, n * (rank + 1) // world) of the first n = min(take_first, npairs)
    pairs.  The shares cover [0, n) exactly once; a rank may get none (world > n)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("need 0 <= rank < world")
    n = npairs if take_first is None else max(0, min(take_first, npairs))
    return n * rank // world, n * (rank + 1) // world


def build_graph(hd: HipDist, data: PairedEndData, k: int, rounds: int = 3, take_first: int | None = None, retain: bool = True,
                simplify: bool = False, walk_pairs=None, classified: bool = True) -> tuple[HipGraph, dict]:
    """One rank's part of the N-rank GraphBuilder (+ GraphSimplifier pairs stage) -> (this rank's graph replica, stats).
    `stats` holds graph_builder's JSON keys (the walk_pairs object only with walk_pairs) plus occurrences_sent,
    occurrences_owned (this rank's windows) and world.  The caller closes the graph."""
    a, b = pair_share(data.count, hd.world, hd.rank, take_first)
    off = dna.bin_pair_offsets(data.bin, b)
    share = np.frombuffer(data.bin, np.uint8)[int(off[a]):int(off[b])]
    pm = DistDNAMap(hd, k)
    try:
        sent, owned = pm.count_reads(share, 2 * (b - a))                   # FreqFilter.scala:44-48
        pm.deleteAll_lt(rounds)                                             # :55
        good = pm.size()                                                    # GraphBuilder.scala:34
        full = pm.gathered(classified=classified)
    finally:
        pm.close()
    try:
        g = buildGraph(k, full)                                             # :36
    finally:
        full.close()
    try:
        nodes, edges, total_len = g.counts()                                # :39
        hist, hist2 = g.componentHistograms()                               # :41-47, on the graph as built
        kept, comps = nodes, 0
        if retain:
            kept, comps = g.retainLargest()                                 # :52-54
        if simplify:
            g.removeBubbles()                                               # GraphSimplifier.scala:317-318
            g.simplifyGraph()
        walk = None
        if walk_pairs is not None:
            cutoff, lo, hi = walk_pairs
            vm = g.getGraphMap()                                            # :188
            sup = Support(hd.ctx)
            try:
                if b > a:
                    g.walkPairs(vm, sup, share, b - a, lo, hi)              # :213-263, this rank's pairs
                hd.reduce_support(g, sup)                                   # every rank's walks summed, before any split
                sup_pairs, bad, walked = sup.sizes()                        # :266
                removed, new_nodes = g.splitBySupport(sup, cutoff)          # :272-316
                g.simplifyGraph()                                           # :318
            finally:
                sup.close()
                vm.close()
            walk = {"supported_edge_pairs": sup_pairs, "bad_pairs": bad, "orientations_walked": walked, "removed_edges": removed,
                    "new_nodes": new_nodes}
        n2, e2, l2 = g.counts()
    except BaseException:
        g.close()
        raise
    stats = {"k": k, "rounds": rounds, "good_kmers": good, "graph_nodes": nodes, "graph_edges": edges, "total_edges_length": total_len,
             "components": comps, "max_component_size": kept, "retained_nodes": n2, "retained_edges": e2, "retained_edges_length": l2}
    if walk is not None:
        stats["walk_pairs"] = walk
    stats["components_histogram"] = [list(x) for x in hist]
    stats["components_histogram_2"] = [list(x) for x in hist2]
    stats.update({"occurrences_sent": sent, "occurrences_owned": owned, "world": hd.world})
    return g, stats
