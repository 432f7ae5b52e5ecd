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

simplify_graph is GraphSimplifier's own stage from a graph file (gk_graph_save / gk_graph_load): every rank loads the same file
and runs step 5.  Every step that moves data is collective: all ranks must call build_graph (or simplify_graph) with the same
arguments."""
from __future__ import annotations

import numpy as np

from . import dna
from .dist import DistDNAMap, HipDist
from .freqfilter import PairedEndData, auto_rounds
from .graph import (LINK_CLASSES, REFERENCE_RANGE, SPAN_STATS, THREAD_STATS, HipGraph, HipLinks, HipSpans, Support, buildGraph, insertRange,
                    loadGraph, scaffoldChains, scaffoldGaps)


def pair_share(npairs: int, world: int, rank: int, take_first: int | None = None) -> tuple[int, int]:
    """Rank `rank` of `world`: the pair range [n * rank // world, n * (rank + 1) // world) of the first n = min(take_first, npairs)
    pairs.  The shares cover [0, n) exactly once; a rank may get none (world > n)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("need 0 <= rank < world")
    n = npairs if take_first is None else max(0, min(take_first, npairs))
    return n * rank // world, n * (rank + 1) // world


def estimate_range(hd: HipDist, g: HipGraph, vm, share, npairs: int, max_insert: int = 4095, trim: int = 25,
                   min_observations: int = 1000) -> dict:
    """The range of the walks measured from the pairs themselves (include/genome_amd.h, "the insert range"): every rank's share
    through gk_dist_pair_distances (bins = max_insert + 1), gk_insert_range over the summed histogram — the same on every rank.
    -> {"lo", "hi", "median" (None without an estimate), "estimated", "classes", "hist", "max_insert", "trim"}; without an
    estimate lo / hi are the reference's 180 / 250 and "estimated" is False.  COLLECTIVE."""
    hist, classes = hd.pair_distances(g, vm, share, npairs, bins=max_insert + 1)
    est = insertRange(hist, trim, min_observations)
    lo, hi, median = est if est is not None else (*REFERENCE_RANGE, None)
    return {"lo": lo, "hi": hi, "median": median, "estimated": est is not None, "classes": classes, "hist": hist, "max_insert": max_insert,
            "trim": trim}


def _pairs_stage(hd: HipDist, g: HipGraph, share, npairs: int, walk_pairs, auto_args=None, thread_reads: bool = False, walk: bool = True) -> dict:
    """GraphSimplifier.scala:188-318 on this rank's replica `g`: getGraphMap, walkPairs over the rank's `npairs` pairs in `share`,
    the supports summed over the ranks (before any node split), splitBySupport at the cutoff, simplifyGraph -> the walk_pairs
    counters.  lo == "auto": the range is estimated first, from the same pairs (estimate_range with `auto_args`); the counters
    then hold "insert_range" (estimate_range's result without its histogram).  thread_reads: both mates of the same pairs are
    threaded through the graph as single reads into the same support before the reduce (HipGraph.threadReads; the counters
    then hold "thread_reads", the seven stats summed over the ranks); walk = False skips the walks."""
    cutoff, lo, hi = walk_pairs
    if not walk and (not thread_reads or isinstance(lo, str)):
        raise ValueError("walk = False goes with thread_reads = True and a range given as numbers (no walk uses it)")
    threaded = None
    vm = g.getGraphMap()                                                    # :188
    sup = Support(hd.ctx)
    auto = None
    try:
        if isinstance(lo, str):
            if lo != "auto":
                raise ValueError("the range is two numbers, or lo = \"auto\"")
            auto = estimate_range(hd, g, vm, share, npairs, **(auto_args or {}))
            lo, hi = auto["lo"], auto["hi"]
        if npairs > 0 and walk:
            g.walkPairs(vm, sup, share, npairs, lo, hi)                     # :213-263, this rank's pairs
        if thread_reads:
            mine = g.threadReads(vm, sup, (share, 2 * npairs))              # this rank's reads
            total = hd.allreduce([float(mine[key]) for key in THREAD_STATS])
            threaded = {key: int(v) for key, v in zip(THREAD_STATS, total)}
        hd.reduce_support(g, sup)                                           # every rank's walks summed, before any split
        sup_pairs, bad, walked = sup.sizes()                                # :266
        removed, new_nodes = g.splitBySupport(sup, cutoff)                  # :272-316
        g.simplifyGraph()                                                   # :318
    finally:
        sup.close()
        vm.close()
    out = {"supported_edge_pairs": sup_pairs, "bad_pairs": bad, "orientations_walked": walked, "removed_edges": removed,
           "new_nodes": new_nodes}
    if auto is not None:
        out["insert_range"] = {key: auto[key] for key in auto if key != "hist"}
    if threaded is not None:
        out["thread_reads"] = threaded
    return out


def _resolve_stage(hd: HipDist, g: HipGraph, share, nreads: int, cutoff: int, rounds: int) -> list:
    """Repeats longer than k, over the ranks (include/genome_amd.h, gk_graph_thread_spans): per round, on every rank, the position
    map of the replica as it is now, threadSpans of the rank's `nreads` records in `share`, the span tables summed over the ranks
    (gk_dist_reduce_spans: the graph is an edited one), splitEdgesBySpans at `cutoff`, simplifyGraph -> per round {"thread_spans"
    (the five stats over all ranks), "split_edges"}.  A round that resolves nothing is the last: the summed table is the same on
    every rank, so every rank stops in the same round."""
    out = []
    for _ in range(max(0, int(rounds))):
        vm, sp = g.getGraphMap(), HipSpans(hd.ctx)
        try:
            mine = g.threadSpans(vm, sp, share, nreads) if nreads > 0 else dict.fromkeys(SPAN_STATS, 0)
            total = hd.allreduce([float(mine[key]) for key in SPAN_STATS])
            hd.reduce_spans(g, sp)
            split = g.splitEdgesBySpans(sp, cutoff)
        finally:
            sp.close()
            vm.close()
        out.append({"thread_spans": {key: int(v) for key, v in zip(SPAN_STATS, total)}, "split_edges": split})
        if not split["resolved"]:
            break
        g.simplifyGraph()
    return out


def _links_stage(hd: HipDist, g: HipGraph, share, npairs: int, min_support: int = 3, min_len: int = 0, max_span: int = 4095, mid=None) -> dict:
    """Scaffold links of the FINAL graph over the ranks (include/genome_amd.h, "scaffold links"): pairLinks of the rank's `npairs`
    pairs in `share` on its replica, the classes summed over the ranks, the link tables summed by gk_dist_reduce_links, then — per
    rank, on the summed table — joins at `min_support`, chains and gaps (mid - floor(sum_u / count); mid defaults to max_span
    div 2) -> {"links" (the HipLinks: the caller closes it), "classes", "joins", "join_stats", "chains", "cycles", "gaps"}.
    Joins, chains and the records of a scaffold text follow THIS rank's edge ids: the ranks agree on the set of joins, chains and
    records, not on their order."""
    vm, links = g.getGraphMap(), HipLinks(hd.ctx)
    try:
        mine = g.pairLinks(vm, (share, npairs), links, min_len=min_len, max_span=max_span) if npairs > 0 else dict.fromkeys(LINK_CLASSES, 0)
        total = hd.allreduce([float(mine[key]) for key in LINK_CLASSES])
        hd.reduce_links(g, links)
        joins, join_stats = links.joins(min_support)
        chains, cycles = scaffoldChains(joins[0], joins[1], with_cycles=True)
        gaps = scaffoldGaps(chains, joins, max_span // 2 if mid is None else mid)
    except BaseException:
        links.close()
        raise
    finally:
        vm.close()
    return {"links": links, "classes": {key: int(v) for key, v in zip(LINK_CLASSES, total)}, "joins": joins, "join_stats": join_stats,
            "chains": chains, "cycles": cycles, "gaps": gaps}


def _rank_share(hd: HipDist, data: PairedEndData, take_first: int | None):
    a, b = pair_share(data.count, hd.world, hd.rank, take_first)
    off = dna.bin_pair_offsets(data.bin, b)
    return a, b, np.frombuffer(data.bin, np.uint8)[int(off[a]):int(off[b])]


def build_graph(hd: HipDist, data: PairedEndData, k: int, rounds=3, take_first: int | None = None, retain: bool = True,
                simplify: bool = False, walk_pairs=None, classified: bool = True, auto_range=None) -> tuple[HipGraph, dict]:
    """One rank's part of the N-rank GraphBuilder (+ GraphSimplifier pairs stage) -> (this rank's graph replica, stats).
    `stats` holds graph_builder's JSON keys (the walk_pairs object only with walk_pairs) plus occurrences_sent,
    occurrences_owned (this rank's windows) and world.  rounds = "auto": the cutoff is the valley of the REDUCED count spectrum
    (gk_dist_spectrum: every rank filters alike), 3 when it has none; `stats` then also holds rounds_auto, valley, peak and
    genome_size_estimate, and "rounds" is the number used.  walk_pairs = (cutoff, "auto", None): the range of the walks is
    estimated from the pairs over all ranks (estimate_range; auto_range = its max_insert / trim / min_observations as a dict).
    The caller closes the graph."""
    auto = None
    a, b, share = _rank_share(hd, data, take_first)
    pm = DistDNAMap(hd, k)
    try:
        sent, owned = pm.count_reads(share, 2 * (b - a))                   # FreqFilter.scala:44-48
        if rounds == "auto":
            auto = auto_rounds(pm)
            rounds = auto["rounds"]
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
            walk = _pairs_stage(hd, g, share, b - a, walk_pairs, auto_range)
        n2, e2, l2 = g.counts()
    except BaseException:
        g.close()
        raise
    stats = {"k": k, "rounds": rounds, "good_kmers": good, "graph_nodes": nodes, "graph_edges": edges, "total_edges_length": total_len,
             "components": comps, "max_component_size": kept, "retained_nodes": n2, "retained_edges": e2, "retained_edges_length": l2}
    if walk is not None:
        stats["walk_pairs"] = walk
    if auto is not None:
        stats.update({key: auto[key] for key in ("rounds_auto", "valley", "peak", "genome_size_estimate")})
    stats["components_histogram"] = [list(x) for x in hist]
    stats["components_histogram_2"] = [list(x) for x in hist2]
    stats.update({"occurrences_sent": sent, "occurrences_owned": owned, "world": hd.world})
    return g, stats


def simplify_graph(hd: HipDist, graph_path, data: PairedEndData, cutoff: int, lo=180, hi=250,
                   take_first: int | None = None, max_insert: int = 4095, trim: int = 25, min_observations: int = 1000,
                   thread_reads: bool = False, walk: bool = True, resolve_repeats=None, links=None) -> tuple[HipGraph, dict]:
    """One rank's part of GraphSimplifier.startup (S/scripts/GraphSimplifier.scala:152-318) over N ranks: every rank loads the
    same graph file (:152-153, so the replicas are identical, ids included), then walks its own share of the pairs and the
    supports are summed over the ranks before the split, as in build_graph's pairs stage.  The range defaults to the
    reference's 180 to 250 (:146); lo = "auto" estimates it from the same pairs over all ranks before walking (estimate_range:
    max_insert, trim and min_observations are its knobs — choices, not measurements — and walk_pairs["insert_range"] says what
    was found; without an estimate the walks fall back to 180 to 250).  -> (this rank's graph, stats): k, the live counts before and after, the walk_pairs object,
    components_histogram_2 and max_component_size of the final graph (:320-331), and world.  thread_reads = True threads each
    rank's share of the reads through the graph into the same support before the reduce (this project's own rule,
    gk_graph_thread_reads; walk_pairs["thread_reads"] holds the stats over all ranks); walk = False skips the walks, so that the
    reads alone are the evidence.
    resolve_repeats = (cutoff, rounds) (default None: off): after the stage's split and simplify, up to `rounds` rounds of
    _resolve_stage over this rank's share of the reads (both mates of its pairs); stats["resolve_repeats"] holds the rounds.
    With it, walk = False without thread_reads is allowed: the paired-end stage is skipped altogether (stats["walk_pairs"] is
    None), as `graph_simplifier --no-pairs --resolve-repeats` does on one GPU.
    links = dict(min_support, min_len, max_span, mid) (default None: off; any key may be left out): _links_stage on the FINAL
    graph; stats["links"] holds its result — the summed HipLinks under "links" (the caller closes it), the classes over all
    ranks, joins, chains and gaps — so that the caller goes on to HipGraph.scaffolds, fillGaps, overlapGaps and judge_scaffolds
    as on one GPU.  Record order in a scaffold text follows a rank's own edge ids: the ranks agree on the SET of records, not
    on their order.  COLLECTIVE.  The caller closes the graph."""
    g = loadGraph(hd.ctx, graph_path)
    try:
        a, b, share = _rank_share(hd, data, take_first)
        n1, e1, l1 = g.counts()
        if not walk and not thread_reads and resolve_repeats is not None:
            walk = None                     # no support was gathered: the node split does not run and the spans alone edit the graph
        else:
            walk = _pairs_stage(hd, g, share, b - a, (cutoff, lo, hi),
                                {"max_insert": max_insert, "trim": trim, "min_observations": min_observations}, thread_reads, walk)
        resolved = _resolve_stage(hd, g, share, 2 * (b - a), *resolve_repeats) if resolve_repeats is not None else None
        linked = _links_stage(hd, g, share, b - a, **links) if links is not None else None
        n2, e2, l2 = g.counts()
        sizes, _ = g.componentStats()
        _, hist2 = g.componentHistograms()
    except BaseException:
        g.close()
        raise
    stats = {"k": g.k, "nodes": n1, "edges": e1, "edges_length": l1, "walk_pairs": walk, "simplified_nodes": n2, "simplified_edges": e2,
             "simplified_edges_length": l2, "components_histogram_2": [list(x) for x in hist2],
             "max_component_size": int(sizes.max()) if len(sizes) else 0, "world": hd.world}
    if resolved is not None:
        stats["resolve_repeats"] = resolved
    if linked is not None:
        stats["links"] = linked
    return g, stats
