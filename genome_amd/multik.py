"""Multi-k assembly (this project's own; the reference builds its graph at one k): assemble at a small k, clean the graph, add the
contigs' k2-mers to the count table of the next k as solid k-mers beside the reads' own counts (HipDNAMap.add_graph_paths;
include/genome_amd.h, "multi-k"), build again.  The small-k contigs carry the connectivity across coverage dips, the reads at the
large k the repeat resolution — the k-iteration of IDBA and SPAdes.  One GPU; all compute happens on it through the C-ABI.
"""
from __future__ import annotations

from .dnamap import GRAPH_PATHS_STATS, Context, HipDNAMap
from .freqfilter import auto_rounds
from .graph import buildGraph

MAX_CLEAN_ROUNDS = 8


def k_supported(k) -> bool:
    """the k a table can be made for (gk_map_create): 2..31 with 8-byte keys, 34..64 with 16-byte keys"""
    return isinstance(k, int) and not isinstance(k, bool) and (2 <= k <= 31 or 34 <= k <= 64)


def check_ks(ks):
    """-> ks as a list; ValueError unless it is non-empty, strictly increasing and every member a supported k"""
    ks = list(ks)
    if not ks:
        raise ValueError("ks is empty")
    for k in ks:
        if not k_supported(k):
            raise ValueError(f"k = {k!r} is not supported (2..31 or 34..64)")
    if any(a >= b for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks must be strictly increasing: {ks}")
    return ks


def clean(graph, counts, clip_tips: bool, pop_bubbles: bool, keep_cycles: bool = False, remove_weak=None) -> int:
    """graph_builder's clean-up loop: clip if asked, pop if asked, remove weak connections if asked, simplifyGraph, until a round
    removes nothing, MAX_CLEAN_ROUNDS at most -> the rounds that removed something.  remove_weak: None (off), or a dict with any of
    "max_len" (default 2k), "ratio" (default 5), "floor" (default 0) — HipGraph.removeWeakEdges' keywords."""
    rounds = 0
    while (clip_tips or pop_bubbles or remove_weak is not None) and rounds < MAX_CLEAN_ROUNDS:
        gone = 0
        if clip_tips:
            gone += graph.clipTips(counts)
        if pop_bubbles:
            gone += graph.popBubbles(counts)[0]
        if remove_weak is not None:
            gone += graph.removeWeakEdges(counts, **remove_weak)["removed"]
        if not gone:
            break
        graph.simplifyGraph(keep_cycles)
        rounds += 1
    return rounds


def assemble(ctx: Context, bin_bytes, nreads: int, ks, rounds=3, clip_tips: bool = False, pop_bubbles: bool = False,
             keep_cycles: bool = False, remove_weak=None):
    """One stage per k of `ks` (strictly increasing, every member supported: ValueError before any device work otherwise):
    count the reads at k; seed the table with the previous stage's contigs at weight = rounds; deleteAll(< rounds); buildGraph;
    the clean-up loop (remove_weak: off by default; a dict of HipGraph.removeWeakEdges' keywords — "max_len", "ratio", "floor", {} for
    its defaults — adds that step to every stage's rounds).  Every stage but the last — a seed stage — ends in simplifyGraph and never retains the largest component
    (that would drop replicons); the last stage's graph is left to the caller as buildGraph + the loop leave it.
    rounds = "auto": the valley of that stage's spectrum BEFORE seeding (the seeds would move it), 3 when it has none.
    -> (map, graph, stages): the last stage's table and graph (the caller closes both) and one dict per stage: "k", "rounds",
    "distinct_before_seed", "distinct_after_seed", the six add_graph_paths stats (zeros for the first stage), "nodes", "edges"."""
    ks = check_ks(ks)
    if remove_weak is not None and not (isinstance(remove_weak, dict) and set(remove_weak) <= {"max_len", "ratio", "floor"}):
        raise ValueError('remove_weak is None or a dict with keys among "max_len", "ratio", "floor"')
    if rounds != "auto" and not (isinstance(rounds, int) and 1 <= rounds <= 65535):
        raise ValueError('rounds is 1..65535 or "auto"')
    stages = []
    prev = None                                   # (map, graph) of the stage before
    for i, k in enumerate(ks):
        m = HipDNAMap(ctx, k)
        g = None
        try:
            m.count_reads(bin_bytes, nreads)
            r = auto_rounds(m)["rounds"] if rounds == "auto" else rounds
            before = m.size()
            if prev is not None:
                seeded = m.add_graph_paths(prev[1], r)
                prev[1].close()
                prev[0].close()
                prev = None
            else:
                seeded = dict.fromkeys(GRAPH_PATHS_STATS, 0)
            after = m.size()
            m.deleteAll_lt(r)
            g = buildGraph(k, m, keep_cycles)
            clean(g, m, clip_tips, pop_bubbles, keep_cycles, remove_weak)
            if i + 1 < len(ks):
                g.simplifyGraph(keep_cycles)
            nodes, edges, _ = g.counts()
        except BaseException:
            if g is not None:
                g.close()
            m.close()
            if prev is not None:
                prev[1].close()
                prev[0].close()
            raise
        stages.append({"k": k, "rounds": r, "distinct_before_seed": before, "distinct_after_seed": after, **seeded,
                       "nodes": nodes, "edges": edges})
        prev = (m, g)
    return prev[0], prev[1], stages
