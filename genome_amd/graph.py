"""Host-side mirror of `object Graph` / `trait Graph` / `MapGraph` (S/data/graph/Graph.scala) over
the HIP library: buildGraph, simplifyGraph, removeBubbles, removeEdge, components+retain, and the
canonical serialisation used for parity.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import _lib as L
from . import dna
from .dnamap import HipDNAMap
from .partitioned import PartitionedDNAMap


class HipGraph:
    """A MapGraph resident in HBM."""

    def __init__(self, ctx, k: int, handle):
        self.ctx, self.k, self.h = ctx, k, handle
        self._cycle_stats = None

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():      # process exit: the HIP runtime may already be gone, and frees everything anyway
            return
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        n, e, ln = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_counts(self.h, C.byref(n), C.byref(e), C.byref(ln)), self.ctx.h)
        return n.value, e.value, ln.value

    def contigStats(self, longer_than: int = 200) -> dict:
        """CheckGraph.scala:37-41 over the live edges longer than `longer_than`: count, summed length, median (= sorted[count/2],
        the reference's "N50"), the real N50 and the maximum; all 0 when there is none.  Computed on the device."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        v = [C.c_uint64() for _ in range(5)]
        L.check(L.lib().gk_graph_contig_stats(self.h, int(longer_than), *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("count", "sum", "median", "n50", "max"), (x.value for x in v)))

    def simplifyGraph(self, keep_cycles: bool = False):    # Graph.scala:211-230
        """keep_cycles: self-loop nodes stay and every cycle of merge-away nodes keeps its anchors (include/genome_amd.h, "perfect
        cycles"); returns the CYCLE_SIMPLIFY_STATS dict then, None otherwise."""
        if not keep_cycles:
            L.check(L.lib().gk_graph_simplify(self.h), self.ctx.h)
            return None
        st = (C.c_uint64 * 4)()
        L.check(L.lib().gk_graph_simplify_keep_cycles(self.h, st), self.ctx.h)
        return dict(zip(CYCLE_SIMPLIFY_STATS, (int(x) for x in st)))

    def cycleStats(self):
        """The CYCLE_BUILD_STATS dict of buildGraph(keep_cycles=True); None for a graph built without it (or loaded)."""
        return self._cycle_stats

    def removeBubbles(self):                       # Graph.scala:125-149
        L.check(L.lib().gk_graph_remove_bubbles(self.h), self.ctx.h)

    def removeEdges(self, edges) -> int:           # Graph.scala:191-195, batched: [(start k-mer str, first base char)]
        lo, hi = dna.pack_many([s for s, _ in edges])
        base = np.array([dna.BASES.index(b) for _, b in edges], np.uint8)
        removed = C.c_uint64()
        L.check(L.lib().gk_graph_remove_edges(self.h, L.ptr(lo, C.c_uint64), L.ptr(hi, C.c_uint64), L.ptr(base, C.c_uint8),
                                              len(base), C.byref(removed)), self.ctx.h)
        return removed.value

    def retainLargest(self):                       # Graph.scala:54-72,161-165; GraphBuilder.scala:52-54
        kept, comps = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_retain_largest(self.h, C.byref(kept), C.byref(comps)), self.ctx.h)
        return kept.value, comps.value

    def componentStats(self):
        """-> (nodes per component, summed out-edge length per component), one entry per component."""
        n = C.c_uint64()
        rc = L.lib().gk_graph_component_stats(self.h, None, None, 0, C.byref(n))
        if rc not in (L.GK_OK, L.GK_E_CAPACITY):
            L.check(rc, self.ctx.h)
        nodes, length = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64)
        if n.value:
            L.check(L.lib().gk_graph_component_stats(self.h, L.ptr(nodes, C.c_uint32), L.ptr(length, C.c_uint64), n.value, C.byref(n)), self.ctx.h)
        return nodes, length

    def componentHistograms(self):
        """GraphBuilder.scala:41-47: `hist` = components by node count, `hist2` = components by summed out-edge length,
        each as a sorted list of (value, number of components)."""
        nodes, length = self.componentStats()
        h1 = sorted((int(a), int(b)) for a, b in zip(*np.unique(nodes, return_counts=True)))
        h2 = sorted((int(a), int(b)) for a, b in zip(*np.unique(length, return_counts=True)))
        return h1, h2

    def checksum(self):
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_checksum(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def buildStats(self):
        ms = (C.c_float * 6)()
        bases, pj = C.c_uint64(), C.c_int()
        L.check(L.lib().gk_graph_build_stats(self.h, ms, C.byref(bases), C.byref(pj)), self.ctx.h)
        names = ("classify", "make_nodes", "unitig_measure", "reserve_pool", "unitig_emit", "index_counts")
        mb_ms, mb_slots = C.c_float(), C.c_uint64()
        L.check(L.lib().gk_graph_bucketed_table_stats(self.h, C.byref(mb_ms), C.byref(mb_slots)), self.ctx.h)
        by_owners = C.c_int()
        L.check(L.lib().gk_graph_classified_by_owners(self.h, C.byref(by_owners)), self.ctx.h)
        return {"phase_ms": {n_: float(x) for n_, x in zip(names, ms)}, "walked_bases": bases.value, "pointer_jumping": bool(pj.value),
                "bucketed_table": {"build_ms": float(mb_ms.value), "slots": mb_slots.value}, "classified_by_owners": bool(by_owners.value)}

    # ---- GraphSimplifier's tools: the position map, ids, point edits ----------------------------
    def getGraphMap(self, capacity_hint: int = 0):         # Graph.scala:90-119
        from .dnamap import HipValueMap
        n, e, ln = self.counts()
        vm = HipValueMap(self.ctx, self.k, capacity_hint or (ln + n - e))
        got = C.c_uint64()
        L.check(L.lib().gk_graph_position_map(self.h, vm.h, C.byref(got)), self.ctx.h)
        assert got.value == ln + n - e                       # the reference prints both, :117
        return vm

    def nodeId(self, kmer: str, base=None):
        """(node id or None, id of its out-edge starting with `base` or None)"""
        lo, hi = dna.pack(kmer)
        a, b = C.c_uint32(), C.c_uint32()
        L.check(L.lib().gk_graph_node_lookup(self.h, lo, hi, -1 if base is None else dna.BASES.index(base), C.byref(a), C.byref(b)), self.ctx.h)
        none = 0xffffffff
        return (None if a.value == none else a.value), (None if b.value == none else b.value)

    def nodesById(self, ids):
        ids = np.ascontiguousarray(ids, np.uint32)
        n = len(ids)
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        alive, ind, outd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        L.check(L.lib().gk_graph_nodes_by_id(self.h, L.ptr(ids, C.c_uint32), n, L.ptr(lo, C.c_uint64), L.ptr(hi, C.c_uint64), L.ptr(alive, C.c_uint8),
                                             L.ptr(ind, C.c_uint32), L.ptr(outd, C.c_uint32)), self.ctx.h)
        return {"lo": lo, "hi": hi, "alive": alive.astype(bool), "in_deg": ind, "out_deg": outd}

    def edgesById(self, ids):
        ids = np.ascontiguousarray(ids, np.uint32)
        n = len(ids)
        s, e = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ln, first, alive = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        L.check(L.lib().gk_graph_edges_by_id(self.h, L.ptr(ids, C.c_uint32), n, L.ptr(s, C.c_uint32), L.ptr(e, C.c_uint32), L.ptr(ln, C.c_uint64),
                                             L.ptr(first, C.c_uint8), L.ptr(alive, C.c_uint8)), self.ctx.h)
        return {"start": s, "end": e, "len": ln, "first": first, "alive": alive.astype(bool)}

    def addNode(self, kmer: str) -> int:                   # Graph.scala:172-176
        lo, hi = dna.pack(kmer)
        out = C.c_uint32()
        L.check(L.lib().gk_graph_add_node(self.h, lo, hi, C.byref(out)), self.ctx.h)
        return out.value

    def replaceStart(self, edge_id: int, node_id: int):    # :197-202
        L.check(L.lib().gk_graph_replace_start(self.h, edge_id, node_id), self.ctx.h)

    def replaceEnd(self, edge_id: int, node_id: int):      # :204-209
        L.check(L.lib().gk_graph_replace_end(self.h, edge_id, node_id), self.ctx.h)

    # ---- paired-end walking (S/scripts/GraphSimplifier.scala:188-318)
    def idBounds(self):
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_id_bounds(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def idFingerprint(self) -> int:
        """an id-exact fingerprint (live nodes and edges WITH their ids, and the id bounds): equal on two replicas iff their ids
        mean the same nodes and edges — what gk_dist_reduce_support checks before it adds supports keyed by edge ids"""
        fp = C.c_uint64()
        L.check(L.lib().gk_graph_id_fingerprint(self.h, C.byref(fp)), self.ctx.h)
        return fp.value

    def removeEdgesById(self, edge_ids) -> int:             # toRemove.foreach(id => graph.removeEdge(graph.getEdge(id)))  :316
        ids = np.ascontiguousarray(edge_ids, np.uint32)
        rm = C.c_uint64()
        L.check(L.lib().gk_graph_remove_edges_by_id(self.h, L.ptr(ids, C.c_uint32), len(ids), C.byref(rm)), self.ctx.h)
        return rm.value

    # ---- edge coverage and tips (this project's own rules: include/genome_amd.h) ---------------------------------------
    def edgeCoverage(self, counts: HipDNAMap, edge_ids=None) -> dict:
        """How often the k-mers of the edges were seen, from the count table `counts` (the one the graph was built from, or any
        table of this k): per id `kmers` (= len + 1 windows, both end nodes included), `sum`, `min`, `max` of their counts (zeros
        for a dead or out-of-range id), and `missing` = windows `counts` does not hold.  Default: every id below idBounds()."""
        ids = np.arange(self.idBounds()[1], dtype=np.uint32) if edge_ids is None else np.ascontiguousarray(edge_ids, np.uint32)
        n = len(ids)
        kmers, total = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        mn, mx = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        missing = C.c_uint64()
        L.check(L.lib().gk_graph_edge_coverage(self.h, counts.h, L.ptr(ids, C.c_uint32), n, L.ptr(kmers, C.c_uint64), L.ptr(total, C.c_uint64),
                                               L.ptr(mn, C.c_uint32), L.ptr(mx, C.c_uint32), C.byref(missing)), self.ctx.h)
        return {"ids": ids, "kmers": kmers, "sum": total, "min": mn, "max": mx, "missing": missing.value}

    def clipTips(self, counts: HipDNAMap, max_len=None) -> int:
        """One round of tip removal: dead-end edges of at most `max_len` bases (default 2k) beside an edge of strictly higher mean
        coverage -> the number removed.  Call simplifyGraph() next.  GkError GK_E_STATE if `counts` is not this graph's table."""
        rm = C.c_uint64()
        L.check(L.lib().gk_graph_clip_tips(self.h, counts.h, 2 * self.k if max_len is None else int(max_len), C.byref(rm)), self.ctx.h)
        return rm.value

    def edgeDistance(self, e1, e2, max_diff: int) -> np.ndarray:
        """Per pair of edge ids min(Levenshtein distance of the two edges' sequences, max_diff + 1), as uint32; 0xffffffff where
        an id is dead or out of range.  max_diff is at most 31 (GkError GK_E_INVALID beyond)."""
        e1, e2 = np.ascontiguousarray(e1, np.uint32), np.ascontiguousarray(e2, np.uint32)
        assert e1.shape == e2.shape and e1.ndim == 1
        dist = np.zeros(len(e1), np.uint32)
        L.check(L.lib().gk_graph_edge_distance(self.h, L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), len(e1), int(max_diff), L.ptr(dist, C.c_uint32)), self.ctx.h)
        return dist

    def popBubbles(self, counts: HipDNAMap, max_len=None, max_diff=None):
        """One round of bubble removal: of two parallel edges (same start and end node) of at most `max_len` bases (default 2k)
        within edit distance `max_diff` (default 3, the reference's commented-out `maxerrors`), the one of strictly lower mean
        coverage goes -> (edges removed, pairs compared).  Call simplifyGraph() next.  GkError GK_E_STATE if `counts` is not this
        graph's table."""
        rm, pairs = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_pop_bubbles(self.h, counts.h, 2 * self.k if max_len is None else int(max_len), 3 if max_diff is None else int(max_diff),
                                             C.byref(rm), C.byref(pairs)), self.ctx.h)
        return rm.value, pairs.value

    def removeWeakEdges(self, counts: HipDNAMap, max_len=None, ratio: int = 5, floor: int = 0) -> dict:
        """One round of weak-connection removal: an edge of at most `max_len` bases (default 2k) whose start node has another way
        out and whose end node another way in goes if at each end one of those other edges has more than `ratio` times its mean
        coverage (ratio = 0: off; at most 65535); so does any edge whose mean coverage is below `floor` (0: off).  -> the four
        numbers of WEAK_STATS.  ratio 5 and 2k are choices, not measurements.  Call simplifyGraph() next.  GkError GK_E_STATE if
        `counts` is not this graph's table."""
        st = np.zeros(len(WEAK_STATS), np.uint64)
        L.check(L.lib().gk_graph_remove_weak_edges(self.h, counts.h, 2 * self.k if max_len is None else int(max_len), int(ratio), int(floor),
                                                   L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(WEAK_STATS, (int(x) for x in st)))

    # ---- contigs as FASTA (this project's own rule: include/genome_amd.h) ----------------------------------------------
    def contigs(self, counts: HipDNAMap = None, min_len: int = 0, line_width: int = 60, strands: int = 1) -> "Contigs":
        """The assembly as FASTA text, planned on the device: one record `>e<id> len=<n>[ cov=<mean>]` per live edge whose path
        (start k-mer ++ seq, n bases) is not above its reverse complement (strands = 2: every live edge), n >= min_len, in
        ascending edge id, the sequence wrapped at `line_width` (0: one line).  `counts` (any table of this k) adds the cov=
        field.  -> a Contigs: stats(), read(), text(), write().  Any edit of the graph makes it stale (GkError GK_E_STATE)."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        h = L.vp()
        L.check(L.lib().gk_graph_contigs_plan(self.h, counts.h if counts is not None else None, int(min_len), int(line_width), int(strands),
                                              C.byref(h)), self.ctx.h)
        return Contigs(self, h)

    # ---- edge twins and the graph as GFA 1.0 (this project's own rules: include/genome_amd.h) ---------------------------
    def edgeTwins(self, ids=None):
        """The twin of every edge asked for (default: every id below idBounds()), by content, exactly -> (twin, cls, stats).
        cls[i] indexes TWIN_CLASSES; twin[i] is the twin's id for `paired`, the edge's own for `self`, 0xffffffff for `missing`,
        `ambiguous` and a dead or out-of-range id.  stats: the six numbers of TWIN_STATS over ALL live edges."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        ids = np.arange(self.idBounds()[1], dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, np.uint32)
        n = len(ids)
        twin, cls = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        st = np.zeros(len(TWIN_STATS), np.uint64)
        L.check(L.lib().gk_graph_edge_twins(self.h, L.ptr(ids, C.c_uint32), n, L.ptr(twin, C.c_uint32), L.ptr(cls, C.c_uint8), L.ptr(st, C.c_uint64)),
                self.ctx.h)
        return twin, cls, dict(zip(TWIN_STATS, (int(x) for x in st)))

    def gfa(self, counts: HipDNAMap = None) -> "Gfa":
        """The graph as GFA 1.0 text, planned on the device: one S line per segment (a twin pair's forward edge, or an edge that
        has no single twin), one L line per pair of edges that meet in a node, each mirror pair once, the overlap being the node's
        k bases.  `counts` (any table of this k) adds KC:i: to the S lines.  -> a Gfa: stats(), read(), text(), write().  Any edit
        of the graph makes it stale (GkError GK_E_STATE)."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        h = L.vp()
        L.check(L.lib().gk_graph_gfa_plan(self.h, counts.h if counts is not None else None, C.byref(h)), self.ctx.h)
        return Gfa(self, h)

    # ---- scaffolds as FASTA (this project's own rule: include/genome_amd.h) --------------------------------------------
    def scaffolds(self, chains, gaps, min_gap: int = 10, min_len: int = 0, line_width: int = 60, strands: int = 1, singletons: bool = True,
                  overlaps=None) -> "Scaffolds":
        """The chains (lists of edge ids, scaffoldChains') as FASTA text, planned on the device: one record
        `>s<c> len=<n> contigs=<m> gaps=<N bases>` per chain whose sequence is not above its reverse complement (strands = 2:
        every chain).  Consecutive members that meet in a node are joined on its k bases; between any others go
        max(gap, min_gap) bases N, `gaps[c][i]` being the gap after member i of chain c (scaffoldGaps; an entry for the last member
        may be left out or is ignored).  singletons: the live edges in no chain follow as contigs() would write them (min_len
        applies to them alone).  min_gap = 10 is a choice, not a measurement.  overlaps: overlapGaps' lists, in the shape of `gaps`;
        where overlaps[c][i] = o > 0 nothing goes between the two members and the next one contributes its path from base o (the
        plan checks every o against the paths: GkError GK_E_INVALID for one that does not hold).  -> a Scaffolds: stats(),
        overlapStats(), read(), text(), write(), segments().  Any edit of the graph makes it stale (GkError GK_E_STATE)."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        chains = [list(c) for c in chains]
        assert _junction_lists(chains, gaps)
        (members, off), gap = _flat_chains(chains), _flat_junctions(chains, gaps, np.int64)
        h = L.vp()
        if overlaps is None:
            L.check(L.lib().gk_graph_scaffolds_plan(self.h, L.ptr(members, C.c_uint32), L.ptr(off, C.c_uint64), len(chains), L.ptr(gap, C.c_int64), int(min_gap),
                                                    int(min_len), int(line_width), int(strands), int(bool(singletons)), C.byref(h)), self.ctx.h)
            return Scaffolds(self, h)
        if not _junction_lists(chains, overlaps):
            raise ValueError("scaffolds: one overlap list per chain, with an entry per junction")
        ovl = _flat_junctions(chains, overlaps, np.uint32)
        L.check(L.lib().gk_graph_scaffolds_plan_overlaps(self.h, L.ptr(members, C.c_uint32), L.ptr(off, C.c_uint64), len(chains), L.ptr(gap, C.c_int64),
                                                         L.ptr(ovl, C.c_uint32), int(min_gap), int(min_len), int(line_width), int(strands), int(bool(singletons)),
                                                         C.byref(h)), self.ctx.h)
        return Scaffolds(self, h)

    # ---- placements on a reference (this project's own rule: include/genome_amd.h) -------------------------------------
    def place(self, positions, records) -> "Placements":
        """Every edge placed on a reference genome: `records` is an iterable of str / bytes, one joined sequence per reference
        record (genome_amd.check.fasta_records splits a FASTA text), `positions` getGraphMap of this graph as it is now.
        -> a Placements: stats(), edges(), last_ms(); Scaffolds.judge takes it.  Any edit of the graph makes it stale."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        p = Placements(self, positions)
        try:
            for r in records:
                p.add(r)
        except Exception:
            p.close()
            raise
        return p

    def alignBlocks(self, positions, records=(), tol=None) -> "Blocks":
        """Every edge aligned to a reference genome in blocks (include/genome_amd.h, "alignment blocks" and "breakpoints"):
        `positions` getGraphMap of this graph as it is now; `records` as for place(), fed at once; with `tol` the result is
        finished too.  -> a Blocks: add_record(), finish(tol), stats(), rows(), edges(), pieces(), na50()."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        b = Blocks(self, positions)
        try:
            for r in records:
                b.add_record(r)
            if tol is not None:
                b.finish(tol)
        except Exception:
            b.close()
            raise
        return b

    # ---- overlap detection (this project's own rule: include/genome_amd.h) ---------------------------------------------
    def overlapGaps(self, chains, gaps, tol: int, min_overlap: int = 10, max_overlap=None):
        """Between fillGaps (or scaffoldChains / scaffoldGaps) and scaffolds(): where the last o bases of a member's path equal the
        first o bases of the next member's, exactly, for exactly one o in min_overlap .. max_overlap within `tol` of -gap (and
        below both path lengths), the junction is an overlap of o bases -> (overlaps, report): overlaps[c][i] = o after member i
        of chain c, else 0, the shape scaffolds(overlaps=) takes; report = the seven stats named as OVERLAP_STATS, plus
        "classes": per chain the class name of every junction (OVERLAP_CLASSES).  max_overlap None means k.  min_overlap = 10 and
        max_overlap = k are choices, not measurements (a chance match of 10 bases is about 1e-6 per candidate).  The graph is not
        edited and the chains are not rewritten."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        chains = [list(c) for c in chains]
        if not _junction_lists(chains, gaps):
            raise ValueError("overlapGaps: one gap list per chain, with an entry per junction")
        (members, off), gap = _flat_chains(chains), _flat_junctions(chains, gaps, np.int64)
        nm = len(members)
        ovl, jclass, st = np.zeros(max(nm, 1), np.uint32), np.zeros(max(nm, 1), np.uint8), np.zeros(len(OVERLAP_STATS), np.uint64)
        L.check(L.lib().gk_graph_overlap_gaps(self.h, L.ptr(members, C.c_uint32), L.ptr(off, C.c_uint64), len(chains), L.ptr(gap, C.c_int64), int(tol),
                                              int(min_overlap), int(self.k if max_overlap is None else max_overlap), L.ptr(ovl, C.c_uint32),
                                              L.ptr(jclass, C.c_uint8), L.ptr(st, C.c_uint64)), self.ctx.h)
        report = dict(zip(OVERLAP_STATS, (int(x) for x in st)))
        report["classes"] = [[OVERLAP_CLASSES[x] for x in c] for c in _per_junction(jclass, off)]
        return _per_junction(ovl, off), report

    # ---- gap filling (this project's own rule: include/genome_amd.h) ---------------------------------------------------
    def fillGaps(self, chains, gaps, tol: int, max_edges: int = 16, max_paths: int = 256):
        """Between scaffoldChains / scaffoldGaps and scaffolds(): where the graph holds exactly one path of at most `max_edges`
        edges from the end of a member to the start of the next whose length is within `tol` bases of the gap, and no edge of it is
        a member or lies on another such path, its edges are spliced in as members -> (chains, gaps, report), the first two in
        the shape scaffolds() takes (a new junction's gap is -k; it is adjacent and never looked at).  report = the ten stats
        named as FILL_STATS, plus "classes": per chain the class name of every junction (FILL_CLASSES) and "lengths": per chain
        the path's gap length L where the class is shared or filled, else 0.  Junctions searched with more than `max_paths`
        bounded paths from both sides stay as they are (overflow).  max_edges = 16 and max_paths = 256 are choices, not
        measurements.  The graph is not edited."""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the graph is closed")
        chains = [list(c) for c in chains]
        if not _junction_lists(chains, gaps):
            raise ValueError("fillGaps: one gap list per chain, with an entry per junction")
        (members, off), gap = _flat_chains(chains), _flat_junctions(chains, gaps, np.int64)
        nm, cap = len(members), self.idBounds()[1]             # (no edge is written twice: the filled chains fit the edge ids)
        out_m, out_g, out_off = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int64), np.zeros(len(chains) + 1, np.uint64)
        jclass, jlen, st, n = np.zeros(max(nm, 1), np.uint8), np.zeros(max(nm, 1), np.int64), np.zeros(len(FILL_STATS), np.uint64), C.c_uint64()
        L.check(L.lib().gk_graph_fill_gaps(self.h, L.ptr(members, C.c_uint32), L.ptr(off, C.c_uint64), len(chains), L.ptr(gap, C.c_int64), int(tol), int(max_edges),
                                           int(max_paths), L.ptr(out_m, C.c_uint32), L.ptr(out_g, C.c_int64), cap, L.ptr(out_off, C.c_uint64),
                                           L.ptr(jclass, C.c_uint8), L.ptr(jlen, C.c_int64), C.byref(n), L.ptr(st, C.c_uint64)), self.ctx.h)
        o = out_off.tolist()
        report = dict(zip(FILL_STATS, (int(x) for x in st)))
        report["classes"] = [[FILL_CLASSES[x] for x in c] for c in _per_junction(jclass, off)]
        report["lengths"] = _per_junction(jlen, off)
        return [out_m[a:b].tolist() for a, b in zip(o, o[1:])], _per_junction(out_g, out_off), report

    def walkPairs(self, positions, support: "Support", bin_bytes, npairs: int, range_lo: int = 180, range_hi: int = 250):
        """:213-247: the pairs' positions through `positions` (getGraphMap of this graph as it is now), annotate, the bounded
        walks; the supported (edge, edge) pairs are counted in `support`."""
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        L.check(L.lib().gk_graph_walk_pairs(self.h, positions.h, support.h, L.ptr(buf, C.c_uint8), buf.size, npairs, range_lo, range_hi), self.ctx.h)

    def pairDistances(self, positions, data, bins: int = 4096, take_first=None):
        """The fragment lengths of the pairs whose mates' first k-mers lie on one edge (the rule: include/genome_amd.h, "the
        insert range") -> (hist, classes): hist[D] = orientations counted at fragment length D (uint64[bins]; bins - 1 is the
        largest length looked for, and part of the rule), classes = {name: orientations} over PAIR_CLASSES.  `data`: a
        PairedEndData (its first `take_first` pairs), or (bin bytes, npairs).  Neither the graph nor `positions` (getGraphMap
        of this graph as it is now) changes."""
        bin_bytes, npairs = (data.bin, data.count) if hasattr(data, "bin") else data
        if take_first is not None:
            npairs = max(0, min(int(take_first), npairs))
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        hist, cls = np.zeros(max(int(bins), 1), np.uint64), np.zeros(len(PAIR_CLASSES), np.uint64)
        L.check(L.lib().gk_graph_pair_distances(self.h, positions.h, L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, npairs, int(bins),
                                                L.ptr(hist, C.c_uint64), L.ptr(cls, C.c_uint64)), self.ctx.h)
        return hist, dict(zip(PAIR_CLASSES, (int(x) for x in cls)))

    def pairLinks(self, positions, data, links: "HipLinks", min_len: int = 0, max_span: int = 4095, take_first=None) -> dict:
        """The pairs whose mates' first k-mers lie on two DIFFERENT edges (the rule: include/genome_amd.h, "scaffold links"), added
        to `links` as (e, f) -> count and sum_u -> {class: orientations} over LINK_CLASSES.  Edges whose contig is shorter than
        `min_len` bases link nothing; a fragment that needs more than `max_span` bases on the two edges is too_far (the tools pass
        the insert range's upper end + k).  `data`: a PairedEndData (its first `take_first` pairs), or (bin bytes, npairs).
        GkError, and `links` unchanged, on any error; the graph and `positions` never change."""
        bin_bytes, npairs = (data.bin, data.count) if hasattr(data, "bin") else data
        if take_first is not None:
            npairs = max(0, min(int(take_first), npairs))
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        cls = np.zeros(len(LINK_CLASSES), np.uint64)
        L.check(L.lib().gk_graph_pair_links(self.h, positions.h, links.h, L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, npairs, int(min_len),
                                            int(max_span), L.ptr(cls, C.c_uint64)), self.ctx.h)
        return dict(zip(LINK_CLASSES, (int(x) for x in cls)))

    def threadReads(self, positions, support: "Support", data, take_first=None) -> dict:
        """Every window of every read through `positions` (getGraphMap of this graph as it is now): a window that is a node's
        k-mer, entered by an in-edge and left by an out-edge of that node, adds one to `support` for that (in, out) pair, on both
        strands (the rule: include/genome_amd.h, gk_graph_thread_reads) -> the seven stats, named as THREAD_STATS.  `data`: a
        PairedEndData (both mates of its first `take_first` pairs, as single reads), or (bin bytes, records) (its first
        `take_first` records).  GkError, and `support` unchanged, on any error; the graph and `positions` never change."""
        if hasattr(data, "bin"):
            bin_bytes, nreads = data.bin, 2 * (data.count if take_first is None else max(0, min(int(take_first), data.count)))
        else:
            bin_bytes, nreads = data
            nreads = nreads if take_first is None else max(0, min(int(take_first), nreads))
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        st = np.zeros(len(THREAD_STATS), np.uint64)
        L.check(L.lib().gk_graph_thread_reads(self.h, positions.h, support.h, L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, nreads,
                                              L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(THREAD_STATS, (int(x) for x in st)))

    def threadReadsDev(self, positions, support: "Support", d_records: int, nreads: int, read_len: int) -> dict:
        """threadReads over records resident in HBM at stride 1 + ceil(read_len / 4) -> the seven stats"""
        st = np.zeros(len(THREAD_STATS), np.uint64)
        L.check(L.lib().gk_graph_thread_reads_dev(self.h, positions.h, support.h, d_records, nreads, read_len, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(THREAD_STATS, (int(x) for x in st)))

    def threadSpans(self, positions, spans: "HipSpans", data, nreads=None) -> dict:
        """Every read through `positions` (getGraphMap of this graph as it is now): for every edge m a strand of a read crosses
        from end to end, one is added to `spans` for (the edge it came by, m, the edge it left by) (the rule: include/genome_amd.h,
        gk_graph_thread_spans) -> the five stats, named as SPAN_STATS.  `data`: a PairedEndData (both mates of every pair, as
        single reads), or bin bytes with `nreads` records, or (bin bytes, records).  GkError, and `spans` unchanged, on any
        error; the graph and `positions` never change."""
        if hasattr(data, "bin"):
            bin_bytes, n = data.bin, 2 * data.count
        elif isinstance(data, tuple):
            bin_bytes, n = data
        else:
            bin_bytes, n = data, nreads
        if nreads is not None:
            n = max(0, min(int(nreads), n))
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        st = np.zeros(len(SPAN_STATS), np.uint64)
        L.check(L.lib().gk_graph_thread_spans(self.h, positions.h, spans.h, L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, n,
                                              L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(SPAN_STATS, (int(x) for x in st)))

    def threadSpansDev(self, positions, spans: "HipSpans", d_records: int, nreads: int, read_len: int) -> dict:
        """threadSpans over records resident in HBM at stride 1 + ceil(read_len / 4) -> the five stats"""
        st = np.zeros(len(SPAN_STATS), np.uint64)
        L.check(L.lib().gk_graph_thread_spans_dev(self.h, positions.h, spans.h, d_records, nreads, read_len, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(SPAN_STATS, (int(x) for x in st)))

    def splitEdgesBySpans(self, spans: "HipSpans", cutoff: int) -> dict:
        """Every edge whose in-edges and out-edges the spans pair off one to one at `cutoff` gets a copy per further pair (the
        rule: include/genome_amd.h, gk_graph_split_edges_by_spans) -> the seven stats, named as SPLIT_EDGE_STATS; call
        simplifyGraph() next."""
        st = np.zeros(len(SPLIT_EDGE_STATS), np.uint64)
        L.check(L.lib().gk_graph_split_edges_by_spans(self.h, spans.h, int(cutoff), L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(SPLIT_EDGE_STATS, (int(x) for x in st)))

    def splitBySupport(self, support: "Support", cutoff: int):
        """:272-316 -> (edges removed, nodes added); call simplifyGraph() next (:318)."""
        rm, nn = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_split_by_support(self.h, support.h, cutoff, C.byref(rm), C.byref(nn)), self.ctx.h)
        return rm.value, nn.value

    def getNodes(self):
        n = self.counts()[0]
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        got = C.c_uint64()
        L.check(L.lib().gk_graph_export_nodes(self.h, L.ptr(lo, C.c_uint64), L.ptr(hi, C.c_uint64), n, C.byref(got)), self.ctx.h)
        return lo, hi

    def getEdges(self):
        _, ne, ln = self.counts()
        a = {key: np.zeros(ne, np.uint64) for key in ("slo", "shi", "elo", "ehi")}
        length, off = np.zeros(ne, np.int64), np.zeros(ne, np.int64)
        cap = (ln + 3 * ne) // 4 + 1
        seq = np.zeros(cap, np.uint8)
        got, used = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_graph_export_edges(self.h, L.ptr(a["slo"], C.c_uint64), L.ptr(a["shi"], C.c_uint64),
                                              L.ptr(a["elo"], C.c_uint64), L.ptr(a["ehi"], C.c_uint64),
                                              L.ptr(length, C.c_int64), L.ptr(off, C.c_int64), ne, C.byref(got),
                                              L.ptr(seq, C.c_uint8), cap, C.byref(used)), self.ctx.h)
        a.update(len=length, off=off, seq=seq[:used.value])
        return a

    def out_order(self, kmer: str):
        lo, hi = dna.pack(kmer)
        arr, cnt = (C.c_int * 4)(), C.c_int()
        L.check(L.lib().gk_graph_out_order(self.h, lo, hi, arr, C.byref(cnt)), self.ctx.h)
        return None if cnt.value < 0 else [arr[i] for i in range(cnt.value)]

    # ---- the graph file (include/genome_amd.h, version 1) -------------------------------------------------------------
    def save(self, path):
        """MapGraph.write (Graph.scala:232-261): the live nodes and edges with their ids; written aside, then renamed onto path."""
        if not self.h:
            raise ValueError("graph is closed")
        L.check(L.lib().gk_graph_save(self.h, os.fsencode(path)), self.ctx.h)

    def canonical(self):
        """(sorted node strings, edges (start, end, seq) sorted by (start k-mer, first base))."""
        k = self.k
        lo, hi = self.getNodes()
        order = np.lexsort((lo, hi))
        nodes = [dna.unpack(int(lo[i]), int(hi[i]), k) for i in order]
        e = self.getEdges()
        first = np.array([(int(e["seq"][o]) & 3) if ln else 0 for o, ln in zip(e["off"], e["len"])], np.int64)
        order = np.lexsort((first, e["slo"], e["shi"]))
        edges = []
        for i in order:
            o, ln = int(e["off"][i]), int(e["len"][i])
            edges.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k),
                          dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k),
                          dna.unpack_2bit(e["seq"][o:o + (ln + 3) // 4], ln)))
        return nodes, edges


# the statistics of gk_contigs_stats, in the order of its `stats9` array: live_edges is the sum of the four after it
CONTIG_STATS = ("live_edges", "short", "forward", "self_twin", "reverse", "records", "bases", "text_bytes", "missing_windows")


class Contigs:
    """A plan of the FASTA text of a graph's contigs (HipGraph.contigs): the text itself is emitted by the device when it is
    read or written.  Holds its graph; stale (GkError GK_E_STATE from read / text / write) once the graph has been edited."""

    def __init__(self, graph: HipGraph, handle):
        self.graph, self.ctx, self.h = graph, graph.ctx, handle

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_contigs_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.h or not self.ctx.h or not self.graph.h:
            raise L.GkError(L.GK_E_STATE, "the contigs or their graph are closed")

    def stats(self) -> dict:
        """the nine numbers of the plan, named as CONTIG_STATS; they still answer when the plan is stale"""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the contigs are closed")
        st = np.zeros(len(CONTIG_STATS), np.uint64)
        L.check(L.lib().gk_contigs_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(CONTIG_STATS, (int(x) for x in st)))

    def read(self, offset: int, n: int) -> bytes:
        """bytes [offset, offset + n) of the text, fewer at its end; GkError GK_E_INVALID for an offset beyond it"""
        self._live()
        buf = np.empty(max(int(n), 1), np.uint8)
        got = C.c_uint64()
        L.check(L.lib().gk_contigs_read(self.h, int(offset), buf.ctypes.data, int(n), C.byref(got)), self.ctx.h)
        return buf[:got.value].tobytes()

    def text(self) -> bytes:
        return self.read(0, self.stats()["text_bytes"])

    def last_ms(self) -> dict:
        """wall ms of the last read / write: the emit kernels (device events), waits for copies, the sink, the whole call"""
        arr = (C.c_float * 4)()
        L.check(L.lib().gk_contigs_last_ms(self.h, arr), self.ctx.h)
        return dict(zip(("emit_kernels", "copies", "sink", "total"), (float(x) for x in arr)))

    def write(self, path):
        """the whole text to `path`; written aside, then renamed onto it"""
        self._live()
        L.check(L.lib().gk_contigs_write(self.h, os.fsencode(path)), self.ctx.h)


# the statistics of gk_graph_edge_twins, in the order of its `stats6` array: live_edges is the sum of the four after it
WEAK_STATS = ("candidates", "removed_ratio", "removed_floor_only", "removed")     # gk_graph_remove_weak_edges' stats4
TWIN_STATS = ("live_edges", "paired", "self", "missing", "ambiguous", "key_collisions")
# the names of gk_graph_edge_twins' class codes, by code (dead: a dead or out-of-range id)
TWIN_CLASSES = ("dead", "paired", "self", "missing", "ambiguous")
# the statistics of gk_gfa_stats, in the order of its `stats9` array: live_edges = segments + folded, pairs = links + mirrored
GFA_STATS = ("live_edges", "segments", "folded", "pairs", "links", "mirrored", "bases", "text_bytes", "missing_windows")


class Gfa:
    """A plan of the GFA 1.0 text of a graph (HipGraph.gfa): the text itself is emitted by the device when it is read or
    written.  Holds its graph; stale (GkError GK_E_STATE from read / text / write) once the graph has been edited."""

    def __init__(self, graph: HipGraph, handle):
        self.graph, self.ctx, self.h = graph, graph.ctx, handle

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_gfa_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.h or not self.ctx.h or not self.graph.h:
            raise L.GkError(L.GK_E_STATE, "the GFA plan or its graph are closed")

    def stats(self) -> dict:
        """the nine numbers of the plan, named as GFA_STATS; they still answer when the plan is stale"""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the GFA plan is closed")
        st = np.zeros(len(GFA_STATS), np.uint64)
        L.check(L.lib().gk_gfa_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(GFA_STATS, (int(x) for x in st)))

    def read(self, offset: int, n: int) -> bytes:
        """bytes [offset, offset + n) of the text, fewer at its end; GkError GK_E_INVALID for an offset beyond it"""
        self._live()
        buf = np.empty(max(int(n), 1), np.uint8)
        got = C.c_uint64()
        L.check(L.lib().gk_gfa_read(self.h, int(offset), buf.ctypes.data, int(n), C.byref(got)), self.ctx.h)
        return buf[:got.value].tobytes()

    def text(self) -> bytes:
        return self.read(0, self.stats()["text_bytes"])

    def last_ms(self) -> dict:
        """wall ms of the last read / write: the emit kernels (device events), waits for copies, the sink, the whole call"""
        arr = (C.c_float * 4)()
        L.check(L.lib().gk_gfa_last_ms(self.h, arr), self.ctx.h)
        return dict(zip(("emit_kernels", "copies", "sink", "total"), (float(x) for x in arr)))

    def write(self, path):
        """the whole text to `path`; written aside, then renamed onto it"""
        self._live()
        L.check(L.lib().gk_gfa_write(self.h, os.fsencode(path)), self.ctx.h)


# the statistics of gk_scaffolds_stats, in the order of its `stats13` array
SCAFFOLD_STATS = ("chains", "chain_forward", "chain_self_twin", "chain_reverse", "singletons", "records", "members", "adjacent", "gapped", "clamped",
                  "n_bases", "bases", "text_bytes")


# the statistics of gk_graph_fill_gaps, in the order of its `stats10` array: junctions is the sum of the six after it
FILL_STATS = ("junctions", "adjacent", "overflow", "none", "ambiguous", "shared", "filled", "filler_edges", "filler_bases", "searched_backward")
# the names of the GK_FILL_* class codes, by code
FILL_CLASSES = ("last", "adjacent", "overflow", "none", "ambiguous", "shared", "filled")
# the statistics of gk_graph_overlap_gaps, in the order of its `stats7` array: junctions is the sum of the five after it
OVERLAP_STATS = ("junctions", "adjacent", "out_of_range", "none", "ambiguous", "overlap", "overlap_bases")
# the names of the GK_OVL_* class codes, by code
OVERLAP_CLASSES = ("last", "adjacent", "out_of_range", "none", "ambiguous", "overlap")


class Scaffolds:
    """A plan of the FASTA text of a graph's scaffolds (HipGraph.scaffolds): the text itself is emitted by the device when it is
    read or written.  Holds its graph; stale (GkError GK_E_STATE from read / text / write) once the graph has been edited."""

    def __init__(self, graph: HipGraph, handle):
        self.graph, self.ctx, self.h = graph, graph.ctx, handle

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_scaffolds_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.h or not self.ctx.h or not self.graph.h:
            raise L.GkError(L.GK_E_STATE, "the scaffolds or their graph are closed")

    def stats(self) -> dict:
        """the thirteen numbers of the plan, named as SCAFFOLD_STATS; they still answer when the plan is stale"""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the scaffolds are closed")
        st = np.zeros(len(SCAFFOLD_STATS), np.uint64)
        L.check(L.lib().gk_scaffolds_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(SCAFFOLD_STATS, (int(x) for x in st)))

    def overlapStats(self) -> dict:
        """{overlapped: junctions of the chain records written that scaffolds(overlaps=) joined on an overlap, dropped: the bases
        they left out}; adjacent + gapped + overlapped = members - chain records"""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the scaffolds are closed")
        st = np.zeros(2, np.uint64)
        L.check(L.lib().gk_scaffolds_overlap_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return {"overlapped": int(st[0]), "dropped": int(st[1])}

    def read(self, offset: int, n: int) -> bytes:
        """bytes [offset, offset + n) of the text, fewer at its end; GkError GK_E_INVALID for an offset beyond it"""
        self._live()
        buf = np.empty(max(int(n), 1), np.uint8)
        got = C.c_uint64()
        L.check(L.lib().gk_scaffolds_read(self.h, int(offset), buf.ctypes.data, int(n), C.byref(got)), self.ctx.h)
        return buf[:got.value].tobytes()

    def text(self) -> bytes:
        return self.read(0, self.stats()["text_bytes"])

    def last_ms(self) -> dict:
        """wall ms of the last read / write: the emit kernels (device events), waits for copies, the sink, the whole call"""
        arr = (C.c_float * 4)()
        L.check(L.lib().gk_scaffolds_last_ms(self.h, arr), self.ctx.h)
        return dict(zip(("emit_kernels", "copies", "sink", "total"), (float(x) for x in arr)))

    def write(self, path):
        """the whole text to `path`; written aside, then renamed onto it"""
        self._live()
        L.check(L.lib().gk_scaffolds_write(self.h, os.fsencode(path)), self.ctx.h)

    def segments(self) -> list:
        """which piece of which edge lies where: [(record index in the text, edge id, first base in the record's sequence, bases
        written, bases of the edge's path skipped before them: 0, k, or an overlap)] in text order; N runs are the bases between rows"""
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the scaffolds are closed")
        st = self.stats()
        n = st["members"] + st["singletons"]
        rec, first, bases = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        edge, skip = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        got = C.c_uint64()
        L.check(L.lib().gk_scaffolds_segments(self.h, L.ptr(rec, C.c_uint64), L.ptr(edge, C.c_uint32), L.ptr(first, C.c_uint64), L.ptr(bases, C.c_uint64),
                                              L.ptr(skip, C.c_uint32), n, C.byref(got)), self.ctx.h)
        assert got.value == n
        return list(zip(rec.tolist(), edge.tolist(), first.tolist(), bases.tolist(), skip.tolist()))

    def judge(self, placements: "Placements", tol: int) -> dict:
        """Every junction of the plan (two consecutive rows of segments() in one record) held against the placements of its two
        edges -> {"classes": the class name of every junction in row order (JUDGE_CLASSES), "err": scaffold distance minus
        reference distance where the class is order, distance or correct, else 0, "stats": the numbers named as JUDGE_STATS}.
        A gapped junction is correct within `tol` bases, an adjacent or overlapped one only at err = 0.  `tol` is a choice, not a
        measurement (half the width of the insert range, the fill / overlap tolerance, is the customary value)."""
        self._live()
        st = self.stats()
        cap = st["members"] + st["singletons"] - st["records"]
        cls, err = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.int64)
        n, js = C.c_uint64(), np.zeros(len(JUDGE_STATS), np.uint64)
        L.check(L.lib().gk_scaffolds_judge(self.h, placements.h, int(tol), L.ptr(cls, C.c_uint8), L.ptr(err, C.c_int64), cap, C.byref(n), L.ptr(js, C.c_uint64)),
                self.ctx.h)
        assert n.value == cap
        return {"classes": [JUDGE_CLASSES[x] for x in cls[:cap]], "err": err[:cap].tolist(), "stats": dict(zip(JUDGE_STATS, (int(x) for x in js)))}


# the statistics of gk_placements_stats, in the order of its array: each strand's four lookup classes add up to windows, the five edge
# classes to the live edges
PLACE_STATS = ("records", "bases", "valid_bases", "windows", "fwd_absent", "fwd_repetitive", "fwd_at_node", "fwd_edge", "rev_absent", "rev_repetitive",
               "rev_at_node", "rev_edge", "unplaced", "both_strands", "scattered", "forward", "reverse", "forward_bases", "reverse_bases", "saturated")
# the names of the GK_PLACE_* edge classes, by code
PLACE_CLASSES = ("unplaced", "both_strands", "scattered", "forward", "reverse")
# the names of the GK_JUDGE_* junction classes, by code, and of the junction kinds
JUDGE_CLASSES = ("unjudged", "other_record", "strand", "order", "distance", "correct")
JUDGE_KINDS = ("adjacent", "gapped", "overlapped")
# the statistics of gk_scaffolds_judge, in the order of its array: junctions is the sum of the six classes, each class the sum of its three kinds
JUDGE_STATS = (("junctions",) + JUDGE_CLASSES + tuple(f"{kd}_{c}" for kd in JUDGE_KINDS for c in JUDGE_CLASSES)
               + ("gapped_correct_abs_err_sum", "gapped_correct_abs_err_max", "records_judged", "records_clean"))


class Placements:
    """Where every edge of a graph lies on a reference genome (include/genome_amd.h, "placements"): per edge and strand the
    windows of the reference that hit it, and the diagonal if there is exactly one.  Holds its graph and position map; stale
    (GkError GK_E_STATE) once the graph has been edited."""

    def __init__(self, graph: HipGraph, positions):
        self.graph, self.ctx, self.positions = graph, graph.ctx, positions
        h = L.vp()
        L.check(L.lib().gk_placements_create(graph.h, positions.h, C.byref(h)), self.ctx.h)
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_placements_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.h or not self.ctx.h or not self.graph.h:
            raise L.GkError(L.GK_E_STATE, "the placements or their graph are closed")

    def add(self, record):
        """the next reference record: its joined sequence characters (str or bytes)"""
        self._live()
        b = record.encode("latin-1") if isinstance(record, str) else bytes(record)
        L.check(L.lib().gk_placements_add_record(self.h, b, len(b)), self.ctx.h)

    def stats(self) -> dict:
        self._live()
        st = np.zeros(len(PLACE_STATS), np.uint64)
        L.check(L.lib().gk_placements_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(PLACE_STATS, (int(x) for x in st)))

    def edges(self, edge_ids=None) -> dict:
        """per id asked for (default: every id below the bound): {"cls": class names (PLACE_CLASSES), "record", "pos": where base 0
        of the edge's path lies (forward and reverse edges; 0 otherwise), "windows_fwd", "windows_rev": the hit counts}"""
        self._live()
        ids = np.arange(self.graph.idBounds()[1], dtype=np.uint32) if edge_ids is None else np.ascontiguousarray(edge_ids, np.uint32)
        n = len(ids)
        cls, rec, pos = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.int64)
        wf, wr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        L.check(L.lib().gk_placements_edges(self.h, L.ptr(ids, C.c_uint32), n, L.ptr(cls, C.c_uint8), L.ptr(rec, C.c_uint32), L.ptr(pos, C.c_int64),
                                            L.ptr(wf, C.c_uint32), L.ptr(wr, C.c_uint32)), self.ctx.h)
        return {"cls": [PLACE_CLASSES[x] for x in cls], "record": rec.tolist(), "pos": pos.tolist(), "windows_fwd": wf.tolist(), "windows_rev": wr.tolist()}

    def last_ms(self) -> dict:
        """wall ms of the last record added: host staging + upload, the lookup kernels (device events), the whole call"""
        arr = (C.c_float * 4)()
        L.check(L.lib().gk_placements_last_ms(self.h, arr), self.ctx.h)
        return {"upload": float(arr[0]), "lookup_kernels": float(arr[2]), "total": float(arr[3])}


# the names of the GK_BREAK_* breakpoint classes and of the GK_BLOCKS_* edge classes, by code; gk_blocks_stats in the order of its array
BLOCK_BREAKS = ("first", "overlap", "translocation", "inversion", "relocation", "indel", "colinear")
BLOCK_CLASSES = ("unaligned", "repeat", "misassembled", "indel", "colinear", "exact")
BLOCK_STATS = (("records", "bases", "valid_bases", "windows", "covered", "rows") + tuple("brk_" + b for b in BLOCK_BREAKS[1:])
               + tuple("edges_" + c for c in BLOCK_CLASSES)
               + ("full_edges", "aligned_kmers", "pieces", "piece_bases", "indel_shift_sum", "indel_shift_max"))


def _nx50(lengths, total: int) -> int:
    run = 0
    for x in sorted((int(v) for v in lengths), reverse=True):
        run += x
        if 2 * run >= total:
            return x
    return 0


class Blocks:
    """Every edge of a graph aligned to a reference genome as exact runs, and the breakpoints between them (include/genome_amd.h,
    "alignment blocks" and "breakpoints").  Feed the records, finish(tol) once or several times, then read.  Holds its graph and
    position map; stale (GkError GK_E_STATE) once the graph has been edited."""

    def __init__(self, graph: HipGraph, positions):
        self.graph, self.ctx, self.positions = graph, graph.ctx, positions
        h = L.vp()
        L.check(L.lib().gk_blocks_create(graph.h, positions.h, C.byref(h)), self.ctx.h)
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_blocks_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self.h or not self.ctx.h or not self.graph.h:
            raise L.GkError(L.GK_E_STATE, "the blocks or their graph are closed")

    def add_record(self, record):
        """the next reference record: its joined sequence characters (str or bytes)"""
        self._live()
        b = record.encode("latin-1") if isinstance(record, str) else bytes(record)
        L.check(L.lib().gk_blocks_add_record(self.h, b, len(b)), self.ctx.h)

    def finish(self, tol: int):
        """order the rows, class every breakpoint and edge, cut the pieces; again with another tol without feeding again"""
        self._live()
        L.check(L.lib().gk_blocks_finish(self.h, int(tol)), self.ctx.h)
        return self

    def stats(self) -> dict:
        self._live()
        st = np.zeros(len(BLOCK_STATS), np.uint64)
        L.check(L.lib().gk_blocks_stats(self.h, L.ptr(st, C.c_uint64)), self.ctx.h)
        return dict(zip(BLOCK_STATS, (int(x) for x in st)))

    def rows(self) -> list:
        """[(edge, strand, record, pos, dlo, dhi, brk, shift)] in the rule's order; brk is the class code (BLOCK_BREAKS)"""
        self._live()
        n = C.c_uint64()
        rc = L.lib().gk_blocks_rows(self.h, None, None, None, None, None, None, None, None, 0, C.byref(n))
        if rc != L.GK_E_CAPACITY:
            L.check(rc, self.ctx.h)
        m = n.value
        a = [np.zeros(max(m, 1), t) for t in (np.uint32, np.uint8, np.uint32, np.int64, np.uint32, np.uint32, np.uint8, np.int64)]
        ct = (C.c_uint32, C.c_uint8, C.c_uint32, C.c_int64, C.c_uint32, C.c_uint32, C.c_uint8, C.c_int64)
        L.check(L.lib().gk_blocks_rows(self.h, *[L.ptr(x, t) for x, t in zip(a, ct)], m, C.byref(n)), self.ctx.h)
        return list(zip(*[x[:m].tolist() for x in a]))

    def edges(self, edge_ids=None) -> dict:
        """per id asked for (default: every id below the bound): {"cls": class names (BLOCK_CLASSES), "full", "first_row", "nrows"}"""
        self._live()
        ids = np.arange(self.graph.idBounds()[1], dtype=np.uint32) if edge_ids is None else np.ascontiguousarray(edge_ids, np.uint32)
        n = len(ids)
        cls, full, first, nrows = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        L.check(L.lib().gk_blocks_edges(self.h, L.ptr(ids, C.c_uint32), n, L.ptr(cls, C.c_uint8), L.ptr(full, C.c_uint8), L.ptr(first, C.c_uint32),
                                        L.ptr(nrows, C.c_uint32)), self.ctx.h)
        return {"cls": [BLOCK_CLASSES[x] for x in cls], "full": full.tolist(), "first_row": first.tolist(), "nrows": nrows.tolist()}

    def pieces(self) -> list:
        """[(bases, edge)] in row order"""
        self._live()
        n = C.c_uint64()
        rc = L.lib().gk_blocks_pieces(self.h, None, None, 0, C.byref(n))
        if rc != L.GK_E_CAPACITY:
            L.check(rc, self.ctx.h)
        m = n.value
        ln, ed = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint32)
        L.check(L.lib().gk_blocks_pieces(self.h, L.ptr(ln, C.c_uint64), L.ptr(ed, C.c_uint32), m, C.byref(n)), self.ctx.h)
        return list(zip(ln[:m].tolist(), ed[:m].tolist()))

    def na50(self) -> dict:
        """{"na50": against the piece bases, "nga50": against the valid bases of the reference (0 if the pieces never reach half)}"""
        st = self.stats()
        lens = [p[0] for p in self.pieces()]
        return {"na50": _nx50(lens, st["piece_bases"]), "nga50": _nx50(lens, st["valid_bases"])}

    def last_ms(self) -> dict:
        """wall ms of the last record added (host staging + upload, count launches, emit launches, the whole call) and of the last
        finish (device time, the whole call)"""
        arr = (C.c_float * 6)()
        L.check(L.lib().gk_blocks_last_ms(self.h, arr), self.ctx.h)
        return dict(zip(("upload", "count_kernels", "emit_kernels", "total", "finish_kernels", "finish_total"), (float(x) for x in arr)))


def scaffoldGaps(chains, joins, mid: int):
    """The gap lists HipGraph.scaffolds takes, from a HipLinks.joins result (e1, e2, count, sum_u): mid - floor(sum_u / count) of
    the join between consecutive members, one entry fewer than a chain has members.  `mid`: the fragment length the library is
    taken to have (the tools pass the median of the insert range).  KeyError if two consecutive members are no join."""
    e1, e2, cnt, su = (np.asarray(a).tolist() for a in joins)
    gap = {(a, b): int(mid) - s // c for a, b, c, s in zip(e1, e2, cnt, su)}
    return [[gap[(a, b)] for a, b in zip(c, c[1:])] for c in chains]


def _junction_lists(chains, lists) -> bool:
    """Is `lists` one list per chain with an entry per junction (one for the last member may be there and is ignored)?"""
    return len(lists) == len(chains) and all(len(c) - 1 <= len(x) <= len(c) for c, x in zip(chains, lists))


def _flat_chains(chains):
    """Chains as the C API takes them -> (members, chain_off)."""
    off = np.zeros(len(chains) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chains])
    return np.array([e for c in chains for e in c], np.uint32), off


def _flat_junctions(chains, lists, dtype):
    """Per-junction lists -> their entries parallel to the members, with 0 behind a chain's last member."""
    return np.array([x for c, g in zip(chains, lists) for x in list(g)[:len(c) - 1] + [0]], dtype)


def _per_junction(flat, off):
    """An array parallel to the members of the chains at `off` -> per chain the list of its junctions' entries."""
    i = off.tolist()
    return [flat[a:b - 1].tolist() for a, b in zip(i, i[1:])]


# the classes of gk_graph_pair_distances, in the order of its `classes` array
PAIR_CLASSES = ("orientations", "unplaced", "repetitive", "apart", "ambiguous", "reversed", "beyond", "near_end", "counted")
# the statistics of gk_graph_thread_reads, in the order of its `stats7` array: inner_windows is the sum of the five after it
THREAD_STATS = ("records", "inner_windows", "off_graph", "repeated", "on_edge", "broken", "crossings")
# the statistics of gk_graph_thread_spans, in the order of its `stats5` array: crossings is the sum of the three after it
SPAN_STATS = ("records", "crossings", "spans", "interrupted", "open")
# the statistics of gk_graph_split_edges_by_spans, in the order of its `stats7` array: candidates is the sum of the four after it
SPLIT_EDGE_STATS = ("candidates", "resolved", "unequal", "ambiguous", "unsupported", "new_edges", "new_nodes")
# the classes of gk_graph_pair_links, in the order of its `classes8` array: orientations is the sum of the seven after it
LINK_CLASSES = ("orientations", "unplaced", "repetitive", "at_node", "same_edge", "short_edge", "too_far", "linked")
# the statistics of gk_links_joins, in the order of its `stats5` array
JOIN_STATS = ("links", "supported", "joins", "forks", "merges")
# what the tools fall back to without an estimate: the reference's `180 to 250` (GraphSimplifier.scala:146)
REFERENCE_RANGE = (180, 250)


def insertRange(hist, trim: int = 25, min_observations: int = 1000):
    """gk_insert_range over a pairDistances histogram -> (lo, hi, median) in bases, or None when the histogram holds fewer than
    max(min_observations, 1) observations ("no estimate": callers fall back to REFERENCE_RANGE and say so).  lo / hi cut `trim`
    thousandths off either tail (0: the smallest and largest length seen; at most 499).  Both defaults are choices, not
    measurements.  Host code: no context, no GPU."""
    h = np.ascontiguousarray(hist, np.uint64)
    lo, hi, med = C.c_uint32(), C.c_uint32(), C.c_uint32()
    L.check(L.lib().gk_insert_range(L.ptr(h, C.c_uint64), len(h), int(trim), int(min_observations), C.byref(lo), C.byref(hi), C.byref(med)))
    if sum(int(x) for x in h) < max(int(min_observations), 1):
        return None
    return lo.value, hi.value, med.value


CYCLE_BUILD_STATS = ("cycle_kmers", "cycles", "anchors", "self_complementary", "longest", "rounds")

CYCLE_SIMPLIFY_STATS = ("kept_self_loops", "cycles_merged", "anchors_kept", "nodes_removed")


def buildGraph(k: int, kmersFreq, keep_cycles: bool = False) -> HipGraph:
    """Graph.buildGraph(k, kmersFreq) (Graph.scala:269-382).  A PartitionedDNAMap is gathered into
    one table first (the walk crosses partitions arbitrarily).
    keep_cycles: perfect cycles, which the reference ignores (:375), become self-loops at their anchors (gk_graph_build_cycles);
    the CYCLE_BUILD_STATS are then HipGraph.cycleStats()."""
    own = None
    if isinstance(kmersFreq, PartitionedDNAMap):
        own = kmersFreq = kmersFreq.merged()
    assert isinstance(kmersFreq, HipDNAMap) and kmersFreq.k == k
    h = L.vp()
    st = (C.c_uint64 * 6)()
    try:
        if keep_cycles:
            L.check(L.lib().gk_graph_build_cycles(kmersFreq.h, C.byref(h), st), kmersFreq.ctx.h)
        else:
            L.check(L.lib().gk_graph_build(kmersFreq.h, C.byref(h)), kmersFreq.ctx.h)
    finally:
        if own is not None:
            own.close()
    g = HipGraph(kmersFreq.ctx, k, h)
    if keep_cycles:
        g._cycle_stats = dict(zip(CYCLE_BUILD_STATS, (int(x) for x in st)))
    return g


def loadGraph(ctx, path) -> HipGraph:
    """Graph(file) (Graph.scala:384-390) with GraphSimplifier's checks of the loaded graph (GraphSimplifier.scala:157-169): the
    saved ids, out-edge orders and checksums; k comes from the file (:153).  GkError GK_E_FORMAT for a malformed or corrupt file."""
    if not ctx.h:
        raise ValueError("context is closed")
    h = L.vp()
    L.check(L.lib().gk_graph_load(ctx.h, os.fsencode(path), C.byref(h)), ctx.h)
    k = L.lib().gk_graph_k(h)
    if k < 0:
        L.lib().gk_graph_destroy(h)
        L.check(k, ctx.h)
    return HipGraph(ctx, k, h)


def graphIoStats(ctx) -> dict:
    """wall ms of the last save / load on `ctx`: file I/O, waits for host<->device copies, device kernels, the whole call"""
    arr = (C.c_float * 4)()
    L.check(L.lib().gk_graph_io_stats(ctx.h, arr), ctx.h)
    return dict(zip(("file_io", "copies", "kernels", "total"), (float(x) for x in arr)))


class Support:
    """pathsMap + badPairs of GraphSimplifier.scala:209-211: (edge id, edge id) -> read pairs whose walk passes through both."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = L.vp()
        L.check(L.lib().gk_support_create(ctx.h, C.byref(h)), ctx.h)
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_support_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def sizes(self):
        """-> (edge pairs, bad pairs, pair orientations walked)"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_support_size(self.h, C.byref(a), C.byref(b), C.byref(c)), self.ctx.h)
        return a.value, b.value, c.value

    def last_ms(self):
        """wall ms of the last walkPairs into this support: keys, getAll batch, snapshot + checks, walks, merge"""
        arr = (C.c_float * 5)()
        L.check(L.lib().gk_support_last_ms(self.h, arr), self.ctx.h)
        return dict(zip(("keys", "lookup", "snapshot", "walks", "merge"), (float(x) for x in arr)))

    def last_walk(self):
        """-> (pair orientations the last walkPairs into this support handed to the walk stage, those of them that outgrew the
        device's sets and were walked on the host).  A test hook: GkError on the product library."""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.test_hook("gk_test_support_last_walk")(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def items(self):
        n = self.sizes()[0]
        e1, e2, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        got = C.c_uint64()
        L.check(L.lib().gk_support_export(self.h, L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), L.ptr(cnt, C.c_uint32), n, C.byref(got)), self.ctx.h)
        return e1, e2, cnt

    def add(self, e1, e2, cnt, bad: int = 0, walked: int = 0):
        """add (e1, e2, count) triples (duplicates add up) and the two counters; GK_E_CAPACITY, and nothing added, if a count
        would pass 2^32-1.  items() of one support added into an empty one reproduces it."""
        e1, e2, cnt = (np.ascontiguousarray(a, np.uint32) for a in (e1, e2, cnt))
        assert len(e1) == len(e2) == len(cnt)
        L.check(L.lib().gk_support_add(self.h, L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), L.ptr(cnt, C.c_uint32), len(e1), bad, walked), self.ctx.h)

    def merge(self, other: "Support"):
        """self += other on the device (same device); other is unchanged.  Same overflow rule as add()."""
        L.check(L.lib().gk_support_merge(self.h, other.h), self.ctx.h)



class HipLinks:
    """Scaffold links (include/genome_amd.h, "scaffold links"): (edge id, edge id) -> the pair orientations whose mates lie on the
    two edges, and the sum of the bases those fragments need on them.  Edge ids are the graph's at the time of pairLinks: the
    table is meaningless after a graph edit."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = L.vp()
        L.check(L.lib().gk_links_create(ctx.h, C.byref(h)), ctx.h)
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_links_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """-> (distinct links, the sum of their counts)"""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_links_size(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def export(self):
        """-> (e1, e2, count, sum_u) arrays, unordered"""
        n = self.size()[0]
        e1, e2, cnt, su = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        got = C.c_uint64()
        L.check(L.lib().gk_links_export(self.h, L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), L.ptr(cnt, C.c_uint32), L.ptr(su, C.c_uint64), n,
                                        C.byref(got)), self.ctx.h)
        return e1, e2, cnt, su

    def add(self, e1, e2, cnt, sum_u):
        """add (e1, e2, count, sum_u) records (duplicates add up); GK_E_CAPACITY, and nothing added, if a count would pass
        2^32-1.  export() of one table added into an empty one reproduces it."""
        e1, e2, cnt = (np.ascontiguousarray(a, np.uint32) for a in (e1, e2, cnt))
        su = np.ascontiguousarray(sum_u, np.uint64)
        assert len(e1) == len(e2) == len(cnt) == len(su)
        L.check(L.lib().gk_links_add(self.h, L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), L.ptr(cnt, C.c_uint32), L.ptr(su, C.c_uint64), len(e1)), self.ctx.h)

    def joins(self, min_support: int = 3, cap=None):
        """The links that are the only one of at least `min_support` observations out of their first edge and into their second
        -> ((e1, e2, count, sum_u) arrays in ascending e1, {stat: count} over JOIN_STATS).  `cap`: room for that many joins
        (default: as many as there are; less is GkError GK_E_CAPACITY)."""
        lib = L.lib()
        n, st = C.c_uint64(), np.zeros(len(JOIN_STATS), np.uint64)
        if cap is None:
            rc = lib.gk_links_joins(self.h, int(min_support), None, None, None, None, 0, C.byref(n), None)
            if rc not in (L.GK_OK, L.GK_E_CAPACITY):
                L.check(rc, self.ctx.h)
            cap = n.value
        e1, e2, cnt, su = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        L.check(lib.gk_links_joins(self.h, int(min_support), L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), L.ptr(cnt, C.c_uint32), L.ptr(su, C.c_uint64),
                                   cap, C.byref(n), L.ptr(st, C.c_uint64)), self.ctx.h)
        m = n.value
        return (e1[:m], e2[:m], cnt[:m], su[:m]), dict(zip(JOIN_STATS, (int(x) for x in st)))


class HipSpans:
    """Spans (include/genome_amd.h, gk_graph_thread_spans): (edge id, edge id, edge id) -> the reads that came by the first edge,
    crossed the second from end to end and left by the third.  Edge ids are the graph's at the time of threadSpans."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = L.vp()
        L.check(L.lib().gk_spans_create(ctx.h, C.byref(h)), ctx.h)
        self.h = h

    def close(self):
        if self.h:
            if self.ctx.h:               # (see HipDNAMap.close)
                L.lib().gk_spans_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """-> (distinct triples, the sum of their counts)"""
        a, b = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_spans_size(self.h, C.byref(a), C.byref(b)), self.ctx.h)
        return a.value, b.value

    def export(self):
        """-> (e, m, f, count) arrays, unordered"""
        got = C.c_uint64()
        L.check(L.lib().gk_spans_size(self.h, C.byref(got), None), self.ctx.h)     # the triples alone: a counter, no table pass
        n = got.value
        e, m, f, cnt = (np.zeros(n, np.uint32) for _ in range(4))
        L.check(L.lib().gk_spans_export(self.h, L.ptr(e, C.c_uint32), L.ptr(m, C.c_uint32), L.ptr(f, C.c_uint32), L.ptr(cnt, C.c_uint32), n, C.byref(got)),
                self.ctx.h)
        return e, m, f, cnt

    def add(self, e, m, f, cnt):
        """add (e, m, f, count) records (duplicates add up); GK_E_CAPACITY, and nothing added, if a count would pass 2^32-1.
        export() of one table added into an empty one reproduces it."""
        e, m, f, cnt = (np.ascontiguousarray(a, np.uint32) for a in (e, m, f, cnt))
        assert len(e) == len(m) == len(f) == len(cnt)
        L.check(L.lib().gk_spans_add(self.h, L.ptr(e, C.c_uint32), L.ptr(m, C.c_uint32), L.ptr(f, C.c_uint32), L.ptr(cnt, C.c_uint32), len(e)), self.ctx.h)


def scaffoldChains(e1, e2, with_cycles: bool = False):
    """gk_scaffold_chains over a join list (HipLinks.joins) -> the chains as lists of edge ids, in ascending order of first member;
    a cycle starts at its smallest id.  with_cycles: -> (chains, number of cycles among them).  GkError GK_E_INVALID if an id
    occurs twice as e1 or twice as e2.  Host code: no context, no GPU."""
    e1, e2 = np.ascontiguousarray(e1, np.uint32), np.ascontiguousarray(e2, np.uint32)
    assert e1.shape == e2.shape and e1.ndim == 1
    n = len(e1)
    members, off = np.zeros(2 * n + 1, np.uint32), np.zeros(n + 1, np.uint64)
    nch, ncy = C.c_uint64(), C.c_uint64()
    L.check(L.lib().gk_scaffold_chains(L.ptr(e1, C.c_uint32), L.ptr(e2, C.c_uint32), n, L.ptr(members, C.c_uint32), 2 * n, L.ptr(off, C.c_uint64), n,
                                       C.byref(nch), C.byref(ncy)))
    chains = [members[int(off[i]):int(off[i + 1])].tolist() for i in range(nch.value)]
    return (chains, ncy.value) if with_cycles else chains
