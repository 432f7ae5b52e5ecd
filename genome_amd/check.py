"""CheckGraph (S/scripts/CheckGraph.scala) on the GPU: the contig statistics of a graph and every k-window of a reference FASTA
looked up in its position map.

The rules of the FASTA check and its deviations from the reference are stated in include/genome_amd.h ("FASTA check").
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import _lib as L
from .fastq import _text, iter_pieces

COUNTERS = ("lines", "records", "bases", "valid_bases", "windows", "found", "missing", "covered_bases", "short_lines")


class FastaCheck:
    """A FASTA check in progress (gk_fasta_check): feed the text in pieces of any size, the last one with last=True.

    vmap: the position map to look the windows up in (Graph.getGraphMap); k is the map's.  per_line: windows never cross a line
    end (the reference's literal rule); otherwise the sequence lines of a record are joined.  max_missing: how many not-found
    windows to keep, the first ones in stream order."""

    def __init__(self, ctx, vmap, per_line: bool = False, max_missing: int = 0):
        if not ctx.h:
            raise ValueError("context is closed")
        self.ctx, self.vmap, self.k = ctx, vmap, vmap.k
        self.h = L.vp()
        L.check(L.lib().gk_fasta_check_create(ctx.h, vmap.h, 1 if per_line else 0, int(max_missing), C.byref(self.h)), ctx.h)

    def close(self):
        if self.h:
            if self.ctx.h:               # (a handle that outlived its context is dropped, not followed)
                L.lib().gk_fasta_check_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if not self.h or not self.ctx.h:
            raise L.GkError(L.GK_E_STATE, "the FASTA check is closed")
        return self.h

    def feed(self, text, last: bool = False):
        buf = _text(text)
        L.check(L.lib().gk_fasta_check_feed(self._handle(), buf.ctypes.data if buf.size else None, buf.size, 1 if last else 0), self.ctx.h)

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in COUNTERS]
        L.check(L.lib().gk_fasta_check_stats(self._handle(), *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(COUNTERS, (x.value for x in v)))

    def missing(self) -> list:
        """[(byte offset of the window's first base, its 0-based line, its 0-based column, lo, hi)], in stream order"""
        n = C.c_uint64()
        L.check(L.lib().gk_fasta_check_missing(self._handle(), None, None, None, None, None, 0, C.byref(n)), self.ctx.h)
        a = [np.zeros(max(n.value, 1), np.uint64) for _ in range(5)]
        L.check(L.lib().gk_fasta_check_missing(self._handle(), *[L.ptr(x, C.c_uint64) for x in a], n.value, C.byref(n)), self.ctx.h)
        return [tuple(int(x[i]) for x in a) for i in range(n.value)]

    def last_ms(self) -> dict:
        out = (C.c_float * 4)()
        L.check(L.lib().gk_fasta_check_last_ms(self._handle(), out), self.ctx.h)
        return dict(zip(("upload", "parse", "lookup", "total"), (float(x) for x in out)))


def fasta_records(text) -> list:
    """The records of a FASTA text as joined sequence bytes, by the record rule of the FASTA check with per_line == 0
    (include/genome_amd.h): a line ends at "\\n", "\\r" or "\\r\\n"; a line that starts with '>' is a header and starts a record;
    sequence characters before the first header are record 0; terminators are dropped, every other character is kept as it is."""
    text = bytes(text)
    records, cur, seen_header = [], [], False
    for line in text.replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n"):
        if line[:1] == b">":
            if seen_header or cur:
                records.append(b"".join(cur))
            cur, seen_header = [], True
        elif line:
            cur.append(line)
    if seen_header or cur:
        records.append(b"".join(cur))
    return records


def n50(lengths) -> int:
    """lengths descending, the first at which twice the running sum reaches the total (gk_graph_contig_stats' n50); 0 for none"""
    c = sorted((int(x) for x in lengths), reverse=True)
    total, run = sum(c), 0
    for x in c:
        run += x
        if 2 * run >= total:
            return x
    return 0


MISJOINS = ("other_record", "strand", "order", "distance")


def scaffold_n50s(segments, classes) -> dict:
    """From Scaffolds.segments() and the junction classes of Scaffolds.judge(): the N50 of the records as written, and the N50 after
    every record is broken at each misjoin (the N run of a broken junction belongs to neither piece)."""
    whole, broken, j = [], [], 0
    for i, (rec, _e, first, bases, _s) in enumerate(segments):
        if i == 0 or segments[i - 1][0] != rec:
            start = piece = first
        elif classes[j - 1] in MISJOINS:
            broken.append(segments[i - 1][2] + segments[i - 1][3] - piece)
            piece = first
        if i + 1 == len(segments) or segments[i + 1][0] != rec:
            whole.append(first + bases - start)
            broken.append(first + bases - piece)
        else:
            j += 1
    return {"n50": n50(whole), "n50_broken": n50(broken), "records": len(whole), "pieces": len(broken)}


def judge_scaffolds(graph, fasta, scaffolds, tol: int) -> dict:
    """The judge for a graph, a reference FASTA (a path, `.gz` read with the standard library, or its bytes) and a Scaffolds plan of
    that graph: the edges are placed on the reference with a position map of the graph as it is, every junction of the plan is
    judged -> {"k", "tol", "placements": the placement stats, "classes", "err", "stats": Scaffolds.judge's, "n50", "n50_broken"}.
    `tol` is a choice, not a measurement."""
    if isinstance(fasta, (str, os.PathLike)):
        text = b"".join(bytes(piece) for piece, _ in iter_pieces(fasta, 256 << 20))
    else:
        text = bytes(fasta)
    vm = graph.getGraphMap()
    try:
        with graph.place(vm, fasta_records(text)) as pl:
            out = {"k": graph.k, "tol": int(tol), "placements": pl.stats()}
            out.update(scaffolds.judge(pl, tol))
    finally:
        vm.close()
    ns = scaffold_n50s(scaffolds.segments(), out["classes"])
    out["n50"], out["n50_broken"] = ns["n50"], ns["n50_broken"]
    return out


def align_contigs(graph, fasta, tol: int = 1000) -> dict:
    """The alignment blocks of a graph against a reference FASTA (a path, `.gz` read with the standard library, or its bytes), with a
    position map of the graph as it is -> {"k", "tol", "stats", "rows", "edges", "pieces", "genome_fraction", "na50", "nga50"}.
    `tol` is a choice, not a measurement."""
    if isinstance(fasta, (str, os.PathLike)):
        text = b"".join(bytes(piece) for piece, _ in iter_pieces(fasta, 256 << 20))
    else:
        text = bytes(fasta)
    vm = graph.getGraphMap()
    try:
        with graph.alignBlocks(vm, fasta_records(text), tol) as b:
            st = b.stats()
            out = {"k": graph.k, "tol": int(tol), "stats": st, "rows": b.rows(), "edges": b.edges(), "pieces": b.pieces()}
            out["genome_fraction"] = st["covered"] / st["windows"] if st["windows"] else 0.0
            out.update(b.na50())
    finally:
        vm.close()
    return out


def check_graph(graph, fasta, longer_than: int = 200, per_line: bool = False, max_missing: int = 0, piece_bytes: int = 256 << 20) -> dict:
    """CheckGraph.startup for a graph and a FASTA file (a path, `.gz` read with the standard library) or its bytes: one dict with
    k, the contig statistics (:37-41), the check's counters (:48-55), the coverage and, with max_missing, the missing list."""
    out = {"k": graph.k, "longer_than": int(longer_than), "per_line": bool(per_line)}
    out["contigs"] = graph.contigStats(longer_than)
    vm = graph.getGraphMap()
    try:
        with FastaCheck(graph.ctx, vm, per_line, max_missing) as fc:
            if isinstance(fasta, (str, os.PathLike)):
                for piece, last in iter_pieces(fasta, piece_bytes):
                    fc.feed(piece, last=last)
            else:
                fc.feed(fasta, last=True)
            st = fc.stats()
            out.update(st)
            out["coverage"] = st["covered_bases"] / st["valid_bases"] if st["valid_bases"] else 0.0
            out["missing_list"] = [{"offset": o, "line": ln, "column": c, "lo": lo, "hi": hi} for o, ln, c, lo, hi in fc.missing()]
    finally:
        vm.close()
    return out
