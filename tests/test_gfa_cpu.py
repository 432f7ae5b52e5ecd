"""The restatement of the twin and GFA rules (tests/gfa_ref.py) held to hand-written cases, and an independent checker of any
GFA text this project writes, run over the oracle's graphs.  No device: tests/test_gfa_gpu.py holds the kernels to the same
restatement and reuses check_gfa.
"""
import random

import pytest

from genome_amd import dna
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import oracle_canonical

import folded_cases as FC
import gfa_ref as GR


# ---- an independent checker ---------------------------------------------------------------------------------------------------

def parse(text):
    """-> (segments: name -> (sequence, tags dict), links: [(a, oa, b, ob, overlap)]) of a GFA 1.0 text; the header comes first, then
    the S lines, then the L lines"""
    lines = text.decode().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == "" and "" not in lines[:-1]
    segs, links = {}, []
    kinds = "".join(x[0] for x in lines[1:-1])
    assert kinds == "S" * kinds.count("S") + "L" * kinds.count("L")
    for line in lines[1:-1]:
        f = line.split("\t")
        if f[0] == "S":
            assert f[1] not in segs, "segment names are unique"
            assert set(f[2]) <= set("ACGT") and f[2]
            tags = {t[:2]: int(t[5:]) for t in f[3:]}
            assert all(t[2:5] == ":i:" for t in f[3:]) and set(tags) <= {"LN", "KC"} and tags["LN"] == len(f[2])
            segs[f[1]] = (f[2], tags)
        else:
            assert len(f) == 6 and f[2] in "+-" and f[4] in "+-" and f[5].endswith("M")
            links.append((f[1], f[2], f[3], f[4], int(f[5][:-1])))
    return segs, links


def oriented(segs, name, o):
    return segs[name][0] if o == "+" else R.rev_comp(segs[name][0])


def check_gfa(text, k, edges=None, twin_stats=None, want_kc=None):
    """every L line's two segments, in the stated orientations, share exactly the stated k bases; LN is the length; names are unique.
    edges (the graph's (start, end, seq), strand-closed and without copies — twin_stats says so): segments == (live + self) / 2 and
    every pair of edges that meet in a node is implied by exactly one line or its flip.  -> (segments, links)"""
    segs, links = parse(text)
    for a, oa, b, ob, ov in links:
        assert ov == k
        assert oriented(segs, a, oa)[-k:] == oriented(segs, b, ob)[:k], (a, oa, b, ob)
    assert len(set(links)) == len(links)
    if want_kc is not None:
        assert all(("KC" in tags) == want_kc for _s, tags in segs.values())
    if edges is not None:
        assert twin_stats["missing"] == 0 and twin_stats["ambiguous"] == 0
        assert 2 * len(segs) == twin_stats["live_edges"] + twin_stats["self"]
        paths = {s + q for s, _e, q in edges}
        assert len(paths) == len(edges)
        for seq, _tags in segs.values():
            assert seq in paths and R.rev_comp(seq) in paths
        implied = {}
        for a, oa, b, ob, _ov in links:
            x, y = oriented(segs, a, oa), oriented(segs, b, ob)
            for pair in {(x, y), (R.rev_comp(y), R.rev_comp(x))}:
                implied[pair] = implied.get(pair, 0) + 1
        by_start = {}
        for s, _e, q in edges:
            by_start.setdefault(s, []).append(s + q)
        met = {(s + q, p) for s, e, q in edges for p in by_start.get(e, [])}
        assert set(implied) == met and set(implied.values()) <= {1}
    return segs, links


def by_id(nodes, oedges):
    """the oracle's canonical (node k-mers, (start, end, seq)) -> (edges, ids, starts, ends) with ids by position"""
    at = {s: i for i, s in enumerate(nodes)}
    return oedges, list(range(len(oedges))), [at[s] for s, _e, _q in oedges], [at[e] for _s, e, _q in oedges]


# ---- hand-written cases -------------------------------------------------------------------------------------------------------
# k = 3.  a: TTA -> ACG, b: ACG -> GGA, c: ACG -> GCC and their twins a', b', c'; ids a b c a' b' c' = 0..5
Y_NODES = {"TTA": 0, "ACG": 1, "GGA": 2, "GCC": 3, "CGT": 4, "TAA": 5, "TCC": 6, "GGC": 7}
Y_EDGES = [("TTA", "ACG", "ACG"), ("ACG", "GGA", "GA"), ("ACG", "GCC", "CC"), ("CGT", "TAA", "TAA"), ("TCC", "CGT", "GT"), ("GGC", "CGT", "GT")]


def y_graph(keep=range(6)):
    edges = [Y_EDGES[i] for i in keep]
    return edges, list(keep), [Y_NODES[s] for s, _e, _q in edges], [Y_NODES[e] for _s, e, _q in edges]


def test_a_strand_closed_y():
    edges, ids, starts, ends = y_graph()
    for (s, e, q) in edges:
        assert (s + q).endswith(e)
    twin, cls, st = GR.twins(edges, ids)
    assert twin == {0: 3, 3: 0, 1: 4, 4: 1, 2: 5, 5: 2} and set(cls.values()) == {"paired"}
    assert st == dict(live_edges=6, paired=6, self=0, missing=0, ambiguous=0, key_collisions=0)
    text, gst = GR.gfa(edges, ids, starts, ends, 3)
    # a = TTAACG is above its reverse complement CGTTAA: the segment is a' (e3), and a is e3 '-'
    assert text == (b"H\tVN:Z:1.0\n"
                    b"S\te1\tACGGA\tLN:i:5\n"
                    b"S\te2\tACGCC\tLN:i:5\n"
                    b"S\te3\tCGTTAA\tLN:i:6\n"
                    b"L\te3\t-\te1\t+\t3M\n"
                    b"L\te3\t-\te2\t+\t3M\n")
    assert gst == dict(live_edges=6, segments=3, folded=3, pairs=4, links=2, mirrored=2, bases=16, text_bytes=len(text), missing_windows=0)
    check_gfa(text, 3, edges, st)
    # with a count table: every window seen 2 times, but ACG (stored as ACG or CGT) 5 times
    counts = {}
    for s, _e, q in edges:
        p = s + q
        for i in range(len(p) - 2):
            counts[R.canon(p[i:i + 3])] = 5 if R.canon(p[i:i + 3]) == R.canon("ACG") else 2
    text, gst = GR.gfa(edges, ids, starts, ends, 3, counts)
    assert b"S\te1\tACGGA\tLN:i:5\tKC:i:9\n" in text and b"S\te3\tCGTTAA\tLN:i:6\tKC:i:11\n" in text and gst["missing_windows"] == 0
    check_gfa(text, 3, edges, st, want_kc=True)


def test_a_self_twin_edge():
    edges, ids = [("ACG", "CGT", "CGT")], [7]
    twin, cls, st = GR.twins(edges, ids)
    assert twin == {7: 7} and cls == {7: "self"} and st["self"] == 1 and st["paired"] == 0
    text, gst = GR.gfa(edges, ids, [0], [1], 3)
    assert text == b"H\tVN:Z:1.0\nS\te7\tACGCGT\tLN:i:6\n"
    assert (gst["segments"], gst["folded"], gst["pairs"], gst["links"]) == (1, 0, 0, 0)
    check_gfa(text, 3, edges, st)


def test_a_pair_that_is_its_own_mirror():
    """k = 4: e runs into the palindromic node ACGT and its twin leaves it: (e, twin e) is its own mirror and is written once"""
    edges, ids = [("GGAC", "ACGT", "GT"), ("ACGT", "GTCC", "CC")], [0, 1]
    assert R.rev_comp("ACGT") == "ACGT" and R.rev_comp("GGACGT") == "ACGTCC"
    twin, cls, st = GR.twins(edges, ids)
    assert twin == {0: 1, 1: 0}
    text, gst = GR.gfa(edges, ids, [0, 1], [1, 2], 4)
    assert text == b"H\tVN:Z:1.0\nS\te1\tACGTCC\tLN:i:6\nL\te1\t-\te1\t+\t4M\n"
    assert (gst["pairs"], gst["links"], gst["mirrored"]) == (1, 1, 0)
    check_gfa(text, 4, edges, st)


def test_one_twin_removed():
    """the Y without a': a is `missing` and its own segment; its links are written, the two on the other strand are gone with a'"""
    edges, ids, starts, ends = y_graph([0, 1, 2, 4, 5])
    twin, cls, st = GR.twins(edges, ids)
    assert cls[0] == "missing" and twin[0] == GR.NONE and st == dict(live_edges=5, paired=4, self=0, missing=1, ambiguous=0, key_collisions=0)
    text, gst = GR.gfa(edges, ids, starts, ends, 3)
    assert text == (b"H\tVN:Z:1.0\n"
                    b"S\te0\tTTAACG\tLN:i:6\n"
                    b"S\te1\tACGGA\tLN:i:5\n"
                    b"S\te2\tACGCC\tLN:i:5\n"
                    b"L\te0\t+\te1\t+\t3M\n"
                    b"L\te0\t+\te2\t+\t3M\n")
    assert (gst["segments"], gst["folded"], gst["pairs"], gst["links"], gst["mirrored"]) == (3, 2, 2, 2, 0)
    check_gfa(text, 3)


def test_two_copies_of_one_path():
    """a path and its reverse complement, each twice (copies have nodes of their own): all four are ambiguous and stay segments"""
    edges = [("ACG", "GGA", "GA"), ("ACG", "GGA", "GA"), ("TCC", "CGT", "GT"), ("TCC", "CGT", "GT")]
    ids, starts, ends = [0, 1, 2, 3], [0, 2, 4, 6], [1, 3, 5, 7]
    twin, cls, st = GR.twins(edges, ids)
    assert set(cls.values()) == {"ambiguous"} and set(twin.values()) == {GR.NONE} and st["ambiguous"] == 4
    text, gst = GR.gfa(edges, ids, starts, ends, 3)
    assert text.count(b"S\t") == 4 and gst["segments"] == 4 and gst["folded"] == 0 and gst["links"] == 0
    check_gfa(text, 3)
    # one copy of the path, two of its reverse complement: the single one is ambiguous too (|C'| > 1)
    twin, cls, st = GR.twins(edges[1:], ids[1:])
    assert set(cls.values()) == {"ambiguous"}


# ---- the oracle's graphs ------------------------------------------------------------------------------------------------------

def whole(k, nodes, oedges):
    edges, ids, starts, ends = by_id(nodes, oedges)
    twin, cls, st = GR.twins(edges, ids)
    assert st["live_edges"] == st["paired"] + st["self"] + st["missing"] + st["ambiguous"] == len(edges) and st["paired"] % 2 == 0
    assert all(twin[twin[i]] == i and cls[twin[i]] == cls[i] for i in ids if cls[i] in ("paired", "self"))
    text, gst = GR.gfa(edges, ids, starts, ends, k)
    assert gst["live_edges"] == gst["segments"] + gst["folded"] and gst["pairs"] == gst["links"] + gst["mirrored"]
    check_gfa(text, k, edges, st)
    return st, gst


@pytest.mark.parametrize("k", FC.KS)
def test_folded_graphs(k):
    """tandem repeats, inverted repeats, hairpins, homopolymers and (even k) palindromic nodes: the oracle's graph is strand-closed
    and without copies, so the full check applies"""
    c = FC.case(k, FC.SEEDS[k], "clean")
    nodes, oedges = c.canonical()
    st, gst = whole(k, nodes, oedges)
    assert st["self"] == FC.TABLE[(k, "clean")]["self_twin"] >= 1 and gst["mirrored"] >= 10


@pytest.mark.parametrize("k", [9, 15, 34])
def test_random_reads(k):
    rnd = random.Random(77 + k)
    g = FC.rand_seq(rnd, 1200)
    reads = [g[s:s + 80] if rnd.random() < 0.5 else R.rev_comp(g[s:s + 80]) for s in range(0, len(g) - 80, 5)]
    reads = ["".join(c if rnd.random() >= 0.01 else rnd.choice("AGCT") for c in r) for r in reads]
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    nodes, oedges = oracle_canonical(O.Graph(ref))
    assert len(oedges) > 40
    whole(k, nodes, oedges)
