"""The restatement of the placement rule and of the judge (tests/judge_ref.py) held to answers written out by hand, the planted
cases (tests/judge_cases.py) held to the classes they are planted for on the oracle's graph, and the host FASTA record splitter
against tests/checkgraph_ref.py's reading of records.  No GPU."""
import pytest

import checkgraph_ref as CK
import judge_cases as JC
import judge_ref as JR
import overlaps_ref as OR
import scaffolds_cases as SC
from genome_amd import check as GC
from genome_amd import graph as GG


def test_names_agree_with_the_package():
    assert GG.PLACE_STATS == JR.PLACE_STATS and GG.PLACE_CLASSES == JR.PLACE_CLASSES
    assert GG.JUDGE_STATS == JR.JUDGE_STATS and GG.JUDGE_CLASSES == JR.JUDGE_CLASSES and GC.MISJOINS == JR.MISJOINS
    assert len(JR.PLACE_STATS) == 20 and len(JR.JUDGE_STATS) == 29


# ---- 1. the placement rule on a graph written out by hand ---------------------------------------------------------------------
# k = 4.  Edge 0: P = GATTACA (start GATT = node 0, seq ACA, end TACA = node 1); its interior k-mers are ATTA (d = 1) and TTAC (d = 2).
# Edge 1 is its twin: P = TGTAATC (start TGTA = node 2, end AATC = node 3), interior GTAA (d = 1) and TAAT (d = 2).
HAND_NODES = {0: "GATT", 1: "TACA", 2: "TGTA", 3: "AATC"}
HAND_EDGES = {0: ("GATT", "ACA"), 1: ("TGTA", "ATC")}


def test_both_diagonals_by_hand():
    # coordinates   0123456789a
    rec = "CCGATTACAGG"
    # forward: ATTA at x = 3 is Edge(0, 1): 3 - 1 = 2; TTAC at x = 4 is Edge(0, 2): 4 - 2 = 2.  P(0) starts at coordinate 2.
    # reverse: rc(ATTA) = TAAT is Edge(1, 2): 3 + 2 + 4 - 1 = 8; rc(TTAC) = GTAA is Edge(1, 1): 4 + 1 + 4 - 1 = 8.  Base 0 of P(1) = T is
    # the complement of rec[8] = A, and P(1) reads toward lower coordinates.
    st, ed = JR.place(4, HAND_NODES, HAND_EDGES, [rec])
    assert ed == {0: ("forward", 0, 2, 2, 0), 1: ("reverse", 0, 8, 0, 2)}
    assert JR.rev_comp(rec[2:9]) == "TGTAATC"
    want = dict(records=1, bases=11, valid_bases=11, windows=8, fwd_absent=4, fwd_repetitive=0, fwd_at_node=2, fwd_edge=2, rev_absent=4, rev_repetitive=0,
                rev_at_node=2, rev_edge=2, unplaced=0, both_strands=0, scattered=0, forward=1, reverse=1, forward_bases=7, reverse_bases=7, saturated=0)
    assert st == want
    JR.identities(pst=st, live_edges=2)


def test_edge_classes_by_hand():
    # a second record on the other strand: both edges are hit on both strands
    _, ed = JR.place(4, HAND_NODES, HAND_EDGES, ["CCGATTACAGG", "TGTAATC"])
    assert [ed[e][0] for e in (0, 1)] == ["both_strands", "both_strands"] and ed[0][3:] == (2, 2)
    # the path twice on one strand: two diagonals (0 and 7 in record 0)
    _, ed = JR.place(4, HAND_NODES, HAND_EDGES, ["GATTACAGATTACA"])
    assert ed[0] == ("scattered", 0, 0, 4, 0) and ed[1] == ("scattered", 0, 0, 0, 4)
    # the same diagonal number in two records is two diagonals; record 1 alone gives record = 1
    _, ed = JR.place(4, HAND_NODES, HAND_EDGES, ["GATTACA", "GATTACA"])
    assert ed[0][0] == "scattered"
    _, ed = JR.place(4, HAND_NODES, HAND_EDGES, ["", "GATTACA"])
    assert ed[0] == ("forward", 1, 0, 2, 0) and ed[1] == ("reverse", 1, 6, 0, 2)
    # N and lowercase break windows: only GATT (a node) and ATTA are left of GATTAcA; a dead id below the bound and an edge never hit are unplaced
    st, ed = JR.place(4, HAND_NODES, HAND_EDGES, ["NGATTAcA"], id_bound=3)
    assert ed[0] == ("forward", 0, 1, 1, 0) and ed[2] == ("unplaced", 0, 0, 0, 0) and (st["windows"], st["valid_bases"], st["bases"]) == (2, 6, 8)
    # a node k-mer stored twice (a node copy) is repetitive, and an edge of length 1 has no interior k-mer
    st, ed = JR.place(4, {**HAND_NODES, 4: "GATT"}, {**HAND_EDGES, 2: ("CCCC", "A")}, ["GATTACA"])
    assert st["fwd_repetitive"] == 1 and st["fwd_at_node"] == 1 and ed[2][0] == "unplaced" and st["unplaced"] == 1


# ---- 2. every junction class once, by hand --------------------------------------------------------------------------------------
def test_judge_classes_by_hand():
    k = 4
    placed = {0: ("forward", 0, 100, 9, 0), 1: ("forward", 0, 130, 9, 0), 2: ("forward", 0, 50, 9, 0), 3: ("reverse", 0, 400, 0, 9),
              4: ("forward", 1, 7, 9, 0), 5: ("scattered", 0, 0, 9, 0), 6: ("reverse", 0, 300, 0, 9), 7: ("reverse", 0, 270, 0, 9),
              8: ("forward", 0, 116, 9, 0), 9: ("forward", 0, 500, 5, 0), 10: ("forward", 0, 520, 5, 0)}
    ends = {e: (2 * e, 2 * e + 1) for e in placed}
    ends[8] = (1, 17)                                      # edge 8 starts where edge 0 ends: adjacent
    rows = [
        (0, 0, 0, 20, 0), (0, 1, 30, 20, 0),               # gapped: dscaf 30, dref 130 - 100 = 30
        (1, 9, 0, 20, 0), (1, 10, 30, 20, 0),              # gapped, dscaf 30, dref 20: err = 10 > tol
        (2, 0, 0, 20, 0), (2, 8, 20, 16, k),               # adjacent: dscaf 20, dref (116 + 4) - 100 = 20
        (3, 1, 0, 20, 0), (3, 2, 30, 20, 0),               # order
        (4, 0, 0, 20, 0), (4, 3, 30, 20, 0),               # strand
        (5, 0, 0, 20, 0), (5, 4, 30, 20, 0),               # other_record
        (6, 0, 0, 20, 0), (6, 5, 30, 20, 0),               # unjudged
        (7, 6, 0, 20, 0), (7, 7, 32, 20, 0),               # reverse: dscaf 32, dref 300 - 270 = 30, err 2 <= tol
        (8, 6, 0, 20, 0), (8, 7, 20, 17, 3),               # overlapped (no N, other nodes): dscaf 20, dref (300) - (270 - 3) = 33: distance
        (9, 5, 0, 20, 0),                                  # a record without junctions
    ]
    classes, errs, st = JR.judge(rows, ends, placed, 3, chain_records=10)
    assert classes == ["correct", "distance", "correct", "order", "strand", "other_record", "unjudged", "correct", "distance"]
    assert errs == [0, 10, 0, 30 - (50 - 130), 0, 0, 0, 2, 20 - 33]
    assert st["junctions"] == 9 and st["gapped_correct"] == 2 and st["adjacent_correct"] == 1 and st["overlapped_distance"] == 1 and st["gapped_distance"] == 1
    assert (st["gapped_correct_abs_err_sum"], st["gapped_correct_abs_err_max"]) == (2, 2)
    assert st["records_judged"] == 8 and st["records_clean"] == 10 - 5
    JR.identities(jst=st)
    # the boundary: |err| = tol is correct, tol + 1 is distance; an adjacent junction must fit exactly
    assert JR.judge(rows[14:16], ends, placed, 2, 1)[0] == ["correct"] and JR.judge(rows[14:16], ends, placed, 1, 1)[0] == ["distance"]
    off = [(2, 0, 0, 20, 0), (2, 8, 21, 16, k)]                  # one N between the pieces: a gapped junction, err = 1
    assert JR.judge(off, ends, placed, 1, 1)[:2] == (["correct"], [1]) and JR.judge(off, ends, placed, 0, 1)[0] == ["distance"]
    off = [(2, 0, 0, 20, 0), (2, 8, 20, 15, k + 1)]              # no N: it must fit exactly, whatever tol
    assert JR.judge(off, ends, placed, 100, 1)[:2] == (["distance"], [-1])


def test_n50_breaks_records_at_misjoins():
    rows = [(0, 0, 0, 100, 0), (0, 1, 110, 50, 0), (0, 2, 160, 40, 4), (1, 3, 0, 30, 0)]
    assert GC.scaffold_n50s(rows, ["correct", "correct"]) == dict(n50=200, n50_broken=200, records=2, pieces=2)
    # broken at the gapped junction: pieces of 100, 90 and 30 bases; at the other: 160 (the unbroken N run stays), 40 and 30
    assert GC.scaffold_n50s(rows, ["order", "correct"]) == dict(n50=200, n50_broken=90, records=2, pieces=3)      # (100 < 220 / 2 <= 100 + 90)
    assert GC.scaffold_n50s(rows, ["unjudged", "distance"]) == dict(n50=200, n50_broken=160, records=2, pieces=3)
    assert GC.n50([]) == 0 and GC.n50([5, 4, 1]) == 5 and GC.n50([3, 3, 3, 1]) == 3


# ---- 3. the planted cases on the oracle's graph -----------------------------------------------------------------------------------
def oracle_model(k, reads):
    """the oracle's graph with ids 0 .. n-1 in content order: nodes are their k-mers"""
    by_key = SC.oracle_edges(k, reads)
    ids = {key: i for i, key in enumerate(sorted(by_key))}
    edges3 = {ids[key]: v for key, v in by_key.items()}
    nodes = {s: s for s, _t, _q in edges3.values()}
    nodes.update({t: t for _s, t, _q in edges3.values()})
    return edges3, nodes, {e: (s, q) for e, (s, _t, q) in edges3.items()}


@pytest.mark.parametrize("k", JC.KS)
def test_planted_cases_hold_every_class(k):
    case = JC.main(k)
    edges3, nodes, edges = oracle_model(k, case["reads"])
    find = lambda path: OR_find(edges3, path)
    pst, placed = JR.place(k, nodes, edges, case["records"])
    JR.identities(pst=pst, live_edges=len(edges))
    for name, (r, x) in JC.coords(k).items():
        path = case["paths"][name]
        assert placed[find(path)][:3] == ("forward", r, x), name
        assert placed[find(JC.rc(path))][:3] == ("reverse", r, x + len(path) - 1), name
        assert placed[find(path)][3] == len(path) - k - 1                        # every interior k-mer once
    assert placed[find(case["paths"]["spur"])][0] == "unplaced"
    for tol, delta, in ((3, 3), (3, 4), (0, 0), (3, -3), (3, -4)):
        chains, gaps = JC.chains(find, case["paths"], k, delta)
        ov = [[0] * len(g) for g in gaps]
        ov[0][2] = JC.OVERLAP
        _text, sst, rows, ost = OR.scaffolds(edges3, chains, gaps, ov, strands=2, singletons=True)
        assert ost["overlapped"] == 1 and sst["adjacent"] == 2
        ends = {e: (s, t) for e, (s, t, _q) in edges3.items()}
        classes, errs, jst = JR.judge(rows, ends, placed, tol, chain_records=len(chains))
        want_c, want_e = JC.expected(tol, delta)
        assert classes == want_c
        assert all(w is None or w == g for w, g in zip(want_e, errs))
        JR.identities(jst=jst)
        assert jst["records_judged"] == 5 and jst["records_clean"] == len(chains) - 3 - (want_c[1] == "distance")
        assert jst["adjacent_correct"] == 2 and jst["overlapped_correct"] == 1 and jst["gapped_unjudged"] == 1
    # the reference variants
    marks = JR.place(k, nodes, edges, JC.variant_marks(case["records"], k))
    c0a, c3, d1 = (find(case["paths"][n]) for n in ("c0a", "c3", "d1"))
    assert marks[1][c0a][:3] == ("forward", 0, 0) and marks[1][c0a][3] < placed[c0a][3]
    assert marks[1][c3][:3] == ("forward", 0, 1760) and marks[1][c3][3] == placed[c3][3] - k
    assert marks[0]["valid_bases"] == marks[0]["bases"] - 6
    dele = JR.place(k, nodes, edges, JC.variant_deletion(case["records"]))[1]
    assert dele[d1][0] == "scattered" and dele[find(JC.rc(case["paths"]["d1"]))][0] == "scattered"


def OR_find(edges3, path):
    got = [e for e, (s, _t, q) in edges3.items() if s + q == path]
    assert len(got) == 1, (path[:20], len(got))
    return got[0]


@pytest.mark.parametrize("k", JC.LONG_KS)
def test_long_record_lies_where_it_is_built_to_lie(k):
    """the inputs of the GPU tile tests: every contig of long_record on its own diagonal with every interior k-mer once, the break
    between e and f on the third tile boundary, and the marks removing exactly the windows that contain a marked character"""
    T = JC.T
    case = JC.long_record(k)
    rec = case["record"]
    assert len(rec) == 3 * T + 700 and max(len(r) for r in case["reads"]) <= 200
    edges3, nodes, edges = oracle_model(k, case["reads"])
    find = lambda path: OR_find(edges3, path)
    assert len(edges) == 12                                                      # the five contigs and the spur, on both strands
    pst, placed = JR.place(k, nodes, edges, [rec])
    JR.identities(pst=pst, live_edges=len(edges))
    coords = JC.long_coords(k)
    assert coords == dict(a=3796, b=8187, e=11888, f=12288, tail=12298)
    for name, x in coords.items():
        path = case["paths"][name]
        n = len(path) - k - 1                                                    # a path's first and last k-mer are nodes
        assert placed[find(path)] == ("forward", 0, x, n, 0), name
        assert placed[find(JC.rc(path))] == ("reverse", 0, x + len(path) - 1, 0, n), name
    assert placed[find(case["paths"]["spur"])][0] == "unplaced"
    # by hand: a's interior windows start at T - 299 .. T + 299 - k, b's at 2T - 4 .. 2T + 399 - k, e's at 3T - 399 .. 3T - 1 (the last
    # window start of the third tile), f's at 3T + 1 .. 3T + 3, the tail's at 3T + 11 .. the record's last window but one
    assert [placed[find(case["paths"][n])][3] for n in ("a", "b", "e", "f", "tail")] == [599 - k, 404 - k, 399, 3, 689 - k]
    assert pst["windows"] == 3 * T + 700 - k + 1 and pst["fwd_at_node"] == 9 and pst["forward"] == pst["reverse"] == 5 and pst["unplaced"] == 2
    assert pst["fwd_edge"] == sum(v[3] for v in placed.values()) == 599 + 404 + 399 + 3 + 689 - 3 * k
    # the marks: an N at T - 1 takes the k windows that start at T - k .. T - 1, all interior to a; a lowercase base at 2T and a
    # substituted one at 2T + k - 2 take the windows 2T - k + 1 .. 2T + k - 2, of which 2T - 4 .. 2T + k - 2 are interior to b
    marked = JC.long_marks(rec, k)
    at = JC.long_marked_at(k)
    assert at == (T - 1, 2 * T, 2 * T + k - 2) and [i for i in range(len(rec)) if rec[i] != marked[i]] == list(at)
    assert marked[at[0]] == "N" and marked[at[1]] == rec[at[1]].lower() and marked[at[2]] in "AGCT"
    mst, mplaced = JR.place(k, nodes, edges, [marked])
    JR.identities(pst=mst, live_edges=len(edges))
    for name, x in coords.items():
        path = case["paths"][name]
        lost = sum(any(w <= m < w + k for m in at) for w in range(x + 1, x + len(path) - k))
        assert lost == dict(a=k, b=k + 3).get(name, 0)
        assert mplaced[find(path)] == ("forward", 0, x, len(path) - k - 1 - lost, 0), name
        assert mplaced[find(JC.rc(path))] == ("reverse", 0, x + len(path) - 1, 0, len(path) - k - 1 - lost), name
    assert mst["valid_bases"] == mst["bases"] - 2 and mst["windows"] == pst["windows"] - 2 * k
    assert mst["fwd_edge"] == pst["fwd_edge"] - (2 * k + 3) and mst["fwd_absent"] == pst["fwd_absent"] + 4 and mst["fwd_at_node"] == 8
    # the truncations: T - 1, T and T + 1 windows, of which a's first 298, 299 and 300 interior ones (the one at T - 300 is a node)
    for cut, windows in zip(JC.long_truncations(rec, k), (T - 1, T, T + 1)):
        tst, tplaced = JR.place(k, nodes, edges, [cut])
        assert len(cut) == windows + k - 1 and tst["windows"] == windows
        assert tplaced[find(case["paths"]["a"])] == ("forward", 0, T - 300, windows - (T - 299), 0)
        assert tst["forward"] == tst["reverse"] == 1 and tst["unplaced"] == 10


@pytest.mark.parametrize("k", JC.KS)
def test_repeats_give_scattered_and_both_strands(k):
    case = JC.repeats(k)
    edges3, nodes, edges = oracle_model(k, case["reads"])
    pst, placed = JR.place(k, nodes, edges, case["records"])
    JR.identities(pst=pst, live_edges=len(edges))
    inside = lambda rep: [e for e, (s, q) in edges.items() if (s + q) in rep or rep in (s + q)]
    assert {placed[e][0] for e in inside(case["R"])} == {"scattered"}
    assert {placed[e][0] for e in inside(case["Q"])} == {"both_strands"}
    assert pst["forward"] == pst["reverse"] > 0


# ---- 4. the FASTA record splitter ---------------------------------------------------------------------------------------------------
TEXTS = [b">a\nACGT\nAC\n>b\nGG\n", b"ACGT\r\nAC\r>b x\n\nGGnN\n>c\n>d\nTT", b"", b">only\n", b"AC\nGT", b"\n\n>a\r\nA\n", b">a\n>b\nACGT\n"]


@pytest.mark.parametrize("text", TEXTS)
def test_splitter_reads_records_as_the_fasta_check_does(text):
    segs, cur, seen = [], [], False
    for _off, body in CK.lines(text):
        if body[:1] == b">":
            if seen or any(cur):                     # (record 0 exists only if a sequence character precedes the first header)
                segs.append(b"".join(cur))
            cur, seen = [], True
        else:
            cur.append(body)
    if seen or any(cur):
        segs.append(b"".join(cur))
    got = GC.fasta_records(text)
    assert got == segs
    st, _ = CK.check(text, 2, False, set())
    assert len(got) == st["records"] and sum(len(r) for r in got) == st["bases"]
    windows = sum(sum(all(c in b"AGCT" for c in r[i:i + 2]) for i in range(len(r) - 1)) for r in got)
    assert windows == st["windows"]


def test_splitter_round_trips_the_cases_fasta():
    recs = JC.main(21)["records"]
    assert GC.fasta_records(JC.fasta(recs, width=61)) == [r.encode() for r in recs]
