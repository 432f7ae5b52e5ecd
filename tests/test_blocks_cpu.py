"""The restatement of the alignment-block and breakpoint rules (tests/blocks_ref.py) on its own: held to answers written out by
hand, to the classes the cases are planted for (tests/blocks_cases.py) on the oracle's graph, to the stats' identities, to the
strand symmetry the header argues, and to judge_ref.place, the rule it refines.  No GPU."""
import pytest

import blocks_cases as BC
import blocks_ref as BR
import judge_cases as JC
import judge_ref as JR
from genome_amd import graph as GG
from test_judge_cpu import HAND_EDGES, HAND_NODES, OR_find, oracle_model


def test_names_agree_with_the_package():
    assert GG.BLOCK_STATS == BR.STATS and GG.BLOCK_BREAKS == BR.BREAKS and GG.BLOCK_CLASSES == BR.EDGE_CLASSES
    assert len(BR.STATS) == 24 and callable(GG.HipGraph.alignBlocks) and callable(GG.Blocks.finish)


# ---- 1. by hand: k = 4, edge 0 = GATTACA (interior ATTA d = 1, TTAC d = 2), edge 1 its twin TGTAATC (GTAA d = 1, TAAT d = 2) ----------
def test_rows_by_hand():
    # coordinates   0123456789a
    out = BR.align(4, HAND_NODES, HAND_EDGES, ["CCGATTACAGG"], tol=2)
    # forward: x = 3, 4 hit Edge(0, 1), Edge(0, 2) with c = 2: one run, d 1 .. 2.  reverse: the same starts hit Edge(1, 2), Edge(1, 1)
    # with c = 8: dlo = 8 - (4 + 3) = 1, dhi = 8 - (3 + 3) = 2
    assert out["rows"] == [(0, 0, 0, 2, 1, 2, 0, 0), (1, 1, 0, 8, 1, 2, 0, 0)]
    assert out["edges"] == {0: ("exact", 1, 0, 1), 1: ("exact", 1, 1, 1)} and out["pieces"] == [(2 - 1 + 4, 0), (5, 1)]
    st = out["stats"]
    assert (st["windows"], st["covered"], st["rows"], st["aligned_kmers"], st["edges_exact"], st["full_edges"], st["pieces"], st["piece_bases"]) == (8, 2, 2, 4, 2, 2, 2, 10)
    assert out["na50"] == 5 and out["nga50"] == 5                       # (10 piece bases: the first 5 is half; 11 valid bases: 5 + 5 passes half)
    BR.identities(st, live_edges=2)
    assert BR.nx50([5, 5], 21) == 0 and BR.nx50([5, 5], 20) == 5 and BR.nx50([], 0) == 0 and BR.nx50([3, 9, 4], 16) == 9


def test_breakpoints_by_hand():
    al = lambda recs, tol=2, **kw: BR.align(4, HAND_NODES, HAND_EDGES, recs, tol, **kw)
    brk = lambda out, e: [BR.BREAKS[r[6]] for r in out["rows"] if r[0] == e]
    # the path twice: the same k-mers at two places
    out = al(["GATTACAGATTACA"])
    assert brk(out, 0) == ["first", "overlap"] and out["edges"][0][0] == "repeat" and out["stats"]["pieces"] == 0
    # in two records: overlap comes before translocation
    assert brk(al(["GATTACA", "GATTACA"]), 0) == ["first", "overlap"]
    # ATTA in record 0, TTAC in record 1: no overlap, another record
    out = al(["GATTAG", "CTTACA"])
    assert brk(out, 0) == ["first", "translocation"] and out["edges"][0] == ("misassembled", 1, 0, 2) and [p for p in out["pieces"] if p[1] == 0] == [(4, 0), (4, 0)]
    # ATTA forward at 1 (c = 0), then TTAC on the other strand: GTAA reads TTAC reversed; x = 8, reverse hit of edge 0 at d = 2: c = 8 + 2 + 3 = 13
    out = al(["GATTAGGGGTAA"])
    assert [r for r in out["rows"] if r[0] == 0] == [(0, 0, 0, 0, 1, 1, 0, 0), (0, 1, 0, 13, 2, 2, 3, 0)] and brk(out, 0) == ["first", "inversion"]
    # ATTA at x = 1 (c = 0), then g bases G, then TTAC at x = 5 + g (c = 3 + g): shift g + 3 = 4, 5 and 6 against tol 5
    for g, want in ((1, "indel"), (2, "indel"), (3, "relocation")):
        out = al(["GATTA" + "G" * g + "TTACA"], tol=5)
        rows = [r for r in out["rows"] if r[0] == 0]
        assert rows[1][6:] == (BR.BREAKS.index(want), g + 3), (g, rows)
    out = al(["GATTAGTTACA"], tol=3)
    assert out["edges"][0][0] == "misassembled" and out["stats"]["indel_shift_sum"] == 0
    out = al(["GATTAGTTACA"], tol=4)
    assert out["edges"][0] == ("indel", 1, 0, 2) and (out["stats"]["indel_shift_sum"], out["stats"]["indel_shift_max"]) == (8, 4)      # (both twins)
    # a dead id below the bound, an edge never hit, a record shorter than k and an empty one
    out = al(["", "GAT", "NGATTAcA"], id_bound=3)
    assert out["edges"][2] == ("unaligned", 0, 0, 0) and out["edges"][0] == ("exact", 0, 0, 1) and out["rows"][0] == (0, 0, 2, 1, 1, 1, 0, 0)
    assert (out["stats"]["records"], out["stats"]["bases"], out["stats"]["valid_bases"], out["stats"]["windows"]) == (3, 11, 9, 2)


# ---- 2. the planted cases on the oracle's graph ---------------------------------------------------------------------------------------
def aligned(k, reads, records, tol=BC.TOL):
    edges3, nodes, edges = oracle_model(k, reads)
    return BR.align(k, nodes, edges, records, tol), edges3, nodes, edges


def record_sets(k):
    """every (reads, records) the GPU comparison runs at this k, but the long record's"""
    ch, mn, rp = BC.chimeras(k), JC.main(k), JC.repeats(k)
    return [(ch["reads"], ch["records"]), (ch["reads"], BC.marked(ch["records"], k)), (mn["reads"], mn["records"]),
            (mn["reads"], JC.variant_marks(mn["records"], k)), (mn["reads"], JC.variant_deletion(mn["records"])), (rp["reads"], rp["records"])]


@pytest.mark.parametrize("k", JC.KS)
def test_planted_contigs_get_their_classes(k):
    case = BC.chimeras(k)
    out, edges3, _nodes, edges = aligned(k, case["reads"], case["records"])
    assert len(edges) == 2 * len(case["paths"])                         # every contig is one edge and its twin
    for name, (cls, full) in case["classes"].items():
        for path in (case["paths"][name], JC.rc(case["paths"][name])):
            assert out["edges"][OR_find(edges3, path)][:2] == (cls, full), name
    rows_of = lambda name: [r for r in out["rows"] if r[0] == OR_find(edges3, case["paths"][name])]
    assert [(r[6], r[7]) for r in rows_of("reloc")] == [(0, 0), (4, 50)] and [(r[6], r[7]) for r in rows_of("near")] == [(0, 0), (5, 40)]
    assert [(r[6], r[7]) for r in rows_of("ins3")] == [(0, 0), (5, -3)] and [(r[6], r[7]) for r in rows_of("del1")] == [(0, 0), (5, 1)]
    assert [(r[1], r[2], r[6]) for r in rows_of("transloc")] == [(0, 0, 0), (0, 1, 2)] and [(r[1], r[6]) for r in rows_of("invert")] == [(0, 0), (1, 3)]
    assert [r[6] for r in rows_of("subst")] == [0, 6] and [r[6] for r in rows_of("twice")] == [0, 1]
    assert [r[2:6] for r in rows_of("kmer")] == [(4, -10, 10, 10)] and rows_of("whole")[0][3:6] == (2100, 1, 200 - k - 1)
    # the boundary: tol one lower turns `near` into a relocation
    lower = BR.align(k, _nodes, edges, case["records"], BC.TOL - 1)
    assert lower["edges"][OR_find(edges3, case["paths"]["near"])][0] == "misassembled" and lower["stats"]["pieces"] == out["stats"]["pieces"] + 2
    # pieces: a misassembled contig gives two, every other aligned contig but the repeat one
    assert out["stats"]["pieces"] == 2 * (3 * 2 + 7) and out["stats"]["edges_unaligned"] == 2 and out["stats"]["edges_repeat"] == 2
    assert out["na50"] > 0 and out["nga50"] > 0


@pytest.mark.parametrize("k", JC.KS)
def test_every_class_occurs_and_the_identities_hold(k):
    """what keeps the GPU comparison from being vacuous: every breakpoint class, every edge class and both values of `full`, in
    the cases of this k"""
    seen_b, seen_e, seen_f = set(), set(), set()
    for reads, records in record_sets(k):
        out, _e3, _nodes, edges = aligned(k, reads, records)
        BR.identities(out["stats"], live_edges=len(edges))
        assert out["stats"]["rows"] == len(out["rows"]) and out["stats"]["pieces"] == len(out["pieces"])
        seen_b |= {r[6] for r in out["rows"]}
        seen_e |= {v[0] for v in out["edges"].values()}
        seen_f |= {v[1] for v in out["edges"].values()}
    assert seen_b == set(range(7)) and seen_e == set(BR.EDGE_CLASSES) and seen_f == {0, 1}


@pytest.mark.parametrize("k", JC.KS)
def test_strand_symmetry(k):
    """the rows of an edge's twin are the mirror of the edge's: strands flipped, d -> len - d, the same records, classes and
    shifts; within a repeat only the multiset of rows and the edge class are compared (the order of overlapping rows may differ)"""
    for reads, records in record_sets(k):
        out, edges3, _nodes, edges = aligned(k, reads, records)
        for e, (s, q) in edges.items():
            t = OR_find(edges3, JC.rc(s + q))
            n = len(q)
            mine, twin = [r for r in out["rows"] if r[0] == e], [r for r in out["rows"] if r[0] == t]
            assert out["edges"][e][:2] == out["edges"][t][:2] and out["edges"][e][3] == out["edges"][t][3]
            mirror = lambda r: (1 - r[1], r[2], r[3] + (n + k - 1 if r[1] == 0 else -(n + k - 1)), n - r[5], n - r[4])
            assert sorted(mirror(r) for r in mine) == sorted(r[1:6] for r in twin)
            if out["edges"][e][0] != "repeat":
                assert [mirror(r) for r in reversed(mine)] == [r[1:6] for r in twin]
                # a breakpoint sits between two rows: read from the other end it moves to the other row of the pair
                assert [r[6:] for r in reversed(mine[1:])] == [r[6:] for r in twin[1:]]


@pytest.mark.parametrize("k", JC.KS)
def test_agreement_with_the_placements(k):
    """per edge and strand: the placement's window count is the sum of n over the rows, its min and max candidate are the min and max
    of (record, pos), in every class; hence scattered iff two rows of the hit strand differ in (record, pos), both_strands iff rows on both strands"""
    for reads, records in record_sets(k):
        out, _e3, nodes, edges = aligned(k, reads, records)
        pst, placed = JR.place(k, nodes, edges, records)
        assert (pst["records"], pst["bases"], pst["valid_bases"], pst["windows"]) == tuple(out["stats"][x] for x in ("records", "bases", "valid_bases", "windows"))
        assert out["stats"]["aligned_kmers"] == pst["fwd_edge"] + pst["rev_edge"]
        # the placements' minimum and maximum of the candidate, taken here window by window as judge_ref.place folds them
        pm = JR.position_map(k, nodes, edges)
        lohi = {}
        for r, rec_ in enumerate(records):
            for x in range(len(rec_) - k + 1):
                w = rec_[x:x + k]
                if all(c in "AGCT" for c in w):
                    for s_, key in ((0, w), (1, JR.rev_comp(w))):
                        c_, p_ = JR.lookup(pm, key)
                        if c_ == "edge":
                            cand = (r, x - p_[2] if s_ == 0 else x + p_[2] + k - 1)
                            lo, hi = lohi.get((p_[1], s_), (cand, cand))
                            lohi[(p_[1], s_)] = (min(lo, cand), max(hi, cand))
        for e in edges:
            cls, rec, pos, wf, wr = placed[e]
            for s_ in (0, 1):
                rp = [(r[2], r[3]) for r in out["rows"] if r[0] == e and r[1] == s_]
                assert ((min(rp), max(rp)) if rp else None) == lohi.get((e, s_))
            by = [[r for r in out["rows"] if r[0] == e and r[1] == s] for s in (0, 1)]
            assert [sum(r[5] - r[4] + 1 for r in rows) for rows in by] == [wf, wr]
            cands = [{(r[2], r[3]) for r in rows} for rows in by]
            if not by[0] and not by[1]:
                assert cls == "unplaced" and out["edges"][e][0] == "unaligned"
            elif by[0] and by[1]:
                assert cls == "both_strands"
            elif len(cands[0] | cands[1]) > 1:
                assert cls == "scattered"
            else:
                assert cls == ("forward" if by[0] else "reverse") and {(rec, pos)} == cands[0] | cands[1]


@pytest.mark.parametrize("k", JC.LONG_KS)
def test_long_record_runs_lie_on_the_tile_boundaries(k):
    """the inputs of the GPU tile tests: one run per contig and strand; e's run ends on window start 3T - 1, the last of the third
    tile, and f's begins at 3T + 1 behind the node at 3T; the marks cut a's and b's runs where the placements lose their windows"""
    T = JC.T
    case = JC.long_record(k)
    out, edges3, _nodes, edges = aligned(k, case["reads"], [case["record"]])
    row = lambda name: [r for r in out["rows"] if r[0] == OR_find(edges3, case["paths"][name])]
    for name, x in JC.long_coords(k).items():
        assert row(name) == [(OR_find(edges3, case["paths"][name]), 0, 0, x, 1, len(case["paths"][name]) - k - 1, 0, 0)]
    assert JC.long_coords(k)["e"] + len(case["paths"]["e"]) - k - 1 == 3 * T - 1 and JC.long_coords(k)["f"] + 1 == 3 * T + 1
    assert out["stats"]["edges_exact"] == 10 and out["stats"]["edges_unaligned"] == 2 and out["stats"]["full_edges"] == 10
    out = aligned(k, case["reads"], [JC.long_marks(case["record"], k)])[0]
    # a: the N at T - 1 takes the starts T - k .. T - 1; b: the two marks take 2T - k + 1 .. 2T + k - 2, b's first start is 2T - 4
    a, b = row("a"), row("b")
    xa, xb = JC.long_coords(k)["a"], JC.long_coords(k)["b"]
    assert [(r[4], r[5], r[6]) for r in a] == [(1, T - k - 1 - xa, 0), (T - xa, len(case["paths"]["a"]) - k - 1, 6)]
    assert [(r[4], r[5], r[6]) for r in b] == [(2 * T + k - 1 - xb, len(case["paths"]["b"]) - k - 1, 0)] and out["edges"][b[0][0]] [:2] == ("exact", 0)
