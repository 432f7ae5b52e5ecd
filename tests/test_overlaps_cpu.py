"""The overlap rule's restatement (tests/overlaps_ref.py) held to hand-computed cases, and the case set of tests/overlaps_cases.py
held to reach every class, without a GPU: the graphs here are the oracle's."""
import pytest

from insert_cases import small_pairs
from links_cases import oracle_graph
from links_ref import chains as ref_chains, joins as ref_joins, pair_links
from pairs_ref import make_pairs
import overlaps_cases as OC
import overlaps_ref as OR
import scaffolds_cases as SC
import scaffolds_ref as SR


def E(*paths, k=3):
    """edges 0, 1, .. of the given paths; the nodes are their first and last k bases"""
    return {i: (p[:k], p[len(p) - k:], p[k:]) for i, p in enumerate(paths)}


def one(edges, G, tol, mn=1, mx=7):
    return OR.junction(edges, None, 0, 1, G, tol, mn, mx)


def test_every_class_by_hand():
    ed = E("AACCGGTTAC", "GTTACGGA")                       # the last 5 of the first are the first 5 of the second, and no other o
    assert one(ed, -5, 0) == ("overlap", 5) and one(ed, -5, 2) == ("overlap", 5) and one(ed, -3, 2) == ("overlap", 5) and one(ed, -7, 2) == ("overlap", 5)
    assert one(ed, -2, 2) == ("none", 0) and one(ed, -8, 2, mx=8) == ("none", 0)        # 1..4 and 6..7: the range just misses 5
    assert one(ed, 10, 2) == ("out_of_range", 0) and one(ed, 0, 0) == ("out_of_range", 0) and one(ed, -5, 0, mn=6) == ("out_of_range", 0)
    assert one(ed, -5, 3, mx=4) == ("none", 0)                                          # max_overlap below the true overlap
    assert one(ed, -9, 1, mx=9) == ("out_of_range", 0)                                  # lo = 8 > |P(f)| - 1 = 7
    per = E("GGACACAC", "ACACTT")
    assert one(per, -3, 1) == ("ambiguous", 0) and one(per, -2, 0) == ("overlap", 2) and one(per, -4, 0) == ("overlap", 4) and one(per, -3, 0) == ("none", 0)
    adj = E("AACCGG", "CGGTTA")
    assert one(adj, -3, 0) == ("adjacent", 0)
    assert OR.junction(adj, {0: (7, 8), 1: (9, 10)}, 0, 1, -3, 0, 1, 7) == ("overlap", 3)    # copies of a node: not adjacent by id
    assert OR.CLASSES[1:] == ("adjacent", "out_of_range", "none", "ambiguous", "overlap")


def test_containment_bounds():
    """o = |P| - 1 is a hit, o = |P| is never a candidate, on either side"""
    assert one(E("AACCGG", "ACCGGT"), -5, 0) == ("overlap", 5)                          # |P(e)| - 1
    assert one(E("TTACCGG", "ACCGGT"), -5, 0) == ("overlap", 5)                         # |P(f)| - 1
    inside = E("TTACCGG", "CCGG")                                                         # all of P(f) ends P(e)
    assert one(inside, -4, 0) == ("out_of_range", 0) and one(inside, -4, 1) == ("none", 0)
    inside = E("CCGG", "CCGGTTA")
    assert one(inside, -4, 0) == ("out_of_range", 0) and one(inside, -4, 1) == ("none", 0)


def test_three_members_whose_overlaps_exceed_the_middle_one():
    ed = E("AACCGGTTAC", "GTTACG", "TACGAAT")
    chains, gaps = [[0, 1, 2]], [[-5, -4]]
    ov, rep = OR.overlaps(ed, chains, gaps, 1, min_overlap=1, max_overlap=7)
    assert ov == [[5, 4]] and rep["classes"] == [["overlap", "overlap"]] and rep["overlap_bases"] == 9 and rep["junctions"] == 2
    seq, pieces, cnt = OR.assemble(ed, chains[0], gaps[0], 10, overlaps=ov[0])
    assert seq == "AACCGGTTACGAAT" and pieces == [(0, 0, 10, 0), (1, 10, 1, 5), (2, 11, 3, 4)]
    assert cnt == dict(adjacent=0, gapped=0, clamped=0, n_bases=0, overlapped=2, dropped=9)
    text, st, rows, ost = OR.scaffolds(ed, chains, gaps, ov, singletons=False, strands=2)
    assert text == b">s0 len=14 contigs=3 gaps=0\nAACCGGTTACGAAT\n" and ost == dict(overlapped=2, dropped=9)
    assert st["adjacent"] + st["gapped"] + ost["overlapped"] == st["members"] - st["records"] and rows == [(0, *p) for p in pieces]
    # the plan refuses what the rule cannot have given
    for bad in ([[4, 4]], [[5, 3]], [[6, 4]], [[5, 128]]):
        assert OR.plan_check(ed, chains, bad) == "GK_E_INVALID"
    assert OR.plan_check(E("AACCGG", "CGGTTA"), [[0, 1]], [[3]]) == "GK_E_INVALID" and OR.plan_check(ed, chains, [[0, 4]]) is None
    # the twin chain: mirrored classes and overlaps, and R(S)
    tw = E(*(SR.rev_comp(ed[i][0] + ed[i][2]) for i in (2, 1, 0)))
    tov, trep = OR.overlaps(tw, chains, [[-4, -5]], 1, min_overlap=1, max_overlap=7)
    assert tov == [[4, 5]] and trep["classes"] == [c[::-1] for c in rep["classes"]]
    assert OR.assemble(tw, chains[0], [-4, -5], 10, overlaps=tov[0])[0] == SR.rev_comp(seq)
    assert {SR.classify(seq), SR.classify(SR.rev_comp(seq))} == {"forward", "reverse"}


def test_errors_of_the_stage():
    ed = E("AACCGGTTAC", "GTTACGGA")
    ok = dict(chains=[[0, 1]], gaps=[[-5]], tol=0, min_overlap=1, max_overlap=7)
    assert OR.check(ed, **ok) is None and OR.check(ed, **dict(ok, min_overlap=127, max_overlap=127)) is None and OR.check(ed, **dict(ok, tol=OR.I31)) is None
    for kw in (dict(tol=OR.I31 + 1), dict(tol=-1), dict(min_overlap=0), dict(min_overlap=128, max_overlap=128), dict(max_overlap=0), dict(max_overlap=128),
               dict(min_overlap=5, max_overlap=4), dict(chains=[[0, 2]]), dict(chains=[[0, 1, 0]], gaps=[[0, 0]]), dict(chains=[[0, 1], []], gaps=[[0], []]),
               dict(gaps=[[OR.I31 + 1]]), dict(gaps=[[-OR.I31 - 1]])):
        assert OR.check(ed, **dict(ok, **kw)) == "GK_E_INVALID", kw


def test_all_zero_overlaps_are_the_scaffold_rule():
    k = 31
    by_key = SC.oracle_edges(k, small_pairs(100 + k, k))
    chains, gaps = SC.constructed(by_key, k)
    num = {key: i for i, key in enumerate(sorted(by_key))}                           # (a record names its edge by a number)
    oe, chains = {num[key]: v for key, v in by_key.items()}, [[num[key] for key in c] for c in chains]
    zeros = [[0] * len(g) for g in gaps]
    for strands in (1, 2):
        want = SR.scaffolds(oe, chains, gaps, strands=strands, line_width=7)
        for ov in (None, zeros):
            got = OR.scaffolds(oe, chains, gaps, ov, strands=strands, line_width=7)
            assert got[:3] == want and got[3] == dict(overlapped=0, dropped=0)
    assert want[1]["adjacent"] > 0 and want[1]["clamped"] > 0


def test_the_cases_reach_every_class():
    seen = set()
    for k in OC.KS:
        for o in OC.dip_overlaps(k):
            reads, left, right, _ = OC.dip(1000 * k + o, k, o)
            oe = SC.oracle_edges(k, reads)
            assert len(oe) == 4                                                       # two contigs and their twins, nothing joined
            e, f = OC.find(oe, left), OC.find(oe, right)
            for tol in OC.TOLS:
                for G in OC.sweep(o, tol):
                    cls, got = OR.junction(oe, None, e, f, G, tol, OC.MIN_OVERLAP, k)
                    inside = abs(G + o) <= tol and o >= OC.MIN_OVERLAP
                    assert (cls == "overlap") == inside and got == (o if inside else 0), (k, o, tol, G, cls)
                    seen.add(cls)
    for k, ds in ((21, (-1, 0, 1, 20)), (31, (-1, 0, 1, 30)), (64, (-1, 0, 1, 20, 62, 63))):
        for d in ds:
            reads, pe, head, X = OC.planted(7 * k + d, k, d)
            oe = SC.oracle_edges(k, reads)
            e, f = OC.find(oe, pe), OC.find(oe, head, head=True)
            ed, ids = OC.plant(oe, None, f, X, ("new", 0))
            assert OR.junction(ed, ids, e, f, -(k + d), 0, OC.MIN_OVERLAP, OR.OVERLAP_MAX) == ("overlap", k + d), (k, d)
            assert OR.junction(ed, ids, e, f, -64, 63, OC.MIN_OVERLAP, OR.OVERLAP_MAX) == ("overlap", k + d)      # 118 candidates
            assert OR.junction(ed, ids, e, f, -(k + d), 3, OC.MIN_OVERLAP, k + d - 1)[0] in ("none", "out_of_range")
            if d == k - 1:
                assert len(ed[f][0] + ed[f][2]) == 2 * k
    assert OR.OVERLAP_MAX == 2 * 64 - 1
    reads, pe, head, X = OC.periodic(5, 31)
    oe = SC.oracle_edges(31, reads)
    e, f = OC.find(oe, pe), OC.find(oe, head, head=True)
    ed, ids = OC.plant(oe, None, f, X, ("new", 0))
    assert OR.junction(ed, ids, e, f, -13, 1, OC.MIN_OVERLAP, 31) == ("ambiguous", 0) and OR.junction(ed, ids, e, f, -12, 0, OC.MIN_OVERLAP, 31) == ("overlap", 12)
    seen.add("ambiguous")
    # adjacent: the fixture graph's constructed chains hold such junctions
    oe = SC.oracle_edges(31, small_pairs(131, 31))
    chains, gaps = SC.constructed(oe, 31)
    seen |= {c for cl in OR.overlaps(oe, chains, gaps, 3)[1]["classes"] for c in cl}
    assert seen == set(OR.CLASSES[1:])
    # many: every genome's junction is found
    reads, pairs = OC.many(9, 31, n=40)
    oe = SC.oracle_edges(31, reads)
    assert len(oe) == 160 and all(OR.junction(oe, None, OC.find(oe, l), OC.find(oe, r), -o, 0, 1, 31) == ("overlap", o) for l, r, o in pairs)


def e2e_restated():
    """the end-to-end case on the oracle's graph -> (edges by index, chains, gaps, overlaps, report, G)"""
    C = OC.E2E
    k = C["k"]
    pieces = OC.e2e_pieces()
    reads = make_pairs(C["seed"], k, glen=C["glen"], nrep=0, L=k + 9, npairs=C["npairs"], ins=C["ins"])
    index, lens, _keys, paths = oracle_graph(k, pieces)
    links, _cls = pair_links(k, index, lens, reads, len(reads) // 2, 0, C["ins"][1] + k)
    jn, _st = ref_joins(links, C["support"])
    chains, _cyc = ref_chains([j[0] for j in jn], [j[1] for j in jn])
    gap = {(a, b): C["mid"] - s // c for a, b, c, s in jn}
    gaps = [[gap[(a, b)] for a, b in zip(c, c[1:])] for c in chains]
    edges = {i: (p[:k], p[len(p) - k:], p[k:]) for i, p in enumerate(paths)}
    ov, rep = OR.overlaps(edges, chains, gaps, C["tol"])
    return edges, chains, gaps, ov, rep, OC.e2e_genome()


def test_the_end_to_end_case_has_three_overlaps_a_strand():
    edges, chains, gaps, ov, rep, G = e2e_restated()
    assert len(edges) == 8 and [len(c) for c in chains] == [4, 4]
    assert rep["overlap"] == 6 and rep["ambiguous"] == 0 and rep["junctions"] == 6
    assert sorted(ov[0]) == sorted(ov[1]) == sorted(OC.E2E["k"] - 1 - w for _p, w in OC.E2E["dips"])
    seqs = [OR.assemble(edges, c, g, 10, overlaps=o)[0] for c, g, o in zip(chains, gaps, ov)]
    assert sorted(seqs) == sorted([G, SR.rev_comp(G)])
    text, st, _rows, ost = OR.scaffolds(edges, chains, gaps, ov, singletons=False)
    assert st["records"] == 1 and st["n_bases"] == st["clamped"] == st["gapped"] == 0 and ost["overlapped"] == 3 and b"N" not in text.split(b"\n", 1)[1]
    assert SR.scaffolds(edges, chains, gaps, singletons=False)[1]["clamped"] == 3
