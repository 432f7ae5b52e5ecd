"""The restatement of the perfect-cycle rules (tests/cycles_ref.py) against hand-worked answers, its identities, strand closure,
and — through the CPU oracle's plain graph — that the members are exactly what the plain build covers with no node and no edge."""
import pytest

import cycles_cases as CC
import cycles_ref as CR
from genome_amd import dna
from oracle import oracle as O

SMALL = ("circular", "beside_linear", "homopolymer", "len2", "len3", "atat", "len63", "len64", "len65", "no_cycles", "one_tip", "bubbles")


def test_homopolymer_by_hand():
    nodes, edges, st = CR.build_edit(["AAAAA"])
    assert sorted(nodes) == ["AAAAA", "TTTTT"]
    assert sorted(edges) == [("AAAAA", "AAAAA", "A"), ("TTTTT", "TTTTT", "T")]
    assert st == {"cycle_kmers": 2, "cycles": 2, "anchors": 2, "self_complementary": 0, "longest": 1, "rounds": 1}


def test_atat_even_k_by_hand():
    """ATAT and TATA are palindromes on one cycle of two: the smaller one is the only anchor, its self-loop has two bases"""
    nodes, edges, st = CR.build_edit(CR.circular_kmers("AT", 4))
    assert dna.pack("TATA") == (51, 0) and dna.pack("ATAT") == (204, 0)        # the LAST base is the most significant
    assert nodes == ["TATA"] and edges == [("TATA", "TATA", "TA")]
    assert st == {"cycle_kmers": 2, "cycles": 1, "anchors": 1, "self_complementary": 1, "longest": 2, "rounds": 1}


def test_atat_odd_k_by_hand():
    """ATATA and TATAT are each other's reverse complement on one cycle: one key, two anchors, two arcs of one base"""
    nodes, edges, st = CR.build_edit(CR.circular_kmers("AT", 5))
    assert sorted(nodes) == ["ATATA", "TATAT"]
    assert sorted(edges) == [("ATATA", "TATAT", "T"), ("TATAT", "ATATA", "A")]
    assert st == {"cycle_kmers": 2, "cycles": 1, "anchors": 2, "self_complementary": 1, "longest": 2, "rounds": 1}


def test_len3_by_hand():
    k = 5
    nodes, edges, st = CR.build_edit(CR.circular_kmers("AGC", k))
    assert st["cycles"] == 2 and st["cycle_kmers"] == 6 and st["anchors"] == 2 and st["longest"] == 3 and st["rounds"] == 3
    fwd = ["AGCAG", "GCAGC", "CAGCA"]
    want = min(fwd, key=CR.anchor_key)
    assert want in nodes and CR.rc(want) in nodes
    e = [x for x in edges if x[0] == want][0]
    assert e[1] == want and len(e[2]) == 3 and (want + e[2])[-k:] == want


def test_anchor_key_is_strand_symmetric_and_by_content():
    for s in ("AGCTTAGGCAT", "TTTTTTTTTTTT", "AGGCCT"):
        assert CR.anchor_key(s) == CR.anchor_key(CR.rc(s))
        lo, hi = dna.pack(min(s, CR.rc(s), key=lambda x: (dna.pack(x)[1], dna.pack(x)[0])))
        assert CR.anchor_key(s) == (hi, lo)


def _oracle_cover(table, k):
    """the oriented k-mers the CPU oracle's plain graph has as a node or inside an edge"""
    ref = O.PMap(k, 1)
    for s in table:
        lo, hi = dna.pack(s)
        ref.update_inc(lo, hi)
    og = O.Graph(ref)
    nlo, nhi = og.nodes()
    cover = {dna.unpack(int(a), int(b), k) for a, b in zip(nlo, nhi)}
    e = og.edges()
    for i in range(len(e["len"])):
        start = dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k)
        seq = "".join(dna.BASES[int(b)] for b in e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        path = start + seq
        cover |= {path[j:j + k] for j in range(1, len(seq))}
    return cover


@pytest.mark.parametrize("k", CC.KS)
@pytest.mark.parametrize("name", SMALL)
def test_identities_closure_and_members(name, k):
    table, _ = CC.table_of(name, k)
    present = CR.oriented(table)
    nodes, edges, st = CR.build_edit(table)
    # identities
    assert sum(len(e[2]) for e in edges) == st["cycle_kmers"]
    two = sum(1 for e in edges if e[0] != e[1]) // 2
    assert st["anchors"] == st["cycles"] + two == len(nodes) == len(edges)
    # strand closure: the twin of every added edge (the reverse complement of its path, read from the end node's twin) is added too
    have = set(edges)
    for s, t, seq in edges:
        p = CR.rc(s + seq)
        assert (p[:k], p[-k:], p[k:]) in have and p[:k] == CR.rc(t) and CR.rc(s) in nodes
    # every path closes on the table: its windows are members, consecutive ones follow each other
    members = {u for c in CR.cycles(present) for u in c}
    for s, t, seq in edges:
        p = s + seq
        assert p[-k:] == t and all(p[j:j + k] in members for j in range(len(seq) + 1))
    # members == all oriented k-mers with one way in and out minus what the plain build covers
    cover = _oracle_cover(table, k)
    one_one = {u for u in present if [len(x) for x in CR.degrees(present, u)] == [1, 1]}
    assert members == one_one - cover
    assert not (members & cover)
    if name == "no_cycles":
        assert (nodes, edges) == ([], []) and st["cycle_kmers"] == 0 and st["rounds"] == 0
    if name in ("circular", "len63", "len64", "len65"):
        n = len(CC.make(name, k)[0][0])
        assert st["cycle_kmers"] == 2 * n and st["longest"] == n and st["cycles"] == 2 and cover == set()
    if name == "atat":
        assert (st["anchors"], st["cycles"], st["self_complementary"]) == ((1, 1, 1) if k % 2 == 0 else (2, 1, 1))


def test_simplify_keep_by_hand():
    """a cycle of three merge-away nodes beside a chain: the smallest key stays as a self-loop of the three sequences joined;
    a self-loop node stays; an isolated node goes; a second call changes nothing"""
    a, b, c = "AAGAC", "GACCA", "CCAAG"
    nodes = [a, b, c, "TTTTT", "GGGGG", "AGAGA", "CGCGA", "TGTGA"]
    edges = [(a, b, "CCA"), (b, c, "AG"), (c, a, "AC"), ("TTTTT", "TTTTT", "T"),
             ("AGAGA", "CGCGA", "CCGCGA"), ("CGCGA", "TGTGA", "TTGTGA"), ("AGAGA", "AGAGA", "GA")]
    (n2, e2), st = CR.simplify_keep(*CR.canonical(nodes, edges))
    keep = min((a, b, c), key=CR.anchor_key)
    i = (a, b, c).index(keep)
    seqs = ["CCA", "AG", "AC"]
    joined = "".join(seqs[(i + j) % 3] for j in range(3))
    assert (keep, keep, joined) in e2 and ("TTTTT", "TTTTT", "T") in e2
    assert ("AGAGA", "TGTGA", "CCGCGATTGTGA") in e2 and ("AGAGA", "AGAGA", "GA") in e2 and len(e2) == 4
    assert sorted(n2) == sorted([keep, "TTTTT", "AGAGA", "TGTGA"])
    assert st == {"kept_self_loops": 1, "cycles_merged": 1, "anchors_kept": 1, "nodes_removed": 4}
    again, st2 = CR.simplify_keep(n2, e2)
    assert again == (n2, e2) and st2["nodes_removed"] == 0 and st2["cycles_merged"] == 0
