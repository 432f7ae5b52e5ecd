"""The scaffold restatement (tests/scaffolds_ref.py) against texts written by hand from the rule in include/genome_amd.h
("scaffolds: this project's own rule"), k = 3.  No device.  Codes A0 G1 C2 T3 N4; the complement swaps A/T and G/C."""
import contigs_ref as CR
import scaffolds_ref as SR

# edges as (start k-mer, end k-mer, seq): the path is start + seq and ends in the end k-mer
E = {
    0: ("AAG", "GGC", "GC"),       # AAGGC
    1: ("GGC", "CTT", "TT"),       # GGCTT   leaves 0's end node
    2: ("TAC", "ACA", "A"),        # TACA    nowhere near
    3: ("GGC", "AAG", "AAG"),      # GGCAAG  leaves 0's end node and ends in 0's start node: (0, 3) is a cycle
    10: ("GCC", "CTT", "TT"),      # GCCTT   the twin of 0
    11: ("AAG", "GCC", "CC"),      # AAGCC   the twin of 1
}
for s, t, q in E.values():
    assert (s + q)[-3:] == t
assert SR.rev_comp("AAGGC") == "GCCTT" and SR.rev_comp("GGCTT") == "AAGCC" and SR.rev_comp("ANG") == "CNT"


def pick(ids):
    return {i: E[i] for i in ids}


def run(ids, chains, gaps, **kw):
    kw.setdefault("singletons", False)
    return SR.scaffolds(pick(ids), chains, gaps, **kw)


def test_adjacent_junction():
    """1 leaves the node 0 ends in: its first k bases are 0's last, nothing goes between, the gap is not looked at"""
    text, st, rows = run([0, 1], [[0, 1]], [[-7]])
    assert text == b">s0 len=7 contigs=2 gaps=0\nAAGGCTT\n"
    assert (st["adjacent"], st["gapped"], st["clamped"], st["n_bases"], st["bases"], st["members"]) == (1, 0, 0, 0, 7, 2)
    assert rows == [(0, 0, 0, 5, 0), (0, 1, 5, 2, 3)]
    assert st["chain_forward"] == 1 and st["records"] == 1 and st["text_bytes"] == len(text)


def test_gapped_junction():
    text, st, rows = run([0, 2], [[0, 2]], [[12]])
    assert text == b">s0 len=21 contigs=2 gaps=12\nAAGGCNNNNNNNNNNNNTACA\n"
    assert (st["adjacent"], st["gapped"], st["clamped"], st["n_bases"], st["bases"]) == (0, 1, 0, 12, 21)
    assert rows == [(0, 0, 0, 5, 0), (0, 2, 17, 4, 0)]
    # min_gap itself is not clamped, one below it is
    assert run([0, 2], [[0, 2]], [[10]])[1]["clamped"] == 0 and run([0, 2], [[0, 2]], [[9]])[1]["clamped"] == 1


def test_a_negative_gap_is_clamped():
    text, st, _ = run([0, 2], [[0, 2]], [[-50]])
    assert text == b">s0 len=19 contigs=2 gaps=10\nAAGGCNNNNNNNNNNTACA\n"
    assert (st["gapped"], st["clamped"], st["n_bases"]) == (1, 1, 10)
    text, st, _ = run([0, 2], [[0, 2]], [[-50]], min_gap=1)
    assert text == b">s0 len=10 contigs=2 gaps=1\nAAGGCNTACA\n"


def test_a_cycle_comes_out_open():
    """(0, 3) closes on itself; the entry at the last member is ignored and nothing wraps around"""
    text, st, rows = run([0, 3], [[0, 3]], [[5, 99]])
    assert text == b">s0 len=8 contigs=2 gaps=0\nAAGGCAAG\n"
    assert rows == [(0, 0, 0, 5, 0), (0, 3, 5, 3, 3)] and st["adjacent"] == 1


def test_a_self_twin_chain():
    """an edge, a gap and its twin read the same on both strands: written once under either selection"""
    for strands in (1, 2):
        text, st, _ = run([0, 10], [[0, 10]], [[10]], strands=strands)
        assert text == b">s0 len=20 contigs=2 gaps=10\nAAGGCNNNNNNNNNNGCCTT\n"
        assert (st["chain_self_twin"], st["chain_forward"], st["chain_reverse"], st["records"]) == (1, 0, 0, 1)


def test_a_chain_and_its_twin_chain_give_one_record():
    """(0, 1) spells AAGGCTT, its twin chain (11, 10) the reverse complement AAGCCTT: G < C, so the first is forward"""
    ids, chains, gaps = [0, 1, 10, 11], [[0, 1], [11, 10]], [[0], [0]]
    text, st, rows = run(ids, chains, gaps, strands=1)
    assert text == b">s0 len=7 contigs=2 gaps=0\nAAGGCTT\n"
    assert (st["chains"], st["chain_forward"], st["chain_reverse"], st["records"], st["members"]) == (2, 1, 1, 1, 2)
    both, st2, rows2 = run(ids, chains, gaps, strands=2)
    assert both == text + b">s1 len=7 contigs=2 gaps=0\nAAGCCTT\n"
    assert (st2["chain_forward"], st2["chain_reverse"], st2["records"], st2["members"], st2["adjacent"]) == (1, 1, 2, 4, 2)
    assert rows2 == rows + [(1, 11, 0, 5, 0), (1, 10, 5, 2, 3)]
    # the other way round the record keeps its input index
    text, _, _ = run(ids, chains[::-1], gaps, strands=1)
    assert text == b">s1 len=7 contigs=2 gaps=0\nAAGGCTT\n"


def test_line_width_dividing_n_leaves_no_empty_line():
    assert run([0, 1], [[0, 1]], [[0]], line_width=7)[0] == b">s0 len=7 contigs=2 gaps=0\nAAGGCTT\n"
    assert run([0, 3], [[0, 3]], [[0]], line_width=4)[0] == b">s0 len=8 contigs=2 gaps=0\nAAGG\nCAAG\n"
    assert run([0, 3], [[0, 3]], [[0]], line_width=3)[0] == b">s0 len=8 contigs=2 gaps=0\nAAG\nGCA\nAG\n"
    assert run([0, 3], [[0, 3]], [[0]], line_width=0)[0] == b">s0 len=8 contigs=2 gaps=0\nAAGGCAAG\n"
    assert run([0, 2], [[0, 2]], [[10]], line_width=5)[0] == b">s0 len=19 contigs=2 gaps=10\nAAGGC\nNNNNN\nNNNNN\nTACA\n"


def test_singletons_are_the_contig_rules_records():
    ids = sorted(E)
    edges = [E[i] for i in ids]
    for strands in (1, 2):
        for min_len in (0, 5, 6):
            for lw in (0, 2, 60):
                want, cst = CR.contigs(edges, ids, min_len=min_len, line_width=lw, strands=strands)
                text, st, rows = SR.scaffolds(E, [], [], min_len=min_len, line_width=lw, strands=strands)
                assert text == want and st["singletons"] == st["records"] == cst["records"] and st["bases"] == cst["bases"] and st["chains"] == 0
                assert [r[1] for r in rows] == [i for i, _n, _c, _s in CR.parse(text)]
    # beside a chain: its members are not repeated, the chain is never dropped for length, the others follow in ascending id
    text, st, rows = SR.scaffolds(E, [[0, 1]], [[0]], min_len=5, strands=2)
    assert text == b">s0 len=7 contigs=2 gaps=0\nAAGGCTT\n>e3 len=6\nGGCAAG\n>e10 len=5\nGCCTT\n>e11 len=5\nAAGCC\n"
    assert (st["singletons"], st["records"], st["members"], st["bases"]) == (3, 4, 2, 23)
    assert rows[2:] == [(1, 3, 0, 6, 0), (2, 10, 0, 5, 0), (3, 11, 0, 5, 0)]
    assert SR.scaffolds(E, [[0, 1]], [[0]], min_len=100)[0] == b">s0 len=7 contigs=2 gaps=0\nAAGGCTT\n"
    assert [(name, n) for name, n, _ in SR.parse(text)] == [("s0", 7), ("e3", 6), ("e10", 5), ("e11", 5)]


def test_the_errors_of_the_rule():
    ok = (pick([0, 1, 2]), [[0, 1], [2]], [[0], []])
    assert SR.check(*ok, 10, 1) is None
    assert SR.check(ok[0], [[0, 1], []], [[0], []], 10, 1) == "GK_E_INVALID"          # an empty chain
    assert SR.check(ok[0], [[0, 1], [1]], [[0], []], 10, 1) == "GK_E_INVALID"         # an edge twice
    assert SR.check(ok[0], [[0, 7]], [[0]], 10, 1) == "GK_E_INVALID"                  # no live edge
    assert SR.check(*ok, 0, 1) == "GK_E_INVALID" and SR.check(*ok, 2 ** 31, 1) == "GK_E_INVALID" and SR.check(*ok, 10, 3) == "GK_E_INVALID"
