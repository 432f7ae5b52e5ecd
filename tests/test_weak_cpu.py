"""The restatement of the weak-connection rule (tests/weak_ref.py) against hand-computed answers on the hand-written graphs of
tests/weak_cases.py, those graphs against the oracle's buildGraph of the same k-mer set, and the properties the header states
as consequences of the rule.  No GPU."""
import pytest

import bubbles_ref as B
import tips_ref as T
import weak_cases as WC
import weak_ref as W
from test_tips_cpu import oracle_edges

CASES = WC.cases()
IDS = [c["name"] for c in CASES]
BY = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_graph_is_the_graph_of_its_kmers(case):
    assert len(set(case["edges"])) == len(case["edges"])
    assert sorted(oracle_edges(case["counts"], WC.K)) == sorted(case["edges"])
    assert T.strand_closed(case["edges"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_gives_the_hand_computed_answers(case):
    edges = case["edges"]
    cov, missing = T.coverage(case["counts"], edges)
    assert missing == 0
    for e, want in case["cov"].items():
        assert cov[edges.index(e)] == want, e
    removed, stats = W.weak(case["counts"], edges, case["max_len"], case["ratio"], case["floor"])
    assert {edges[i] for i in removed} == case["removed"]
    assert stats == case["stats"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_properties_of_the_rule(case):
    counts, edges, max_len = case["counts"], case["edges"], case["max_len"]
    ratios, floors = (0, 1, 2, 4, 5, 6, 50, W.MAX_RATIO), (0, 1, 2, 20, 50, 101, 1000)
    got = {(r, f): W.weak(counts, edges, max_len, r, f)[0] for r in ratios for f in floors}
    for (r, f), removed in got.items():
        # a strand-closed edge set stays strand-closed: under (A), under (B) and under both together
        assert T.strand_closed([e for i, e in enumerate(edges) if i not in removed]), (r, f)
        if f == 0:
            # under (A) no node loses its strongest out-edge or its strongest in-edge
            assert W.strongest_survive(counts, edges, removed), r
    assert not got[(0, 0)]
    # the removed set only grows as ratio falls (from 65535 down to 1; 0 is "off") and as floor rises
    for f in floors:
        on = [r for r in ratios if r >= 1]
        assert all(got[(hi, f)] <= got[(lo, f)] for lo, hi in zip(on, on[1:]))
    for r in ratios:
        assert all(got[(r, lo)] <= got[(r, hi)] for lo, hi in zip(floors, floors[1:]))
    # max_len = 0 removes nothing and sees no candidate
    assert W.weak(counts, edges, 0, 1, 1000) == (set(), dict.fromkeys(W.STATS, 0))


def test_named_consequences_of_the_rule():
    assert len(BY["chimeric_bridge"]["removed"]) == 2
    for kept in ("bridge_at_exactly_ratio", "bridge_strong_at_one_end", "bridge_over_max_len", "low_coverage_out_tip", "lone_contig_ratio_only"):
        assert not BY[kept]["removed"], kept
    # only the bridge's count, the ratio or max_len differ between these
    assert BY["chimeric_bridge"]["edges"] == BY["bridge_at_exactly_ratio"]["edges"] == BY["bridge_over_max_len"]["edges"]
    assert BY["bridge_at_exactly_ratio"]["counts"] == BY["bridge_tie_under_ratio_4"]["counts"] and BY["bridge_tie_under_ratio_4"]["removed"]
    assert all(len(e[2]) == WC.K for e in BY["bridge_at_max_len"]["removed"])
    # the tip is a tip: the tip rule takes it, this rule does not, at any ratio
    tip = BY["low_coverage_out_tip"]
    assert len(T.tips(tip["counts"], tip["edges"], 2 * WC.K)) == 2
    assert not W.weak(tip["counts"], tip["edges"], 2 * WC.K, 1, 0)[0]
    # the weak arm is parallel to the strong one and within max_len, yet too far from it for the bubble rule at max_diff 2
    arm = BY["dissimilar_bubble_arm"]
    popped, compared = B.pop(arm["counts"], arm["edges"], 2 * WC.K, 2)
    assert not popped and compared == 2
    weak_arm, strong_arm = arm["edges"][4], arm["edges"][2]
    assert weak_arm in arm["removed"] and weak_arm[:2] == strong_arm[:2] and B.distance(weak_arm[2], strong_arm[2], 6) == 5
    # the self-loop is one: it starts where it ends, at a node G runs through
    loop = [e for e in BY["weak_self_loop"]["removed"] if e[0] == WC.G[22:22 + WC.K]]
    assert len(loop) == 1 and loop[0][0] == loop[0][1]
    assert sum(1 for e in BY["weak_self_loop"]["edges"] if e[0] == loop[0][0]) == 2 == sum(1 for e in BY["weak_self_loop"]["edges"] if e[1] == loop[0][0])
    # two bridges leave one node, which has three ways out
    two = BY["two_bridges_at_one_junction"]
    starts = {e[0] for e in two["removed"]}
    assert len(two["removed"]) == 4 and sum(1 for e in two["edges"] if e[0] == WC.G[WC.A - WC.K:WC.A]) == 3 and WC.G[WC.A - WC.K:WC.A] in starts
    assert set(WC.both(WC.TC.LONE)) == BY["lone_contig_under_floor"]["removed"] and not BY["lone_contig_at_the_floor"]["removed"]


def test_node_identity_decides_the_competitors():
    """with `ends` the nodes are what the caller says: the bridge's end node given a copy of its own has in-degree 1 there"""
    c = BY["chimeric_bridge"]
    edges = c["edges"]
    i = edges.index(WC.edge(WC.bridge(WC.B)[1]))
    ends = [(s, e) for s, e, _q in edges]
    assert W.weak(c["counts"], edges, 2 * WC.K, 5, 0, ends)[0] == W.weak(c["counts"], edges, 2 * WC.K, 5, 0)[0]
    ends[i] = (ends[i][0], "copy")
    removed, stats = W.weak(c["counts"], edges, 2 * WC.K, 5, 0, ends)
    assert i not in removed and len(removed) == 1 and stats["candidates"] == 1


def test_exact_comparison():
    # 5 * (7 / 3) < 12 / 1 < 6 * (7 / 3) ... in integers: a = (kmers, sum)
    assert W.below(5, (3, 7), (1, 12)) and not W.below(6, (3, 7), (1, 12))
    assert not W.below(5, (12, 240), (10, 1000)) and W.below(5, (12, 239), (10, 1000))     # a tie is not below
    big = 2 ** 47
    assert W.below(W.MAX_RATIO, (big, 1), (big, W.MAX_RATIO + 1)) and not W.below(W.MAX_RATIO, (big, 1), (big, W.MAX_RATIO))


def test_planted_read_set_is_what_the_host_test_relies_on():
    """tests/weak_planted.py with the oracle and the restatement alone: ten edges, the bridge a connection the tip and bubble rules
    leave and this rule removes, and two contigs per strand after the merge"""
    from genome_amd import dna
    from oracle import oracle as O
    from test_tips_gpu import oracle_graph_edges
    import weak_planted as P

    reads = P.reads()
    ref = O.PMap(P.K, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    ref.delete_lt(P.ROUNDS)
    lo, hi, cnt = ref.export_sorted()
    counts = {dna.unpack(int(a), int(b), P.K): int(c) for a, b, c in zip(lo, hi, cnt)}
    og = O.Graph(ref)
    edges = sorted(oracle_graph_edges(og))
    assert len(edges) == 10 and T.strand_closed(edges)
    cov, missing = T.coverage(counts, edges)
    i = edges.index(P.bridge())
    halves = [c for c in cov if c[0] > 22]                               # the weakest competitor: (280 windows, sum 15610)
    assert missing == 0 and cov[i][:2] == (22, 194) and (280, 15610) in [c[:2] for c in halves] and not any(T._weaker(c, (280, 15610)) for c in halves)
    assert not T.tips(counts, edges, 2 * P.K) and B.pop(counts, edges, 2 * P.K, 3) == (set(), 0)
    removed, stats = W.weak(counts, edges, 2 * P.K, 5, 0)
    assert {edges[j] for j in removed} == {P.bridge(), twin_of(P.bridge())} and stats == dict(zip(W.STATS, (2, 2, 0, 2)))
    for s, _e, q in (edges[j] for j in removed):
        assert og.remove_edge(*dna.pack(s), "AGCT".index(q[0]))
    og.simplify()
    merged = sorted(oracle_graph_edges(og))
    s1, s2 = P.segments()
    assert merged == sorted((p[:P.K], p[-P.K:], p[P.K:]) for s in (s1, s2) for p in (s, WC.R.rev_comp(s)))
    assert W.weak(counts, merged, 2 * P.K, 5, 0) == (set(), dict.fromkeys(W.STATS, 0))


def twin_of(e):
    rpath = WC.R.rev_comp(e[0] + e[2])
    k = len(e[0])
    return (rpath[:k], rpath[-k:], rpath[k:])


def test_multik_assemble_refuses_a_malformed_remove_weak_before_any_device_work():
    from genome_amd import multik
    for bad in (True, 5, {"ratios": 5}, [5]):
        with pytest.raises(ValueError):
            multik.assemble(None, b"", 0, [21], remove_weak=bad)
