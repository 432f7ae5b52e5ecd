"""The restatement of the edge-coverage and tip rules (tests/tips_ref.py) against hand-computed answers on the hand-written
graphs of tests/tips_cases.py, and those graphs against the oracle's buildGraph of the same k-mer set.  No GPU."""
import pytest

from genome_amd import dna, synth
from oracle import oracle as O
from oracle import pyref as R

import tips_cases as TC
import tips_ref as T

CASES = TC.cases()


def oracle_edges(counts, k):
    """the edges of the reference's buildGraph over the k-mer set of `counts`"""
    ref = O.PMap(k, 1)
    for key in counts:
        ref.update_inc(*dna.pack(key))
    e = O.Graph(ref).edges()
    out = []
    for i in range(len(e["len"])):
        seq = synth.bases_to_str(e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        out.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k), dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k), seq))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_graph_is_the_graph_of_its_kmers(case):
    assert len(set(case["edges"])) == len(case["edges"])
    assert sorted(oracle_edges(case["counts"], TC.K)) == sorted(case["edges"])
    assert T.strand_closed(case["edges"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_hand_computed_answers(case):
    edges = case["edges"]
    cov, missing = T.coverage(case["counts"], edges)
    assert missing == 0
    for e, want in case["cov"].items():
        assert cov[edges.index(e)] == want, e
    removed = {edges[i] for i in T.tips(case["counts"], edges, case["max_len"])}
    assert removed == case["removed"]
    assert T.strand_closed([e for e in edges if e not in removed])       # a strand-closed edge set stays strand-closed


def test_named_consequences_of_the_rule():
    by = {c["name"]: c for c in CASES}
    assert len(by["y_weak_arm"]["removed"]) == 2 and not by["y_equal_coverage"]["removed"]
    assert by["arm_at_max_len"]["removed"] and not by["arm_over_max_len"]["removed"]
    assert by["arm_at_max_len"]["edges"] == by["arm_over_max_len"]["edges"]              # only max_len differs
    assert all(len(e[2]) == 1 for e in by["arm_of_one_base"]["removed"])
    two = by["two_tips_and_a_lone_contig"]
    assert len(two["removed"]) == 4 and not (set(TC.both(TC.LONE)) & two["removed"])
    # the in-tip is an in-tip on the strand it was written on: its start has no in-edge, its end two
    c = by["in_tip"]
    arm = [e for e in c["removed"] if e[0] == c["edges"][4][0]][0]
    assert sum(1 for e in c["edges"] if e[1] == arm[0]) == 0 and sum(1 for e in c["edges"] if e[1] == arm[1]) == 2


def test_coverage_counts_an_absent_kmer_as_zero_and_adds_both_strands_of_a_verbatim_table():
    c = CASES[0]
    counts = dict(c["counts"])
    arm = c["edges"][4]
    gone = R.canon((arm[0] + arm[2])[2:2 + TC.K])
    del counts[gone]
    cov, missing = T.coverage(counts, c["edges"])
    assert missing == 2                                                  # the window and its twin's
    assert cov[4] == (5, TC.C_G + 3 * 2, 0, TC.C_G)
    flipped = [(R.rev_comp(s), n) for s, n in c["counts"].items()] + [(s, 1) for s in list(c["counts"])[::3]]
    folded = T.canonical_counts(flipped)
    assert sum(folded.values()) == sum(c["counts"].values()) + len(list(c["counts"])[::3])
    assert set(folded) == set(c["counts"])


def test_exact_comparison_of_means():
    # 7/3 < 12/5 < 5/2: decided in integers
    assert T._weaker((3, 7, 0, 0), (5, 12, 0, 0)) and T._weaker((5, 12, 0, 0), (2, 5, 0, 0))
    assert not T._weaker((2, 4, 0, 0), (3, 6, 0, 0)) and not T._weaker((3, 6, 0, 0), (2, 4, 0, 0))
    big = 2 ** 63
    assert T._weaker((big + 1, big, 0, 0), (big, big, 0, 0)) and not T._weaker((big, big, 0, 0), (big + 1, big, 0, 0))
