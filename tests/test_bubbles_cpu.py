"""The restatement of the edge-distance and bubble rules (tests/bubbles_ref.py) against hand-written answers on the hand-written
graphs of tests/bubbles_cases.py, and those graphs against the oracle's buildGraph of the same k-mer set.  No GPU."""
import random

import pytest

from genome_amd import dna, synth
from oracle import oracle as O
from oracle import pyref as R

import bubbles_cases as BC
import bubbles_ref as B
import tips_ref as T

CASES = BC.cases()
IDS = [c["name"] for c in CASES]


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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hand_graph_is_the_graph_of_its_kmers(case):
    assert len(set(case["edges"])) == len(case["edges"])
    assert sorted(oracle_edges(case["counts"], BC.K)) == sorted(case["edges"])
    assert B.strand_closed(case["edges"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_gives_the_hand_written_answers(case):
    edges = case["edges"]
    cov, missing = T.coverage(case["counts"], edges)
    assert missing == 0
    for e, want in case["cov"].items():
        assert cov[edges.index(e)] == want, e
    for (a, b), want in case["dist"].items():
        assert B.levenshtein(a[2], b[2]) == B.levenshtein(b[2], a[2]) == want
        for d in (0, 1, 3, 4, 31):
            assert B.distance(a[2], b[2], d) == min(want, d + 1)
    rm, pairs = B.pop(case["counts"], edges, case["max_len"], case["max_diff"])
    assert {edges[i] for i in rm} == case["removed"] and pairs == case["pairs"]
    left = [e for i, e in enumerate(edges) if i not in rm]
    assert B.strand_closed(left)                                         # a strand-closed edge set stays strand-closed
    assert all(e in left for e in case["keep"])
    assert B.pop(case["counts"], left, case["max_len"], case["max_diff"])[0] == set()        # a second round removes nothing
    assert B.pop(case["counts"], edges, 0, case["max_diff"]) == (set(), 0)                   # max_len = 0
    assert B.pop(case["counts"], edges, case["max_len"], 0) == (set(), case["pairs_at_0"])   # max_diff = 0


def test_named_consequences_of_the_rule():
    by = {c["name"]: c for c in CASES}
    assert len(by["snp_weak_branch"]["removed"]) == 2 and not by["snp_equal_coverage"]["removed"]
    assert by["snp_weak_branch"]["edges"] == by["snp_equal_coverage"]["edges"]               # only the counts differ
    ins = by["insertion_in_weak_branch"]
    assert sorted(len(e[2]) for e in ins["removed"]) == [BC.K + 1] * 2 and BC.edge(BC.strong_path(0)) in ins["edges"]
    assert len(BC.edge(BC.strong_path(0))[2]) == BC.K
    assert not by["four_differences_at_3"]["removed"] and len(by["four_differences_at_4"]["removed"]) == 2
    assert by["four_differences_at_3"]["edges"] == by["four_differences_at_4"]["edges"]      # only max_diff differs
    assert by["branch_at_max_len"]["removed"] and not by["branch_over_max_len"]["removed"]
    assert by["branch_at_max_len"]["edges"] == by["branch_over_max_len"]["edges"]            # only max_len differs
    assert all(len(e[2]) == by["branch_at_max_len"]["max_len"] for e in by["branch_at_max_len"]["removed"])
    # the chain: the strongest of the three survives, and e goes although it is too far from g — f, which goes too, condemns it
    ch = by["chain_of_three"]
    assert len(ch["removed"]) == 4 and BC.edge(BC.strong_path(5)) not in ch["removed"]
    assert sorted(ch["dist"].values()) == [3, 3, 4]
    tip = by["bubble_next_to_a_tip"]
    assert len(tip["keep"]) == 2 and not (set(tip["keep"]) & tip["removed"])
    assert {tip["edges"][i] for i in T.tips(tip["counts"], tip["edges"], 2 * BC.K)} == set(tip["keep"])   # (the tip rule would take it)


def test_levenshtein_on_known_pairs():
    assert B.levenshtein("", "") == 0 and B.levenshtein("", "ACG") == 3 and B.levenshtein("ACG", "") == 3
    assert B.levenshtein("ACGT", "ACGT") == 0
    assert B.levenshtein("ACGT", "ACGA") == 1                            # a substitution at the last base
    assert B.levenshtein("ACGT", "ATCGT") == 1                           # an insertion right after the first base
    assert B.levenshtein("ACGT", "ACG") == 1                             # a deletion at the end
    assert B.levenshtein("ACGT", "CGTA") == 2                            # a shift is two indels, not four substitutions
    assert B.levenshtein("AAAA", "CCCC") == 4
    rnd = random.Random(5)
    for _ in range(200):                                                 # never below the difference of the lengths
        x, y = ("".join(rnd.choice("AGCT") for _ in range(rnd.randrange(0, 40))) for _ in range(2))
        assert abs(len(x) - len(y)) <= B.levenshtein(x, y) <= max(len(x), len(y))
        assert all(B.distance(x, y, d) == min(B.levenshtein(x, y), d + 1) for d in (0, 1, 3, 31))
    strs = ["".join(rnd.choice("AGCT") for _ in range(n)) for n in (0, 1, 2, 5, 31, 32, 33, 64, 70, 3, 12, 12)] + ["ACGT", "ACGA"]
    for x in strs:                                                       # the many-at-once form is the same matrix
        assert B.levenshtein_many(x, strs) == [B.levenshtein(x, y) for y in strs]
    assert B.levenshtein_many("ACGT", []) == []
    assert B.distance("AAAA", "CCCC", 2) == 3 and B.distance("AAAA", "CCCC", 4) == 4 and B.distance("AAAA", "AAAA", 0) == 0


def test_self_loops_are_parallel_and_mutual_twins_tie():
    # two self-loops at one node are a parallel pair
    n = "ACGTTGCATGA"
    edges = [(n, n, "C" + n), (n, n, "G" + n), (n, "TTTTTTTTTTT", "T")]
    assert B.parallel_pairs(edges, 100) == [(0, 1)] and B.parallel_pairs(edges, 11) == []
    # an edge and its twin read the same windows, whatever the counts: where the two are parallel to each other neither is below
    path = "ACGTTGCATGACCTCATGGAACGT"
    rp = R.rev_comp(path)
    pair = [(path[:11], path[-11:], path[11:]), (rp[:11], rp[-11:], rp[11:])]
    counts = {R.canon(path[i:i + 11]): 5 + i for i in range(len(path) - 10)}
    cov, missing = T.coverage(counts, pair)
    assert missing == 0 and cov[0] == cov[1] and not T._weaker(cov[0], cov[1]) and not T._weaker(cov[1], cov[0])
