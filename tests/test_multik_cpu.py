"""The multi-k restatement (tests/multik_ref.py) held to the oracle alone, no device: hand-worked cases, the identity with counting
the contig records as reads, and the end-to-end construction the GPU test runs (tests/multik_cases.py) shown on the oracle."""
import functools

import pytest
from hypothesis import given, settings
from hypothesis import strategies as st

from genome_amd import dna
from genome_amd.multik import check_ks
from oracle import oracle as O
from oracle import pyref as R

import multik_cases as MC
import multik_ref as MR
from pairs_ref import oracle_canonical


canon = functools.lru_cache(maxsize=None)(R.canon)          # (the dip construction sees every window some 80 times)


def counted(seqs, k, times=1):
    """stored k-mer -> count after counting `seqs` as reads `times` times with pyref's rule"""
    out = {}
    for s in seqs:
        for i in range(len(s) - k + 1):
            key = canon(s[i:i + k])
            out[key] = out.get(key, 0) + times
    return out


def test_three_edges_at_k1_3_k2_5_by_hand():
    # AAGC: path AAG + C (4 bases < 5: short).  ACCTT: forward (A < rc's first base... rc = AAGGT: ACCTT vs AAGGT, C > A: reverse).
    edges = [("AAG", "AGC", "C"), ("ACC", "CTT", "TT"), ("AAG", "GGT", "GT"), ("AGA", "GCT", "GCT")]
    added, stats = MR.add_graph_paths(edges, 5, 2)
    # paths: AAGC short; ACCTT vs rc AAGGT -> reverse; AAGGT vs rc ACCTT -> forward, 1 window; AGAGCT vs rc AGCTCT -> forward, 2 windows
    assert stats == {"live_edges": 4, "short": 1, "forward": 2, "self_twin": 0, "reverse": 1, "windows": 3}
    assert added == {R.canon("AAGGT"): 2, R.canon("AGAGC"): 2, R.canon("GAGCT"): 2}
    assert sum(added.values()) == 2 * stats["windows"]


def test_self_twin_path_counts_mirrored_windows_twice_and_the_palindrome_once():
    x = "AAGCTGA"
    s = x + R.rev_comp(x)                                     # 14 bases, its own reverse complement
    assert s == R.rev_comp(s)
    added, stats = MR.add_graph_paths([(s[:3], s[-3:], s[3:])], 4, 5)
    assert stats == {"live_edges": 1, "short": 0, "forward": 0, "self_twin": 1, "reverse": 0, "windows": 11}
    mid = s[5:9]
    assert mid == R.rev_comp(mid) and added[R.canon(mid)] == 5
    assert all(c == 10 for key, c in added.items() if key != R.canon(mid)) and len(added) == 6


def test_a_window_whose_strands_tie_goes_to_the_reverse_complement():
    # 18 bases: hashCode = (b0..b15) ^ (b16 b17).  With b_i + b_(17-i) = 3 for i = 2..15 the two strands agree above the low four
    # bits, and b0 = b1 = b16 = b17 = A makes those equal too, while x is not its own reverse complement (that needs b0 = 3 - b17)
    mid = "GCTAGCA"
    x = "AA" + mid + R.rev_comp(mid) + "AA"
    rc = R.rev_comp(x)
    assert len(x) == 18 and x != rc and R.hash_code(x) == R.hash_code(rc)
    assert R.canon(x) == rc and R.canon(rc) == x              # each strand is filed under the other
    path = "C" + x
    added, stats = MR.add_graph_paths([(path[:5], path[-5:], path[5:])], 18, 1)
    assert stats["forward"] == 1 and stats["windows"] == 2
    assert added == {R.canon(path[:18]): 1, rc: 1} and x not in added


seqs = st.text(alphabet="AGCT", min_size=6, max_size=40)


@settings(max_examples=60, deadline=None)
@given(st.lists(seqs, min_size=1, max_size=6), st.integers(2, 5), st.integers(1, 6), st.integers(1, 4))
def test_restatement_is_counting_the_contig_records_as_reads(genomes, k1, dk, weight):
    k2 = k1 + dk
    m = R.extract_filtered_kmers(genomes, k1, 1)
    g = R.build_graph(k1, m)
    edges = g.canonical()[1]
    added, stats = MR.add_graph_paths(edges, k2, weight)
    assert added == counted(MR.records(edges, k2), k2, weight)
    assert stats["live_edges"] == len(edges) == stats["short"] + stats["forward"] + stats["self_twin"] + stats["reverse"]
    assert stats["windows"] * weight == sum(added.values())
    assert stats["forward"] == stats["reverse"]               # the oracle's graph is strand-closed


def oracle_edges(k, counts):
    """the oracle's graph of a table given as stored k-mer -> count, simplified -> [(start, end, seq)]"""
    ref = O.PMap(k, 1)
    for key, c in counts.items():
        lo, hi = dna.pack(key)
        for _ in range(c):
            ref.update_inc(lo, hi)
    g = O.Graph(ref)
    g.simplify()
    return oracle_canonical(g)[1]


def forward_paths(edges):
    return MR.records(edges, 0)


def test_the_dip_construction_on_the_oracle_alone():
    genome = MC.dip_genome()
    assert MC.GENOME_SEED == 1 and not MC.repeats_kmer(genome, 20)
    reads = MC.dip_reads(genome)
    one = reads[:len(reads) // MC.COPIES]

    def table(k):
        return {key: c for key, c in counted(one, k, MC.COPIES).items() if c >= 3}

    t21, t55 = table(21), table(55)
    assert len(t21) == len(genome) - 21 + 1 and len(t55) == len(genome) - 55 + 1 - MC.MISSING_55
    # k = 55 alone: two contigs; k = 21: one
    alone = forward_paths(oracle_edges(55, t55))
    assert len(alone) == 2 and all(p in genome or R.rev_comp(p) in genome for p in alone)
    e21 = oracle_edges(21, t21)
    assert forward_paths(e21) in ([genome], [R.rev_comp(genome)])
    # the seeded k = 55 table: one contig, the genome
    added, stats = MR.add_graph_paths(e21, 55, 3)
    assert stats == {"live_edges": 2, "short": 0, "forward": 1, "self_twin": 0, "reverse": 1, "windows": len(genome) - 55 + 1}
    seeded = dict(counted(one, 55, MC.COPIES))
    before = len(seeded)
    for key, c in added.items():
        seeded[key] = seeded.get(key, 0) + c
    assert len(seeded) - before == MC.MISSING_55
    seeded = {key: c for key, c in seeded.items() if c >= 3}
    assert forward_paths(oracle_edges(55, seeded)) in ([genome], [R.rev_comp(genome)])


def test_check_ks():
    assert check_ks((21, 31, 55)) == [21, 31, 55] and check_ks([64]) == [64]
    for ks in ([], [31, 21], [21, 21], [32], [21, 33], [1, 21], [21, 65], ["21"], [True, 21]):
        with pytest.raises(ValueError):
            check_ks(ks)
