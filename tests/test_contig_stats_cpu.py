"""The planted contig-statistics cases (tests/contig_stats_cases.py) on the CPU: every case has the property it is named for, by the
plain restatement tests/checkgraph_ref.py; the restatement and genome_amd.check.n50 against multi-byte answers worked out by hand;
the chromosome overhead from the CPU model; and the condition under which the graph is the planted one.  No GPU."""
import random

import pytest

import checkgraph_ref as ref
import contig_stats_cases as S
from genome_amd.check import n50
from oracle import pyref as R


def stats(name, cutoff=0):
    return ref.contig_stats(S.lengths_of(name), cutoff)


def test_by_hand_over_several_bytes():
    hand = [
        # 5 lengths: sorted[2]; descending 65537 + 65537 = 131074, + 65536 = 196610, 2 * 196610 >= 327682
        ([65536, 65536, 65536, 65537, 65537], 0, dict(count=5, sum=327682, median=65536, n50=65536, max=65537)),
        ([65536, 65536, 65536, 65537, 65537], 65536, dict(count=2, sum=131074, median=65537, n50=65537, max=65537)),
        ([1, 2, 70000], 0, dict(count=3, sum=70003, median=2, n50=70000, max=70000)),
        ([1, 2, 70000], 2, dict(count=1, sum=70000, median=70000, n50=70000, max=70000)),
        # 2 * (260 + 257) = 1034 < 1283, 2 * (260 + 257 + 256) = 1546 >= 1283
        ([255, 255, 256, 257, 260], 0, dict(count=5, sum=1283, median=256, n50=256, max=260)),
        ([255, 256], 0, dict(count=2, sum=511, median=256, n50=256, max=256)),          # 2 * 256 >= 511
        ([255, 256], 255, dict(count=1, sum=256, median=256, n50=256, max=256)),
        # 2 * 40000 = 80000 < 80600, then the first 300 reaches it; sorted[3] of six is the upper middle
        ([300, 300, 300, 300, 300, 40000], 0, dict(count=6, sum=41500, median=300, n50=40000, max=40000)),
        ([300] * 200 + [40000], 0, dict(count=201, sum=100000, median=300, n50=300, max=40000)),
        # 2 * 16777216 >= 16777216 + 65536 + 255: the fourth byte
        ([255, 65536, 16777216], 0, dict(count=3, sum=16843007, median=65536, n50=16777216, max=16777216)),
    ]
    for lengths, cutoff, want in hand:
        assert ref.contig_stats(lengths, cutoff) == want, (lengths, cutoff)
        assert n50([x for x in lengths if x > cutoff]) == want["n50"], (lengths, cutoff)
    assert n50([]) == 0 and ref.contig_stats([], 0) == S.ZERO


def test_the_n50_is_never_below_the_median():
    """why there is no case "median 256, N50 255": the lengths from sorted[count / 2] up are at least half of them and each is at
    least as long as any below, so the descending running sum reaches half the total no later than there"""
    rnd = random.Random(1)
    for _ in range(2000):
        lengths = [rnd.choice((1, 2, 255, 256, 257, 65535, 65536, rnd.randrange(1, 70000))) for _ in range(rnd.randrange(1, 9))]
        st = ref.contig_stats(lengths, 0)
        assert st["median"] <= st["n50"] <= st["max"], lengths


def test_every_case_plants_what_the_module_says():
    assert set(S.BOUNDARY_256) <= set(S.CASES)
    for name, targets in S.CASES.items():
        assert targets and min(targets) >= 1, name
        assert len(S.lengths_of(name)) == 2 * len(targets), name
    assert sum(sum(t) for t in S.CASES.values()) < 1_100_000 and max(sum(t) for t in S.CASES.values()) < 350_000


def test_one_level():
    lengths, st = S.lengths_of("one_level"), stats("one_level")
    assert st["max"] == 255 and S.levels(st["max"]) == 1 and min(lengths) == 1
    assert len(set(lengths)) < len(S.CASES["one_level"])                            # duplicates among the targets themselves
    assert st["count"] % 2 == 0 and st["median"] == lengths[st["count"] // 2] > lengths[st["count"] // 2 - 1]      # the upper middle
    assert st["median"] != st["n50"]


@pytest.mark.parametrize("name,median,n50_", [("boundary_256_split", 255, 256), ("boundary_256_above", 256, 256), ("boundary_256_below", 255, 255)])
def test_boundary_256(name, median, n50_):
    lengths, st = S.lengths_of(name), stats(name)
    assert {255, 256, 257} <= set(lengths) and 256 < st["max"] <= 260 and S.levels(st["max"]) == 2
    assert (st["median"], st["n50"]) == (median, n50_)
    assert (st["median"] >> 8, st["n50"] >> 8) == (median >> 8, n50_ >> 8)          # which side of the byte boundary each lands on
    assert {254, 255, 256} & set(S.cutoffs(lengths)) >= {255, 256}
    # the cutoffs at the boundary move the start level: above 256 two passes are left, above the maximum's neighbour one value
    assert stats(name, 255)["median"] >= 256 and stats(name, st["max"] - 1)["count"] == 2 and stats(name, st["max"]) == S.ZERO


def test_the_boundary_arrangements_differ_in_their_prefixes():
    got = {name: (stats(name)["median"] >> 8, stats(name)["n50"] >> 8) for name in S.BOUNDARY_256}
    assert got == {"boundary_256_split": (0, 1), "boundary_256_above": (1, 1), "boundary_256_below": (0, 0)}


def test_two_level_split():
    lengths, st = S.lengths_of("two_level_split"), stats("two_level_split")
    assert 256 <= st["max"] < 65536 and S.levels(st["max"]) == 2
    assert st["median"] >> 8 == 1 and st["n50"] >> 8 == 156 and st["n50"] == 40000
    assert sum(1 for x in lengths if 290 <= x < 330) == 80 and sum(1 for x in lengths if x > 39000) == 6
    # the N50's bin is not the top one, so the sum carried into the second pass is not 0; and its bin holds two values, so a sum
    # that forgot the carry stops at the other one
    above = sum(x for x in lengths if x >> 8 > 156)
    in_bin = sorted((x for x in lengths if x >> 8 == 156), reverse=True)
    assert above == 2 * 41234 and in_bin == [40000, 40000, 39999, 39999]
    half = (st["sum"] + 1) // 2
    assert above + 40000 < half <= above + 2 * 40000 and 2 * 40000 < half <= 2 * 40000 + 2 * 39999


def test_three_level():
    lengths, st = S.lengths_of("three_level"), stats("three_level")
    assert {65535, 65536, 65537, 70000} <= set(lengths) and st["max"] == 70000 and S.levels(st["max"]) == 3
    assert sum(1 for x in lengths if x > 300) == 8 and st["count"] == 308
    assert st["n50"] == 65536 and st["n50"] >> 16 == 1 and st["median"] >> 16 == 0 and st["median"] < 256
    assert st["median"] >> 8 != st["n50"] >> 8
    assert {65535, 65536} <= set(S.cutoffs(lengths))
    # the dead-edge steps of the device test: without the 70 000s the maximum is 65 537 and the N50 stays (the two 65 537 and one
    # 65 536 are 196 610 of a half total of 196 608 + the short edges, so the second 65 536 is needed: still 65 536); without the
    # 65 537s it moves below the byte boundary under a maximum that still has three bytes; without the 65 536s the select starts
    # one level lower
    a = [x for x in lengths if x != 70000]
    b = [x for x in a if x != 65537]
    c = [x for x in b if x != 65536]
    sa, sb, sc = (ref.contig_stats(v, 0) for v in (a, b, c))
    assert (sa["max"], sa["n50"], S.levels(sa["max"])) == (65537, 65536, 3)
    assert (sb["max"], sb["n50"], S.levels(sb["max"])) == (65536, 65535, 3) and sb["n50"] >> 16 == 0
    assert (sc["max"], sc["n50"], S.levels(sc["max"])) == (65535, 65535, 2)
    assert max(sa["median"], sb["median"], sc["median"]) <= 300                    # a short edge throughout


def test_three_level_ties():
    lengths, st = S.lengths_of("three_level_tie"), stats("three_level_tie")
    assert lengths == [65536] * 6 + [65537] * 4 and S.levels(st["max"]) == 3
    assert (st["median"], st["n50"]) == (65536, 65536) and st["median"] >> 8 == st["n50"] >> 8 == 0x0100
    up = stats("three_level_tie", 65536)
    assert (up["median"], up["n50"], up["count"]) == (65537, 65537, 4)             # the same prefix, the other last byte
    lengths, st = S.lengths_of("three_level_tie_split"), stats("three_level_tie_split")
    assert lengths == [1, 1] + [65536] * 4 + [65537] * 4
    assert (st["median"], st["n50"]) == (65536, 65537) and st["median"] >> 8 == st["n50"] >> 8 == 0x0100
    for a in range(2, 12, 2):                                                       # with nothing beside them the two never part
        for b in range(2, 12, 2):
            t = ref.contig_stats([65536] * a + [65537] * b, 0)
            assert t["median"] == t["n50"], (a, b)


def test_all_equal_and_single():
    lengths, st = S.lengths_of("all_equal"), stats("all_equal")
    assert len(lengths) == 40 and set(lengths) == {300} and S.levels(300) == 2
    assert st == dict(count=40, sum=12000, median=300, n50=300, max=300)
    assert S.cutoffs(lengths) == [0, 299, 300] and stats("all_equal", 299) == st and stats("all_equal", 300) == S.ZERO
    assert S.lengths_of("single") == [1000, 1000] and stats("single") == dict(count=2, sum=2000, median=1000, n50=1000, max=1000)


def test_levels_and_cutoffs():
    assert [S.levels(x) for x in (0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert S.cutoffs([3, 255, 256, 700]) == [0, 3, 255, 256, 699, 700]
    assert S.cutoffs([65535, 65536, 65536]) == [0, 65535, 65536]
    for name in S.CASES:
        lengths = S.lengths_of(name)
        cs = S.cutoffs(lengths)
        assert {0, min(lengths), max(lengths) - 1, max(lengths)} <= set(cs)
        assert ref.contig_stats(lengths, cs[-1]) == S.ZERO and ref.contig_stats(lengths, max(lengths) - 1)["count"] == lengths.count(max(lengths))


@pytest.mark.parametrize("k", S.KS)
def test_overhead_from_the_model(k):
    """a linear chromosome of n bases gives one edge per strand of n - overhead(k) bases; the model says so at 200 bases, and at the
    lengths where a chromosome is shorter than a read, exactly a read, and one base more"""
    c = S.overhead(k)
    assert 0 < c < 200
    rnd = random.Random(7 * k)
    for target in (1, 2, S.READ_LEN - c - 1, S.READ_LEN - c, S.READ_LEN - c + 1, S.READ_LEN + S.READ_STEP - c + 1, 400):
        chrom = "".join(rnd.choices(R.BASES, k=target + c))
        assert S.model_lengths(k, [chrom]) == [target, target], target


@pytest.mark.parametrize("k", S.KS)
@pytest.mark.parametrize("name", ["one_level"] + list(S.BOUNDARY_256))
def test_the_model_builds_the_planted_lengths(name, k):
    """the small cases whole, through the model: reads -> count -> buildGraph -> simplify gives every target twice"""
    assert S.model_lengths(k, S.chromosomes(name, k)) == S.lengths_of(name)


def windows(chroms, w):
    out = []
    for c in chroms:
        for s in (c, R.rev_comp(c)):
            out += [s[i:i + w] for i in range(len(s) - w + 1)]
    return out


@pytest.mark.parametrize("k", S.KS)
@pytest.mark.parametrize("name", list(S.CASES))
def test_the_graph_is_the_planted_one(name, k):
    """all k-mers of all chromosomes, reverse complements included, are distinct, and so are all (k-1)-mers: every k-mer has the one
    neighbour on either side that its chromosome gives it and no other, so the edges are the chromosomes' and nothing else.  The
    reads cover every k-window: consecutive reads share at least k - 1 bases."""
    chroms = S.chromosomes(name, k)
    assert [len(c) - S.overhead(k) for c in chroms] == S.CASES[name]
    assert S.READ_LEN - S.READ_STEP >= k - 1 and S.READ_LEN <= 255
    for w in (k, k - 1):
        ws = windows(chroms, w)
        assert len(ws) == 2 * sum(len(c) - w + 1 for c in chroms) and len(set(ws)) == len(ws), w
    for c in chroms[:3] + chroms[-3:]:
        covered = set()
        for r in S.tiled_reads(c)[::2]:
            covered.update(r[i:i + k] for i in range(len(r) - k + 1))
        assert covered == {c[i:i + k] for i in range(len(c) - k + 1)}
