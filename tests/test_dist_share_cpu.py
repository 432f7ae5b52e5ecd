"""How dist_pipeline shares the pairs out over N ranks (no GPU): rank r of W takes the contiguous range
[n * r // W, n * (r + 1) // W) of the first n = min(take_first, count) pairs — for the count and for the walks alike."""
import random

import pytest

from genome_amd import dna
from genome_amd.dist_pipeline import pair_share


@pytest.mark.parametrize("world", range(1, 10))
@pytest.mark.parametrize("npairs,take_first", [(0, None), (1, None), (5, None), (7, 3), (8, 0), (100, None), (100, 1000), (1001, 999)])
def test_shares_cover_the_first_pairs_exactly_once(world, npairs, take_first):
    n = npairs if take_first is None else min(take_first, npairs)
    shares = [pair_share(npairs, world, r, take_first) for r in range(world)]
    assert shares[0][0] == 0 and shares[-1][1] == n
    for (a0, b0), (a1, b1) in zip(shares, shares[1:]):
        assert a0 <= b0 == a1 <= b1                       # contiguous, in rank order, never overlapping
    covered = [p for a, b in shares for p in range(a, b)]
    assert covered == list(range(n))
    assert max(b - a for a, b in shares) - min(b - a for a, b in shares) <= 1     # as even as it gets; W > n leaves ranks empty


def test_bad_rank_is_refused():
    for world, rank in [(0, 0), (3, 3), (2, -1)]:
        with pytest.raises(ValueError):
            pair_share(10, world, rank)


def test_shares_of_a_ragged_stream_concatenate_to_its_head():
    """the byte slices of the shares (dna.bin_pair_offsets) put back together are the first n pairs of the stream"""
    rnd = random.Random(5)
    reads = ["".join(rnd.choice("AGCT") for _ in range(rnd.choice([0, 3, 20, 77, 150, 255]))) for _ in range(2 * 41)]
    binb = dna.reads_to_bin(reads)
    for world in (1, 2, 5, 9):
        parts = []
        for r in range(world):
            a, b = pair_share(41, world, r, 37)
            parts.append(dna.bin_pairs(binb, a, b))
        assert b"".join(parts) == dna.reads_to_bin(reads[:2 * 37])
