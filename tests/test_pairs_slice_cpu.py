"""The `.bin` pair helpers a rank uses to hand walkPairs its own share of the pairs (dna.bin_pair_offsets / dna.bin_pairs),
against the reference reader (oracle/pyref.py reads_from_bin) on random streams: mates of every length from 0 to 255, shorter
than k included.  No GPU."""
import random

import pytest

from genome_amd import dna
from oracle import pyref as R


def random_pairs(rnd, npairs):
    reads = []
    for _ in range(2 * npairs):
        ln = rnd.choice([0, 1, 3, 4, 5, 20, 31, rnd.randint(0, 255), rnd.randint(30, 160)])
        reads.append("".join(rnd.choice("AGCT") for _ in range(ln)))
    return reads


@pytest.mark.parametrize("seed", range(6))
def test_pair_offsets_and_slices_match_the_reference_reader(seed):
    rnd = random.Random(seed)
    npairs = rnd.randint(1, 120)
    reads = random_pairs(rnd, npairs)
    binb = R.reads_to_bin(reads)
    off = dna.bin_pair_offsets(binb, npairs)
    assert len(off) == npairs + 1 and off[0] == 0 and off[-1] == len(binb)
    for i in range(npairs):
        assert R.reads_from_bin(binb[off[i]:off[i + 1]], 2) == reads[2 * i:2 * i + 2]
    for _ in range(10):
        a = rnd.randint(0, npairs)
        b = rnd.randint(a, npairs)
        part = dna.bin_pairs(binb, a, b)
        assert R.reads_from_bin(part, 2 * (b - a)) == reads[2 * a:2 * b]
        assert len(part) == sum(1 + (len(r) + 3) // 4 for r in reads[2 * a:2 * b])
    # the first pairs of a longer stream; a stream that ends inside a pair
    assert list(dna.bin_pair_offsets(binb, 0)) == [0]
    with pytest.raises(ValueError):
        dna.bin_pair_offsets(binb[:-1], npairs)
    with pytest.raises(ValueError):
        dna.bin_pair_offsets(binb, npairs + 1)


def test_shares_of_a_uniform_stream_concatenate_to_the_stream():
    rnd = random.Random(99)
    reads = ["".join(rnd.choice("AGCT") for _ in range(40)) for _ in range(2 * 300)]
    binb = dna.reads_to_bin(reads)
    cuts = [0, 0, 17, 150, 151, 300]
    parts = [dna.bin_pairs(binb, a, b) for a, b in zip(cuts, cuts[1:])]
    assert b"".join(parts) == binb and parts[0] == b""
    assert list(dna.bin_pair_offsets(binb, 300)) == [22 * i for i in range(301)]
