"""The restatement of the singleton pre-filter (tests/prefilter_ref.py) held to hand cases, to its own symmetries and to the
exactness theorem, and the populations of every input tests/test_prefilter_gpu.py feeds the device (tests/prefilter_cases.py).
No GPU, no library: this file is what makes the restatement worth comparing the device with."""
import random

import numpy as np
import pytest

import prefilter_cases as PC
import prefilter_ref as P
import slot_ref as S
from oracle import pyref as R


def key(s):
    return R.pack(R.canon(s))


def test_nbuckets():
    assert P.nbuckets(0) == P.nbuckets(1) == P.nbuckets(65536) == 262144
    assert P.nbuckets(65537) == 262148 and P.nbuckets(100003) == 400012 and P.nbuckets(10 ** 6) == 4 * 10 ** 6


def test_hand_cases():
    # one k-mer three times: one saturated bucket, the k-mer with its count
    r = P.run(["AAAAA"], 3, 1)
    assert (r.windows, r.seen_once, r.seen_twice_or_more, r.admitted) == (3, 0, 1, 3)
    assert r.table == {key("AAA"): 3} and (r.multi, r.single_admitted, r.single_rejected) == (1, 0, 0)
    assert int(r.state[P.bucket(3, *key("AAA"), r.buckets)]) == 2 and int(r.state.sum()) == 2
    # a k-mer and its reverse complement are one k-mer seen twice
    r = P.run(["AAA", "TTT"], 3, 1)
    assert r.table == {key("AAA"): 2} and (r.windows, r.seen_once, r.seen_twice_or_more, r.admitted) == (2, 0, 1, 2)
    # two k-mers once each, in different buckets: nothing enters the table
    assert P.bucket(3, *key("AAA"), 262144) != P.bucket(3, *key("AAC"), 262144)
    r = P.run(["AAAC"], 3, 1)
    assert r.table == {} and (r.windows, r.seen_once, r.seen_twice_or_more, r.admitted) == (2, 2, 0, 0)
    assert (r.multi, r.single_admitted, r.single_rejected) == (0, 0, 2)
    # reads shorter than k, and the empty read, have no window
    r = P.run(["", "AG", "AAAC"], 5, 1)
    assert (r.windows, r.seen_once, r.seen_twice_or_more, r.table) == (0, 0, 0, {})


def test_two_singletons_that_collide_are_both_admitted():
    """the first two 6-mers (in the order of their packed value) that share a bucket of the smallest filter"""
    k, nb, seen, pair = 6, P.nbuckets(1), {}, None
    for v in range(4 ** k):
        s = R.unpack(v, 0, k)
        if R.canon(s) != s:
            continue
        b = P.bucket(k, v, 0, nb)
        if b in seen:
            pair = (seen[b], s)
            break
        seen[b] = s
    assert pair and pair[0] != pair[1] and R.rev_comp(pair[0]) != pair[1]
    r = P.run(list(pair) + ["AAAAAAA"], k, 1)
    assert r.table == {key(pair[0]): 1, key(pair[1]): 1, key("AAAAAA"): 2}
    assert (r.windows, r.seen_once, r.seen_twice_or_more, r.admitted) == (4, 0, 2, 4)
    assert (r.multi, r.single_admitted, r.single_rejected) == (1, 2, 0)
    # either one alone stays out
    assert P.run([pair[0]], k, 1).table == {} and P.run([pair[1]], k, 1).seen_once == 1


@pytest.mark.parametrize("k", [4, 6, 32, 34, 64])
def test_palindrome_at_even_k(k):
    rnd = random.Random(k)
    half = "".join(rnd.choice("AGCT") for _ in range(k // 2))
    pal = half + R.rev_comp(half)
    assert R.rev_comp(pal) == pal
    r = P.run([pal, pal], k, 1)
    assert r.table == {R.pack(pal): 2} and (r.seen_once, r.seen_twice_or_more) == (0, 1)
    # inside a longer read, seen from either strand
    read = "AC" + pal + "GGT"
    a, b = P.run([read], k, 1), P.run([R.rev_comp(read)], k, 1)
    assert np.array_equal(a.state, b.state) and a.counts == b.counts and a.counts[R.pack(pal)] == 1


@pytest.mark.parametrize("k", [2, 5, 21, 31, 34, 47, 63, 64])
def test_strand_symmetry(k):
    reads = PC.reads("fixed_255", k)[:12] + ["", "AG"]
    a = P.run(reads, k, 1)
    b = P.run([R.rev_comp(r) for r in reversed(reads)], k, 1)
    assert np.array_equal(a.state, b.state) and a.table == b.table and a.counts == b.counts
    assert (a.windows, a.admitted, a.seen_once, a.seen_twice_or_more) == (b.windows, b.admitted, b.seen_once, b.seen_twice_or_more)


@pytest.mark.parametrize("k", [31, 34, 64])
def test_bucket_in_range_and_vector_form_equals_scalar(k):
    rng = np.random.default_rng(k)
    n = 100_000
    W = S.words_for_k(k)
    lo = rng.integers(0, 1 << 62, n, dtype=np.uint64) << np.uint64(2) | rng.integers(0, 4, n, dtype=np.uint64)
    hi = rng.integers(0, 1 << 62, n, dtype=np.uint64) << np.uint64(2) | rng.integers(0, 4, n, dtype=np.uint64)
    if W == 1:
        lo &= np.uint64((1 << (2 * k)) - 1)
        hi[:] = 0
    elif k < 64:
        hi &= np.uint64((1 << (2 * (k - 32))) - 1)
    for nb in (262144, 400012, (1 << 40) + 12, (1 << 64) - 4):
        got = P.bucket_np(k, lo, hi, nb)
        assert got.dtype == np.uint64 and int(got.max()) < nb
        want = [P.bucket(k, int(a), int(b), nb) for a, b in zip(lo[:20000], hi[:20000])] if nb != 262144 else \
               [P.bucket(k, int(a), int(b), nb) for a, b in zip(lo, hi)]
        assert got[:len(want)].tolist() == want
    # the multiply alone, at the corners
    corners = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 0x9E3779B97F4A7C15], np.uint64)
    for b in (1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 262144):
        assert P.mulhi64_np(corners, b).tolist() == [(int(a) * b) >> 64 for a in corners]


ALL_CASES = [("ragged", k) for k in PC.KS_ALL] + [("fixed_255", k) for k in PC.KS_ALL] + [("fixed_k", k) for k in PC.KS_ALL] + \
            [(c, k) for c in ("grow", "by_windows", "mixed", "dev_loop", "short_records") for k in PC.KS_CHUNK] + \
            [("collide", k) for k in PC.KS_COLLIDE]


@pytest.mark.parametrize("case,k", ALL_CASES)
def test_populations_and_exactness_of_every_gpu_input(case, k):
    reads, r = PC.reads(case, k), PC.restated(case, k)
    assert r.buckets == P.nbuckets(PC.expected_distinct(case, k)) and r.state.shape == (r.buckets,)
    assert r.windows == sum(max(0, len(s) - k + 1) for s in reads) == sum(r.counts.values()) > 0
    assert r.multi + r.single_admitted + r.single_rejected == len(r.counts)
    assert r.admitted == sum(r.table.values()) == r.windows - r.single_rejected
    # a bucket in state 1 holds one rejected singleton; a saturated one holds table k-mers only, at least one
    assert r.seen_once == r.single_rejected and 0 < r.seen_twice_or_more <= len(r.table) == r.multi + r.single_admitted
    assert r.multi > 0
    if k >= 21:
        assert r.single_rejected > 0 and r.single_admitted > 0, "both branches of pass 2 for singletons"
    # the exactness theorem, on the restatement itself
    for rounds in (2, 3, 5):
        assert r.filtered(rounds) == r.plain_filtered(rounds)
    assert all(c == r.counts[kk] for kk, c in r.table.items())


# the populations of the collision case, (k-mers of count >= 2, singletons admitted, singletons kept out)
COLLIDE_POPULATIONS = {31: (29624, 7852, 28108), 47: (21361, 9336, 33554)}       # of 65 584 / 64 251 distinct k-mers


@pytest.mark.parametrize("k", PC.KS_COLLIDE)
def test_collision_case_has_every_population(k):
    r = PC.restated("collide", k)
    assert r.buckets == 262144 and 60_000 <= len(r.counts) <= 80_000
    assert r.multi >= 1000 and r.single_admitted >= 1000 and r.single_rejected >= 1000
    assert (r.multi, r.single_admitted, r.single_rejected) == COLLIDE_POPULATIONS[k]


@pytest.mark.parametrize("k", [21, 55])
def test_chunked_pass_one_depends_on_the_union_only(k):
    reads = PC.reads("by_windows", k)
    whole = PC.restated("by_windows", k)
    e = PC.expected_distinct("by_windows", k)
    for calls in ([reads[:1], reads[1:]], [reads[100:], [], reads[:100]], [[r] for r in reads[::-1]]):
        got = P.run_chunked(calls, k, e)
        assert np.array_equal(got.state, whole.state) and got.table == whole.table
        assert (got.windows, got.admitted, got.seen_once, got.seen_twice_or_more) == (whole.windows, whole.admitted, whole.seen_once, whole.seen_twice_or_more)
    # pass 1 over half the reads only is a different filter: the theorem needs pass 1 to have seen everything
    f = P.Filter(k, e)
    f.add(reads[:75])
    assert f.count(reads).table != whole.table
