"""tests/slot_ref.py against itself, one key at a time on Python ints: the finder's groups really share their first stored word,
their start position and their tag; the stored forms round-trip; no stored word of a valid key is a sentinel.  No GPU."""
import random
import time

import numpy as np
import pytest

import slot_ref as SR
from oracle import pyref as R

CASES = [(k, name) for name in ("count12", "slot24", "tagged", "slot16") for k in SR.KS[name]]
SHAPES = {1: (8, 64), 2: (8, 32), 64: (8, 16)}        # groups x keys, as tests/test_adversarial_keys_gpu.py asks for them


def _shape(k):
    return SHAPES[64 if k == 64 else SR.words_for_k(k)]


def _fmix(x):
    """MurmurHash3's 64-bit finaliser, written out once more so that the check below is not slot_ref's own code"""
    m = (1 << 64) - 1
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & m
    x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & m
    return x ^ (x >> 33)


def test_mix64_scalar_and_vector_forms_agree():
    assert SR.mix64(0) == 0
    rnd = random.Random(1)
    xs = [0, 1, SR.M64, SR.M63, 1 << 63] + [rnd.getrandbits(64) for _ in range(1000)]
    got = SR.mix64_np(np.array(xs, np.uint64))
    assert [int(g) for g in got] == [SR.mix64(x) for x in xs] == [_fmix(x) for x in xs]
    assert len(set(int(g) for g in got)) == len(set(xs))            # (a bijection: no two of these collide)
    his = [rnd.getrandbits(64) for _ in xs]
    got2 = SR.slot_hash_np(2, np.array(xs, np.uint64), np.array(his, np.uint64))
    assert [int(g) for g in got2] == [_fmix(a ^ ((_fmix(b) + 0x9e3779b97f4a7c15) & SR.M64)) for a, b in zip(xs, his)]
    assert [SR.slot_hash(2, a, b) for a, b in zip(xs, his)] == [int(g) for g in got2]
    assert [SR.slot_hash(1, a) for a in xs] == [int(g) for g in got]


@pytest.mark.parametrize("canonical_only", [False, True])
@pytest.mark.parametrize("k,layout", CASES)
def test_groups_share_first_word_start_and_tag(k, layout, canonical_only):
    n_groups, size = _shape(k)
    G = SR.find_groups(k, n_groups, size, canonical_only, seed=5)
    W, S = SR.words_for_k(k), SR.seg_slots(k)
    assert (G.W, G.S, G.tagged) == (W, S, k == 64) and len(G.groups) == n_groups
    seen = set()
    for g in G.groups:
        assert len(g.keys) == size and len(g.siblings) == SR.N_SIBLINGS
        for lo, hi in g.keys + g.siblings:
            assert (lo, hi) not in seen
            seen.add((lo, hi))
            # a k-mer: nothing above 2k bits
            assert 0 <= lo < 1 << 64 and 0 <= hi < 1 << 64
            assert (lo | (hi << 64)) >> (2 * k) == 0
            # the first stored word, by the layout's own rule
            if W == 1:
                assert lo % (1 << 31) == G.w0
                h = _fmix(lo)
            else:
                assert (lo | (hi << 64)) % (1 << 63) == G.w0
                h = _fmix(lo ^ ((_fmix(hi) + 0x9e3779b97f4a7c15) % (1 << 64)))
            pos = h % S
            if k == 64:
                assert hi >> 62 == g.tag
                pos = pos - pos % 4 + g.tag
            else:
                assert g.tag == 0
            assert pos == g.start == SR.start_pos(k, lo, hi)
            if canonical_only:
                s = R.unpack(lo, hi, k)
                assert R.hash_code(s) < R.hash_code(R.rev_comp(s))
    # one group at the last start position, the others in the lower half; two chains that run into each other
    assert G.groups[0].start // (4 if k == 64 else 1) == (S // 4 if k == 64 else S) - 1
    assert all(g.start < S // 2 for g in G.groups[1:])
    a, b = (1, 5) if k == 64 else (1, 2)
    assert G.groups[b].start - G.groups[a].start == (4 if k == 64 else 3)
    if k == 64:
        assert sorted(g.tag for g in G.groups) == [0, 0, 1, 1, 2, 2, 3, 3]
        assert G.groups[a].tag == G.groups[b].tag


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("k", [27, 31, 47, 63, 64])
def test_start_positions_are_valid_under_any_seed(k, seed):
    G = SR.find_groups(k, 9, 4, seed=seed)
    starts = [g.start for g in G.groups]
    assert len(set(starts)) == 9 and all(0 <= x < G.S // 2 for x in starts[1:]) and starts[0] >= G.S - 4


def test_the_search_is_quick():
    """about 0.2 s for the largest shape the GPU tests ask for; the bound only says "no committed fixture needed", with room for
    a loaded host"""
    t0 = time.perf_counter()
    SR.find_groups(27, 9, 64, True, seed=5)
    assert time.perf_counter() - t0 < 10.0


def test_finder_is_deterministic_and_refuses_short_keys():
    a, b = SR.find_groups(31, 3, 8, seed=9), SR.find_groups(31, 3, 8, seed=9)
    assert a == b and a != SR.find_groups(31, 3, 8, seed=10)
    for k in (21, 35):
        with pytest.raises(ValueError):
            SR.find_groups(k, 2, 8)


def _extreme(k):
    top = (1 << (2 * k)) - 1
    out = [0, top, 1, 1 << (2 * k - 1), 1 << (2 * k - 2), top >> 1, top >> 2]                 # all-A, all-T, single bits at the ends
    if k >= 63:
        out += [1 << 125, 1 << 124, 3 << 124, (1 << 126) - 1]
    if k == 64:
        out += [1 << 127, 1 << 126, 3 << 126, top ^ (3 << 126), (1 << 63), (1 << 63) - 1, 1 << 62]
    return out


@pytest.mark.parametrize("k", [34, 47, 63, 64])
def test_stored_form_round_trips_16_byte_keys(k):
    rnd = random.Random(k)
    for x in _extreme(k) + [rnd.getrandbits(2 * k) for _ in range(2000)]:
        lo, hi = x & SR.M64, x >> 64
        w0, w1 = SR.to_stored(lo, hi)
        assert w0 == x % (1 << 63) and w1 == (x >> 63) % (1 << 63)
        tag = SR.key_tag(2, hi)
        assert tag == x >> 126 and (tag == 0 or k == 64)
        assert SR.from_stored(w0, w1, tag) == (lo, hi)
        # no stored word of a valid key is a sentinel: both have their top bit clear
        assert w0 < 1 << 63 and w1 < 1 << 63
        assert w0 not in (SR.KEY_EMPTY, SR.KEY_TOMB) and w1 not in (SR.KEY_EMPTY, SR.KEY_TOMB)


@pytest.mark.parametrize("k", [2, 16, 21, 27, 31])
def test_count_slot_halves_give_the_key_back(k):
    rnd = random.Random(k)
    for x in _extreme(k) + [rnd.getrandbits(2 * k) for _ in range(2000)]:
        w0, w1 = SR.c_w0(x), SR.c_w1(x)
        assert w0 | w1 << 31 == x
        assert w0 < 1 << 31 and w1 < 1 << 31
        assert w0 not in (SR.KEY_EMPTY32, SR.KEY_TOMB32) and w1 not in (SR.KEY_EMPTY32, SR.KEY_TOMB32)
        assert x not in (SR.KEY_EMPTY, SR.KEY_TOMB)                   # the 16-byte slot stores the key itself
        assert SR.key_tag(1) == 0 and SR.first_word(k, x) == w0


def test_sentinels_are_what_the_header_says():
    assert SR.KEY_EMPTY == 2**64 - 1 and SR.KEY_TOMB == 2**64 - 2
    assert SR.KEY_EMPTY32 == 2**32 - 1 and SR.KEY_TOMB32 == 2**32 - 2
    assert SR.SEG_BITS == {1: 11, 2: 10}
