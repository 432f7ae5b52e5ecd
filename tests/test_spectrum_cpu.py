"""gk_spectrum_cutoff (pure host code: runs without a GPU) against the Python restatement of its rule (tests/spectrum_ref.py),
the argument checks of the three spectrum entry points, and a recorded spectrum that pins the rule."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd.freqfilter import spectrum_cutoff
from spectrum_ref import cutoff_of, spectrum_of

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "spectrum", "genome3000_k21.json")


def _hist(counted, overflow=0):
    """[0] + counted bins + [overflow]"""
    return np.array([0] + list(counted) + [overflow], np.uint64)


def test_random_histograms_match_the_restatement():
    rnd = random.Random(4242)
    some_valley = 0
    for i in range(400):
        bins = rnd.choice([2, 3, 4, 5, 8, 17, 64, 300])
        top = rnd.choice([1, 2, 3, 10, 1000, 1 << 40])          # small ranges make ties and plateaus common
        h = _hist([rnd.randrange(0, top + 1) for _ in range(bins - 2)], rnd.randrange(0, 1 << 50))
        for min_count in (1, 2, rnd.randrange(1, bins + 2)):
            want = cutoff_of(h, min_count)
            assert spectrum_cutoff(h, min_count) == want, (i, h.tolist(), min_count)
            some_valley += want[0] != 0
    assert some_valley > 100


CASES = {
    # name: (hist, min_count, expected (valley, peak, genome_size))
    "clean bimodal": (_hist([900, 200, 40, 5, 30, 120, 400, 700, 400, 100, 10]), 1, (4, 8, (4 * 5 + 5 * 30 + 6 * 120 + 7 * 400 + 8 * 700 + 9 * 400 + 10 * 100 + 11 * 10) // 8)),
    "error free: the rise is at c = 1": (_hist([2, 9, 40, 90, 40, 9]), 1, (1, 4, (2 + 18 + 120 + 360 + 200 + 54) // 4)),
    "monotone non-increasing: no valley": (_hist([50, 50, 20, 20, 3, 0, 0]), 1, (0, 0, 0)),
    "tie at the peak: the smallest c": (_hist([9, 1, 7, 7, 2, 7]), 1, (2, 3, (2 + 21 + 28 + 10 + 42) // 3)),
    "tie in the valley: the smallest c": (_hist([9, 2, 2, 5, 8, 3]), 1, (2, 5, (4 + 6 + 20 + 40 + 18) // 5)),
    "min_count = 2 ignores bin 1": (_hist([0, 7, 3, 6, 11, 4]), 2, (3, 5, (9 + 24 + 55 + 24) // 5)),
    "the same with min_count = 1: bin 1 is the valley": (_hist([0, 7, 3, 6, 11, 4]), 1, (1, 5, (14 + 9 + 24 + 55 + 24) // 5)),
    "peak in the last counted bin": (_hist([8, 3, 4, 5, 6]), 1, (2, 5, (6 + 12 + 20 + 30) // 5)),
    "a huge overflow bin is ignored": (_hist([8, 3, 9, 4], 1 << 60), 1, (2, 3, (6 + 27 + 16) // 3)),
    "an overflow bin above the last counted bin is no rise": (_hist([8, 3, 1], 1 << 60), 1, (0, 0, 0)),
    "bins = 2": (_hist([], 77), 1, (0, 0, 0)),
    "bins = 3": (_hist([5], 77), 1, (0, 0, 0)),
    "bins = 4: one rise": (_hist([5, 6], 77), 1, (1, 2, (5 + 12) // 2)),
    "min_count beyond the range": (_hist([1, 2, 3]), 9, (0, 0, 0)),
    "a sum beyond 2^64 does not wrap": (_hist([5, 1] + [0] * 997 + [1 << 60]), 1, (3, 1000, 1 << 60)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(name):
    h, min_count, want = CASES[name]
    assert cutoff_of(h, min_count) == want          # the restatement against the hand-worked answer
    assert spectrum_cutoff(h, min_count) == want


def test_null_out_pointers_are_skipped():
    h = _hist([9, 1, 7])
    v = C.c_uint32(99)
    assert L.lib().gk_spectrum_cutoff(L.ptr(h, C.c_uint64), len(h), 1, C.byref(v), None, None) == L.GK_OK
    assert v.value == 2
    assert L.lib().gk_spectrum_cutoff(L.ptr(h, C.c_uint64), len(h), 1, None, None, None) == L.GK_OK


def test_bad_arguments_are_errors_not_crashes():
    lib = L.lib()
    h = _hist([3, 1, 4])
    v, p, g = C.c_uint32(), C.c_uint32(), C.c_uint64()
    out = (C.byref(v), C.byref(p), C.byref(g))
    assert lib.gk_spectrum_cutoff(None, 5, 1, *out) == L.GK_E_INVALID
    for bins in (0, 1, (1 << 20) + 1, 0xffffffff):
        assert lib.gk_spectrum_cutoff(L.ptr(h, C.c_uint64), bins, 1, *out) == L.GK_E_INVALID
    assert lib.gk_spectrum_cutoff(L.ptr(h, C.c_uint64), len(h), 0, *out) == L.GK_E_INVALID       # no key has count 0
    assert b"gk_spectrum_cutoff" in lib.gk_last_error(None)
    n, occ, mx = C.c_uint64(), C.c_uint64(), C.c_uint32()
    assert lib.gk_map_spectrum(None, L.ptr(h, C.c_uint64), len(h), C.byref(n), C.byref(occ), C.byref(mx)) == L.GK_E_INVALID
    assert lib.gk_dist_spectrum(None, None, L.ptr(h, C.c_uint64), len(h), C.byref(n), C.byref(occ), C.byref(mx)) == L.GK_E_INVALID


def test_the_largest_histogram_is_accepted():
    h = np.zeros(1 << 20, np.uint64)
    h[1], h[40], h[(1 << 20) - 2] = 5, 9, 9
    assert spectrum_cutoff(h) == cutoff_of(h) == (2, 40, (40 * 9 + ((1 << 20) - 2) * 9) // 40)


def test_spectrum_of_folds_the_overflow():
    counts = [1, 1, 2, 5, 5, 9]
    assert spectrum_of(counts, 16).tolist() == [0, 2, 1, 0, 0, 2, 0, 0, 0, 1] + [0] * 6
    assert spectrum_of(counts, 6).tolist() == [0, 2, 1, 0, 0, 3]           # bins = max count - 3: 5 and 9 fold
    assert spectrum_of(counts, 2).tolist() == [0, 6]


def test_recorded_spectrum_pins_the_rule():
    """The oracle's table over a seeded 3 000-base genome at 30x with 1 % errors, k = 21 (tests/golden/spectrum/): the error
    bins fall from 13 275 singletons to a floor at counts 5-6, the coverage peak is at 18 and the estimate within 7 % of 3 000."""
    fx = json.load(open(GOLDEN))
    h = np.array(fx["hist"], np.uint64)
    assert len(h) == fx["bins"] and int(h.sum()) == fx["distinct"] and h[-1] == 0
    assert sum(c * int(x) for c, x in enumerate(h)) == fx["occurrences"]
    want = (fx["valley"], fx["peak"], fx["genome_size"])
    assert want == (5, 18, 3205)
    assert cutoff_of(h, fx["min_count"]) == want
    assert spectrum_cutoff(h, fx["min_count"]) == want
