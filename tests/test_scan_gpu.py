"""gk_scan.h's scan_counts on its own (the test-build hook gk_test_scan_counts) against numpy.cumsum over uint64, exactly, at
every edge of its three levels: a thread's 16 elements and a wave inside k_scan_fill, a workgroup trip and a SCAN_CHUNK of 4096,
and the 1024 chunks beyond which the single workgroup of k_scan_sums_excl gives every thread per = ceil(nchunks / 1024) > 1
chunks.  Every offset list of the library comes from this scan; the stages that use it reach per > 1 only at production sizes.
Both overloads run; the result (and the caller's scratch, sized to exactly n / 4096 + 2 words) lies between guard words."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd.dnamap import Context

pytestmark = pytest.mark.gpu

CHUNK = 4096                 # SCAN_CHUNK
WG = 1024                    # threads of k_scan_sums_excl: per = ceil(nchunks / WG)
FF = 0xFFFFFFFF

SMALL = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097, 2 * CHUNK, 2 * CHUNK + 1]
LARGE = [WG * CHUNK - 1, WG * CHUNK, WG * CHUNK + 1,         # 1024 chunks, and the first size with 1025: per goes 1 -> 2
         1025 * CHUNK,                                       # per = 2: thread 512 has one chunk, the threads after it none
         2047 * CHUNK + 5,                                   # per = 2, 2048 chunks: the last thread's second chunk holds 5 elements
         2049 * CHUNK + 4095,                                # per = 3, 2050 chunks: thread 683 has one chunk, 340 threads idle
         3 * WG * CHUNK + 37 * CHUNK + 1234]                 # per = 4, ragged


def _per(n):
    return ((n + CHUNK - 1) // CHUNK + WG - 1) // WG


def _spikes(n):
    """name -> position of the single 0xFFFFFFFF, for the positions that exist among n elements"""
    per = _per(n)
    pos = {"spike_first": 0, "spike_last": n - 1,
           "spike_chunk0_last": CHUNK - 1, "spike_chunk1_first": CHUNK, "spike_chunk1_last": 2 * CHUNK - 1,
           "spike_chunk1024_first": WG * CHUNK}
    if per >= 2:
        # thread 511 owns the chunks 511 * per .. 511 * per + per - 1: the first element of its SECOND chunk
        pos["spike_second_chunk_of_thread"] = (511 * per + 1) * CHUNK
    return {name: p for name, p in pos.items() if 0 <= p < n}


FILLS = ("zeros", "ones", "ff", "random")
CASES = [(n, c) for n in SMALL for c in FILLS + tuple(_spikes(n))] + [(n, c) for n in LARGE for c in ("ff", "random") + tuple(_spikes(n))]


def _counts(n, content):
    if content == "zeros":
        return np.zeros(n, np.uint32)
    if content == "ones":
        return np.ones(n, np.uint32)
    if content == "ff":
        return np.full(n, FF, np.uint32)
    a = np.zeros(n, np.uint32)
    if content == "random":                   # mostly zeros, one element in 64 or so large
        rng = np.random.default_rng(n)
        idx = rng.integers(0, max(n, 1), n // 64 + min(n, 1))
        a[idx] = rng.integers(1 << 31, 1 << 32, len(idx), dtype=np.uint64).astype(np.uint32)
        return a
    a[_spikes(n)[content]] = FF
    return a


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _scan(ctx, counts, via_scratch):
    n = len(counts)
    out = np.full(n + 1, 0x5555555555555555, np.uint64)
    hits = C.c_uint64(1 << 40)
    L.check(L.test_hook("gk_test_scan_counts")(ctx.h, L.ptr(counts, C.c_uint32), n, via_scratch, L.ptr(out, C.c_uint64), C.byref(hits)), ctx.h)
    return out, hits.value


def test_cases_cover_the_second_level():
    """the sizes reach per = 1, 2, 3 and 4, and every spike position occurs at some size"""
    assert {_per(n) for n in SMALL} == {0, 1} and [_per(n) for n in LARGE] == [1, 1, 2, 2, 2, 3, 4]
    assert {c for _, c in CASES} == set(FILLS) | set(_spikes(LARGE[-3]))


@pytest.mark.parametrize("n,content", CASES, ids=[f"{n}-{c}" for n, c in CASES])
def test_scan_counts_is_the_exclusive_cumsum(ctx, n, content):
    counts = _counts(n, content)
    want = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, dtype=np.uint64, out=want[1:])
    if content == "ff" and n >= 2:
        assert int(want[2]) > 1 << 32 and (n < WG * CHUNK - 1 or int(want[n]) > 1 << 44)
    for via_scratch in (0, 1):
        got, hits = _scan(ctx, counts, via_scratch)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"via_scratch={via_scratch}: {bad.size} offsets differ, the first at {int(bad[0])} (chunk {int(bad[0]) // CHUNK}): "
                               f"{int(got[bad[0]])} != {int(want[bad[0]])}")
        assert hits == 0, f"via_scratch={via_scratch}: {hits} guard words changed"


def test_null_arguments_are_invalid(ctx):
    f = L.test_hook("gk_test_scan_counts")
    a, out, hits = np.ones(4, np.uint32), np.zeros(5, np.uint64), C.c_uint64()
    pa, po = L.ptr(a, C.c_uint32), L.ptr(out, C.c_uint64)
    assert f(None, pa, 4, 0, po, C.byref(hits)) == L.GK_E_INVALID
    assert f(ctx.h, None, 4, 0, po, C.byref(hits)) == L.GK_E_INVALID
    assert f(ctx.h, pa, 4, 0, None, C.byref(hits)) == L.GK_E_INVALID
    assert f(ctx.h, pa, 4, 1, po, None) == L.GK_E_INVALID
    assert f(ctx.h, None, 0, 0, po, C.byref(hits)) == L.GK_OK and out[0] == 0 and hits.value == 0
