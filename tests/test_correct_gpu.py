"""gk_reads_correct / gk_reads_correct_dev on the device against the restatement of their rule (tests/correct_ref.py): the output
byte for byte and all ten statistics (-m gpu).

Random cases: per k one seeded sequencing run (RUNS: genome, reads of 100 bases from either strand, 1 % substitutions), its
restatement computed once and shared by every table that holds the same counts: the table counting leaves (12-byte slots at
k <= 31, 24-byte at k >= 34), the graph layout deleteAll leaves (16-byte slots at k <= 31; the cutoff is below `solid`, so the same
windows are weak), and a table filled with verbatim keys in both orientations.  The seeds and thresholds were fixed with the
restatement alone: in every run it reports corrected > 0, ambiguous + unresolved > 0 and skipped > 0 (asserted below), so that
equality with it cannot hide a category the kernel never takes.  At k = 5 every 5-mer of a random genome is solid, so that run
draws its genome from a skewed base distribution.
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from oracle import pyref as R

import correct_ref as X
import spectrum_ref as SP
from test_correct_cpu import HAND_CASES, K as HAND_K, SOLID as HAND_SOLID

pytestmark = pytest.mark.gpu
KS = [5, 21, 31, 34, 47, 63, 64]
# k -> (seed, genome length, reads, the fixed threshold, base weights of the genome A G C T)
RUNS = {
    5: (1, 2000, 2000, 40, (0.48, 0.03, 0.03, 0.46)),
    21: (21, 3000, 2000, 3, None),
    31: (31, 3000, 2000, 3, None),
    34: (34, 2500, 2000, 4, None),
    47: (47, 4000, 3000, 3, None),
    63: (63, 2000, 2000, 3, None),
    64: (64, 2000, 2000, 5, None),
}
READ_LEN = 100


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def run_of(k):
    """-> (reads, counts, `.bin` stream): computed once per k"""
    seed, glen, nreads, _solid, weights = RUNS[k]
    rnd = random.Random(seed)
    genome = "".join(rnd.choices("AGCT", weights=weights, k=glen))
    reads = []
    for _ in range(nreads):
        p = rnd.randrange(glen - READ_LEN + 1)
        t = genome[p:p + READ_LEN]
        if rnd.random() < 0.5:
            t = R.rev_comp(t)
        reads.append("".join(rnd.choice([b for b in "AGCT" if b != c]) if rnd.random() < 0.01 else c for c in t))
    return reads, X.count_reads(reads, k), dna.reads_to_bin(reads)


def valley_of(counts):
    """what solid="auto" must choose: the valley of the spectrum (tests/spectrum_ref.py), 3 when there is none"""
    valley = SP.cutoff_of(SP.spectrum_of(list(counts.values()), 4096))[0]
    return valley if valley else 3


@functools.lru_cache(maxsize=None)
def expected(k, solid):
    reads, counts, raw = run_of(k)
    out, st = X.correct_bin(counts, raw, len(reads), k, solid)
    # every category is taken, or equality below would prove nothing about it
    assert st["corrected"] > 0 and st["ambiguous"] + st["unresolved"] > 0 and st["skipped"] > 0, st
    assert st["weak_runs"] == st["corrected"] + st["ambiguous"] + st["unresolved"] + st["skipped"]
    return out, st


def table_of(ctx, k, kind, below):
    """a table whose window counts are run_of(k)'s wherever they matter: below `below` a count may read lower (deleteAll)"""
    reads, counts, raw = run_of(k)
    if kind == "counted":
        m = HipDNAMap(ctx, k, 0)
        m.set_insert_path("partitioned")
        m.count_reads(raw, len(reads))
        st = m.stats()
        assert st["slot_bytes"] == (12 if k <= 31 else 24)
    elif kind == "filtered":
        m = HipDNAMap(ctx, k, 0)
        m.count_reads(raw, len(reads))
        m.deleteAll_lt(below)
        assert m.stats()["slot_bytes"] == (16 if k <= 31 else 24)
    else:
        # verbatim keys: a third of the k-mers as stored, a third reverse-complemented, a third split over both orientations
        assert kind == "verbatim"
        keys, cnt = [], []
        for i, (s, c) in enumerate(counts.items()):
            rc = R.rev_comp(s)
            if i % 3 == 0 or rc == s:
                keys.append(s); cnt.append(c)
            elif i % 3 == 1:
                keys.append(rc); cnt.append(c)
            elif c >= 2:
                keys += [s, rc]; cnt += [c - c // 2, c // 2]
            else:
                keys.append(rc); cnt.append(c)
        m = HipDNAMap(ctx, k, 2 * len(keys) + 64)
        lo, hi = dna.pack_many(keys)
        m.update_inc((lo[:64], hi[:64]))                                  # gk_map_update_inc itself, then what is left of the counts
        left = np.array(cnt, np.int32)
        left[:64] -= 1
        more = left > 0
        m.add_counts(lo[more], hi[more], left[more])
        assert m.stats()["noncanonical_keys"] is True and m.size() == len(keys)
    return m


def check_stats(got, want):
    assert {name: got[name] for name in X.STATS} == want


@pytest.mark.parametrize("kind", ["counted", "filtered", "verbatim"])
@pytest.mark.parametrize("k", KS)
def test_random_run_fixed_threshold(ctx, k, kind):
    reads, counts, raw = run_of(k)
    solid = RUNS[k][3]
    want, want_st = expected(k, solid)
    m = table_of(ctx, k, kind, min(solid, 2))
    before = m.verify_checksum()
    got, st = m.correct_reads(raw, len(reads), solid)
    assert got == want
    check_stats(st, want_st)
    assert m.verify_checksum() == before and before[1] == 0               # the map is never changed
    # correcting the output again changes nothing
    again, st2 = m.correct_reads(got, len(reads), solid)
    assert again == got and st2["corrected"] == 0 and st2["reads_changed"] == 0
    m.close()


@pytest.mark.parametrize("k", KS)
def test_random_run_threshold_from_the_valley(ctx, k):
    reads, counts, raw = run_of(k)
    solid = valley_of(counts)
    want, want_st = expected(k, solid)
    m = table_of(ctx, k, "counted", 0)
    got, st = m.correct_reads(raw, len(reads), "auto")
    assert st["solid"] == solid and st["solid_auto"] == bool(SP.cutoff_of(SP.spectrum_of(list(counts.values()), 4096))[0])
    assert got == want
    check_stats(st, want_st)
    m.close()


def fill(ctx, k, counts):
    m = HipDNAMap(ctx, k, 2 * len(counts) + 64)
    if counts:
        lo, hi = dna.pack_many(list(counts))
        m.add_counts(lo, hi, np.array(list(counts.values()), np.int32))
    return m


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0].split(":")[0] for c in HAND_CASES])
def test_hand_cases_through_the_device(ctx, case):
    _name, counts, reads, want, want_st = case
    m = fill(ctx, HAND_K, counts)
    got, st = m.correct_reads(dna.reads_to_bin(reads), len(reads), HAND_SOLID)
    assert R.reads_from_bin(got, len(reads)) == want and got == dna.reads_to_bin(want)
    check_stats(st, want_st)
    m.close()


@pytest.mark.parametrize("nreads", [1, 63, 64, 65, 64 * 5 + 1])
def test_tile_edges(ctx, nreads):
    k = 31
    reads, counts, _ = run_of(k)
    raw = dna.reads_to_bin(reads[:nreads])
    want, want_st = X.correct_bin(counts, raw, nreads, k, 3)
    m = table_of(ctx, k, "counted", 0)
    got, st = m.correct_reads(raw, nreads, 3)
    assert got == want
    check_stats(st, want_st)
    m.close()


def ragged_stream(k):
    """records of every kind in one stream: 0-length, shorter than k, exactly k, 255 bases, and the run's reads cut at random"""
    reads, counts, _ = run_of(k)
    rnd = random.Random(7 * k)
    long = (reads[0] + reads[1] + reads[2])[:255]
    out = ["", reads[3][:k - 1], reads[4][:k], long]
    for r in reads[5:400]:
        out.append(r[:rnd.randrange(0, READ_LEN + 1)])
    out += ["", long[::-1], reads[401]]
    return out, counts


@pytest.mark.parametrize("k", [21, 47])
def test_ragged_host_stream(ctx, k):
    reads, counts = ragged_stream(k)
    raw = bytearray(dna.reads_to_bin(reads))
    # nonzero padding bits in the last byte of every record that has any
    pos = 0
    for r in reads:
        nb = (len(r) + 3) // 4
        if len(r) % 4:
            raw[pos + nb] |= (0xFF << (2 * (len(r) % 4))) & 0xFF
        pos += 1 + nb
    raw = bytes(raw)
    want, want_st = X.correct_bin(counts, raw, len(reads), k, 3)
    assert want_st["corrected"] > 0 and want_st["short"] >= 3 and want_st["skipped"] > 0
    assert R.reads_from_bin(want, len(reads)) != reads
    m = table_of(ctx, k, "counted", 0)
    got, st = m.correct_reads(raw, len(reads), 3)
    assert got == want
    check_stats(st, want_st)
    # in several chunks (the test build's staging limit): the same bytes
    ctx.set_option("test_max_stage", 4096)
    try:
        got2, st2 = m.correct_reads(raw, len(reads), 3)
    finally:
        ctx.set_option("test_max_stage", 0)
    assert got2 == want
    check_stats(st2, want_st)
    # in place: bin_out == bin_host
    buf = np.frombuffer(raw, np.uint8).copy()
    stats = np.zeros(10, np.uint64)
    L.check(L.lib().gk_reads_correct(m.h, L.ptr(buf, C.c_uint8), buf.size, len(reads), 3, L.ptr(buf, C.c_uint8), L.ptr(stats, C.c_uint64)), ctx.h)
    assert buf.tobytes() == want and [int(x) for x in stats] == [want_st[n] for n in X.STATS]
    # a truncated stream is refused before anything is written
    out = np.full(buf.size, 0xAB, np.uint8)
    rc = L.lib().gk_reads_correct(m.h, L.ptr(np.frombuffer(raw, np.uint8).copy(), C.c_uint8), len(raw) - 3, len(reads), 3, L.ptr(out, C.c_uint8), None)
    assert rc == L.GK_E_FORMAT and (out == 0xAB).all()
    m.close()


def test_every_record_its_own_chunk(ctx):
    """a staging limit of one byte: every piece is a single record, so both staging areas and the copy stream's event
    alternate on every record, and every record comes back from the area it went to"""
    k = 21
    reads, counts = ragged_stream(k)
    reads = reads[:40]
    assert len(reads) == 40 and len({len(r) for r in reads}) >= 5
    raw = dna.reads_to_bin(reads)
    m = table_of(ctx, k, "counted", 0)
    want, want_st = m.correct_reads(raw, len(reads), 3)          # unchunked
    assert want != raw and want_st["corrected"] > 0
    assert (want, {n: want_st[n] for n in X.STATS}) == X.correct_bin(counts, raw, len(reads), k, 3)
    ctx.set_option("test_max_stage", 1)
    try:
        got, st = m.correct_reads(raw, len(reads), 3)
    finally:
        ctx.set_option("test_max_stage", 0)
    assert got == want
    check_stats(st, {n: want_st[n] for n in X.STATS})
    m.close()


def fixed_records(reads, read_len):
    """records at the fixed stride 1 + ceil(read_len / 4); the bytes a shorter record leaves are filled with 0xEE"""
    stride = 1 + (read_len + 3) // 4
    rec = np.full((len(reads), stride), 0xEE, np.uint8)
    for i, r in enumerate(reads):
        b = np.frombuffer(dna.reads_to_bin([r]), np.uint8)
        rec[i, :b.size] = b
    return rec


def expected_fixed(counts, rec, reads, k, solid):
    fixed, st = X.correct(counts, reads, k, solid)
    want = rec.copy()
    for i, (a, b) in enumerate(zip(reads, fixed)):
        for p, (x, y) in enumerate(zip(a, b)):
            if x != y:
                want[i, 1 + p // 4] = (int(want[i, 1 + p // 4]) & ~(3 << (2 * (p % 4)))) | (R.BASES.index(y) << (2 * (p % 4)))
    return want, st


@pytest.mark.parametrize("k", [31, 64])
def test_dev_form_in_place_and_out_of_place(ctx, k):
    """read_len = 99 (no multiple of 4), shorter records inside the stride, 64 * 3 + 5 records"""
    reads, counts, _ = run_of(k)
    rnd = random.Random(k)
    mine = [r[:99] if i % 7 else r[:rnd.randrange(0, 99)] for i, r in enumerate(reads[:64 * 3 + 5])]
    rec = fixed_records(mine, 99)
    want, want_st = expected_fixed(counts, rec, mine, k, 3)
    assert want_st["corrected"] > 0 and want_st["short"] > 0 and (want != rec).any()
    m = table_of(ctx, k, "counted", 0)
    nbytes = rec.size
    d_in, d_out = ctx.alloc(nbytes + 64), ctx.alloc(nbytes + 64 + 16)
    ctx.upload(d_in, rec.reshape(-1))
    # out of place, `out` aligned as `in` and 5 bytes off that alignment; the input stays as it was
    for shift in (0, 5):
        ctx.upload(d_out, np.full(nbytes + 64 + 16, 0x77, np.uint8))
        st = m.correct_reads_dev(d_in, len(mine), 99, 3, d_out + shift)
        check_stats(st, want_st)
        got = ctx.download(d_out, nbytes + 64 + 16)
        assert (got[shift:shift + nbytes].reshape(rec.shape) == want).all()
        assert (got[:shift] == 0x77).all() and (got[shift + nbytes:] == 0x77).all()       # nothing beside the records is written
        assert (ctx.download(d_in, nbytes).reshape(rec.shape) == rec).all()
    # in place
    st = m.correct_reads_dev(d_in, len(mine), 99, 3)
    check_stats(st, want_st)
    assert (ctx.download(d_in, nbytes).reshape(rec.shape) == want).all()
    # idempotent through the device
    st = m.correct_reads_dev(d_in, len(mine), 99, 3)
    assert st["corrected"] == 0 and (ctx.download(d_in, nbytes).reshape(rec.shape) == want).all()
    # errors: solid = 0, a partly overlapping output, an oversized length byte
    stride = rec.shape[1]
    assert L.lib().gk_reads_correct_dev(m.h, d_in, len(mine), 99, 0, d_in, None) == L.GK_E_INVALID
    assert L.lib().gk_reads_correct_dev(m.h, d_in, len(mine) - 1, 99, 3, d_in + stride, None) == L.GK_E_INVALID
    assert L.lib().gk_reads_correct_dev(m.h, d_in, len(mine), 99, 3, None, None) == L.GK_E_INVALID
    assert L.lib().gk_reads_correct(m.h, None, 10, 1, 3, None, None) == L.GK_E_INVALID
    bad = rec.copy()
    bad[70, 0] = 100                                                       # one more than read_len: still inside the stride
    ctx.upload(d_in, bad.reshape(-1))
    assert L.lib().gk_reads_correct_dev(m.h, d_in, len(mine), 99, 3, d_out, None) == L.GK_E_FORMAT
    st = m.correct_reads_dev(d_in, 64, 99, 3, d_out)                      # the flag does not stick
    assert st["reads"] == 64
    ctx.free(d_in); ctx.free(d_out); m.close()


def test_two_corrections_inside_one_byte(ctx):
    """Two corrected bases p1 < p2 of one record need a solid window between their runs, which holds neither: p2 >= p1 + k + 1.
    Inside one byte (four bases) that is k = 2 and nothing else: bases 4 and 7 of a 12-base read, windows 3, 4 and 6, 7, both
    interior runs of k, window 5 solid.  The table holds the one 2-mer AA."""
    k = 2
    g = "A" * 12
    counts = {R.canon("AA"): 9}
    bad = g[:4] + "G" + g[5:7] + "G" + g[8:]
    want, want_st = X.correct(counts, [bad], k, 2)
    assert want == [g] and want_st["corrected"] == 2 and want_st["weak_runs"] == 2 and want_st["weak_windows"] == 4
    m = fill(ctx, k, counts)
    raw = dna.reads_to_bin([bad])
    got, st = m.correct_reads(raw, 1, 2)
    assert got == dna.reads_to_bin([g]) and [i for i in range(len(raw)) if raw[i] != got[i]] == [2]
    check_stats(st, want_st)
    m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_empty_and_cleared_maps_copy_the_stream(ctx, k):
    reads, counts, raw = run_of(k)
    n = 200
    raw = dna.reads_to_bin(reads[:n])
    want_st = dict.fromkeys(X.STATS, 0)
    want_st.update(reads=n, windows=n * (READ_LEN - k + 1), weak_windows=n * (READ_LEN - k + 1), weak_runs=n, skipped=n)
    new = HipDNAMap(ctx, k, 1 << 12)
    got, st = new.correct_reads(raw, n, 1)
    assert got == raw
    check_stats(st, want_st)
    new.count_reads(raw, n)
    assert new.correct_reads(raw, n, 1)[1]["weak_windows"] == 0            # its own reads: every window was seen
    new.clear()
    got, st = new.correct_reads(raw, n, 1)
    assert got == raw
    check_stats(st, want_st)
    assert new.size() == 0
    new.close()
