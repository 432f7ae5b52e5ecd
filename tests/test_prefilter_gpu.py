"""Exact two-pass singleton pre-filter against the CPU oracle (-m gpu).

The reference has no such stage on its hot path (its BloomFilter, S/ds/BloomFilter.scala, is unused), so the
checker is the property the design promises: for rounds >= 2 the table after deleteAll(v < rounds)
(FreqFilter.scala:55) is bit-identical to the plain path's — i.e. to the oracle's — and before the filter
every k-mer seen at least twice already holds its exact count while every other entry has count 1.
"""
import contextlib
import random

import numpy as np
import pytest

import prefilter_cases as PC
from genome_amd import dna, synth
from genome_amd._lib import GK_E_FORMAT, GkError
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData, extractFilteredKmers
from genome_amd.prefilter import HipPrefilter
from oracle import oracle as O
from oracle import pyref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def same(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)


def check_prefiltered_table(m, ref):
    """m = table after pass 2, ref = oracle PMap after plain counting."""
    lo, hi, cnt = ref.export_sorted()
    want = {(int(a), int(b)): int(c) for a, b, c in zip(lo, hi, cnt)}
    glo, ghi, gcnt = m.sorted_items()
    got = {(int(a), int(b)): int(c) for a, b, c in zip(glo, ghi, gcnt)}
    assert set(got) <= set(want)
    for key, c in want.items():
        if c >= 2:
            assert got.get(key) == c, (key, c, got.get(key))       # exact count, never missing
        else:
            assert got.get(key, 1) == 1                             # absent, or a false positive with count 1
    return sum(1 for c in want.values() if c == 1), sum(1 for key, c in want.items() if c == 1 and key in got)


@pytest.mark.parametrize("k", [5, 21, 31, 47, 64])
def test_ragged_host_stream(ctx, k):
    rnd = random.Random(100 + k)
    g = "".join(rnd.choice("AGCT") for _ in range(3000))
    reads = []
    for _ in range(600):
        ln = rnd.randint(max(1, k - 3), min(255, k + 90))
        st = rnd.randrange(0, len(g) - ln + 1)
        r = g[st:st + ln]
        if rnd.random() < 0.5:
            r = R.rev_comp(r)
        reads.append("".join(c if rnd.random() >= 0.03 else rnd.choice([x for x in "AGCT" if x != c]) for c in r))
    reads += ["", "AG", "".join(rnd.choice("AGCT") for _ in range(255))]
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, len(reads))
    for expected in (1, ref.size(), 50 * ref.size()):          # absurdly small, right, generous filter
        pf = HipPrefilter(ctx, k, expected)
        pf.add_reads(binb, len(reads))
        m = HipDNAMap(ctx, k, 64)
        looked, admitted = pf.count_reads(m, binb, len(reads))
        assert looked == occ and admitted <= occ
        st = pf.stats()
        assert st["windows_added"] == occ and st["seen_once"] + st["seen_twice_or_more"] <= st["buckets"]
        singles, fp = check_prefiltered_table(m, ref)
        if expected >= 50 * ref.size() and singles > 200 and k >= 21:
            assert fp < singles // 4, "a generous filter must keep most singletons out"
        for rounds in (2, 3, 5):
            m.deleteAll_lt(rounds)
            r2 = O.PMap(k, 1); r2.count_reads(binb, len(reads)); r2.delete_lt(rounds)
            same(m.sorted_items(), r2.export_sorted())
        m.close(); pf.close()


@pytest.mark.parametrize("k,L_", [(21, 100), (31, 150), (55, 150)])
def test_device_records_in_chunks(ctx, k, L_):
    """Pass 1 fed in two chunks, pass 2 in one call: only the union matters."""
    n, G, e, cid = 4000, 30000, 0.02, 11
    rec = synth.reads_mode_g(n, L_, G, e, cid)
    d = ctx.alloc(rec.size + 64)
    ctx.synth_reads(d, n, L_, "G", cid, 0, G, e)
    ref = O.PMap(k, 1)
    occ = ref.count_reads(rec.tobytes(), n)
    pf = HipPrefilter(ctx, k, ref.size())
    half = n // 3
    pf.add_reads_dev(d, half, L_)
    pf.add_reads_dev(d + half * rec.shape[1], n - half, L_)
    m = HipDNAMap(ctx, k, 1000)
    looked, admitted = pf.count_reads_dev(m, d, n, L_)
    assert looked == occ == n * (L_ - k + 1)
    singles, fp = check_prefiltered_table(m, ref)
    assert m.size() < ref.size(), "the filter kept nothing out"
    m.deleteAll_lt(3)
    ref.delete_lt(3)
    same(m.sorted_items(), ref.export_sorted())
    m.close(); pf.close(); ctx.free(d)


def test_freqfilter_entry_point_and_errors(ctx):
    rnd = random.Random(5)
    g = "".join(rnd.choice("AGCT") for _ in range(2000))
    reads = [g[s:s + 80] for s in (rnd.randrange(0, len(g) - 80) for _ in range(400))]
    data = PairedEndData(len(reads) // 2, dna.reads_to_bin(reads))
    a = extractFilteredKmers(data, 21, 3, ctx=ctx)
    b = extractFilteredKmers(data, 21, 3, ctx=ctx, prefilter_distinct=5000)
    same(a.sorted_items(), b.sorted_items())
    a.close(); b.close()
    with pytest.raises(ValueError):
        extractFilteredKmers(data, 21, 1, ctx=ctx, prefilter_distinct=5000)
    # k mismatch between filter and table
    from genome_amd._lib import GkError
    pf = HipPrefilter(ctx, 21, 100)
    m = HipDNAMap(ctx, 31)
    with pytest.raises(GkError):
        pf.count_reads(m, data.bin, 10)
    with pytest.raises(GkError):
        HipPrefilter(ctx, 33, 100)
    m.close(); pf.close()


# ---- the filter held to its restatement, exactly ---------------------------------------------------------------------------------
# tests/prefilter_ref.py says which bucket a k-mer goes to, what the counters hold after pass 1 and which table pass 2 leaves;
# tests/test_prefilter_cpu.py holds that restatement to hand cases and to the theorem; tests/prefilter_cases.py has the inputs.
# Everything below is integer equality.
_oracle = {}


def oracle_filtered(case, k):
    """{rounds: the oracle's table after plain counting and deleteAll(v < rounds)} for rounds 2, 3, 5 (computed once)"""
    if (case, k) not in _oracle:
        reads = PC.reads(case, k)
        ref = O.PMap(k, 1)
        ref.count_reads(dna.reads_to_bin(reads), len(reads))
        out = {}
        for rounds in (2, 3, 5):
            ref.delete_lt(rounds)
            out[rounds] = ref.export_sorted()
        _oracle[case, k] = out
    return _oracle[case, k]


@contextlib.contextmanager
def options(ctx, **kw):
    try:
        for name, v in kw.items():
            ctx.set_option(name, v)
        yield
    finally:
        for name in kw:
            ctx.set_option(name, 0)


def upload(ctx, data: bytes):
    d = ctx.alloc(len(data) + 64)
    ctx.upload(d, np.frombuffer(data, np.uint8))
    return d


def check_exact(case, k, m, pf, looked, admitted):
    """the whole pass-2 table, the counters and the call's figures against the restatement; then deleteAll against the oracle"""
    res = PC.restated(case, k)
    wlo, whi, wcnt = res.sorted_table()
    glo, ghi, gcnt = m.sorted_items()
    assert glo.shape == wlo.shape, (glo.size, wlo.size)
    assert np.array_equal(glo, wlo) and np.array_equal(ghi, whi) and np.array_equal(gcnt, wcnt)
    assert (looked, admitted) == (res.windows, res.admitted)
    st = pf.stats()
    assert (st["buckets"], st["seen_once"], st["seen_twice_or_more"], st["windows_added"]) == \
           (res.buckets, res.seen_once, res.seen_twice_or_more, res.windows)
    want = oracle_filtered(case, k)
    for rounds in (2, 3, 5):
        m.deleteAll_lt(rounds)
        same(m.sorted_items(), want[rounds])


def host_run(ctx, case, k, check=True):
    """both passes over the case's reads as ONE host stream -> (sorted table, looked, admitted, echo after pass 1, echo after pass 2)"""
    reads = PC.reads(case, k)
    binb = dna.reads_to_bin(reads)
    pf = HipPrefilter(ctx, k, PC.expected_distinct(case, k))
    m = HipDNAMap(ctx, k, 64)
    try:
        pf.add_reads(binb, len(reads))
        e1 = pf.chunks()
        looked, admitted = pf.count_reads(m, binb, len(reads))
        e2 = pf.chunks()
        items = m.sorted_items()
        if check:
            check_exact(case, k, m, pf, looked, admitted)
        return items, looked, admitted, e1, e2
    finally:
        m.close(); pf.close()


def dev_run(ctx, case, k, read_len, d=None, split=None):
    """both passes through the `_dev` entry points over records of one stride -> (looked, admitted, echo)"""
    reads = PC.reads(case, k)
    own = d is None
    if own:
        d = upload(ctx, PC.fixed_stride_records(reads, read_len))
    pf = HipPrefilter(ctx, k, PC.expected_distinct(case, k))
    m = HipDNAMap(ctx, k, 64)
    try:
        if split:                                                    # pass 1 in two calls
            pf.add_reads_dev(d, split, read_len)
            pf.add_reads_dev(d + split * PC.record_bytes(read_len), len(reads) - split, read_len)
        else:
            pf.add_reads_dev(d, len(reads), read_len)
        looked, admitted = pf.count_reads_dev(m, d, len(reads), read_len)
        echo = pf.chunks()
        items = m.sorted_items()
        check_exact(case, k, m, pf, looked, admitted)
        return items, looked, admitted, echo
    finally:
        m.close(); pf.close()
        if own:
            ctx.free(d)


# (a) every key form
@pytest.mark.parametrize("k", PC.KS_ALL)
def test_exact_ragged_host_stream(ctx, k):
    """k = 2: the 255-base reads have 254 windows and a pass-2 tile holds 32 reads; k = 34: 222 windows of two words, 18 reads.
    400 012 buckets: no power of two, and the last counter word is only partly in use."""
    _, _, _, e1, e2 = host_run(ctx, "ragged", k)
    assert (e1["host_offsets"], e2["host_offsets"], e2["host_fixed"], e2["pass2_launches"]) == (1, 2, 0, 1)


@pytest.mark.parametrize("k", PC.KS_ALL)
def test_exact_device_records_of_255_bases(ctx, k):
    _, _, _, echo = dev_run(ctx, "fixed_255", k, 255, split=33)
    assert echo["dev_pass2"] == 1


@pytest.mark.parametrize("k", PC.KS_ALL)
def test_exact_device_records_of_k_bases(ctx, k):
    """one window per read: 47 tiles of pass 2, each with at most 64 keys to park"""
    dev_run(ctx, "fixed_k", k, k)


# (b) collisions at the smallest filter the library makes
@pytest.mark.parametrize("k", PC.KS_COLLIDE)
def test_exact_collisions_at_the_smallest_filter(ctx, k):
    """expected_distinct = 1 -> 262 144 buckets.  1900 reads of 100 bases from both strands of a 40 000-base genome, 0.8 %
    substitutions; random.Random(3101) at k = 31, random.Random(4701) at k = 47 (tests/prefilter_cases.py: collide).
    Populations by the restatement (k-mers of count >= 2 / singletons admitted by a collision / singletons kept out):
      k = 31:  29 624 / 7852 / 28 108  of 65 584 distinct k-mers, 133 000 windows
      k = 47:  21 361 / 9336 / 33 554  of 64 251 distinct k-mers, 102 600 windows
    Each is at least 1000, so equality with the restatement shows each branch of pass 2 a thousand times."""
    res = PC.restated("collide", k)
    assert res.buckets == 262144 and res.multi >= 1000 and res.single_admitted >= 1000 and res.single_rejected >= 1000
    host_run(ctx, "collide", k)


# (c) host chunking
@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_host_chunks_that_grow(ctx, k):
    """Cut by bytes ("test_max_stage" = 1000) into offset-table chunks; the fifth chunk has more bytes and more windows than any
    before it, a later one more records (tests/prefilter_cases.py: grow), so the staging area, the key buffer and the offset
    table are each replaced in the middle of the stream."""
    whole = host_run(ctx, "grow", k, check=False)
    with options(ctx, test_max_stage=PC.GROW_STAGE, test_prefilter_chunk_windows=1 << 20):
        items, looked, admitted, e1, e2 = host_run(ctx, "grow", k)
    same(items, whole[0])
    assert (looked, admitted) == whole[1:3] and whole[4]["host_offsets"] == 2
    assert e1["host_fixed"] == e2["host_fixed"] == 0 and e1["host_offsets"] >= 5 and e2["host_offsets"] == 2 * e1["host_offsets"]
    assert e2["pass2_launches"] == e1["host_offsets"]


@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_host_chunks_cut_by_windows(ctx, k):
    """a stage far larger than the stream, 1500 windows per pass-2 chunk: pass 1 is one chunk, pass 2 many"""
    whole = host_run(ctx, "by_windows", k, check=False)
    with options(ctx, test_max_stage=1 << 20, test_prefilter_chunk_windows=1500):
        items, looked, admitted, e1, e2 = host_run(ctx, "by_windows", k)
    same(items, whole[0])
    assert (looked, admitted) == whole[1:3]
    assert e1["host_offsets"] == 1 and e2["host_offsets"] - 1 >= PC.restated("by_windows", k).windows // 1500 >= 5
    assert e2["host_fixed"] == 0 and e2["pass2_launches"] == e2["host_offsets"] - 1


@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_host_chunks_mixed(ctx, k):
    """Fixed-stride prefixes and offset-table chunks in one stream (tests/prefilter_cases.py: mixed): two fixed-stride chunks of
    5000 records, one offset-table chunk (the 1700 left of that run, the ragged records and the head of the next run), one
    fixed-stride chunk of 4500 records without a window — pass 2 launches nothing for it —, the closing run as the remainder."""
    whole = host_run(ctx, "mixed", k, check=False)
    with options(ctx, test_max_stage=PC.mixed_stage(k), test_prefilter_chunk_windows=1 << 22):
        items, looked, admitted, e1, e2 = host_run(ctx, "mixed", k)
    same(items, whole[0])
    assert (looked, admitted) == whole[1:3]
    assert (e1["host_fixed"], e1["host_offsets"]) == (4, 1) and (e2["host_fixed"], e2["host_offsets"]) == (8, 2)
    assert e2["pass2_launches"] == 4


@pytest.mark.parametrize("chunked", [False, True])
def test_truncated_host_streams(ctx, chunked):
    """a stream cut inside record r, and one whose record r starts past the end: GK_E_FORMAT naming r from either pass, and the
    handles go on working"""
    k, case = 21, "grow"
    reads = PC.reads(case, k)
    binb = dna.reads_to_bin(reads)
    r = 300
    start = len(dna.reads_to_bin(reads[:r]))
    cuts = {"inside record %d" % r: (binb[:start + 3], r + 1), "record %d starts past the end" % r: (binb[:start], r + 1)}
    opts = dict(test_max_stage=PC.GROW_STAGE, test_prefilter_chunk_windows=2000) if chunked else {}
    with options(ctx, **opts):
        pf = HipPrefilter(ctx, k, PC.expected_distinct(case, k))
        m = HipDNAMap(ctx, k, 64)
        try:
            if not chunked:                                   # one chunk: the framing fails before anything is launched
                for text, (cut, n) in cuts.items():
                    with pytest.raises(GkError, match=text) as ei:
                        pf.add_reads(cut, n)
                    assert ei.value.code == GK_E_FORMAT
                assert pf.stats()["windows_added"] == 0 and pf.stats()["seen_once"] == 0
            pf.add_reads(binb, len(reads))
            for text, (cut, n) in cuts.items():
                m2 = HipDNAMap(ctx, k, 64)
                try:
                    with pytest.raises(GkError, match=text) as ei:
                        pf.count_reads(m2, cut, n)
                    assert ei.value.code == GK_E_FORMAT
                finally:
                    m2.close()
            looked, admitted = pf.count_reads(m, binb, len(reads))
            check_exact(case, k, m, pf, looked, admitted)
        finally:
            m.close(); pf.close()
        if chunked:                                           # pass 1 fails in a later chunk: the error names r, the handle answers
            for text, (cut, n) in cuts.items():
                pf = HipPrefilter(ctx, k, 1)
                try:
                    with pytest.raises(GkError, match=text) as ei:
                        pf.add_reads(cut, n)
                    assert ei.value.code == GK_E_FORMAT and pf.chunks()["host_offsets"] >= 5
                    assert 0 < pf.stats()["windows_added"] < PC.restated(case, k).windows
                finally:
                    pf.close()


# (d) the pass-2 chunk loop of the `_dev` entry point
def dev_loop_run(ctx, k):
    rec = PC.dev_records()
    d = upload(ctx, rec.tobytes())
    try:
        return dev_run(ctx, "dev_loop", k, PC.DEV_L, d=d, split=PC.DEV_N // 3)
    finally:
        ctx.free(d)


@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_device_pass2_chunk_loop(ctx, k):
    """4000 records of 100 bases (26 bytes) in chunks of 999: the second chunk starts 25 974 bytes in, 6 past a multiple of 16"""
    assert (PC.DEV_CHUNK_READS * PC.record_bytes(PC.DEV_L)) % 16 != 0
    whole = dev_loop_run(ctx, k)
    assert whole[3]["dev_pass2"] == 1
    with options(ctx, test_prefilter_chunk_windows=PC.DEV_CHUNK_READS * (PC.DEV_L - k + 1) + 1):
        items, looked, admitted, echo = dev_loop_run(ctx, k)
    same(items, whole[0])
    assert (looked, admitted) == whole[1:3]
    assert echo["dev_pass2"] == echo["pass2_launches"] == 5


# (e) the three launches under "test_max_grid"
@pytest.mark.parametrize("grid", [1, 3])
def test_grid_caps(ctx, grid):
    """every workgroup takes several tiles (pass 1: 64 reads each; pass 2: as many as park) and, with one workgroup, the census of
    gk_prefilter_stats sums all the counter words alone; grid_cap_uses rises by one per pre-filter launch and by nothing else"""
    with options(ctx, test_max_grid=grid):
        for k in (31, 47):
            reads = PC.reads("ragged", k)
            binb = dna.reads_to_bin(reads)
            pf = HipPrefilter(ctx, k, PC.expected_distinct("ragged", k))
            m = HipDNAMap(ctx, k, 64)
            try:
                u0 = ctx.grid_cap_uses()
                pf.add_reads(binb, len(reads))
                u1 = ctx.grid_cap_uses()
                looked, admitted = pf.count_reads(m, binb, len(reads))
                u2 = ctx.grid_cap_uses()
                pf.stats()
                u3 = ctx.grid_cap_uses()
                assert (u1 - u0, u2 - u1, u3 - u2) == (1, 1, 1)
                check_exact("ragged", k, m, pf, looked, admitted)
            finally:
                m.close(); pf.close()
        for k in PC.KS_CHUNK:
            u0 = ctx.grid_cap_uses()
            with options(ctx, test_prefilter_chunk_windows=PC.DEV_CHUNK_READS * (PC.DEV_L - k + 1) + 1):
                _, _, _, echo = dev_loop_run(ctx, k)
            assert echo["dev_pass2"] == 5
            # two calls of pass 1, five chunks of pass 2, one census (check_exact)
            assert ctx.grid_cap_uses() - u0 == 2 + 5 + 1


# (f) untrusted length bytes, and records shorter than the declared length
@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_short_device_records_count_their_own_windows(ctx, k):
    """declared read_len = 100, every seventh record shorter (0, 1, k - 1, k, 60 .. 99 bases): legal, and `looked`, `admitted` and
    windows_added count the windows the records have, not nreads x (100 - k + 1)"""
    res = PC.restated("short_records", k)
    assert res.windows < len(PC.reads("short_records", k)) * (100 - k + 1)
    dev_run(ctx, "short_records", k, 100, split=100)


@pytest.mark.parametrize("k", PC.KS_CHUNK)
def test_length_byte_above_the_declared_length_is_refused(ctx, k):
    case, L_ = "short_records", 100
    reads = PC.reads(case, k)
    stride = PC.record_bytes(L_)
    good = PC.fixed_stride_records(reads, L_)
    bad = bytearray(good)
    for r, ln in ((0, 101), (77, 180), (len(reads) - 1, 255)):
        bad[r * stride] = ln
    d_bad, d_good = upload(ctx, bytes(bad)), upload(ctx, good)
    pf = HipPrefilter(ctx, k, PC.expected_distinct(case, k))
    m = HipDNAMap(ctx, k, 64)
    try:
        with pytest.raises(GkError, match="length byte") as ei:
            pf.add_reads_dev(d_bad, len(reads), L_)
        assert ei.value.code == GK_E_FORMAT
        with pytest.raises(GkError, match="length byte") as ei:
            pf.count_reads_dev(m, d_bad, len(reads), L_)
        assert ei.value.code == GK_E_FORMAT
    finally:
        m.close(); pf.close()
    try:
        dev_run(ctx, case, k, L_, d=d_good)                   # the context is as good as new: fresh handles, exact result
    finally:
        ctx.free(d_bad); ctx.free(d_good)
