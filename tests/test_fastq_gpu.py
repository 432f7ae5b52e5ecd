"""FASTQ -> `.bin` on the device (gk_fastq_*, genome_amd.fastq) held to the plain restatement tests/fastq_ref.py.  -m gpu.

Byte parity on seeded fuzzed FASTQ in one piece, in random pieces and split inside every "\\r\\n"; the same with a tiny device
chunk; every GK_E_FORMAT case with its record number; capacity and argument errors; gk_fastq_count against gk_map_count_reads of
the converted stream on both insert paths; max_pairs; the `.gz` path of convert2bin."""
import ctypes as C
import gzip
import random

import numpy as np
import pytest

import fastq_ref as ref
from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.fastq import FastqReader, convert2bin
from oracle import pyref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


SEQ_CHARS = b"ACGT" * 40 + b"N" * 4 + b"acgtn" + b".-*"


def fuzz_fastq(seed: int, nrec: int, split_at: int) -> bytes:
    """line lengths 0..300 (a mate stays <= 255), headers up to 10 KB, N / lowercase / punctuation, mixed terminators, quality
    lines longer and shorter than the sequence"""
    rnd = random.Random(seed)
    max_line = min(300, split_at + 255) if split_at else 255
    out = bytearray()
    prev_cr = False

    def line(content: bytes):
        nonlocal prev_cr
        eols = [b"\n", b"\r\n", b"\r"]
        if prev_cr and not content:
            eols = [b"\r\n", b"\r"]          # ("\r" + "\n" would merge into one terminator and swallow the empty line)
        eol = rnd.choice(eols)
        out.extend(content + eol)
        prev_cr = eol == b"\r"

    for _ in range(nrec):
        hl = rnd.choice([0, 3, 12, 40]) if rnd.random() > 0.03 else rnd.randint(0, 10000)
        line(b"@" + bytes(rnd.choice(b"abcXYZ:_ 0123/\xc3\xa9\x80") for _ in range(hl)))
        sl = rnd.choice([rnd.randint(0, max_line), max_line, rnd.randint(0, 40)])
        seq = bytes(rnd.choice(SEQ_CHARS) for _ in range(sl))
        line(seq)
        line(b"+" + (b"sep" if rnd.random() < 0.2 else b""))
        ql = max(0, min(max_line, sl + rnd.choice([0, 0, 0, -3, 5, -sl // 2, 40])))
        line(bytes(rnd.choice(b"!#?IJ5") for _ in range(ql)))
    if rnd.random() < 0.5 and out.endswith(b"\n") and not out.endswith(b"\r\n"):
        out = out[:-1]                       # an unterminated last line
    return bytes(out)


def random_pieces(data: bytes, rnd: random.Random):
    pieces, i = [], 0
    while i < len(data):
        n = rnd.choice([1, 1, 2, 3, 7, 64, 333, 4096, rnd.randint(1, 50000)])
        pieces.append(data[i:i + n])
        i += n
    return pieces or [b""]


def run_convert(ctx, pieces, split_at, k=23, max_pairs=0):
    """-> (bin bytes, stats, error or None)"""
    rd = FastqReader(ctx, split_at, k, max_pairs)
    out = bytearray()
    err = None
    try:
        for i, p in enumerate(pieces):
            out += rd.convert(p, last=(i == len(pieces) - 1))
    except L.GkError as e:
        err = e
    st = rd.stats()
    rd.close()
    return bytes(out), st, err


def check_parity(ctx, data, pieces, split_at, k=23, max_pairs=0):
    try:
        want, wst = ref.convert(data, split_at, k, max_pairs)
        werr = None
    except ref.FastqFormatError as e:
        werr = e.record
    got, st, err = run_convert(ctx, pieces, split_at, k, max_pairs)
    if werr is not None:
        assert err is not None and err.code == L.GK_E_FORMAT, err
        assert f"FASTQ record {werr}:" in str(err), (str(err), werr)
        return
    assert err is None, err
    assert got == want
    assert {x: st[x] for x in ("pairs", "short_pairs", "kmers")} == wst
    assert st["carried_bytes"] == 0
    assert st["text_bytes"] == len(data)


@pytest.mark.parametrize("split_at", [1, 36, 150, 0])
def test_byte_parity_fuzz(ctx, split_at):
    for seed in range(4):
        data = fuzz_fastq(1000 * split_at + seed, 300 if seed else 2, split_at)
        if split_at == 0 and (len(ref.lines(data)) // 4) % 2:
            data += ref.record(b"@x", b"ACGT", b"IIII")
        rnd = random.Random(seed)
        check_parity(ctx, data, [data], split_at)
        check_parity(ctx, data, random_pieces(data, rnd), split_at)
        if seed == 0:
            check_parity(ctx, data, [data[i:i + 1] for i in range(len(data))], split_at)     # byte by byte


def test_every_crlf_split_point(ctx):
    data = b"".join(ref.record(b"@r%d" % i, b"ACGTN"[i % 5:] + b"GATTACA" * (i % 4), b"I" * 40, eol=b"\r\n") for i in range(12))
    sites = [i for i in range(len(data) - 1) if data[i:i + 2] == b"\r\n"]
    assert len(sites) == 48
    for p in sites:
        check_parity(ctx, data, [data[:p + 1], data[p + 1:]], 4)


def test_internal_chunking(ctx):
    c = Context(0)
    try:
        c.set_option("test_fastq_chunk", 4096)
        for split_at in (36, 0):
            data = fuzz_fastq(77 + split_at, 600, split_at)
            if split_at == 0 and (len(ref.lines(data)) // 4) % 2:
                data += ref.record(b"@x", b"ACGT", b"IIII")
            check_parity(c, data, [data], split_at)
            check_parity(c, data, random_pieces(data, random.Random(5)), split_at)
        # a record much larger than a chunk (10 KB header) is carried over several chunks
        big = ref.record(b"@" + b"h" * 20000, b"ACGT" * 30, b"I" * 120) * 3 + ref.record(b"@", b"GG", b"II")
        check_parity(c, big, [big], 36)
    finally:
        c.close()


def format_error(ctx, data, split_at, record, pieces=None):
    rd = FastqReader(ctx, split_at, 23)
    pieces = pieces or [data]
    with pytest.raises(L.GkError) as e:
        for i, p in enumerate(pieces):
            rd.convert(p, last=(i == len(pieces) - 1))
    assert e.value.code == L.GK_E_FORMAT
    assert f"FASTQ record {record}:" in str(e.value), str(e.value)
    with pytest.raises(L.GkError) as e2:
        rd.convert(b"@r\nACGT\n+\nIIII\n")
    assert e2.value.code == L.GK_E_STATE
    rd.close()


def test_format_errors(ctx):
    good = ref.record(b"@r", b"ACGT", b"IIII")
    for tail in (b"@h\nACGT\n", b"@h\nACGT\n+\n", b"@h\nACGT\n+"):
        format_error(ctx, good * 3 + tail, 36, 3)
    format_error(ctx, good + ref.record(b"@r", b"A" * 256, b"I" * 256), 300, 1)
    format_error(ctx, good * 2 + ref.record(b"@r", b"A" * 300, b"I" * 300), 36, 2)          # mate 2 = 264 bases
    format_error(ctx, good + ref.record(b"@r", b"AC\xc3\xa9T", b"IIII"), 36, 1)
    format_error(ctx, good * 2 + ref.record(b"@r", b"ACGT", b"II\x80I"), 36, 2)
    format_error(ctx, good * 3, 0, 2)                                                   # interleaved, odd
    big = ref.record(b"@" + b"h" * (64 << 20), b"ACGT", b"IIII")
    format_error(ctx, good + big, 36, 1)
    format_error(ctx, good + big[:(64 << 20) + 100], 36, 1, pieces=[good + big[:(64 << 20) + 100], b"x"])


def test_format_error_keeps_the_good_pairs(ctx):
    good = [ref.record(b"@r", b"ACGTACGTAC"[: 4 + i], b"I" * 10) for i in range(5)]
    bad = ref.record(b"@r", b"AC\x99T", b"IIII")
    data = b"".join(good) + bad + b"".join(good)
    rd = FastqReader(ctx, 3, 23)
    out = np.zeros(len(data), np.uint8)
    n = C.c_size_t()
    rc = L.lib().gk_fastq_convert(rd.h, data, len(data), 1, out.ctypes.data, len(data), C.byref(n))
    assert rc == L.GK_E_FORMAT
    want, _ = ref.convert(b"".join(good), 3, 23)
    assert out[:n.value].tobytes() == want
    assert not out[n.value:].any()
    rd.close()


def test_capacity_then_retry(ctx):
    data = fuzz_fastq(5, 50, 36)
    want, _ = ref.convert(data, 36, 23)
    rd = FastqReader(ctx, 36, 23)
    head = data[:len(data) // 2]
    first = rd.convert(head)
    carried = rd.stats()["carried_bytes"]
    rest = data[len(data) // 2:]
    out = np.zeros(carried + len(rest), np.uint8)
    n = C.c_size_t()
    rc = L.lib().gk_fastq_convert(rd.h, rest, len(rest), 1, out.ctypes.data, carried + len(rest) - 1, C.byref(n))
    assert rc == L.GK_E_CAPACITY and n.value == 0
    assert rd.stats()["carried_bytes"] == carried
    second = rd.convert(rest, last=True)
    assert first + second == want
    rd.close()


def test_invalid_arguments(ctx):
    lib = L.lib()
    h = L.vp()
    assert lib.gk_fastq_create(ctx.h, -1, 23, 0, C.byref(h)) == L.GK_E_INVALID
    assert lib.gk_fastq_create(ctx.h, 36, 0, 0, C.byref(h)) == L.GK_E_INVALID
    assert lib.gk_fastq_create(ctx.h, 36, 256, 0, C.byref(h)) == L.GK_E_INVALID
    assert lib.gk_fastq_create(None, 36, 23, 0, C.byref(h)) == L.GK_E_INVALID
    n = C.c_size_t()
    assert lib.gk_fastq_convert(None, b"x", 1, 0, None, 0, C.byref(n)) == L.GK_E_INVALID
    rd = FastqReader(ctx, 36, 23)
    buf = np.zeros(16, np.uint8)
    assert lib.gk_fastq_convert(rd.h, None, 5, 0, buf.ctypes.data, 16, C.byref(n)) == L.GK_E_INVALID
    assert lib.gk_fastq_convert(rd.h, b"@r\n", 3, 0, None, 16, C.byref(n)) == L.GK_E_INVALID
    assert lib.gk_fastq_count(rd.h, None, b"@r\n", 3, 0, None) == L.GK_E_INVALID
    assert lib.gk_fastq_stats(None, None, None, None, None, None) == L.GK_E_INVALID
    assert rd.convert(b"@r\nACGT\n+\nIIII\n", last=True) == bytes([4, 0xD8, 0])         # (invalid calls did not poison the handle)
    with pytest.raises(L.GkError) as e:
        rd.convert(b"@r\n")
    assert e.value.code == L.GK_E_STATE                                                   # the input has ended
    rd.close()
    lib.gk_fastq_destroy(None)


def test_device_memory_is_pooled_and_released(ctx):
    c = Context(0)
    try:
        before = c.mem_stats()["live"]
        c.set_option("test_fastq_chunk", 2 << 20)
        rd = FastqReader(c, 150, 23)
        data = synth_fastq(20000, 150, seed=3)
        rd.convert(data, last=True)
        assert c.mem_stats()["live"] > before
        rd.close()
        assert c.mem_stats()["live"] == before
    finally:
        c.close()


def synth_fastq(npairs: int, mate_len: int, seed: int, n_rate: float = 0.002) -> bytes:
    """fixed-layout 2 x mate_len records with N injected (numpy, fast enough for 10^5 pairs)"""
    rng = np.random.default_rng(seed)
    L2 = 2 * mate_len
    hdr = b"@synthetic/1\n"
    rec_len = len(hdr) + L2 + 3 + L2 + 1
    a = np.empty((npairs, rec_len), np.uint8)
    a[:, :len(hdr)] = np.frombuffer(hdr, np.uint8)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (npairs, L2))]
    seq[rng.random((npairs, L2)) < n_rate] = ord("N")
    o = len(hdr)
    a[:, o:o + L2] = seq
    a[:, o + L2:o + L2 + 3] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, o + L2 + 3:o + 2 * L2 + 3] = ord("I")
    a[:, -1] = ord("\n")
    return a.tobytes()


def table(m):
    return [x.copy() for x in m.sorted_items()]


@pytest.mark.parametrize("k", [11, 23, 31, 35, 63, 64])
def test_count_parity(ctx, k):
    """k = 64 is the tagged table: the 36-base first mates hold no window there; the second mates, up to 164 bases behind the split
    of the 2 x 100-base lines, hold all of them (occ > 0)"""
    data = fuzz_fastq(k, 400, 36)
    data += (b"" if data.endswith((b"\n", b"\r")) else b"\n") + synth_fastq(3000, 100, seed=k)
    bin_ = FastqReader(ctx, 36, 23).convert(data, last=True)
    nreads = 2 * ref.convert(data, 36, 23)[1]["pairs"]
    for path in ("direct", "partitioned"):
        a, b = HipDNAMap(ctx, k, 1 << 12), HipDNAMap(ctx, k, 1 << 12)
        a.set_insert_path(path); b.set_insert_path(path)
        pairs, occ = a.count_fastq(data, split_at=36)
        occ_b = b.count_reads(bin_, nreads)
        assert pairs * 2 == nreads and occ == occ_b and occ > 0
        assert a.verify_checksum() == b.verify_checksum()
        for x, y in zip(table(a), table(b)):
            assert np.array_equal(x, y)
        a.close(); b.close()


def test_count_parity_large_partitioned_and_chunked(ctx):
    data = synth_fastq(200000, 150, seed=11)
    c = Context(0)
    try:
        rd = FastqReader(c, 150, 23)
        bin_ = rd.convert(data, last=True)
        rd.close()
        for k, chunk in ((31, 0), (35, 32 << 20)):
            c.set_option("test_fastq_chunk", chunk)      # one chunk cut into several framed batches; several chunks
            a, b = HipDNAMap(c, k, 0), HipDNAMap(c, k, 0)
            a.set_insert_path("partitioned"); b.set_insert_path("partitioned")
            a.set_max_batch_keys(1 << 20)          # window limit per insert: what the table has room for (>= 2^24) < 4.8e7 windows
            pairs, occ = a.count_fastq(data, split_at=150)
            assert pairs == 200000
            assert occ == b.count_reads(bin_, 2 * pairs)
            assert a.verify_checksum() == b.verify_checksum()
            assert a.stats()["partitioned_launches"] >= 3
            a.close(); b.close()
    finally:
        c.close()


def test_count_small_against_pyref(ctx):
    data = fuzz_fastq(9, 60, 36)
    bin_, st = ref.convert(data, 36, 23)
    k = 15
    reads = R.reads_from_bin(bin_, 2 * st["pairs"])
    want = R.extract_filtered_kmers(reads, k, 1, 1, do_filter=False)
    m = HipDNAMap(ctx, k, 1 << 10)
    m.count_fastq(data, split_at=36)
    lo, hi, cnt = m.sorted_items()
    got = sorted((dna.unpack(int(a), int(b), k), int(c)) for a, b, c in zip(lo, hi, cnt))
    assert got == sorted(want.items())
    m.close()


def test_max_pairs(ctx):
    data = fuzz_fastq(21, 200, 36)
    recs = ref.lines(data)
    for n in (1, 17, 150):
        head = data[:recs[4 * n - 1][2]]
        got, st, err = run_convert(ctx, [data], 36, 23, max_pairs=n)
        want, wst, _ = run_convert(ctx, [head], 36, 23)
        assert err is None and got == want == ref.convert(head, 36, 23)[0]
        assert st["pairs"] == wst["pairs"] == n and st["kmers"] == wst["kmers"]


def test_convert2bin_gz_matches_plain(ctx, tmp_path):
    data = fuzz_fastq(3, 500, 36)
    plain, gz = tmp_path / "r.fastq", tmp_path / "r.fastq.gz"
    plain.write_bytes(data)
    with gzip.open(gz, "wb") as f:
        f.write(data)
    s1 = convert2bin(ctx, plain, tmp_path / "a", piece_bytes=1000)
    s2 = convert2bin(ctx, gz, tmp_path / "b", piece_bytes=777)
    want, wst = ref.convert(data, 36, 23)
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes() == want
    assert s1 == s2 and s1["bin_bytes"] == len(want) and s1["text_bytes"] == len(data)
    assert {x: s1[x] for x in wst} == wst
    assert not (tmp_path / "a.bin.tmp").exists()
