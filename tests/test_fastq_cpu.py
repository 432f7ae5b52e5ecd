"""The FASTQ conversion rules (include/genome_amd.h, "FASTQ") pinned to hand-worked answers through the plain restatement
tests/fastq_ref.py, which the GPU tests then hold the device converter to."""
import pytest

from fastq_ref import FastqFormatError, convert, lines, record


def rec(seq, qual=None, h=b"@r", eol=b"\n"):
    return record(h, seq, qual if qual is not None else b"I" * len(seq), eol=eol)


def test_pack_and_lengths_by_hand():
    # split at 4: mate 1 = ACGT (A0 C2 G1 T3 -> 0b11_01_10_00 = 0xD8), mate 2 = GA (G1 A0 -> 0x01)
    out, st = convert(rec(b"ACGTGA"), split_at=4, k=2)
    assert out == bytes([4, 0xD8, 2, 0x01])
    assert st == {"pairs": 1, "short_pairs": 0, "kmers": 3 + 1}


def test_n_and_lowercase_end_a_mate():
    out, _ = convert(rec(b"ACNTacgt"), split_at=4, k=2)
    assert out == bytes([2, 0x08, 0])               # "AC" then lowercase "a" ends mate 2 at once
    out, _ = convert(rec(b"AGcT") + rec(b"T"), split_at=0, k=2)
    assert out == bytes([2, 0x04, 1, 0x03])


def test_quality_shorter_than_sequence():
    out, _ = convert(rec(b"ACGTACGT", b"III"), split_at=4, k=2)
    assert out == bytes([3, 0x18, 0])               # mate 1 = zip with 3 quality chars; mate 2 has no quality left
    out, _ = convert(rec(b"ACGTACGT", b"IIIIII"), split_at=4, k=2)
    assert out == bytes([4, 0xD8, 2, 0x18 & 0x0F])


def test_short_and_empty_sequences():
    out, st = convert(rec(b"ACG") + rec(b""), split_at=36, k=2)
    assert out == bytes([3, 0x18, 0]) + bytes([0, 0])
    assert st == {"pairs": 2, "short_pairs": 2, "kmers": 2}


def test_terminators_agree():
    body = [(b"ACGTTGCA", b"IIIIIIII"), (b"GGGNAAA", b"IIIIIII"), (b"", b"")]
    outs = set()
    for eol in (b"\n", b"\r\n", b"\r"):
        out, st = convert(b"".join(rec(s, q, eol=eol) for s, q in body), split_at=4, k=3)
        outs.add((out, tuple(sorted(st.items()))))
    assert len(outs) == 1
    assert lines(b"a\r\nb\rc\n\nd") == [(b"a", 0, 3), (b"b", 3, 5), (b"c", 5, 7), (b"", 7, 8), (b"d", 8, 9)]
    assert lines(b"a\n") == [(b"a", 0, 2)]


def test_unterminated_last_line():
    assert convert(b"@r\nACGT\n+\nIIII", split_at=2, k=2) == convert(rec(b"ACGT"), split_at=2, k=2)


def test_end_of_input():
    good = rec(b"ACGT")
    assert convert(good + b"@lone header\n", 2, 2) == convert(good, 2, 2)
    assert convert(good + b"@lone header", 2, 2) == convert(good, 2, 2)
    for tail in (b"@h\nACGT\n", b"@h\nACGT\n+\n"):
        with pytest.raises(FastqFormatError) as e:
            convert(good + tail, 2, 2)
        assert e.value.record == 1


def test_long_mate_and_high_bytes():
    with pytest.raises(FastqFormatError) as e:
        convert(rec(b"ACGT") + rec(b"A" * 256), split_at=300, k=2)
    assert e.value.record == 1
    out, _ = convert(rec(b"A" * 255), split_at=300, k=2)
    assert out[0] == 255 and len(out) == 1 + 64 + 1
    out, _ = convert(rec(b"A" * 255 + b"N" + b"A" * 10), split_at=300, k=2)
    assert out[0] == 255
    with pytest.raises(FastqFormatError) as e:
        convert(rec(b"ACGT") + rec(b"ACGT", b"II\xc3\xa9"), 2, 2)
    assert e.value.record == 1


def test_interleaved():
    out, st = convert(rec(b"ACGT") + rec(b"GGA"), split_at=0, k=3)
    assert out == bytes([4, 0xD8, 3, 0x05]) and st == {"pairs": 1, "short_pairs": 0, "kmers": 2 + 1}
    with pytest.raises(FastqFormatError) as e:
        convert(rec(b"ACGT") + rec(b"GGA") + rec(b"T"), split_at=0, k=3)
    assert e.value.record == 2


def test_k_statistics_and_max_pairs():
    data = rec(b"A" * 40 + b"C" * 30) + rec(b"A" * 10)
    _, st = convert(data, split_at=36, k=23)
    # record 0: mates 36 and 34 -> 14 + 12 windows; record 1: mates 10 and 0 -> short
    assert st == {"pairs": 2, "short_pairs": 1, "kmers": 26}
    out1, st1 = convert(data, split_at=36, k=23, max_pairs=1)
    assert out1 == convert(rec(b"A" * 40 + b"C" * 30), 36, 23)[0] and st1["pairs"] == 1
