"""The restatement of the FASTA check (tests/checkgraph_ref.py) against answers worked out by hand, and the new entry points'
null-handle errors.  No GPU."""
import ctypes as C

import checkgraph_ref as ref
from genome_amd import _lib as L

# 92 bytes, k = 4.  Lines (0-based; offset of the first byte):
#    0 @0  ACGTA            sequence before the first header: record 0
#    1 @6  >r1 desc         ends in "\r\n"
#    2 @16 ACGTAC           ends in a lone "\r"
#    3 @23 GTNAC
#    4 @29 ac               lowercase: invalid; a short line
#    5 @32                  empty
#    6 @33 >r2              an empty record
#    7 @37 >r3              two headers in a row
#    8 @41 TTTTT
#    9 @47 >r4
#   10 @51 GGGGCCCCAAAATTTTGGGGCCCCAAAATTTT<0x80>ACGT
#   11 @89 CGT              no trailing newline; a short line
TEXT = (b"ACGTA\n>r1 desc\r\nACGTAC\rGTNAC\nac\n\n>r2\n>r3\nTTTTT\n>r4\n"
        b"GGGGCCCCAAAATTTTGGGGCCCCAAAATTTT\x80ACGT\nCGT")
PRESENT = {"ACGT", "CGTA", "GTAC", "TTTT", "GGGG", "CCCC"}


def test_lines_are_readline_lines():
    assert len(TEXT) == 92
    assert [o for o, _ in ref.lines(TEXT)] == [0, 6, 16, 23, 29, 32, 33, 37, 41, 47, 51, 89]
    assert ref.lines(b"") == [] and ref.lines(b"A\n") == [(0, b"A")] and ref.lines(b"A\n\n") == [(0, b"A"), (2, b"")]
    assert ref.lines(b"A\r\nC\rG") == [(0, b"A"), (3, b"C"), (5, b"G")]


def test_per_line_mode_by_hand():
    """line 0: ACGT CGTA found; line 2: ACGT CGTA GTAC found; line 3: both windows hold N; line 8: TTTT twice; line 10: 29 windows
    of the 32-base run, of which GGGG (0, 16), CCCC (4, 20), TTTT (12, 28) are found, then ACGT after the 0x80 byte."""
    st, missing = ref.check(TEXT, 4, True, PRESENT)
    assert st == dict(lines=12, records=5, bases=63, valid_bases=59, windows=37, found=14, missing=23, covered_bases=44, short_lines=2)
    assert len(missing) == 23
    assert missing[0] == (52, 10, 1, 149, 0)            # GGGC: 1 | 1<<2 | 1<<4 | 2<<6
    assert missing[1] == (53, 10, 2, 165, 0)            # GGCC


def test_joined_mode_by_hand():
    """record r1 = ACGTAC GTNAC ac joined: ACGT CGTA GTAC found, TACG (line 2, column 3) missing, ACGT (crossing the "\\r") found,
    the rest holds N or lowercase; record r4's tail ACGT CGT joined: ACGT found, CGTC GTCG TCGT missing."""
    st, missing = ref.check(TEXT, 4, False, PRESENT)
    assert st == dict(lines=12, records=5, bases=63, valid_bases=59, windows=42, found=15, missing=27, covered_bases=46, short_lines=2)
    assert missing[0] == (19, 2, 3, 99, 0)              # TACG: 3 | 0<<2 | 2<<4 | 1<<6
    assert missing[1] == (52, 10, 1, 149, 0)
    assert missing[-1] == (87, 10, 36, 219, 0)          # TCGT starts on line 10 and ends on line 11


def test_contig_stats_by_hand():
    assert ref.contig_stats([5, 300, 201, 200, 1000, 250], 200) == dict(count=4, sum=1751, median=300, n50=1000, max=1000)
    assert ref.contig_stats([10, 10, 10, 10], 0) == dict(count=4, sum=40, median=10, n50=10, max=10)
    assert ref.contig_stats([1, 2, 3, 4], 0) == dict(count=4, sum=10, median=3, n50=3, max=4)       # 4 + 3 = 7, 2 * 7 >= 10
    assert ref.contig_stats([7, 9], 9) == dict(count=0, sum=0, median=0, n50=0, max=0)


def test_null_handles_are_errors_not_crashes():
    lib = L.lib()
    v = [C.c_uint64() for _ in range(9)]
    assert lib.gk_fasta_check_feed(None, b"ACGT", 4, 1) == L.GK_E_INVALID
    assert lib.gk_fasta_check_stats(None, *[C.byref(x) for x in v]) == L.GK_E_INVALID
    assert lib.gk_fasta_check_missing(None, None, None, None, None, None, 0, C.byref(v[0])) == L.GK_E_INVALID
    assert lib.gk_fasta_check_last_ms(None, (C.c_float * 4)()) == L.GK_E_INVALID
    h = L.vp()
    assert lib.gk_fasta_check_create(None, None, 0, 0, C.byref(h)) == L.GK_E_INVALID and not h
    assert lib.gk_graph_contig_stats(None, 200, *[C.byref(x) for x in v[:5]]) == L.GK_E_INVALID
    lib.gk_fasta_check_destroy(None)
