"""The restatement of the contig rule (tests/contigs_ref.py) against answers written out by hand.  No GPU.

k = 3.  Codes A0 G1 C2 T3, complement = 3 - code.
  AAGCA   codes 0 0 1 2 0, reverse complement TGCTT = 3 1 2 3 3: forward; its twin TGCTT is reverse.
  AGATCT  = AGA ++ rc(AGA): its own reverse complement: self_twin.
  ACGA    4 bases: short under min_len = 5.
"""
import random

import pytest

from oracle import pyref as R

import contigs_ref as CR

FWD = ("AAG", "GCA", "CA")
REV = ("TGC", "CTT", "TT")
SELF = ("AGA", "TCT", "TCT")
SHORT = ("ACG", "CGA", "A")
EDGES = [SELF, SHORT, REV, FWD]                              # (any order: the records come out by id)
IDS = [99, 100, 10, 9]


def stats(**kw):
    return {**dict.fromkeys(CR.STATS, 0), **kw}


def test_classes_of_the_hand_made_paths():
    assert CR.classify("AAGCA") == "forward" and CR.classify("TGCTT") == "reverse"
    assert CR.classify("AGATCT") == "self_twin"
    assert CR.classify("ACGA", 5) == "short" and CR.classify("ACGA", 4) != "short"
    assert CR.classify("AGA") == "forward"                   # odd n: the middle base differs from its complement at the latest
    for p in ("AAGCA", "AGATCT", "ACGA"):
        assert CR.rev_comp_codes([CR.CODE[c] for c in p]) == [CR.CODE[c] for c in R.rev_comp(p)]


def test_one_strand_one_line():
    text, st = CR.contigs(EDGES, IDS, min_len=5, line_width=0, strands=1)
    assert text == b">e9 len=5\nAAGCA\n>e99 len=6\nAGATCT\n"
    assert st == stats(live_edges=4, short=1, forward=1, self_twin=1, reverse=1, records=2, bases=11, text_bytes=34)


def test_both_strands_width_one():
    text, st = CR.contigs(EDGES, IDS, min_len=5, line_width=1, strands=2)
    assert text == (b">e9 len=5\nA\nA\nG\nC\nA\n" b">e10 len=5\nT\nG\nC\nT\nT\n" b">e99 len=6\nA\nG\nA\nT\nC\nT\n")
    assert st == stats(live_edges=4, short=1, forward=1, self_twin=1, reverse=1, records=3, bases=16, text_bytes=len(text))
    # the self_twin edge once, under either selection; a record is the same text under both
    one, _ = CR.contigs(EDGES, IDS, min_len=5, line_width=1, strands=1)
    assert one.count(b">e99 ") == 1 and text.count(b">e99 ") == 1
    assert one == text.replace(b">e10 len=5\nT\nG\nC\nT\nT\n", b"")


def test_width_that_divides_n_leaves_no_empty_line():
    text, st = CR.contigs(EDGES, IDS, min_len=0, line_width=3, strands=1)
    assert text == b">e9 len=5\nAAG\nCA\n>e99 len=6\nAGA\nTCT\n>e100 len=4\nACG\nA\n"
    assert st["short"] == 0 and st["forward"] == 2 and st["records"] == 3
    text, _ = CR.contigs([FWD], [9], line_width=5)
    assert text == b">e9 len=5\nAAGCA\n"
    text, _ = CR.contigs([SELF], [0], line_width=2)
    assert text == b">e0 len=6\nAG\nAT\nCT\n"
    assert b"\n\n" not in b"".join(CR.contigs(EDGES, IDS, line_width=w, strands=2)[0] for w in range(0, 8))


@pytest.mark.parametrize("n, eid, head", [(9, 9, b">e9 len=9\n"), (10, 10, b">e10 len=10\n"), (99, 99, b">e99 len=99\n"), (100, 100, b">e100 len=100\n"),
                                          (10, 9, b">e9 len=10\n"), (99, 100, b">e100 len=99\n")])
def test_ids_and_lengths_across_a_digit_boundary(n, eid, head):
    path = "A" * (n - 1) + "C"                               # 0 .. 0 2 against 1 3 .. 3: forward
    text, st = CR.contigs([(path[:3], path[-3:], path[3:])], [eid], line_width=0)
    assert text == head + path.encode() + b"\n"
    assert st["text_bytes"] == len(head) + n + 1 and st["bases"] == n and st["forward"] == 1


def test_cov_field():
    assert CR.cov_field(201, 20) == " cov=10.05"             # hundredths with a leading zero
    assert CR.cov_field(7, 100) == " cov=0.07"
    assert CR.cov_field(2, 3) == " cov=0.66"                 # floor, not rounded
    assert CR.cov_field(999, 100) == " cov=9.99" and CR.cov_field(1000, 100) == " cov=10.00"
    assert CR.cov_field(2 ** 63, 1) == " cov=%d.00" % 2 ** 63            # 100 * sum passes 2^64
    assert CR.cov_field(0, 5) == " cov=0.00"


def test_cov_from_a_table_with_a_window_missing():
    # the windows of AAGCA: AAG, AGC, GCA; the table holds two of them
    counts = {R.canon("AAG"): 10, R.canon("GCA"): 5}
    text, st = CR.contigs([FWD], [9], counts=counts, line_width=0)
    assert text == b">e9 len=5 cov=5.00\nAAGCA\n"
    assert st["missing_windows"] == 1 and st["text_bytes"] == len(text)
    counts[R.canon("AGC")] = 16
    assert CR.contigs([FWD], [9], counts=counts, line_width=0)[0] == b">e9 len=5 cov=10.33\nAAGCA\n"
    # missing windows are summed over the records only
    _, st = CR.contigs([FWD, REV], [9, 10], counts={}, strands=1)
    assert st["missing_windows"] == 3
    _, st = CR.contigs([FWD, REV], [9, 10], counts={}, strands=2)
    assert st["missing_windows"] == 6


def test_parse_reads_back_what_was_written():
    text, _ = CR.contigs(EDGES, IDS, counts={}, line_width=2, strands=2)
    assert CR.parse(text) == [(9, 5, "0.00", "AAGCA"), (10, 5, "0.00", "TGCTT"), (99, 6, "0.00", "AGATCT"), (100, 4, "0.00", "ACGA")]


def test_a_strand_closed_edge_set_has_as_many_forward_as_reverse():
    rnd = random.Random(11)
    k = 5
    edges = set()
    for _ in range(300):
        path = "".join(rnd.choice("AGCT") for _ in range(k + rnd.randint(1, 30)))
        if rnd.random() < 0.1:
            x = path[:len(path) // 2 + 1]
            path = x + R.rev_comp(x)
        for p in (path, R.rev_comp(path)):
            edges.add((p[:k], p[-k:], p[k:]))
    edges = sorted(edges)
    _, st = CR.contigs(edges, list(range(len(edges))), strands=1)
    assert st["forward"] == st["reverse"] > 100 and st["self_twin"] > 5
    assert st["records"] == st["forward"] + st["self_twin"] and st["live_edges"] == len(edges)
    _, st2 = CR.contigs(edges, list(range(len(edges))), strands=2)
    assert st2["records"] == len(edges) and {n: st2[n] for n in CR.STATS[:5]} == {n: st[n] for n in CR.STATS[:5]}
