"""The restatement of the owner routing (tests/route_ref.py) held to what can be checked WITHOUT a GPU:

  * its owner against gk_owner_of (host-callable) for every window of every shared case (tests/route_cases.py) and, at every key
    width and on both sides of m = 11 and of the 1-word / 2-word boundary, for homopolymers, (AC)n, reverse-complement
    palindromes and random k-mers — on both strands;
  * its record cutting against hand-written expectations: the P = 1 closed form, an owner sequence cut by hand, literal bytes;
  * that nothing past a read's length byte matters;
  * that the records of a case ARE the read set: parsed as `.bin` reads and counted by the naive oracle (oracle/pyref.py) they
    give the reads' table;
  * that the mixed regroup set has the run counts that make tests/test_route_gpu.py take both paths of the kernel."""
import random

import numpy as np
import pytest

import route_cases as RC
import route_ref as RR
from genome_amd import _lib as L
from oracle import pyref as R

M64 = (1 << 64) - 1
DESC_CAP = 4096          # csrc/gk_skm.hip: runs the descriptor list of one tile (or one group of 16 reads) holds


def lib_owner(k, x, P):
    return L.lib().gk_owner_of(k, x & M64, x >> 64, P)


def _value(seq):
    return sum("AGCT".index(c) << (2 * i) for i, c in enumerate(seq))


_SETS = sorted({("fixed", k, L_) for k, L_, _ in RC.CASES} | {("ragged", k, L_) for k, L_, _ in RC.RAGGED_CASES} | {("mixed", RC.MIXED_K, RC.MIXED_L)})


@pytest.mark.parametrize("kind,k,L_", _SETS)
def test_owner_of_every_window_of_every_case(kind, k, L_):
    cases = {"fixed": RC.CASES, "ragged": RC.RAGGED_CASES, "mixed": [(RC.MIXED_K, RC.MIXED_L, RC.MIXED_P)]}[kind]
    Ps = sorted({P for kk, LL, P in cases if (kk, LL) == (k, L_)})
    windows = 0
    for v, n in RC.view(kind, k, L_).reads():
        for p, best in enumerate(RR.window_minimizers(v, n, k)):
            x = (v >> (2 * p)) & RR.mask(k)
            for P in Ps:
                assert RR.owner_of_minimizer(best, P) == lib_owner(k, x, P), (k, L_, P, p)
            windows += 1
    assert windows > 200


@pytest.mark.parametrize("k", [2, 7, 10, 11, 12, 21, 31, 34, 35, 63, 64])
def test_owner_special_sequences_and_strand_symmetry(k):
    rnd = random.Random(k)
    seqs = [c * k for c in "AGCT"] + [("AC" * k)[:k], ("CA" * k)[:k], ("AGCT" * k)[:k], ("AT" * k)[:k]]
    for _ in range(6):                                    # x + rc(x) is its own reverse complement (even length)
        half = "".join(rnd.choice("AGCT") for _ in range(k // 2))
        seqs.append(half + R.rev_comp(half) if k % 2 == 0 else half + "A" + R.rev_comp(half))
    seqs += ["".join(rnd.choice("AGCT") for _ in range(k)) for _ in range(40)]
    long_read = "".join(rnd.choice("AGCT") for _ in range(k + 70))
    seqs += [long_read[i:i + k] for i in range(71)]
    seen = set()
    for s in seqs:
        x, rc = _value(s), _value(R.rev_comp(s))
        assert RR.rev_comp(x, k) == rc
        for P in (1, 2, 3, 16, 64):
            o = RR.owner_of_kmer(x, k, P)
            assert 0 <= o < P
            assert o == lib_owner(k, x, P) == lib_owner(k, rc, P) == RR.owner_of_kmer(rc, k, P), (s, P)
            seen.add((P, o))
    if k >= 7:                                            # (k = 2 has ten canonical k-mers)
        assert len({o for P, o in seen if P == 64}) > 16  # the owners spread
    # a window's owner inside a read is the owner of the window alone
    v = _value(long_read)
    for P in (3, 64):
        assert RR.window_owners(v, len(long_read), k, P) == [RR.owner_of_kmer(_value(long_read[i:i + k]), k, P) for i in range(71)]


def test_hash32_literals():
    """two values worked by hand from gk_device.h's constants, and the fixed point"""
    assert RR.hash32(0) == 0
    x = 1
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    assert RR.hash32(1) == x
    assert len({RR.hash32(i) for i in range(4096)}) == 4096            # a bijection does not collide


def _closed_form_lengths(n, k):
    """P = 1: the windows of every block of 64 in pieces of rmax, then the rest"""
    rmax, out = RR.max_run(k), []
    nk = max(0, n - k + 1)
    for b0 in range(0, nk, 64):
        b = min(64, nk - b0)
        out += [rmax] * (b // rmax) + ([b % rmax] if b % rmax else [])
    return out


def test_closed_form_example():
    assert RR.slot_bytes(31) == 16 and RR.slot_bytes(34) == 32 and RR.max_run(31) == 30 and RR.max_run(34) == 91 and RR.max_run(64) == 61
    assert _closed_form_lengths(150, 31) == [30, 30, 4, 30, 26]
    assert _closed_form_lengths(150, 34) == [64, 53] and _closed_form_lengths(255, 64) == [61, 3] * 3
    rnd = random.Random(5)
    v = rnd.getrandbits(300)
    reg, = RR.superkmer_records(RR.OffsetTable(bytes([150]) + v.to_bytes(38, "little"), [0, 39]), 31, 1)
    assert (reg.recs, reg.kmers) == (5, 120)
    assert sorted(r[0] - 30 for r in reg.rows) == [4, 26, 30, 30, 30]
    starts = {0: 30, 30: 30, 60: 4, 64: 30, 94: 26}
    want = sorted(bytes([wl + 30]) + ((v >> (2 * p)) & RR.mask(wl + 30)).to_bytes(15, "little") for p, wl in starts.items())
    assert reg.rows == want


@pytest.mark.parametrize("k,L_", [(31, 60), (31, 150), (31, 255), (34, 60), (34, 150), (34, 255)])
def test_one_owner_records_follow_from_the_lengths(k, L_):
    view = RC.fixed_set(k, L_)[1]
    reg, = RC.expected_records("fixed", k, L_, 1)
    want = sorted(wl + k - 1 for _, n in view.reads() for wl in _closed_form_lengths(n, k))
    assert sorted(r[0] for r in reg.rows) == want and reg.recs == len(want)
    assert reg.kmers == sum(max(0, n - k + 1) for _, n in view.reads())
    assert set(RC.edge_lengths(k, L_)) == {n for _, n in view.reads()}


def test_cut_of_a_hand_written_owner_sequence():
    owners = [0] * 3 + [1] * 70 + [0] * 2
    assert RR.pieces_of_read(owners, 31) == [(0, 0, 3), (1, 3, 30), (1, 33, 30), (1, 63, 1), (1, 64, 9), (0, 73, 2)]
    assert RR.runs_of_read(owners) == 4
    assert RR.pieces_of_read(owners, 34) == [(0, 0, 3), (1, 3, 61), (1, 64, 9), (0, 73, 2)]
    assert RR.pieces_of_read([5] * 64, 64) == [(5, 0, 61), (5, 61, 3)]
    assert RR.pieces_of_read([], 31) == [] and RR.pieces_of_read([2], 31) == [(2, 0, 1)]


def test_literal_records():
    def one(seq, k):
        body = _value(seq).to_bytes((len(seq) + 3) // 4, "little")
        reg, = RR.superkmer_records(RR.OffsetTable(bytes([len(seq)]) + body, [0, 1 + len(body)]), k, 1)
        return reg
    assert one("A" * 31, 31).rows == [bytes([31]) + bytes(15)]
    assert one("T" * 32, 31) == RR.Region([bytes([32]) + b"\xff" * 8 + bytes(7)], 1, 2)
    assert one("AGCTAGC", 7).rows == [bytes([7, 0xE4, 0x24]) + bytes(13)]
    assert one("G" * 34, 34).rows == [bytes([34]) + b"\x55" * 8 + b"\x05" + bytes(22)]
    assert one("AGCTAG", 7) == RR.Region([], 0, 0)                       # shorter than k
    # k = 7, 90 bases of T: 84 windows = blocks of 64 and 20; rmax = 54: pieces of 54, 10 and 20 windows
    reg = one("T" * 90, 7)
    assert [r[0] for r in reg.rows] == [16, 26, 60] and reg.kmers == 84
    assert reg.rows[2] == bytes([60]) + b"\xff" * 15 and reg.rows[0] == bytes([16]) + b"\xff" * 4 + bytes(11)


@pytest.mark.parametrize("k,L_,P", [(21, 150, 3), (34, 60, 16), (7, 60, 64)])
def test_bases_past_the_length_byte_are_ignored(k, L_, P):
    rec, view = RC.fixed_set(k, L_)
    other = rec.copy()
    changed = 0
    for r in range(len(other)):
        n = int(other[r, 0])
        if 2 * n < 8 * (other.shape[1] - 1):
            other[r, 1 + n // 4] ^= np.uint8((0xFF << (2 * (n % 4))) & 0xFF)          # every base past the last one, in its byte ...
            other[r, 2 + n // 4:] ^= np.uint8(0xA5)                                 # ... and every byte after it
            changed += 1
    assert changed > 100 and not np.array_equal(other, rec)
    view2 = RR.FixedStride(other.tobytes(), view.nreads, view.read_len)
    assert view2.reads() == view.reads()
    assert RR.superkmer_records(view2, k, P) == RC.expected_records("fixed", k, L_, P)
    assert RR.shard_keys(view2, k, P) == RC.expected_keys("fixed", k, L_, P)


@pytest.mark.parametrize("kind,k,L_,P", [("fixed", 31, 60, 64), ("fixed", 7, 60, 64), ("fixed", 34, 60, 16), ("ragged", 11, 60, 3), ("fixed", 64, 150, 3)])
def test_records_are_the_read_set(kind, k, L_, P):
    """every window exactly once: the records, read as `.bin` reads, have the reads' k-mer table (the naive oracle counts both);
    the routed keys are the same multiset"""
    view = RC.view(kind, k, L_)
    reads = ["".join("AGCT"[(v >> (2 * i)) & 3] for i in range(n)) for v, n in view.reads()]
    want = R.extract_filtered_kmers(reads, k, 0, do_filter=False).sorted_items()
    regions = RC.expected_records(kind, k, L_, P)
    stream = b"".join(row[:1 + (row[0] + 3) // 4] for reg in regions for row in reg.rows)
    nrec = sum(reg.recs for reg in regions)
    got = R.extract_filtered_kmers(R.reads_from_bin(stream, nrec), k, 0, do_filter=False).sorted_items()
    assert got == want and len(want) > 50
    assert sum(reg.kmers for reg in regions) == sum(c for _, c in want)
    keys, counts = RC.expected_keys(kind, k, L_, P)
    assert counts == [reg.kmers for reg in regions]
    table = {}
    for ks in keys:
        for lo, hi in ks:
            table[(lo, hi)] = table.get((lo, hi), 0) + 1
    assert table == {R.pack(s): c for s, c in want}
    # every key sits with the owner of its own k-mer, and no key is at two owners
    for p, ks in enumerate(keys):
        for lo, hi in ks[::17]:
            assert lib_owner(k, lo | (hi << 64), P) == p
    assert sum(len(set(ks)) for ks in keys) == len(table)


def test_mixed_set_takes_both_paths():
    """the first tile has more runs than the descriptor list holds, every group of 16 reads of it and every later tile fit"""
    k, P = RC.MIXED_K, RC.MIXED_P
    runs = [RR.runs_of_read(RR.window_owners(v, n, k, P)) for v, n in RC.mixed_set()[1].reads()]
    assert len(runs) == RC.NREADS == 200
    assert sum(runs[:64]) > DESC_CAP
    assert all(sum(runs[g:g + 16]) <= DESC_CAP for g in range(0, 64, 16))
    assert all(0 < sum(runs[t:t + 64]) <= DESC_CAP for t in range(64, RC.NREADS, 64))


def test_case_tables():
    assert {k for k, _, _ in RC.RAGGED_CASES} == set(RC.K_ALL) and {P for _, _, P in RC.RAGGED_CASES} == {1, 3, 16}
    for k, L_, _ in RC.RAGGED_CASES:
        buf, off, view, windows = RC.ragged_set(k, L_)
        reads = view.reads()
        assert len(reads) == RC.NREADS and int(off[-1]) == len(buf) and all(n < k for _, n in reads[64:128])
        assert windows == sum(max(0, n - k + 1) for _, n in reads) > 0
