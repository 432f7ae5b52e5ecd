"""The restatement of gk_reads_correct's rule (tests/correct_ref.py) against answers worked out by hand on tiny cases (k = 5), its
own properties on random reads, and the library's side of the bargain that needs no GPU: both symbols exported and bound.

The hand cases share one 24-base sequence G whose 5-mers are all distinct on both strands (checked below), each counted 10 times;
solid = 3.  A read is G[2:22] (20 bases, 16 windows) with bases replaced: a wrong
base at position e makes exactly the windows max(0, e-4) .. min(15, e) weak.  HAND_CASES is also what the device is run on
(tests/test_correct_gpu.py).
"""
import ctypes as C
import os
import random

import pytest

from genome_amd import _lib as L
from oracle import pyref as R

import correct_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SOLID = 5, 3
G = "TGTAGTTGCGGTCATAGCACTGCC"
READ = G[2:22]


def g_counts():
    return {R.canon(G[i:i + K]): 10 for i in range(len(G) - K + 1)}


def sub(s, *edits):
    s = list(s)
    for pos, base in edits:
        assert s[pos] != base
        s[pos] = base
    return "".join(s)


def other(base, skip=""):
    """a base that is neither `base` nor in `skip`: the first in A, G, C, T order"""
    return [b for b in "AGCT" if b != base and b not in skip][0]


def stats(**kw):
    st = dict.fromkeys(X.STATS, 0)
    st.update(kw)
    return st


def hand_cases():
    """-> list of (name, counts, reads, expected reads, expected stats)"""
    c = g_counts()
    cases = []

    def one_error(name, e, weak):
        bad = sub(READ, (e, other(READ[e])))
        cases.append((name, c, [bad], [READ], stats(reads=1, windows=16, weak_windows=weak, weak_runs=1, corrected=1, reads_changed=1)))

    one_error("error at 0: head run of one window, p = b = 0", 0, 1)
    one_error("error at k - 1: head run of k windows, p = b = 4", K - 1, 5)
    one_error("error at k: interior run of k windows 1..5, p = b = 5", K, 5)
    one_error("error at L - k: tail run 11..15, p = a + k - 1 = 15", len(READ) - K, 5)
    one_error("error at L - 1: tail run of the last window, p = 15 + 4 = 19", len(READ) - 1, 1)
    far = sub(READ, (5, other(READ[5])), (12, other(READ[12])))          # windows 1..5 and 8..12: 6 and 7 stay solid
    cases.append(("two errors more than k apart: both fixed", c, [far], [READ],
                  stats(reads=1, windows=16, weak_windows=10, weak_runs=2, corrected=2, reads_changed=1)))
    near = sub(READ, (6, other(READ[6])), (9, other(READ[9])))           # windows 2..9: an interior run of 8 != k
    cases.append(("two errors less than k apart: skipped, untouched", c, [near], [near],
                  stats(reads=1, windows=16, weak_windows=8, weak_runs=1, skipped=1)))
    gap = {key: v for key, v in c.items() if key not in (R.canon(READ[7:12]), R.canon(READ[8:13]))}
    cases.append(("an interior run shorter than k (windows 7, 8 not in the table): skipped", gap, [READ], [READ],
                  stats(reads=1, windows=16, weak_windows=2, weak_runs=1, skipped=1)))
    alien = "ACACACACACACACACACAC"
    cases.append(("a whole-read run: skipped", c, [alien], [alien], stats(reads=1, windows=16, weak_windows=16, weak_runs=1, skipped=1)))
    lk_bad = sub(READ[:K], (0, other(READ[0])))
    cases.append(("L = k: the one window is the whole read, weak or solid", c, [lk_bad, READ[:K]], [lk_bad, READ[:K]],
                  stats(reads=2, windows=2, weak_windows=1, weak_runs=1, skipped=1)))
    cases.append(("L < k and L = 0: copied, counted as short", c, [READ[:K - 1], ""], [READ[:K - 1], ""], stats(reads=2, short=2)))
    x = other(READ[0])
    y = other(READ[0], skip=x)
    two = dict(c)
    two[R.canon(y + READ[1:K])] = 7                                      # a second way to make window 0 solid
    cases.append(("ambiguous: two replacements make the run solid", two, [sub(READ, (0, x))], [sub(READ, (0, x))],
                  stats(reads=1, windows=16, weak_windows=1, weak_runs=1, ambiguous=1)))
    none = {key: v for key, v in c.items() if key != R.canon(READ[:K])}
    cases.append(("unresolved: window 0 is weak and no replacement of base 0 is in the table", none, [READ], [READ],
                  stats(reads=1, windows=16, weak_windows=1, weak_runs=1, unresolved=1)))
    low = dict(c)
    low[R.canon(READ[:K])] = SOLID - 1                                   # below the threshold is weak, at it solid
    cases.append(("count = solid - 1 is weak", low, [READ], [READ], stats(reads=1, windows=16, weak_windows=1, weak_runs=1, unresolved=1)))
    at = dict(c)
    at[R.canon(READ[:K])] = SOLID
    cases.append(("count = solid is solid", at, [READ], [READ], stats(reads=1, windows=16)))
    return cases


HAND_CASES = hand_cases()


def test_the_hand_sequence_is_what_the_cases_assume():
    """every 5-mer of G once on either strand, no palindrome, no hash tie: the table holds one entry per window of G"""
    kmers = [G[i:i + K] for i in range(len(G) - K + 1)]
    both = set(kmers) | {R.rev_comp(s) for s in kmers}
    assert len(both) == 2 * len(kmers)
    assert all(R.hash_code(s) != R.hash_code(R.rev_comp(s)) for s in kmers)
    assert not any(s in both for s in ("ACACA", "CACAC"))


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0].split(":")[0] for c in HAND_CASES])
def test_hand_cases(case):
    _name, counts, reads, want, want_stats = case
    got, st = X.correct(counts, reads, K, SOLID)
    assert got == want
    assert st == want_stats
    # the stream form: same bases, framing untouched
    raw = R.reads_to_bin(reads)
    out, st2 = X.correct_bin(counts, raw, len(reads), K, SOLID)
    assert out == R.reads_to_bin(want) and st2 == want_stats


def noisy_reads(rnd, genome, n, length, err):
    reads, truth = [], []
    for _ in range(n):
        p = rnd.randrange(len(genome) - length + 1)
        t = genome[p:p + length]
        if rnd.random() < 0.5:
            t = R.rev_comp(t)
        s = "".join(rnd.choice([b for b in "AGCT" if b != c]) if rnd.random() < err else c for c in t)
        reads.append(s)
        truth.append(t)
    return reads, truth


@pytest.mark.parametrize("k", [5, 9, 21])
def test_properties_on_random_reads(k):
    rnd = random.Random(40 + k)
    genome = "".join(rnd.choice("AGCT") for _ in range(600))
    reads, truth = noisy_reads(rnd, genome, 300, 60, 0.01)
    counts = X.count_reads(reads, k)
    solid = 3
    fixed, st = X.correct(counts, reads, k, solid)
    assert st["weak_runs"] == st["corrected"] + st["ambiguous"] + st["unresolved"] + st["skipped"]
    assert st["reads"] == 300 and st["windows"] == 300 * (60 - k + 1) and st["corrected"] > 0 and st["skipped"] > 0
    assert st["reads_changed"] == sum(a != b for a, b in zip(reads, fixed))
    assert st["corrected"] == sum(x != y for a, b in zip(reads, fixed) for x, y in zip(a, b))
    # idempotent, and every window that was solid stays solid
    again, st2 = X.correct(counts, fixed, k, solid)
    assert again == fixed and st2["corrected"] == 0 and st2["reads_changed"] == 0
    for a, b in zip(reads, fixed):
        for i in range(len(a) - k + 1):
            if X.kmer_count(counts, a[i:i + k]) >= solid:
                assert b[i:i + k] == a[i:i + k]
            elif a[i:i + k] != b[i:i + k]:
                assert X.kmer_count(counts, b[i:i + k]) >= solid
    # it does what it is for: more reads equal their error-free source than before (k = 5 is too short to tell errors apart)
    if k >= 9:
        assert sum(a == t for a, t in zip(fixed, truth)) > sum(a == t for a, t in zip(reads, truth))
    # ... and a recount of the corrected reads holds strictly fewer weak k-mers
    recount = X.count_reads(fixed, k)
    assert sum(1 for v in recount.values() if v < solid) < sum(1 for v in counts.values() if v < solid)


def test_stream_form_keeps_framing_and_padding():
    counts = g_counts()
    reads = [sub(READ, (0, other(READ[0]))), READ[:7], "", sub(READ[:18], (17, other(READ[17])))]
    raw = bytearray(R.reads_to_bin(reads))
    raw[1 + 6 + 1] |= 0xC0                                   # 7 bases fill 14 bits of two bytes: set the 2 padding bits of that record
    pad_at = 1 + 5 + 1 + 1                                   # record 0: 1 + 5 bytes; record 1: length byte, then its second data byte
    assert raw[pad_at] & 0xC0 == 0xC0
    out, st = X.correct_bin(counts, bytes(raw), len(reads), K, SOLID)
    assert len(out) == len(raw) and out[pad_at] == raw[pad_at]
    assert R.reads_from_bin(out, len(reads)) == [READ, READ[:7], "", READ[:18]]
    assert st["corrected"] == 2 and st["reads_changed"] == 2 and st["short"] == 1


def test_library_exports_and_binds_both_entry_points():
    """what fails without the feature, GPU or not"""
    product = C.CDLL(os.path.join(ROOT, "genome_amd", "libgenome_amd.so"))
    for name in ("gk_reads_correct", "gk_reads_correct_dev"):
        assert hasattr(product, name), name
        assert name in L.SIGNATURES
    assert L.SIGNATURES["gk_reads_correct"][1][4] is C.c_uint32 and len(L.SIGNATURES["gk_reads_correct_dev"][1]) == 7
    from genome_amd.dnamap import CORRECT_STATS
    assert tuple(CORRECT_STATS) == X.STATS and len(CORRECT_STATS) == 10
    hdr = open(os.path.join(ROOT, "include", "genome_amd.h")).read()
    assert "GK_CORRECT_NSTATS = 10" in hdr
    # argument checks that need no device: a NULL handle is refused, and solid = 0 never gets as far as the device
    st = (C.c_uint64 * 10)()
    assert L.lib().gk_reads_correct(None, None, 0, 0, 3, None, st) == L.GK_E_INVALID
    assert L.lib().gk_reads_correct_dev(None, None, 0, 100, 3, None, st) == L.GK_E_INVALID
