"""The rule of gk_reads_correct (include/genome_amd.h) restated on strings, from the header's text: the device is held to this
byte for byte (tests/test_correct_gpu.py), and this file to hand-computed answers (tests/test_correct_cpu.py).

Input: `counts`, a dict stored k-mer (string) -> count as a table filled by the hash rule holds it (key = oracle.pyref.canon of
every window counted; tips_ref.canonical_counts makes one from verbatim keys), and the reads as base strings.  Nothing here
calls the library.
"""
from oracle import pyref as R

STATS = ("reads", "short", "windows", "weak_windows", "weak_runs", "corrected", "ambiguous", "unresolved", "skipped", "reads_changed")


def kmer_count(counts, w, memo=None):
    """Count of one window: the stored count of its hash-rule orientation, 0 if absent.  Where the rule cannot tell the two
    strands apart (equal hashes, the k-mer not its own reverse complement) the table may hold both: their counts add up.
    memo: a dict of answers already given for this `counts` (sequencing coverage asks for the same window many times)."""
    if memo is not None and w in memo:
        return memo[w]
    rc = R.rev_comp(w)
    hw, hr = R.hash_code(w), R.hash_code(rc)
    c = counts.get(w if hw < hr else rc, 0)                       # oracle.pyref.canon: the smaller hash, a tie goes to rc
    if w != rc and hw == hr:
        c += counts.get(w, 0)
    if memo is not None:
        memo[w] = memo[rc] = c
    return c


def count_reads(reads, k):
    """the table counting leaves: canonical k-mer -> occurrences over the reads"""
    counts, canon = {}, {}
    for s in reads:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            key = canon.get(w)
            if key is None:
                key = canon[w] = R.canon(w)
            counts[key] = counts.get(key, 0) + 1
    return counts


def weak_runs(flags):
    """maximal runs [a, b] of False in a list of solid flags"""
    runs, i, n = [], 0, len(flags)
    while i < n:
        if flags[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and not flags[j + 1]:
            j += 1
        runs.append((i, j))
        i = j + 1
    return runs


def correct_read(counts, read, k, solid, st, memo=None):
    n = len(read) - k + 1
    st["reads"] += 1
    if n <= 0:
        st["short"] += 1
        return read
    flags = [kmer_count(counts, read[i:i + k], memo) >= solid for i in range(n)]
    st["windows"] += n
    st["weak_windows"] += flags.count(False)
    out = list(read)
    for a, b in weak_runs(flags):
        st["weak_runs"] += 1
        m = b - a + 1
        p = None
        if a == 0 and b == n - 1:
            pass
        elif a == 0:
            p = b if m <= k else None
        elif b == n - 1:
            p = a + k - 1 if m <= k else None
        elif m == k:
            p = b
        if p is None:
            st["skipped"] += 1
            continue
        assert [w for w in range(n) if w <= p < w + k] == list(range(a, b + 1))
        valid = []
        for c in "AGCT":
            if c == read[p]:
                continue
            cand = read[:p] + c + read[p + 1:]                    # every run is judged from the INPUT read
            if all(kmer_count(counts, cand[w:w + k], memo) >= solid for w in range(a, b + 1)):
                valid.append(c)
        if len(valid) == 1:
            out[p] = valid[0]
            st["corrected"] += 1
        elif valid:
            st["ambiguous"] += 1
        else:
            st["unresolved"] += 1
    out = "".join(out)
    if out != read:
        st["reads_changed"] += 1
    return out


def correct(counts, reads, k, solid):
    """-> (corrected reads, the ten statistics as a dict named by STATS)"""
    assert solid >= 1
    st, memo = dict.fromkeys(STATS, 0), {}
    return [correct_read(counts, r, k, solid, st, memo) for r in reads], st


def correct_bin(counts, bin_bytes, nreads, k, solid):
    """the same over a `.bin` stream: only the 2-bit fields of corrected bases differ; length bytes and padding bits stay"""
    reads = R.reads_from_bin(bin_bytes, nreads)
    fixed, st = correct(counts, reads, k, solid)
    out = bytearray(bin_bytes)
    pos = 0
    for old, new in zip(reads, fixed):
        assert out[pos] == len(old)
        for i, (x, y) in enumerate(zip(old, new)):
            if x != y:
                j = pos + 1 + i // 4
                out[j] = (out[j] & ~(3 << (2 * (i % 4)))) | (R.BASES.index(y) << (2 * (i % 4)))
        pos += 1 + (len(old) + 3) // 4
    return bytes(out), st
