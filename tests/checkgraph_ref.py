"""A plain restatement of the FASTA check's rules (include/genome_amd.h, "FASTA check"), taken literally from
S/scripts/CheckGraph.scala:37-55, for the tests to compare the device against.  A helper, not a test.

    for (line <- getLines() if !line.startsWith(">"))            :48
      for (str <- line.sliding(k) if str.forall(Base.fromChar.contains(_)))   :49
        if (!graphMap.contains(read)()) "Not found"              :51-52

getLines() / readLine: a line ends at "\\n", at "\\r" or at "\\r\\n"; a non-empty unterminated tail is a line.  per_line is that loop
as it stands; the joined mode concatenates the sequence lines of a record (header to header) before sliding.  The one deviation,
in both modes: a non-header line of 1..k-1 characters has no window here (sliding(k) would yield it whole); it is counted in
short_lines.
"""
BASES = "AGCT"          # Base.scala:13-18: A0 G1 C2 T3


def lines(text: bytes):
    """[(offset of the line's first byte, the line's bytes)] by readLine's rule"""
    out, i, n = [], 0, len(text)
    start = 0
    while i < n:
        c = text[i]
        if c == 0x0A or c == 0x0D:
            out.append((start, text[start:i]))
            i += 2 if (c == 0x0D and i + 1 < n and text[i + 1] == 0x0A) else 1
            start = i
        else:
            i += 1
    if start < n:
        out.append((start, text[start:n]))
    return out


def pack(s: str):
    lo = hi = 0
    for i, c in enumerate(s):
        v = BASES.index(c)
        if i < 32:
            lo |= v << (2 * i)
        else:
            hi |= v << (2 * (i - 32))
    return lo, hi


def check(text: bytes, k: int, per_line: bool, present):
    """present: the set of k-mer strings the map holds.  -> (the nine counters, the whole missing list
    [(offset, line, column, lo, hi)] in stream order)"""
    st = dict(lines=0, records=0, bases=0, valid_bases=0, windows=0, found=0, missing=0, covered_bases=0, short_lines=0)
    valid = set(b"AGCT")
    segments, cur = [], []                  # a segment: the characters windows may run over, each (char, offset, line, column)
    seen_header = seen_seq_first = False
    for ln, (off, body) in enumerate(lines(text)):
        st["lines"] += 1
        if body[:1] == b">":
            st["records"] += 1
            seen_header = True
            segments.append(cur)
            cur = []
            continue
        if body and not seen_header and not seen_seq_first:
            seen_seq_first = True
            st["records"] += 1
        if 1 <= len(body) < k:
            st["short_lines"] += 1
        for col, c in enumerate(body):
            st["bases"] += 1
            st["valid_bases"] += c in valid
            cur.append((c, off + col, ln, col))
        if per_line:
            segments.append(cur)
            cur = []
    segments.append(cur)
    missing, covered = [], set()
    for seg in segments:
        for i in range(len(seg) - k + 1):
            w = seg[i:i + k]
            if not all(c in valid for c, _, _, _ in w):
                continue
            st["windows"] += 1
            s = "".join(chr(c) for c, _, _, _ in w)
            if s in present:
                st["found"] += 1
                covered.update(o for _, o, _, _ in w)
            else:
                st["missing"] += 1
                missing.append((w[0][1], w[0][2], w[0][3]) + pack(s))
    st["covered_bases"] = len(covered)
    return st, missing


def contig_stats(lengths, longer_than: int):
    """CheckGraph.scala:37-41: the lengths above the cutoff, sorted.  median = sorted(count / 2) (the reference's "N50"); n50 = the
    real one: lengths descending, the first at which twice the running sum reaches the total.  No such length: all zeros."""
    c = sorted(int(x) for x in lengths if int(x) > longer_than)
    if not c:
        return dict(count=0, sum=0, median=0, n50=0, max=0)
    total, run, n50 = sum(c), 0, 0
    for x in reversed(c):
        run += x
        if 2 * run >= total:
            n50 = x
            break
    return dict(count=len(c), sum=total, median=c[len(c) // 2], n50=n50, max=c[-1])
