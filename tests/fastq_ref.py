"""A plain restatement of the FASTQ -> `.bin` conversion rules (include/genome_amd.h, "FASTQ"): test infrastructure, written from
the rules.  convert() returns the `.bin` bytes and the statistics, or raises FastqFormatError naming the 0-based record."""
from __future__ import annotations

ACGT = {ord("A"): 0, ord("G"): 1, ord("C"): 2, ord("T"): 3}
MAX_RECORD = 64 << 20


class FastqFormatError(ValueError):
    def __init__(self, record: int, why: str):
        super().__init__(f"FASTQ record {record}: {why}")
        self.record = record


def lines(data: bytes):
    """Java BufferedReader.readLine over the whole input: (line, start, end-of-terminator) triples"""
    out = []
    i, n, start = 0, len(data), 0
    while i < n:
        c = data[i]
        if c == 0x0A or c == 0x0D:
            nxt = i + 2 if c == 0x0D and i + 1 < n and data[i + 1] == 0x0A else i + 1
            out.append((data[start:i], start, nxt))
            start = i = nxt
            continue
        i += 1
    if start < n:
        out.append((data[start:], start, n))
    return out


def mate_len(seq: bytes, qual: bytes) -> int:
    n = 0
    for s, _ in zip(seq, qual):
        if s not in ACGT:
            break
        n += 1
    return n


def pack(seq: bytes, n: int) -> bytes:
    out = bytearray([n])
    for i in range(0, n, 4):
        v = 0
        for j in range(4):
            if i + j < n:
                v |= ACGT[seq[i + j]] << (2 * j)
        out.append(v)
    return bytes(out)


def convert(data: bytes, split_at: int = 36, k: int = 23, max_pairs: int = 0):
    """-> (bin bytes, {"pairs", "short_pairs", "kmers"}); split_at = 0: interleaved"""
    ls = lines(data)
    nrec = len(ls) // 4
    tail = len(ls) % 4
    mates = []                      # (record, len, seq) in order
    for r in range(nrec):
        h, seq, sep, qual = ls[4 * r:4 * r + 4]
        if qual[2] - h[1] > MAX_RECORD:
            raise FastqFormatError(r, "a record of more than 64 MiB of text")
        if any(b >= 0x80 for b in seq[0]) or any(b >= 0x80 for b in qual[0]):
            raise FastqFormatError(r, "a byte >= 0x80 in a sequence or quality line")
        halves = [(seq[0][:split_at], qual[0][:split_at]), (seq[0][split_at:], qual[0][split_at:])] if split_at else [(seq[0], qual[0])]
        for s, q in halves:
            n = mate_len(s, q)
            if n > 255:
                raise FastqFormatError(r, "a mate longer than 255 bases")
            mates.append((r, n, s))
    if not split_at and nrec % 2:
        raise FastqFormatError(nrec - 1, "interleaved input ends with an odd number of records")
    if tail >= 2:
        raise FastqFormatError(nrec, "the input ends inside a record")
    out = bytearray()
    pairs = shorts = kmers = 0
    for p in range(len(mates) // 2):
        if max_pairs and p >= max_pairs:
            break
        (_, l1, s1), (_, l2, s2) = mates[2 * p], mates[2 * p + 1]
        out += pack(s1, l1) + pack(s2, l2)
        pairs += 1
        shorts += 1 if (l1 < k or l2 < k) else 0
        kmers += max(0, l1 - k + 1) + max(0, l2 - k + 1)
    return bytes(out), {"pairs": pairs, "short_pairs": shorts, "kmers": kmers}


def record(header: bytes, seq: bytes, qual: bytes, sep: bytes = b"+", eol: bytes = b"\n") -> bytes:
    return header + eol + seq + eol + sep + eol + qual + eol
