"""Placed inputs for the line-end passes of csrc/gk_text.h (k_fq_terms, fq_line_start) and for the slice cuts of gk_fastq.hip and
gk_fasta.hip: FASTQ and FASTA texts whose chosen terminator starts at a given byte, so that every tile, stripe and cut edge is
hit on purpose.  A helper, not a test: pure Python, no GPU.  tests/test_text_edges_cpu.py proves that every case is what it
claims to be; tests/test_text_edges_gpu.py runs them on the device against fastq_ref / checkgraph_ref."""
import random

import fastq_ref as ref

TILE = 16384                         # gk_text.h: FQ_TILE, text bytes per workgroup of the line-end passes
BLOCK = 256                          # FQ_BLOCK: four waves, each owns one stripe of the tile
STRIPE = TILE // (BLOCK // 64)       # 4096

LF, CR, CRLF, CR_EMPTY_CRLF = b"\n", b"\r", b"\r\n", b"\r\r\n"      # the last: "\r", then an empty line ended with "\r\n" (two lines)
FORMS = (LF, CR, CRLF, CR_EMPTY_CRLF)
EOLS = (LF, CRLF, CR)
KINDS = ("header", "sequence", "plus", "quality")
BOUNDARIES = (STRIPE, 2 * STRIPE, 3 * STRIPE, TILE, TILE + STRIPE, 2 * TILE)
POSITIONS = tuple(b + d for b in BOUNDARIES for d in (-2, -1, 0))
# the positions in front of which a whole record does not fit: (pos, the kinds of line that can end there).  pos 0: the text starts
# with an empty header line; pos 1, sequence: byte 0 is the "\n" of an empty header and the chosen terminator ends an empty sequence
SMALL = ((0, ("header",)), (1, ("header", "sequence")))


def boundary_of(pos: int) -> int:
    """the boundary a position belongs to; 0 for the start of the text"""
    return 0 if pos <= 1 else min(BOUNDARIES, key=lambda b: abs(b - pos))


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------
def _records(n: int, seed: int):
    """[(header, sequence, separator, quality)]: sequence lines of 9..150 characters, most of a length % 4 != 0, with N and lower
    case behind a run of ACGT long enough for a 64-window of the second mate at split 36; one quality line shorter, one longer"""
    rnd = random.Random(seed)
    lens = [101, 135, 77, 150, 9, 143, 118, 122]
    out = []
    for i in range(n):
        ln = lens[i % len(lens)]
        seq = bytearray(rnd.choice(b"ACGT") for _ in range(ln))
        if i % 3 == 0 and ln > 125:
            seq[ln - 8] = ord("N")
        if i % 3 == 1 and ln > 110:
            seq[ln - 5:] = bytes(seq[ln - 5:]).lower()
        if i % 4 == 2:
            seq[3] = ord("N")
        qlen = ln - 3 if i % 5 == 1 else ln + 2 if i % 5 == 3 else ln
        out.append((b"@r%d/%d" % (i, seed), bytes(seq), b"+" if i % 2 else b"+r%d" % i, bytes(rnd.choice(b"!#5?IJ") for _ in range(qlen))))
    return out


def _join(lines) -> bytes:
    return b"".join(c + e for c, e in lines)


def _text(recs, eol: bytes = LF) -> bytes:
    return _join([(c, eol) for r in recs for c in r])


def fastq_with_terminator_at(pos: int, form: bytes, which_line: str, eol_rest: bytes = LF, nrec: int = 6, seed: int = 1):
    """-> (text, index of the chosen line).  A FASTQ text of `nrec` records (two less where `pos` leaves no room for the two in
    front) whose line `which_line` of one record ends with `form`, the first byte of `form` at byte `pos`; every other line ends
    with `eol_rest`.  That record's header is padded to get there.  In front of a tiny `pos` the chosen line and the lines before
    it are empty and end with "\\n", but for a header of one byte where that byte is needed."""
    assert form in FORMS and which_line in KINDS and eol_rest in EOLS
    kind = KINDS.index(which_line)
    recs = _records(nrec, seed)
    first = 2                                         # the record that holds the chosen line
    lines = [[c, eol_rest] for r in recs for c in r]
    natural = len(_join(lines[:4 * first + kind])) + len(lines[4 * first + kind][0])
    if natural > pos:                                 # (an even number of records stays: the interleaved reading keeps its pairs)
        first, lines = 0, lines[8:]
        natural = len(_join(lines[:kind])) + len(lines[kind][0])
    t = 4 * first + kind
    if natural < pos:
        lines[4 * first][0] += b" " + b"p" * (pos - natural - 1)
    elif natural > pos:
        if pos - kind not in (0, 1):
            raise ValueError(f"no {which_line} line can end at byte {pos}")
        for i in range(kind + 1):
            lines[i] = [b"", LF]
        lines[0][0] = b"@" * (pos - kind)
    lines[t][1] = form
    # "\r" in front of an empty line ended with "\n" would read as one "\r\n": the builder never makes that
    for (_, e0), (c1, e1) in zip(lines, lines[1:]):
        assert not (e0.endswith(CR) and not c1 and e1.startswith(LF))
    text = _join(lines)
    assert text[pos:pos + len(form)] == form and len(_join(lines[:t])) + len(lines[t][0]) == pos
    return text, t


def fastq_cases():
    """[(name, text, claims)] for every position, form and line kind; claims = {"pos", "form", "line": index of the chosen line,
    "boundary"}.  The terminator of the other lines goes round "\\n", "\\r\\n", "\\r" with the case number."""
    out = []
    for pos, kinds in [(p, KINDS) for p in POSITIONS] + list(SMALL):
        for form in FORMS:
            for which in kinds:
                rest = EOLS[len(out) % 3] if pos > 1 else LF
                text, t = fastq_with_terminator_at(pos, form, which, rest)
                out.append((f"{which}@{pos}{form!r}/{rest!r}", text, {"pos": pos, "form": form, "line": t, "boundary": boundary_of(pos)}))
    return out


def _sized(size: int, final: bytes, eol: bytes = LF) -> bytes:
    """four records, the last one's header padded so that the text has exactly `size` bytes; final: the last line's terminator"""
    lines = [[c, eol] for r in _records(4, 7) for c in r]
    lines[-1][1] = final
    pad = size - len(_join(lines))
    lines[12][0] += b" " + b"s" * (pad - 1)
    return _join(lines)


def fastq_extremes():
    """[(name, text, claims)]: the stripe and tile prefix at its ends, and texts that end at, one before and one after a tile's end.
    claims: {"empty": (a, b) a byte range without a terminator byte, "full": (a, b) a range of terminator bytes only, "size"}"""
    out = []
    # a stripe without a terminator: a header from the first stripe into the third
    text, _ = fastq_with_terminator_at(2 * STRIPE + 100, LF, "header")
    out.append(("stripe_without_terminator", text, {"empty": (STRIPE, 2 * STRIPE)}))
    # whole tiles without a terminator: a header of TILE + 300 bytes over tile 0, and one over tile 1 behind a tile of short records
    long_rec = (b"@" + b"h" * (TILE + 299), b"ACGTTGCAAC", b"+", b"IIIIIIIIII")
    rest = _text(_records(4, 3)[1:])
    out.append(("tile_0_without_terminator", _text([long_rec]) + rest, {"empty": (0, TILE)}))
    many, i = bytearray(), 0
    while len(many) <= TILE - 250 or i % 2:
        many += _text([(b"@m%d" % i, b"ACGTNACGTAC"[:5 + i % 7], b"+", b"IIIIIIIIIII"[:5 + i % 7])], EOLS[i % 3])
        i += 1
    assert TILE - 300 < len(many) <= TILE, len(many)
    out.append(("tile_1_without_terminator", bytes(many) + _text([long_rec]) + rest, {"empty": (TILE, 2 * TILE)}))
    # stripes of nothing but terminators, from the stripe's first byte to its last: 4096 "\n" or "\r" are 1024 empty records,
    # 2048 "\r\n" are 512; one "\n" more shifts every later line by one, and fastq_ref says what becomes of that
    front, _ = fastq_with_terminator_at(STRIPE - 1, LF, "quality", nrec=4)
    front = front[:STRIPE]
    assert front.endswith(LF) and len(ref.lines(front)) == 12
    for nm, run in (("lf", LF * STRIPE), ("cr", CR * STRIPE), ("crlf", CRLF * (STRIPE // 2)), ("lf_plus_one", LF * (STRIPE + 1)),
                    ("lf_plus_two", LF * (STRIPE + 2))):
        out.append((f"stripe_of_{nm}", front + run + rest, {"full": (STRIPE, STRIPE + len(run))}))
    # exactly a tile, one byte less, one more: with and without the final terminator, and ending in "\r\n"
    for size in (TILE - 1, TILE, TILE + 1):
        out.append((f"size_{size}_terminated", _sized(size, LF), {"size": size}))
        out.append((f"size_{size}_open", _sized(size, b""), {"size": size}))
        out.append((f"size_{size}_crlf", _sized(size, CRLF, CRLF), {"size": size}))
    return out


# ---- the internal slice cut of the FASTQ reader ------------------------------------------------------------------------------
def crlf_base() -> bytes:
    """the text of test_fastq_gpu.test_every_crlf_split_point: 12 records, 48 "\\r\\n\""""
    return b"".join(ref.record(b"@r%d" % i, b"ACGTN"[i % 5:] + b"GATTACA" * (i % 4), b"I" * 40, eol=CRLF) for i in range(12))


def crlf_sites(data: bytes):
    return [i for i in range(len(data) - 1) if data[i:i + 2] == CRLF]


def crlf_cut_cases(chunk: int):
    """[(site number, text)]: the base text with its leading header padded so that site s has its "\\r" at byte chunk - 1 of the
    feed — the last byte of the first device slice — and its "\\n" first in the second.  The header of the site's own record
    takes s % 16 of the padding: the bytes carried into the second chunk start at that record, so their number goes through
    every residue mod 16, and with it the alignment of the second chunk's text."""
    base = crlf_base()
    starts = [ln[1] for ln in ref.lines(base)][::4]                 # where each record's "@" stands
    out = []
    for s, at in enumerate(crlf_sites(base)):
        own = s % 16 if s >= 4 else 0
        pad = chunk - 1 - at - own
        assert pad > 0
        text = bytearray(base)
        h = starts[s // 4] + 2                                      # behind "@r"
        text[h:h] = b"x" * own
        text[3:3] = b"p" * pad                                      # "@r0" + pad: the header of record 0
        out.append((s, bytes(text)))
    return out


def fastq_slice_plan(data: bytes, chunk: int, split_at: int):
    """gk_fastq.hip's slicing of ONE feed (last = 1), restated: the feed is cut every `chunk` bytes; a device chunk is the carried
    tail + the slice; a "\\r" that is the chunk's last byte does not end a line yet; the records completed are the full groups of
    four ended lines (an even number of them when interleaved); the tail from there on is carried.
    -> [{"cut": the feed offset the slice ends at, "n": bytes of the device chunk, "carry": bytes carried out of it}]"""
    out, carry, pos = [], b"", 0
    while pos < len(data):
        sl = data[pos:pos + chunk]
        last = pos + len(sl) == len(data)
        T = carry + sl
        ended = [ln for ln in ref.lines(T) if ln[2] > ln[1] + len(ln[0])]
        L = len(ended) - (1 if not last and T.endswith(CR) else 0)
        R = L // 4 if split_at else L // 4 & ~1
        start = len(T) if last else ended[4 * R - 1][2] if R else 0
        out.append({"cut": pos + len(sl), "n": len(T), "carry": len(T) - start})
        carry, pos = T[start:], pos + len(sl)
    return out


# ---- FASTA -------------------------------------------------------------------------------------------------------------------------
WIDTH = 60
LINES_BEFORE = 5                     # whole sequence lines in front of the chosen terminator: 300 bases, more than 2 k
SEQ_INDEX = WIDTH * LINES_BEFORE     # the first sequence character behind the chosen terminator


def fasta_with_terminator_at(pos: int, form: bytes, seq: str, eol_rest: bytes = LF) -> bytes:
    """">" header (padded), then `seq` wrapped at 60: the fifth sequence line ends with `form`, the first byte of `form` at byte
    `pos`, every other line with `eol_rest`.  pos 0: no header, the text starts with the terminator; pos 1: no header, one base
    in front of it.  The bytes in front of and behind the terminator are sequence: the windows across it are what gets checked."""
    assert form in FORMS and eol_rest in EOLS
    s = seq.encode()
    if pos <= 1:
        return s[:pos] + form + b"".join(s[i:i + WIDTH] + eol_rest for i in range(pos, len(s), WIDTH))
    body = [s[i:i + WIDTH] for i in range(0, len(s), WIDTH)]
    assert len(body) > LINES_BEFORE + 2
    front = b"".join(ln + eol_rest for ln in body[:LINES_BEFORE - 1]) + body[LINES_BEFORE - 1]
    hdr = b">ref "
    pad = pos - len(front) - len(hdr) - len(eol_rest)
    assert pad >= 0
    text = hdr + b"p" * pad + eol_rest + front + form + b"".join(ln + eol_rest for ln in body[LINES_BEFORE:])
    assert text[pos:pos + len(form)] == form
    return text


def plant(seq: str, k: int, at: int) -> str:
    """`seq` with one invalid character k-1 sequence characters behind index `at` (the first one behind the terminator), a
    substituted base three in front of `at`, so that all but one of its k windows run across the terminator, and another behind
    the invalid character"""
    g = list(seq)
    flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
    for i in (at - 3, at + 2 * k + 9):
        if 0 <= i < len(g):
            g[i] = flip[g[i]]
    g[at + k - 1] = "N"
    return "".join(g)


def fasta_cases(seq: str, k: int):
    """[(name, text, claims)] for every position and form; claims = {"pos", "form", "boundary", "seq": the planted sequence,
    "at": the index in it of the first character behind the chosen terminator}"""
    out = []
    for pos in POSITIONS + (0, 1):
        for form in FORMS:
            rest = EOLS[len(out) % 3]
            at = SEQ_INDEX if pos > 1 else pos
            planted = plant(seq, k, at)
            text = fasta_with_terminator_at(pos, form, planted, rest)
            out.append((f"fa@{pos}{form!r}/{rest!r}", text, {"pos": pos, "form": form, "boundary": boundary_of(pos), "seq": planted, "at": at}))
    return out
