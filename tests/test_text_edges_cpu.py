"""The placed inputs of tests/text_edge_cases.py are what they claim to be (no GPU): the chosen terminator sits at its byte, both
restatements split there as Java's readLine does, the extremes hold no (or only) terminators where they say, and the slice-cut
sweep puts every one of the 48 "\\r\\n" on the cut and carries every residue mod 16."""
import os
import random
import re

import checkgraph_ref as cref
import fastq_ref as ref
import text_edge_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM = b"\r\n"


def test_constants_are_the_header_s_cpu():
    src = open(os.path.join(ROOT, "genome_amd", "csrc", "gk_text.h")).read()
    assert re.search(r"constexpr u32 FQ_TILE = 16384;", src) and re.search(r"constexpr u32 FQ_BLOCK = 256;", src)
    assert "PER_WAVE = FQ_TILE / (FQ_BLOCK / 64)" in src
    assert (T.TILE, T.BLOCK, T.STRIPE) == (16384, 256, 4096)


def test_readline_rule_by_hand_cpu():
    """BufferedReader.readLine: a line ends at "\\n", at "\\r", or at "\\r\\n" taken as one; the end of the input ends a non-empty
    tail.  So "\\r\\r\\n" is two line ends (the second line empty) and "\\n\\r" is two as well."""
    text = b"a\rbc\n\r\nd\r\r\ne\n\rf"
    want = [(b"a", 0, 2), (b"bc", 2, 5), (b"", 5, 7), (b"d", 7, 9), (b"", 9, 11), (b"e", 11, 13), (b"", 13, 14), (b"f", 14, 15)]
    assert ref.lines(text) == want
    assert cref.lines(text) == [(s, c) for c, s, _ in want]
    assert ref.lines(b"") == [] and ref.lines(b"\n") == [(b"", 0, 1)] and ref.lines(b"\r\n") == [(b"", 0, 2)]
    assert ref.lines(b"x\r") == [(b"x", 0, 2)] and ref.lines(b"\r\nx") == [(b"", 0, 2), (b"x", 2, 3)]


def same_lines(text: bytes):
    a = ref.lines(text)
    assert cref.lines(text) == [(s, c) for c, s, _ in a]
    return a


def check_site(text: bytes, ls, t: int, pos: int, form: bytes):
    """line t ends at pos with the first terminator of `form`; "\\r\\r\\n" adds an empty line ended by "\\r\\n\""""
    assert text[pos:pos + len(form)] == form
    assert pos + len(form) == len(text) or text[pos + len(form)] not in TERM or not form.endswith(b"\r")
    content, start, end = ls[t]
    assert start + len(content) == pos and not any(b in TERM for b in content)
    if form == T.CR_EMPTY_CRLF:
        assert end == pos + 1 and ls[t + 1] == (b"", pos + 1, pos + 3)
    else:
        assert end == pos + len(form)
    if t + 1 < len(ls):
        assert ls[t + 1][1] == end


def test_fastq_cases_are_what_they_claim_cpu():
    cases = T.fastq_cases()
    assert len(cases) == len(T.POSITIONS) * 16 + 12 and len({n for n, _, _ in cases}) == len(cases)
    seen = set()
    for name, text, c in cases:
        ls = same_lines(text)
        pos, form, t = c["pos"], c["form"], c["line"]
        check_site(text, ls, t, pos, form)
        seen.add((pos, form, T.KINDS[t % 4]))
        assert len(text) <= 2 * T.TILE + 1024 and len(text) <= (c["boundary"] or 1) + T.TILE
        if pos > 1:
            assert text[pos - 1] not in TERM                 # the chosen line is not empty: the look-back of its terminator sees text
            assert 0 <= c["boundary"] - pos <= 2
            # the line kinds in front are in step (the chosen line is what its name says), and what follows still is FASTQ
            assert ls[t - t % 4][0].startswith(b"@r") and (form == T.CR_EMPTY_CRLF or len(ls) % 4 == 0)
    assert seen == {(p, f, k) for p in T.POSITIONS for f in T.FORMS for k in T.KINDS} | {(p, f, k) for p, ks in T.SMALL for f in T.FORMS for k in ks}
    # the sequence lines of every text: N, lower case, lengths that are no multiple of 4, and one longer than 36 + 64
    seqs = [ln[0] for ln in ref.lines(cases[0][1])[1::4]]
    assert any(b"N" in s for s in seqs) and any(s != s.upper() for s in seqs) and sum(len(s) % 4 != 0 for s in seqs) >= 4
    assert max(len(s) for s in seqs) == 150
    # byte 0 of the text is "\n" in one case, and the text starts with an empty header line in another
    assert any(text[:1] == b"\n" and c["pos"] == 1 for _, text, c in cases) and any(c["pos"] == 0 and c["form"] == T.LF for _, _, c in cases)


def test_fastq_cases_convert_cpu():
    """most placed texts are good FASTQ at both splits: the device tests compare bytes, not only an error's record number"""
    good = 0
    cases = T.fastq_cases()[::7]
    for _, text, _ in cases:
        for split_at in (36, 0):
            try:
                out, st = ref.convert(text, split_at)
                good += st["pairs"] > 0 and len(out) > 2 * st["pairs"]
            except ref.FastqFormatError:
                pass
    assert good >= len(cases)


def terminators_in(text: bytes, a: int, b: int) -> int:
    return sum(x in TERM for x in text[a:b])


def test_fastq_extremes_are_what_they_claim_cpu():
    ex = {n: (t, c) for n, t, c in T.fastq_extremes()}
    assert len(ex) == 17
    for name, (text, c) in ex.items():
        same_lines(text)
        assert len(text) <= 2 * T.TILE + 1024
        if "empty" in c:
            a, b = c["empty"]
            assert terminators_in(text, a, b) == 0 and terminators_in(text, 0, len(text)) > 8 and len(text) > b
            assert a % T.STRIPE == 0 and b % T.STRIPE == 0
        if "full" in c:
            a, b = c["full"]
            assert terminators_in(text, a, b) == b - a >= T.STRIPE and a == T.STRIPE and text[a - 1:a] == b"\n"
            assert text[b] not in TERM
        if "size" in c:
            assert len(text) == c["size"]
            assert text.endswith(b"\r\n") if name.endswith("crlf") else (text[-1:] == b"\n") == name.endswith("terminated")
            assert text[-1] in TERM or name.endswith("open")
    assert ex["tile_1_without_terminator"][1]["empty"] == (T.TILE, 2 * T.TILE)
    assert terminators_in(ex["tile_1_without_terminator"][0], 0, T.TILE) > 100
    # what the restatement makes of the stripes of terminators: 1024 (512) empty records between the others, all good; one "\n"
    # more leaves a lone last line, which is ignored; two more end the input inside record 3 + 1024 + 3
    for nm, recs in (("lf", 1030), ("cr", 1030), ("crlf", 518), ("lf_plus_one", 1030)):
        text = ex["stripe_of_" + nm][0]
        assert len(ref.lines(text)) // 4 == recs and ref.convert(text, 36)[1]["pairs"] == recs and ref.convert(text, 0)[1]["pairs"] == recs // 2
    for split_at in (36, 0):
        try:
            ref.convert(ex["stripe_of_lf_plus_two"][0], split_at)
            assert False
        except ref.FastqFormatError as e:
            assert e.record == 1030


def test_slice_plan_by_hand_cpu():
    """three records of 16 bytes cut every 20 bytes.  Chunk 0 = bytes 0..19 ends with the "\\r" of record 1's header line, which
    therefore ends no line yet: record 0 complete, "@ab\\r" carried.  Chunk 1 = 4 + 20 bytes ends with the "\\r" of record 2's
    sequence line: record 1 complete, "@ab\\r\\nAC\\r" carried.  Chunk 2 = 8 + 8 bytes is the last"""
    rec = b"@ab\r\nAC\r\n+\r\nII\r\n"
    data = rec * 3
    assert len(rec) == 16 and data[19:21] == b"\r\n" and data[39:41] == b"\r\n"
    assert T.fastq_slice_plan(data, 20, 4) == [{"cut": 20, "n": 20, "carry": 4}, {"cut": 40, "n": 24, "carry": 8},
                                               {"cut": 48, "n": 16, "carry": 0}]
    # interleaved: records complete in pairs, so record 0 waits for record 1 and record 2 for record 3
    assert [p["carry"] for p in T.fastq_slice_plan(rec * 4, 20, 0)] == [20, 8, 28, 0]


def test_slice_cut_sweep_covers_every_site_and_residue_cpu():
    base = T.crlf_base()
    assert len(T.crlf_sites(base)) == 48
    residues, kinds = set(), set()
    for chunk in (4096, 4097):
        cases = T.crlf_cut_cases(chunk)
        assert [s for s, _ in cases] == list(range(48))
        for s, data in cases:
            sites = T.crlf_sites(data)
            assert len(sites) == 48 and sites[s] == chunk - 1 and data[chunk - 1:chunk + 1] == b"\r\n"
            ls = same_lines(data)
            assert len(ls) == 48 and ls[s][1] + len(ls[s][0]) == chunk - 1         # site s ends line s: kind s % 4
            assert data.replace(b"p", b"").replace(b"x", b"") == base and data.count(b"x") == (s % 16 if s >= 4 else 0)
            plan = T.fastq_slice_plan(data, chunk, 4)
            assert [p["cut"] for p in plan] == [chunk, len(data)] and plan[1]["carry"] == 0
            # the carried bytes start at the record the cut falls in and end with the "\r"
            rec_start = ls[4 * (s // 4)][1]
            assert plan[0]["carry"] == chunk - rec_start and plan[1]["n"] == len(data) - rec_start
            residues.add(plan[0]["carry"] % 16)
            kinds.add(T.KINDS[s % 4])
    assert residues == set(range(16)) and kinds == set(T.KINDS)


def random_seq(n: int, seed: int) -> str:
    rnd = random.Random(seed)
    return "".join(rnd.choice("AGCT") for _ in range(n))


def test_fasta_cases_are_what_they_claim_cpu():
    seq = random_seq(900, 5)
    for k in (31, 64):
        cases = T.fasta_cases(seq, k)
        assert len(cases) == (len(T.POSITIONS) + 2) * 4
        present = {seq[i:i + k] for i in range(len(seq) - k + 1)}
        for name, text, c in cases:
            ls = same_lines(text)
            pos, form, at, planted = c["pos"], c["form"], c["at"], c["seq"]
            t = T.LINES_BEFORE if pos > 1 else 0
            check_site(text, ls, t, pos, form)
            assert len(text) <= 2 * T.TILE + 1024
            body = [ln for ln in ls if not ln[0].startswith(b">")]
            assert b"".join(ln[0] for ln in body).decode() == planted and planted[at + k - 1] == "N" and planted.count("N") == 1
            after = ls[t + (2 if form == T.CR_EMPTY_CRLF else 1)]
            assert after[0][:1].decode() == planted[at] and after[1] == pos + len(form)
            if pos > 1:
                assert ls[0][0].startswith(b">ref ") and len(ls[t][0]) == T.WIDTH and 0 <= c["boundary"] - pos <= 2
                assert chr(text[pos - 1]) in "AGCT"
                # windows run across the terminator: the invalid character takes the k windows that start behind it; the base
                # substituted three in front of it makes k windows missing, the last of them starting at that base; the next
                # missing window is the first behind the invalid character that holds the second substituted base
                st, missing = cref.check(text, k, False, present)
                assert st["records"] == 1 and st["missing"] == 2 * k and st["windows"] == len(planted) - k + 1 - k
                assert missing[k - 1][:3] == (pos - 3, t, T.WIDTH - 3)
                behind = t + (2 if form == T.CR_EMPTY_CRLF else 1)
                assert missing[k][1:3] == (behind + (k + 10) // T.WIDTH, (k + 10) % T.WIDTH)
