"""The line-end passes of csrc/gk_text.h (k_fq_terms, fq_line_start) and the slice cuts of gk_fastq.hip / gk_fasta.hip at every
tile, stripe and cut edge: the placed inputs of tests/text_edge_cases.py (proved to be what they claim by
tests/test_text_edges_cpu.py) against the plain restatements tests/fastq_ref.py and tests/checkgraph_ref.py.  -m gpu.

Every comparison is exact: `.bin` bytes and statistics, an error's record number, count tables, the nine counters of the FASTA
check and its whole missing list (offset, line, column, key)."""
import random

import pytest

import checkgraph_ref as cref
import fastq_ref as ref
import text_edge_cases as T
from genome_amd import dna
from genome_amd.check import fasta_records
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.fastq import FastqReader
from oracle import pyref as R
from test_checkgraph_gpu import BIG, Case
from test_checkgraph_gpu import run as run_check
from test_fastq_gpu import check_parity, random_pieces

pytestmark = pytest.mark.gpu
GROUPS = [str(b) for b in T.BOUNDARIES] + ["start", "extremes"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fastq_groups():
    groups = {g: [] for g in GROUPS}
    for name, text, c in T.fastq_cases():
        groups[str(c["boundary"]) if c["boundary"] else "start"].append((name, text))
    groups["extremes"] = [(name, text) for name, text, _ in T.fastq_extremes()]
    assert sum(len(v) for v in groups.values()) == 317 and all(groups.values())
    return groups


@pytest.mark.parametrize("split_at", [36, 0])
@pytest.mark.parametrize("group", GROUPS)
def test_fastq_conversion_parity(ctx, fastq_groups, group, split_at):
    """every placed text as one feed: the terminator on each side of each stripe and tile edge, in each form, ending each kind
    of line; the prefix extremes also in random pieces"""
    for i, (name, text) in enumerate(fastq_groups[group]):
        print(name)
        check_parity(ctx, text, [text], split_at)
        if group == "extremes":
            check_parity(ctx, text, random_pieces(text, random.Random(i)), split_at)


def test_internal_slice_cut_on_every_terminator_byte():
    """a device slice that ends between the "\\r" and the "\\n" of each of the 48 terminators in turn (a cut on each kind of line):
    the "\\r" ends no line yet, its record is carried, and the "\\n" that opens the next slice is no line of its own.  The cut and
    the carried bytes are the restated plan's; the same cut as a feed boundary shows the carried bytes, whose number takes every
    residue mod 16 — the alignment of the next chunk's text, which stage_tile rounds down from"""
    residues = set()
    for chunk in (4096, 4097):
        c = Context(0)
        try:
            c.set_option("test_fastq_chunk", chunk)
            for s, data in T.crlf_cut_cases(chunk):
                plan = T.fastq_slice_plan(data, chunk, 4)
                assert [p["cut"] for p in plan] == [chunk, len(data)] and data[chunk - 1:chunk + 1] == b"\r\n", (chunk, s)
                check_parity(c, data, [data], 4)                       # the cut inside one feed
                want, _ = ref.convert(data, 4)
                rd = FastqReader(c, 4, 23)
                got = rd.convert(data[:chunk])                         # the same cut between two feeds of one slice each
                assert rd.stats()["carried_bytes"] == plan[0]["carry"], (chunk, s)
                residues.add(rd.stats()["carried_bytes"] % 16)
                got += rd.convert(data[chunk:], last=True)
                assert got == want and rd.stats()["carried_bytes"] == 0, (chunk, s)
                rd.close()
            c.set_option("test_fastq_chunk", 0)
        finally:
            c.close()
    assert residues == set(range(16))


def representative_texts():
    """one text per boundary and form: the terminator's first byte is the last byte in front of the boundary, the kind of line
    goes round"""
    out = []
    for b in T.BOUNDARIES:
        for form in T.FORMS:
            which = T.KINDS[len(out) % 4]
            out.append((f"{which}@{b - 1}{form!r}", T.fastq_with_terminator_at(b - 1, form, which, T.EOLS[len(out) % 3])[0]))
    return out


@pytest.fixture(scope="module")
def count_inputs():
    made = []
    for name, text in representative_texts():
        bin_, st = ref.convert(text, 36, 23)
        made.append((name, text, R.reads_from_bin(bin_, 2 * st["pairs"]), st["pairs"]))
    return made


@pytest.mark.parametrize("k", [23, 35, 64])
def test_count_fastq_on_the_placed_texts(ctx, count_inputs, k):
    """the table counted straight from the text is the table of the restatement's `.bin` counted by oracle.pyref"""
    some = 0
    for name, text, reads, npairs in count_inputs:
        want = sorted(R.extract_filtered_kmers(reads, k, 1, 1, do_filter=False).items())
        m = HipDNAMap(ctx, k, 1 << 10)
        pairs, occ = m.count_fastq(text, split_at=36)
        lo, hi, cnt = m.sorted_items()
        m.close()
        got = sorted((dna.unpack(int(a), int(b), k), int(c)) for a, b, c in zip(lo, hi, cnt))
        assert pairs == npairs and occ == sum(c for _, c in want), name
        assert got == want, name
        some += len(want)
    assert some > 24 * 50


def stale_lf_text(g: str, chunk: int) -> bytes:
    """a text of two slices and m more bytes that ends with "\\r", whose byte m is "\\n": the third slice lands on the first one's
    buffer, so the byte behind its last "\\r" is a "\\n" that is none of its own (fq_line_start's `e + 1 < n`)"""
    m = 1000
    first = b">" + b"h" * (m - 1) + b"\n"
    body = "".join(g[i:i + T.WIDTH] + "\n" for i in range(0, 1800, T.WIDTH)).encode()[:-1] + b"\r"
    second = b">" + b"x" * (2 * chunk + m - len(first) - len(body) - 2) + b"\n"
    text = first + second + body
    assert len(text) == 2 * chunk + m and text[m] == 0x0A and text[-1] == 0x0D and text[-2] != 0x0A
    return text


@pytest.mark.parametrize("per_line", [False, True])
@pytest.mark.parametrize("k", [31, 64])
def test_fasta_check_at_the_edges(k, per_line):
    """a reference whose line end sits on each side of each stripe and tile edge, in each form, with the k-windows running across
    it, an invalid character k-1 behind it and a substituted base on either side: unsliced, and in device slices of 4096 and 4097
    bytes (a cut between "\\r" and "\\n" included), all nine counters and the whole missing list are the restatement's"""
    c = Context(0)
    try:
        case = Case(c, k, 3000, 100 + k)
        cases = [(name, text) for name, text, _ in T.fasta_cases(case.genome[:900], k)]
        cases.append(("stale_lf", stale_lf_text(case.genome, 4096)))
        want = [cref.check(text, k, per_line, case.present) for _, text in cases]
        if not per_line:                                               # (a line of 60 holds no window of 64)
            assert all(0 < st["missing"] < st["windows"] for st, _ in want[:-1])
        for chunk in (0, 4096, 4097):
            c.set_option("test_fastq_chunk", chunk)
            for (name, text), (st, missing) in zip(cases, want):
                got = run_check(c, case, text, per_line, BIG)
                assert got[0] == st, (name, chunk)
                assert got[1] == missing, (name, chunk)
        c.set_option("test_fastq_chunk", 0)
        case.close()
    finally:
        c.close()


def test_placements_do_not_see_the_terminators(ctx):
    """one reference wrapped with "\\r\\n" (a terminator across the first tile's end, inside the contig) and with "\\n": the same
    records reach the device, and every edge is placed alike"""
    case = Case(ctx, 31, 3000, 131)
    try:
        crlf = T.fasta_with_terminator_at(T.TILE - 1, T.CRLF, case.genome, T.CRLF)
        lf = T.fasta_with_terminator_at(T.TILE - 1, T.LF, case.genome, T.LF)
        assert crlf[T.TILE - 1:T.TILE + 1] == b"\r\n" and crlf != lf and fasta_records(lf) == [case.genome.encode()]
        with case.graph.place(case.vm, fasta_records(crlf)) as a, case.graph.place(case.vm, fasta_records(lf)) as b:
            ea, eb = a.edges(), b.edges()
            assert ea == eb and a.stats() == b.stats()
            assert sum(ea["windows_fwd"]) + sum(ea["windows_rev"]) >= 3000 - 31 + 1
    finally:
        case.close()
