"""CheckGraph on the device (S/scripts/CheckGraph.scala:37-55): the FASTA k-window check (gk_fasta_check) and the contig statistics
(gk_graph_contig_stats) against the plain restatement tests/checkgraph_ref.py and the oracle.  -m gpu.

Every comparison is of exact integers: all nine counters and the whole missing list, in order."""
import os
import random

import numpy as np
import pytest

import checkgraph_ref as ref
from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.check import FastaCheck
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph, loadGraph
from oracle import oracle as O
from oracle import pyref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [11, 31, 34, 63, 64]            # both slot widths and the tagged table
BIG = 1 << 20                        # a max_missing above every count here


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def make_genome(seed, size, repeat=200):
    rnd = random.Random(seed)
    g = [rnd.choice("AGCT") for _ in range(size)]
    a, b = size // 5, 3 * size // 5
    g[b:b + repeat] = g[a:a + repeat]
    return "".join(g)


def tiled_reads(g, length=100, step=20):
    reads = []
    for s in list(range(0, len(g) - length + 1, step)) + [len(g) - length]:
        reads += [g[s:s + length], R.rev_comp(g[s:s + length])]
    return reads


class Case:
    """a genome, the graph of its error-free reads and the position map; the key set of the restatement comes from the map"""

    def __init__(self, ctx, k, size, seed):
        self.k, self.genome = k, make_genome(seed, size)
        reads = tiled_reads(self.genome)
        self.bin, self.nreads = dna.reads_to_bin(reads), len(reads)
        self.m = HipDNAMap(ctx, k)
        self.m.count_reads(self.bin, self.nreads)
        self.graph = buildGraph(k, self.m)
        self.vm = self.graph.getGraphMap()
        lo, hi, _ = self.vm.items()
        self.present = {dna.unpack(int(a), int(b), k) for a, b in zip(lo, hi)}

    def close(self):
        self.vm.close(); self.graph.close(); self.m.close()


@pytest.fixture(scope="module")
def cases(ctx):
    made = {}

    def get(k, size=3000):
        if (k, size) not in made:
            made[(k, size)] = Case(ctx, k, size, 100 + k)
        return made[(k, size)]

    yield get
    for c in made.values():
        c.close()


def wrap(s, width, eol):
    return "".join(s[i:i + width] + eol for i in range(0, len(s), width))


def make_fasta(g, k, seed):
    """one text with every case of the issue's list; returns (bytes, {name: offset} of places the feed tests cut at)"""
    rnd = random.Random(seed)
    rc = R.rev_comp(g)
    alien = "".join(rnd.choice("AGCT") for _ in range(300))
    marks = {}
    parts = []

    def add(s):
        parts.append(s if isinstance(s, bytes) else s.encode())

    def here():
        return sum(len(p) for p in parts)

    add(g[40:40 + 2 * k] + "\n")                                     # sequence before the first header
    add(">genome wrapped at 60\n")
    marks["record"] = here()                                         # the first byte of a record's sequence
    add(wrap(g, 60, "\n"))
    marks["header"] = here() + 5
    add(">reverse complement wrapped at 20, CRLF\r\n")
    marks["crlf"] = here() - 1                                       # between the '\r' and its '\n'
    add(wrap(rc, 20, "\r\n"))
    add(">unwrapped, lone CR\r" + g[500:1500] + "\r")
    add(">empty record\n>two headers in a row\n")
    add(g[100:200] + "NNNNNNNN" + g[200:260].lower() + g[260:400] + "\n")      # a run of N, lowercase
    add(g[300:330] + "N" + g[331:331 + k - 1] + "\n")                # an invalid character exactly k-1 from a line end ...
    add(g[600:650] + "n" + g[651:651 + k - 1] + "\n>next record\n")  # ... and from a record end
    add(g[800:840].encode() + b"\xc3" + g[841:841 + k + 5].encode() + b"\n")   # a byte >= 0x80
    add(g[900:900 + k - 1] + "\n" + g[900 + k - 1:960] + "\n")       # a short line (k-1 characters), then its continuation
    add(">alien\n" + wrap(alien, 100, "\n"))                         # (lines longer than every k: missing windows in per_line mode too)
    add(">tail\n" + g[700:700 + k + 3])                              # no trailing newline
    return b"".join(parts), marks


def run(ctx, case, text, per_line, max_missing, pieces=None):
    """-> (counters, missing list); pieces: the feed sizes (a list of cut offsets), None = one feed"""
    with FastaCheck(ctx, case.vm, per_line, max_missing) as fc:
        if pieces is None:
            fc.feed(text, last=True)
        else:
            cuts = [0] + list(pieces) + [len(text)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                fc.feed(text[a:b], last=b == len(text))
        st = fc.stats()
        assert st["found"] + st["missing"] == st["windows"]
        return st, fc.missing()


@pytest.fixture(scope="module")
def parity_inputs(cases):
    made = {}

    def get(k, per_line):
        if (k, per_line) not in made:
            case = cases(k)
            text, marks = make_fasta(case.genome, k, k)
            made[(k, per_line)] = (case, text, marks) + ref.check(text, k, per_line, case.present)
        return made[(k, per_line)]

    return get


@pytest.mark.parametrize("per_line", [False, True])
@pytest.mark.parametrize("k", KS)
def test_parity_with_the_restatement(ctx, parity_inputs, k, per_line):
    case, text, _, want, want_missing = parity_inputs(k, per_line)
    assert 0 < want["missing"] < want["windows"] and want["short_lines"] > 0 and want["valid_bases"] < want["bases"]
    assert want["records"] == 9 and len(want_missing) == want["missing"] > 5
    if per_line and k >= 31:
        assert want["short_lines"] >= 150                 # every 20-character line of the reverse complement is a short line
    for max_missing in (0, 5, BIG):
        st, missing = run(ctx, case, text, per_line, max_missing)
        print(k, per_line, max_missing, st)
        assert st == want
        assert missing == want_missing[:max_missing]


@pytest.mark.parametrize("per_line", [False, True])
@pytest.mark.parametrize("k", KS)
def test_feed_invariance(ctx, parity_inputs, k, per_line):
    """the same text in pieces of 1, 7 and 4097 bytes, and cut at the places where state crosses a feed: every counter and the
    whole missing list (offsets, lines, columns) equal the one-shot result"""
    case, text, marks, want, want_missing = parity_inputs(k, per_line)
    n = len(text)
    for step in (1, 7, 4097):
        assert run(ctx, case, text, per_line, BIG, list(range(step, n, step))) == (want, want_missing), step
    singles = [marks["crlf"], marks["header"], marks["record"] + k - 1, marks["record"] + k, n - 1]
    for cut in singles:
        assert text[marks["crlf"] - 1:marks["crlf"] + 1] == b"\r\n"
        assert run(ctx, case, text, per_line, BIG, [cut]) == (want, want_missing), cut
    assert run(ctx, case, text, per_line, BIG, sorted(singles)) == (want, want_missing)


@pytest.mark.parametrize("k", [31, 64])
def test_tile_edges(ctx, cases, k):
    """a 40 kbp genome: one unwrapped 40 kB line (three 16 KiB text tiles, ten window tiles) and wrapped at 70; the genome itself
    is all found and all covered; an alien record's windows are missing and the genome after it is found again"""
    case = cases(k, 40000)
    g = case.genome
    alien = "".join(random.Random(k).choice("AGCT") for _ in range(3000))
    for body in (g + "\n", wrap(g, 70, "\n")):
        text = (">genome\n" + body).encode()
        for per_line in (False, True):
            want, want_missing = ref.check(text, k, per_line, case.present)
            st, missing = run(ctx, case, text, per_line, BIG)
            assert st == want and missing == want_missing
            if not per_line:
                assert st["missing"] == 0 and st["covered_bases"] == st["valid_bases"] == 40000 and st["windows"] == 40000 - k + 1
        text = (">genome\n" + body + ">alien\n" + alien + "\n>genome again\n" + body).encode()
        want, want_missing = ref.check(text, k, False, case.present)
        st, missing = run(ctx, case, text, False, BIG)
        assert st == want and missing == want_missing
        assert st["missing"] >= 3000 - k + 1 - 5 and st["found"] == 2 * (40000 - k + 1) + (3000 - k + 1 - st["missing"])
        assert all(len(">genome\n" + body + ">alien\n") <= m[0] < len(">genome\n" + body + ">alien\n") + 3000 for m in missing)


def test_device_slices_of_one_feed(cases):
    """one feed cut into many device slices (the next slice's upload runs beside the current slice's kernels), slices that end
    between a '\\r' and its '\\n' included: the same result as one slice"""
    c = Context(0)
    try:
        case = Case(c, 31, 3000, 131)
        text, _ = make_fasta(case.genome, 31, 31)
        want, want_missing = ref.check(text, 31, False, case.present)
        for chunk in (4096, 1000, 61):
            c.set_option("test_fastq_chunk", chunk)
            assert run(c, case, text, False, BIG) == (want, want_missing), chunk
        c.set_option("test_fastq_chunk", 0)
        case.close()
    finally:
        c.close()


def oracle_pair(ctx, k, seed):
    rnd = random.Random(seed)
    g = make_genome(seed, 6000, 300)
    reads = []
    for _ in range(1500):
        ln = rnd.randint(k + 5, min(255, k + 90))
        s = rnd.randrange(0, len(g) - ln + 1)
        r = "".join(c if rnd.random() >= 0.005 else rnd.choice([x for x in "AGCT" if x != c]) for c in g[s:s + ln])
        reads.append(R.rev_comp(r) if rnd.random() < 0.5 else r)
    binb = dna.reads_to_bin(reads)
    m, pm = HipDNAMap(ctx, k), O.PMap(k, 1)
    m.count_reads(binb, len(reads)); pm.count_reads(binb, len(reads))
    m.deleteAll_lt(2); pm.delete_lt(2)
    return m, buildGraph(k, m), O.Graph(pm)


def check_contigs(graph, lengths_other=None):
    lengths = [len(e[2]) for e in graph.canonical()[1]]
    if lengths_other is not None:
        assert sorted(lengths) == sorted(int(x) for x in lengths_other)
    assert lengths
    some = False
    for cutoff in (0, 100, 200, max(lengths)):
        got = graph.contigStats(cutoff)
        assert got == ref.contig_stats(lengths, cutoff), cutoff
        some |= got["count"] > 0
    assert some and graph.contigStats(max(lengths)) == dict(count=0, sum=0, median=0, n50=0, max=0)
    return lengths


@pytest.mark.parametrize("k,seed", [(31, 2), (47, 3)])
def test_contig_stats(ctx, k, seed):
    m, graph, og = oracle_pair(ctx, k, seed)
    check_contigs(graph, og.edges()["len"])                          # straight after buildGraph
    graph.removeBubbles(); og.remove_bubbles(); graph.simplifyGraph(); og.simplify()
    lengths = check_contigs(graph, og.edges()["len"])
    assert max(lengths) > 200
    _, edge_bound = graph.idBounds()
    info = graph.edgesById(np.arange(edge_bound, dtype=np.uint32))
    alive = np.flatnonzero(info["alive"])
    longest = alive[np.argsort(info["len"][alive])[-3:]]
    assert graph.removeEdgesById(longest) == 3                       # dead edges do not count
    after = check_contigs(graph)
    assert len(after) == len(lengths) - 3 and max(after) <= max(lengths)
    graph.close(); m.close()


def test_contig_stats_of_a_loaded_graph(ctx):
    graph = loadGraph(ctx, os.path.join(ROOT, "tests", "golden", "graph_v1_k35.gkg"))
    check_contigs(graph)
    graph.close()


def test_handle_errors(ctx, cases):
    case = cases(31)
    live0 = ctx.mem_stats()["live"]
    fc = FastaCheck(ctx, case.vm, False, 10)
    fc.feed(b">x\n" + case.genome.encode(), last=False)
    fc.feed(b"ACGT" * (1 << 19), last=True)                          # (2 MiB: the feed's buffers are blocks the pool counts)
    with pytest.raises(L.GkError) as e:
        fc.feed(b"ACGT", last=True)
    assert e.value.code == L.GK_E_STATE
    assert len(fc.missing()) == 10
    fc.close()
    assert ctx.mem_stats()["live"] == live0
    for call in (lambda: fc.feed(b"A"), fc.stats, fc.missing, fc.last_ms):
        with pytest.raises(L.GkError):
            call()
    fc.close()
