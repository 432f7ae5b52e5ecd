"""gk_graph_contigs_plan / gk_contigs_read / gk_contigs_write on the device against the restatement (tests/contigs_ref.py): the
FASTA text byte for byte and the nine stats (-m gpu).

The graphs are those of tests/test_edge_coverage_gpu.py (a 400-base sequence with a 12-window branch, filled through add_counts) for
every key width, every line width that changes the shape of a record, both selections, with and without a count table; a
self-complementary sequence; an edge of 70 000 bases emitted in chunks of 4 KiB; a graph of a few thousand edges under launch
grids of 1 and 3 workgroups; graphs after simplifyGraph, after a node split's point edits and after the removal of one twin; a
stale plan; the text fed back through the FASTA check; and the error paths.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.check import FastaCheck
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import CONTIG_STATS, buildGraph, loadGraph
from oracle import pyref as R

import contigs_ref as CR
import small_grid_cases as SG
import test_edge_coverage_gpu as EC

pytestmark = pytest.mark.gpu
KS = [5, 21, 31, 34, 47, 63, 64]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def compare(g, named, m=None, counts=None, **kw):
    """the device's text and stats == the restatement's, for the edges `named` = edges_with_ids(g); -> (Contigs, text)"""
    edges, ids = named
    want_text, want_stats = CR.contigs(edges, ids, counts, **kw)
    c = g.contigs(m, **kw)
    got = c.stats()
    assert tuple(got) == CONTIG_STATS == CR.STATS
    assert got == want_stats
    assert got["live_edges"] == got["short"] + got["forward"] + got["self_twin"] + got["reverse"] == g.counts()[1]
    text = c.text()
    assert text == want_text
    return c, text


@pytest.mark.parametrize("k", KS)
def test_every_key_width_line_width_and_selection(ctx, k):
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    fp, chk = g.idFingerprint(), g.checksum()
    named = EC.edges_with_ids(g)
    n = max(len(s + q) for s, _e, q in named[0])
    assert n > k and (n > 60 + k or k == 5)                  # (at k = 5 the 400 bases branch everywhere: edges of a few bases)
    for lw in (0, 1, 7, 60, n - 1, n, n + 1):
        for strands in (1, 2):
            c, text = compare(g, named, line_width=lw, strands=strands)
            assert b"\n\n" not in text and b"cov=" not in text
            c.close()
            c, text = compare(g, named, m, counts, line_width=lw, strands=strands)
            st = c.stats()
            assert st["missing_windows"] == 0 and text.count(b" cov=") == st["records"]
            assert st["forward"] == st["reverse"] >= 3 and st["short"] == 0
            assert st["records"] == (st["forward"] + st["self_twin"] if strands == 1 else st["live_edges"])
            c.close()
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)                # the graph is as it was
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_other_tables_and_missing_kmers(ctx, k):
    """a count table in the layout counting leaves (12-byte slots at k = 31) that the graph was not built from, and a table that
    lacks some k-mers: they count 0 and missing_windows is exact"""
    counts = EC.branch_counts(k)
    built_from = EC.fill(ctx, k, counts)
    g = buildGraph(k, built_from)
    named = EC.edges_with_ids(g)
    rnd = random.Random(k)
    keys = list(counts)
    reads = [s if rnd.random() < 0.5 else R.rev_comp(s) for s in keys for _ in range(rnd.randint(1, 4))]
    read_counts = {}
    for s in reads:
        read_counts[R.canon(s)] = read_counts.get(R.canon(s), 0) + 1
    m = HipDNAMap(ctx, k, 0)
    m.set_insert_path("partitioned")
    assert m.count_reads(dna.reads_to_bin(reads), len(reads)) == len(reads)
    assert m.stats()["slot_bytes"] == (12 if k <= 31 else 24)
    for strands in (1, 2):
        compare(g, named, m, read_counts, strands=strands)[0].close()
    m.close()
    # every 7th k-mer gone
    fewer = {key: c for i, (key, c) in enumerate(counts.items()) if i % 7}
    lacking = EC.fill(ctx, k, fewer)
    for strands in (1, 2):
        c, _ = compare(g, named, lacking, fewer, line_width=7, strands=strands)
        assert c.stats()["missing_windows"] > 10 * strands
        c.close()
    lacking.close(); g.close(); built_from.close()


def test_min_len_keeps_n_at_least_min_len(ctx):
    k = 31
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    lens = sorted({len(s + q) for s, _e, q in named[0]})
    n = lens[len(lens) // 2]
    seen = []
    for min_len in (n - 1, n, n + 1, 0, 10 ** 9):
        c, _ = compare(g, named, min_len=min_len, strands=2)
        seen.append(c.stats()["short"])
        c.close()
    assert seen[0] == seen[1] < seen[2] and seen[3] == 0 and seen[4] == len(named[0])
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_self_twin_edge_appears_once(ctx, k):
    """X ++ rc(X) is its own reverse complement: the oracle builds ONE edge of it, of even n, whose twin is itself"""
    rnd = random.Random(9 * k)
    x = EC.rand_seq(rnd, 60)
    s = x + R.rev_comp(x)
    counts = {R.canon(s[i:i + k]): 4 for i in range(len(s) - k + 1)}
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    selfs = [i for (a, _b, q), i in zip(*named) if CR.classify(a + q) == "self_twin"]
    assert len(selfs) >= 1 and all(len(a + q) % 2 == 0 for (a, _b, q) in named[0] if CR.classify(a + q) == "self_twin")
    for strands in (1, 2):
        for mm, cc in ((None, None), (m, counts)):
            c, text = compare(g, named, mm, cc, strands=strands)
            assert c.stats()["self_twin"] == len(selfs)
            for i in selfs:
                assert text.count(b">e%d " % i) == 1
            c.close()
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_long_edge_in_small_chunks(ctx, k, tmp_path):
    """one edge of 70 000 bases (and its twin): more than 65 535, text of 4 KiB chunks through both staging buffers"""
    rnd = random.Random(31 * k)
    s = EC.rand_seq(rnd, 70000)
    keys = {R.canon(s[i:i + k]) for i in range(len(s) - k + 1)}
    assert len(keys) == len(s) - k + 1
    m = EC.fill(ctx, k, dict.fromkeys(keys, 3))
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    assert len(named[0]) == 2 and len(named[0][0][2]) == 70000 - k
    ctx.set_option("contigs_chunk_bytes", 4096)
    try:
        c, text = compare(g, named, line_width=60, strands=2)
        assert len(text) > 2 * 70000 and c.stats()["records"] == 2
        path = tmp_path / "long.fa"
        c.write(path)
        assert path.read_bytes() == text and not os.path.exists(str(path) + ".tmp")
        parts, at, i = [], 0, 0
        while at < len(text):
            piece = c.read(at, (1, 7, 4095, 4097)[i % 4])
            assert piece
            parts.append(piece)
            at += len(piece)
            i += 1
        assert b"".join(parts) == text
        # unaligned reads across a header's end, a line end, the record boundary, a chunk boundary and the text's end
        hdr = text.index(b"\n") + 1
        rec2 = text.index(b">", 1)
        for off, n in ((hdr - 3, 9), (hdr + 60 - 2, 7), (rec2 - 5, 13), (rec2 - 1, 2), (4093, 9), (3, 4095), (1, 1), (len(text) - 5, 50), (len(text), 4),
                       (rec2 + 1, 8200)):
            assert c.read(off, n) == text[off:off + n], (off, n)
        one, _ = compare(g, named, line_width=60, strands=1)
        assert one.stats()["records"] == 1
        one.close(); c.close()
    finally:
        ctx.set_option("contigs_chunk_bytes", 0)
    g.close(); m.close()


@pytest.mark.parametrize("grid", [1, 3])
def test_small_launch_grids(ctx, grid):
    """a graph of thousands of edges under 1 and 3 workgroups per launch: every workgroup takes several trips through every loop"""
    k = 11
    reads = SG.reads_case(k)
    m = HipDNAMap(ctx, k, 0)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    m.deleteAll_lt(2)
    lo, hi, cnt = m.items()                                  # (the table itself is held to the oracle by tests/test_table_gpu.py)
    counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    assert len(named[0]) > 3 * SG.BLOCK
    ctx.set_option("test_max_grid", grid)
    ctx.set_option("contigs_chunk_bytes", 8192)
    try:
        uses = ctx.grid_cap_uses()
        c, text = compare(g, named, m, counts, line_width=60, strands=1)
        assert ctx.grid_cap_uses() > uses and len(text) > 3 * 8192
        c.close()
        compare(g, named, line_width=0, strands=2)[0].close()
    finally:
        ctx.set_option("test_max_grid", 0)
        ctx.set_option("contigs_chunk_bytes", 0)
    g.close(); m.close()


def test_edited_graphs_and_stale_plans(ctx, tmp_path):
    k = 31
    rnd = random.Random(5 * k)
    counts = {key: 1 + rnd.randrange(40) for key in EC.branch_counts(k)}
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    old, old_text = compare(g, named, m, counts)
    old_stats = old.stats()
    # the branch goes on both strands, simplifyGraph merges what is left
    arm = [i for (s, e, q), i in zip(*named) if len(q) == 12]
    assert len(arm) == 2 and g.removeEdgesById(arm) == 2
    for call in (lambda: old.read(0, 10), old.text, lambda: old.write(tmp_path / "stale.fa")):
        with pytest.raises(L.GkError) as err:
            call()
        assert err.value.code == L.GK_E_STATE
    assert old.stats() == old_stats and not os.path.exists(tmp_path / "stale.fa") and not os.path.exists(tmp_path / "stale.fa.tmp")
    old.close()
    g.simplifyGraph()
    named = EC.edges_with_ids(g)
    for strands in (1, 2):
        compare(g, named, m, counts, strands=strands)[0].close()
    # node copies that share a k-mer: a copy of an edge's end node takes the edge's end, a copy of another's start its start
    (s0, e0, _q0), (s1, _e1, _q1) = named[0][0], named[0][1]
    c, _ = compare(g, named, strands=2)
    g.replaceEnd(named[1][0], g.addNode(e0))
    with pytest.raises(L.GkError) as err:
        c.read(0, 1)
    assert err.value.code == L.GK_E_STATE
    c.close()
    g.replaceStart(named[1][1], g.addNode(s1))
    named2 = EC.edges_with_ids(g)
    assert named2 == named
    for strands in (1, 2):
        compare(g, named2, m, counts, strands=strands)[0].close()
    # one twin only: the set is no longer strand-closed, and the stats say so
    c, _ = compare(g, named2)
    st = c.stats()
    assert st["forward"] == st["reverse"]
    fwd = [i for (s, e, q), i in zip(*named2) if CR.classify(s + q) == "forward"]
    assert g.removeEdgesById(fwd[:1]) == 1
    assert c.stats() == st
    c.close()
    named3 = EC.edges_with_ids(g)
    c, text = compare(g, named3, m, counts)
    st = c.stats()
    assert st["forward"] == st["reverse"] - 1 and b">e%d " % fwd[0] not in text
    c.close()
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_a_loaded_graph_writes_what_the_saved_one_did(ctx, k, tmp_path):
    """ids survive the graph file, so the text does; the coverage of a loaded graph's edges comes from a table counted afresh"""
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    c, text = compare(g, EC.edges_with_ids(g), m, counts, strands=2)
    c.close()
    g.save(tmp_path / "g.gkg")
    loaded = loadGraph(ctx, tmp_path / "g.gkg")
    c, text2 = compare(loaded, EC.edges_with_ids(loaded), m, counts, strands=2)
    assert text2 == text and c.stats()["missing_windows"] == 0
    EC.check(loaded, m, counts)                              # gk_graph_edge_coverage on the loaded graph, against its restatement
    c.close(); loaded.close(); g.close(); m.close()


@pytest.mark.parametrize("k", [21, 47])
def test_the_text_passes_the_fasta_check_of_its_own_graph(ctx, k):
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    c = g.contigs(line_width=60, strands=1)
    text = c.text()
    vm = g.getGraphMap()
    with FastaCheck(ctx, vm, per_line=False) as fc:
        fc.feed(text, last=True)
        st = fc.stats()
    recs = CR.parse(text)
    assert st["records"] == len(recs) == c.stats()["records"]
    assert st["missing"] == 0 and st["windows"] == sum(n - k + 1 for _i, n, _c, _s in recs) == st["found"]
    assert st["valid_bases"] == st["bases"] == c.stats()["bases"]
    vm.close(); c.close(); g.close(); m.close()


def test_errors_and_the_empty_text(ctx, tmp_path):
    k = 31
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    lib = L.lib()
    for strands in (0, 3, -1):
        with pytest.raises(L.GkError) as err:
            g.contigs(strands=strands)
        assert err.value.code == L.GK_E_INVALID
    other = HipDNAMap(ctx, k - 2, 64)
    with pytest.raises(L.GkError) as err:
        g.contigs(other)
    assert err.value.code == L.GK_E_INVALID
    # NULL handles; *out stays NULL on an error
    h = L.vp(0x1234)
    assert lib.gk_graph_contigs_plan(None, None, 0, 60, 1, C.byref(h)) == L.GK_E_INVALID and not h.value
    h = L.vp(0x1234)
    assert lib.gk_graph_contigs_plan(g.h, None, 0, 60, 7, C.byref(h)) == L.GK_E_INVALID and not h.value
    h = L.vp(0x1234)
    assert lib.gk_graph_contigs_plan(g.h, other.h, 0, 60, 1, C.byref(h)) == L.GK_E_INVALID and not h.value
    assert lib.gk_graph_contigs_plan(g.h, None, 0, 60, 1, None) == L.GK_E_INVALID
    st9 = np.zeros(9, np.uint64)
    n = C.c_uint64()
    assert lib.gk_contigs_stats(None, L.ptr(st9, C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_contigs_read(None, 0, None, 0, C.byref(n)) == L.GK_E_INVALID
    assert lib.gk_contigs_write(None, b"/dev/null") == L.GK_E_INVALID
    lib.gk_contigs_destroy(None)
    c = g.contigs()
    assert lib.gk_contigs_stats(c.h, None) == L.GK_E_INVALID and lib.gk_contigs_write(c.h, None) == L.GK_E_INVALID
    size = c.stats()["text_bytes"]
    assert size > 400 and c.read(size, 10) == b"" and c.read(size - 1, 10) == b"\n" and c.read(5, 0) == b""
    with pytest.raises(L.GkError) as err:
        c.read(size + 1, 1)
    assert err.value.code == L.GK_E_INVALID
    # a path that cannot be opened, and one that cannot be renamed onto: nothing at the path, no .tmp
    for bad in (tmp_path / "no_such_dir" / "c.fa", tmp_path / "a_dir"):
        if bad.name == "a_dir":
            bad.mkdir()
            (bad / "x").write_text("x")
        with pytest.raises(L.GkError) as err:
            c.write(bad)
        assert err.value.code == L.GK_E_INVALID and bad.name in str(err.value)
        assert not os.path.exists(str(bad) + ".tmp") and not bad.is_file()
    c.write(tmp_path / "ok.fa")
    assert (tmp_path / "ok.fa").read_bytes() == c.text() and sorted(p.name for p in tmp_path.iterdir()) == ["a_dir", "ok.fa"]
    c.close()
    # no live edge: an empty text
    live = g.counts()[1]
    assert g.removeEdgesById(np.arange(g.idBounds()[1], dtype=np.uint32)) == live and g.counts()[1] == 0
    c = g.contigs(m)
    assert c.stats() == dict.fromkeys(CONTIG_STATS, 0) and c.text() == b"" and c.read(0, 5) == b""
    c.write(tmp_path / "empty.fa")
    assert (tmp_path / "empty.fa").read_bytes() == b""
    c.close()
    other.close(); g.close(); m.close()
