"""gk_graph_edge_twins and gk_graph_gfa_plan / gk_gfa_* on the device against the restatement (tests/gfa_ref.py): twins, classes
and the six stats; the GFA text byte for byte and the nine stats (-m gpu).  Every text also passes the independent checker of
tests/test_gfa_cpu.py.

The graphs: the branch graphs of tests/test_edge_coverage_gpu.py for every key width, with and without a count table; the folded
graphs of tests/folded_cases.py; graphs after simplifyGraph, after the removal of one twin, after a span split that leaves two
copies of one path and after the simplifyGraph that merges them, after clipTips and popBubbles; content keys cut to 0 and 3 bits;
an edge of 70 000 bases read in pieces; a graph of a few thousand edges under launch grids of 1 and 3 workgroups; a loaded
graph; and the error paths.
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import GFA_STATS, TWIN_CLASSES, TWIN_STATS, buildGraph, loadGraph
from oracle import pyref as R

import folded_cases as FC
import gfa_ref as GR
import small_grid_cases as SG
import test_edge_coverage_gpu as EC
from test_gfa_cpu import check_gfa
from test_spans_gpu import by_id, graph_of, pieces, spans_of

pytestmark = pytest.mark.gpu
KS = [5, 21, 31, 34, 47, 63, 64]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_option("test_max_grid", 0)
    c.set_option("twin_key_bits", 128)
    c.set_option("contigs_chunk_bytes", 0)
    c.close()


def model(g):
    """the device graph as the restatement takes it -> (edges (start k-mer, end k-mer, seq), ids, start node ids, end node ids)"""
    nodes, edges = by_id(g)
    ids = [e for e, x in enumerate(edges) if x is not None]
    return [(nodes[edges[e][0]], nodes[edges[e][1]], edges[e][2]) for e in ids], ids, [edges[e][0] for e in ids], [edges[e][1] for e in ids]


def compare(g, m=None, counts=None, strand_closed=True, mdl=None):
    """device twins, classes, stats, GFA text and stats == the restatement's -> (twin stats, gfa stats, text)"""
    assert GR.TWIN_STATS == TWIN_STATS and GR.TWIN_CLASSES == TWIN_CLASSES and GR.GFA_STATS == GFA_STATS
    edges, ids, starts, ends = mdl or model(g)
    want_twin, want_cls, want_st = GR.twins(edges, ids)
    twin, cls, st = g.edgeTwins()
    collisions = st.pop("key_collisions")
    want_st = {x: v for x, v in want_st.items() if x != "key_collisions"}
    assert st == want_st
    assert st["live_edges"] == st["paired"] + st["self"] + st["missing"] + st["ambiguous"] == g.counts()[1] and st["paired"] % 2 == 0
    live = set(ids)
    for e in range(len(twin)):
        if e in live:
            assert (int(twin[e]), TWIN_CLASSES[cls[e]]) == (want_twin[e], want_cls[e]), e
        else:
            assert (int(twin[e]), TWIN_CLASSES[cls[e]]) == (GR.NONE, "dead")
    # asked by id, in another order, with an out-of-range id
    ask = np.array(ids[::-1][:7] + [len(twin) + 5], np.uint32)
    t2, c2, st2 = g.edgeTwins(ask)
    assert st2["live_edges"] == st["live_edges"] and t2[-1] == GR.NONE and c2[-1] == 0
    assert t2[:-1].tolist() == [want_twin[e] for e in ask[:-1].tolist()]
    want_text, want_gst = GR.gfa(edges, ids, starts, ends, g.k, counts)
    p = g.gfa(m)
    gst = p.stats()
    assert tuple(gst) == GFA_STATS and gst == want_gst
    assert gst["live_edges"] == gst["segments"] + gst["folded"] and gst["pairs"] == gst["links"] + gst["mirrored"]
    text = p.text()
    assert text == want_text
    p.close()
    closed = strand_closed and st["missing"] == 0 and st["ambiguous"] == 0
    check_gfa(text, g.k, edges if closed else None, st if closed else None, want_kc=counts is not None)
    st["key_collisions"] = collisions
    return st, gst, text


@pytest.mark.parametrize("k", KS)
def test_every_key_width(ctx, k):
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    fp, chk = g.idFingerprint(), g.checksum()
    mdl = model(g)
    st, gst, text = compare(g, mdl=mdl)
    assert st["missing"] == st["ambiguous"] == st["key_collisions"] == 0 and st["paired"] >= 6 and gst["links"] >= 2 and b"KC:i:" not in text
    st, gst, text = compare(g, m, counts, mdl=mdl)
    assert gst["missing_windows"] == 0 and text.count(b"\tKC:i:") == gst["segments"]
    # a table that lacks every 7th k-mer: they count 0 and missing_windows is exact
    fewer = {key: c for i, (key, c) in enumerate(counts.items()) if i % 7}
    lacking = EC.fill(ctx, k, fewer)
    assert compare(g, lacking, fewer, mdl=mdl)[1]["missing_windows"] > 10
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)                # the graph is as it was
    lacking.close(); g.close(); m.close()


@pytest.mark.parametrize("variant", ["clean", "noisy"])
@pytest.mark.parametrize("k", FC.KS)
def test_folded_graphs(ctx, k, variant):
    """self-loops, self-twin edges, two-cycles and (even k) palindromic nodes, whose pair with its twin is its own mirror"""
    c = FC.case(k, FC.SEEDS[k], variant)
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(c.graph_reads), len(c.graph_reads))
    if c.min_count > 1:
        m.deleteAll_lt(c.min_count)
    g = buildGraph(k, m)
    st, gst, _ = compare(g, m, c.counts())
    want = FC.TABLE[(k, variant)]
    assert st["live_edges"] == want["edges"] and st["self"] == want["self_twin"] >= 1 and st["missing"] == st["ambiguous"] == 0
    assert gst["mirrored"] >= 10 and gst["missing_windows"] == 0
    g.close(); m.close()


def test_edited_graphs(ctx):
    k = 31
    rnd = random.Random(5 * k)
    counts = {key: 1 + rnd.randrange(40) for key in EC.branch_counts(k)}
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    named = EC.edges_with_ids(g)
    arm = [i for (s, e, q), i in zip(*named) if len(q) == 12]
    assert len(arm) == 2 and g.removeEdgesById(arm) == 2
    compare(g, m, counts)
    g.simplifyGraph()
    st, gst, _ = compare(g, m, counts)
    assert st["missing"] == 0 and st["paired"] == st["live_edges"]
    # one twin goes: the other is `missing`, stays a segment of its own and keeps its links
    edges, ids, _s, _e = model(g)
    victim = [i for (s, _e2, q), i in zip(edges, ids) if GR.classify(s + q) == "forward"][0]
    twin_of = int(g.edgeTwins([victim])[0][0])
    assert g.removeEdgesById([victim]) == 1
    st, gst, text = compare(g, m, counts, strand_closed=False)
    assert st["missing"] == 1 and g.edgeTwins([twin_of])[1][0] == TWIN_CLASSES.index("missing") and b"S\te%d\t" % twin_of in text
    g.close(); m.close()


def test_copies_of_one_path_and_their_merge(ctx):
    """A R B R C: the span split leaves two live copies of the repeat's edge per strand (the copies of a split share every k-mer)
    until simplifyGraph merges them with their flanks"""
    k = 35
    A, Rp, B, Cc = pieces(k, k, [300, k + 60, 280, 310], lambda A, Rp, B, Cc: [A + Rp + B + Rp + Cc])
    g, reads = graph_of(ctx, k, [A + Rp + B + Rp + Cc])
    st, _, _ = compare(g)
    assert st["ambiguous"] == 0 and st["missing"] == 0
    sp, _ = spans_of(g, reads)
    assert g.splitEdgesBySpans(sp, 3)["new_edges"] == 2
    st, gst, text = compare(g, strand_closed=False)
    assert st["ambiguous"] == 4 and st["missing"] == 0 and gst["segments"] == 4 + st["paired"] // 2 + st["self"]
    assert text.count(b"\t" + Rp.encode() + b"\t") == 2 and text.count(b"\t" + R.rev_comp(Rp).encode() + b"\t") == 2
    g.simplifyGraph()
    st, _, _ = compare(g)
    assert st["ambiguous"] == 0 and st["missing"] == 0
    sp.close(); g.close()


def test_tips_and_bubbles_keep_the_graph_strand_closed(ctx):
    """the check the header's twin arguments for clipTips and popBubbles never had: no edge loses its twin"""
    k = 11
    reads = SG.reads_case(k)
    m = HipDNAMap(ctx, k, 0)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    m.deleteAll_lt(2)
    g = buildGraph(k, m)
    before = g.edgeTwins()[2]
    assert before["missing"] == 0 and before["ambiguous"] == 0
    clipped = g.clipTips(m)
    st = g.edgeTwins()[2]
    assert clipped > 0 and st["missing"] == 0 and st["live_edges"] == before["live_edges"] - clipped
    g.simplifyGraph()
    assert g.edgeTwins()[2]["missing"] == 0
    popped, _ = g.popBubbles(m)
    st = g.edgeTwins()[2]
    assert popped > 0 and st["missing"] == 0
    g.simplifyGraph()
    st = g.edgeTwins()[2]
    assert st["missing"] == 0 and st["ambiguous"] == 0
    g.close(); m.close()


def test_truncated_keys_give_the_same_answers(ctx):
    """content keys of 0 and 3 bits: every run holds many edges of other content, and the confirmation decides"""
    k = 12
    c = FC.case(k, FC.SEEDS[k], "noisy")
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(c.graph_reads), len(c.graph_reads))
    m.deleteAll_lt(c.min_count)
    g = buildGraph(k, m)
    mdl = model(g)
    assert 150 <= len(mdl[1]) <= 600
    seen = {}
    try:
        for bits in (128, 3, 0):
            ctx.set_option("twin_key_bits", bits)
            st, _, text = compare(g, mdl=mdl)
            twin, cls, _ = g.edgeTwins()
            seen[bits] = (twin.tolist(), cls.tolist(), text, st["key_collisions"])
    finally:
        ctx.set_option("twin_key_bits", 128)
    assert seen[0][:3] == seen[3][:3] == seen[128][:3]
    assert seen[128][3] == 0 and seen[3][3] > 0 and seen[0][3] > seen[3][3]
    for bad in (-1, 129):
        with pytest.raises(L.GkError) as err:
            ctx.set_option("twin_key_bits", bad)
        assert err.value.code == L.GK_E_INVALID
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_long_edge_in_small_pieces(ctx, k, tmp_path):
    """one edge of 70 000 bases and its twin: one S line of more than 65 535 bytes, read in pieces of 8 bytes and 4 KiB"""
    rnd = random.Random(31 * k)
    s = EC.rand_seq(rnd, 70000)
    keys = {R.canon(s[i:i + k]) for i in range(len(s) - k + 1)}
    assert len(keys) == len(s) - k + 1
    m = EC.fill(ctx, k, dict.fromkeys(keys, 3))
    g = buildGraph(k, m)
    fwd = s if GR.classify(s) == "forward" else R.rev_comp(s)
    edges, ids, starts, ends = model(g)
    assert len(ids) == 2
    ctx.set_option("contigs_chunk_bytes", 4096)
    try:
        twin, cls, st = g.edgeTwins()
        assert st["paired"] == 2 and int(twin[ids[0]]) == ids[1] and int(twin[ids[1]]) == ids[0]
        p = g.gfa(m)
        text = p.text()
        want, want_st = GR.gfa(edges, ids, starts, ends, k, dict.fromkeys(keys, 3))
        assert text == want and p.stats() == want_st and want_st["segments"] == 1 and want_st["links"] == 0
        assert b"\t" + fwd.encode() + b"\tLN:i:70000\tKC:i:%d\n" % (3 * (70000 - k + 1)) in text
        for size in (8, 4096):
            parts, at = [], 0
            while at < len(text):
                piece = p.read(at, size)
                assert len(piece) == min(size, len(text) - at)
                parts.append(piece)
                at += len(piece)
            assert b"".join(parts) == text
        for off, n in ((0, 11), (9, 5), (3, 4095), (4093, 9), (len(text) - 5, 50), (len(text), 4), (12, 8200), (1, 1)):
            assert p.read(off, n) == text[off:off + n], (off, n)
        p.write(tmp_path / "long.gfa")
        assert (tmp_path / "long.gfa").read_bytes() == text and not os.path.exists(str(tmp_path / "long.gfa") + ".tmp")
        assert p.last_ms()["total"] > 0
        p.close()
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
    lo, hi, cnt = m.items()
    counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
    g = buildGraph(k, m)
    mdl = model(g)
    assert len(mdl[1]) > 3 * SG.BLOCK and len(mdl[1]) % 64
    ctx.set_option("test_max_grid", grid)
    ctx.set_option("contigs_chunk_bytes", 8192)
    try:
        uses = ctx.grid_cap_uses()
        st, gst, text = compare(g, m, counts, mdl=mdl)
        assert ctx.grid_cap_uses() > uses and len(text) > 3 * 8192 and gst["mirrored"] > SG.BLOCK
    finally:
        ctx.set_option("test_max_grid", 0)
        ctx.set_option("contigs_chunk_bytes", 0)
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_a_loaded_graph_writes_what_the_saved_one_did(ctx, k, tmp_path):
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    _, _, text = compare(g, m, counts)
    g.save(tmp_path / "g.gkg")
    loaded = loadGraph(ctx, tmp_path / "g.gkg")
    assert compare(loaded, m, counts)[2] == text
    loaded.close(); g.close(); m.close()


def test_errors_stale_plans_and_the_empty_graph(ctx, tmp_path):
    k = 31
    counts = EC.branch_counts(k)
    m = EC.fill(ctx, k, counts)
    g = buildGraph(k, m)
    lib = L.lib()
    other = HipDNAMap(ctx, k - 2, 64)
    with pytest.raises(L.GkError) as err:
        g.gfa(other)
    assert err.value.code == L.GK_E_INVALID
    h = L.vp(0x1234)
    assert lib.gk_graph_gfa_plan(None, None, C.byref(h)) == L.GK_E_INVALID and not h.value
    h = L.vp(0x1234)
    assert lib.gk_graph_gfa_plan(g.h, other.h, C.byref(h)) == L.GK_E_INVALID and not h.value
    assert lib.gk_graph_gfa_plan(g.h, None, None) == L.GK_E_INVALID
    st9, st6 = np.zeros(9, np.uint64), np.zeros(6, np.uint64)
    n = C.c_uint64()
    assert lib.gk_gfa_stats(None, L.ptr(st9, C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_gfa_read(None, 0, None, 0, C.byref(n)) == L.GK_E_INVALID
    assert lib.gk_gfa_write(None, b"/dev/null") == L.GK_E_INVALID
    assert lib.gk_gfa_last_ms(None, (C.c_float * 4)()) == L.GK_E_INVALID
    assert lib.gk_graph_edge_twins(None, None, 0, None, None, L.ptr(st6, C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_graph_edge_twins(g.h, None, 3, None, None, None) == L.GK_E_INVALID
    assert lib.gk_graph_edge_twins(g.h, None, 0, None, None, L.ptr(st6, C.c_uint64)) == L.GK_OK and st6[0] == g.counts()[1]
    lib.gk_gfa_destroy(None)
    p = g.gfa()
    assert lib.gk_gfa_stats(p.h, None) == L.GK_E_INVALID and lib.gk_gfa_write(p.h, None) == L.GK_E_INVALID
    size = p.stats()["text_bytes"]
    assert size > 400 and p.read(size, 10) == b"" and p.read(size - 1, 10) == b"\n" and p.read(5, 0) == b""
    with pytest.raises(L.GkError) as err:
        p.read(size + 1, 1)
    assert err.value.code == L.GK_E_INVALID
    with pytest.raises(L.GkError) as err:
        p.write(tmp_path / "no_such_dir" / "g.gfa")
    assert err.value.code == L.GK_E_INVALID
    # any edit makes the plan stale; its stats still answer
    old_stats = p.stats()
    live = g.counts()[1]
    assert g.removeEdgesById(np.arange(g.idBounds()[1], dtype=np.uint32)) == live and g.counts()[1] == 0
    for call in (lambda: p.read(0, 10), p.text, lambda: p.write(tmp_path / "stale.gfa")):
        with pytest.raises(L.GkError) as err:
            call()
        assert err.value.code == L.GK_E_STATE
    assert p.stats() == old_stats and not os.path.exists(tmp_path / "stale.gfa") and not os.path.exists(tmp_path / "stale.gfa.tmp")
    p.close()
    with pytest.raises(L.GkError):
        p.stats()
    # no live edge: the header alone
    p = g.gfa(m)
    want = dict.fromkeys(GFA_STATS, 0)
    want["text_bytes"] = 11
    assert p.stats() == want and p.text() == b"H\tVN:Z:1.0\n" and p.read(2, 4) == b"VN:Z"
    p.write(tmp_path / "empty.gfa")
    assert (tmp_path / "empty.gfa").read_bytes() == b"H\tVN:Z:1.0\n"
    p.close()
    assert g.edgeTwins()[2] == dict.fromkeys(TWIN_STATS, 0)
    other.close(); g.close(); m.close()
