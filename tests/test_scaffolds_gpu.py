"""gk_graph_scaffolds_plan / gk_scaffolds_read / gk_scaffolds_write / gk_scaffolds_segments on the device (-m gpu) against the
restatement (tests/scaffolds_ref.py, held to hand-written texts by tests/test_scaffolds_cpu.py) on the ORACLE's graph of the same
reads: the text byte for byte, the thirteen stats and the segment rows.  An edge is its content (start k-mer, first base); the
device's id of it names it in the text.  Fixtures: insert_cases.small_pairs, a 2400-base genome, at most 800 pairs, as the links
tests.  Every case first asserts, on the restatement alone, that the classes it is about are populated."""
import ctypes as C
import os

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd.dnamap import Context
from genome_amd.graph import SCAFFOLD_STATS, loadGraph, scaffoldChains, scaffoldGaps
from insert_cases import small_pairs
from links_cases import settings
import scaffolds_cases as SC
import scaffolds_ref as SR
from test_links_gpu import TABLE, device_graph, edge_keys, link

pytestmark = pytest.mark.gpu
assert SCAFFOLD_STATS == SR.STATS
I31 = (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def named_edges(g, k, reads):
    """the oracle's edges under the device's ids: {id: (start k-mer, end k-mer, seq)}, and content key -> id"""
    oe = SC.oracle_edges(k, reads)
    keys = edge_keys(g)
    assert sorted(keys.values()) == sorted(oe)
    return {i: oe[key] for i, key in keys.items()}, {key: i for i, key in keys.items()}


def compare(g, edges, chains, gaps, **kw):
    """the device's text, stats and segments == the restatement's; -> (Scaffolds, text, stats)"""
    want_text, want_st, want_rows = SR.scaffolds(edges, chains, gaps, **kw)
    s = g.scaffolds(chains, gaps, **kw)
    st = s.stats()
    assert tuple(st) == SR.STATS and st == want_st
    assert st["chains"] == st["chain_forward"] + st["chain_self_twin"] + st["chain_reverse"] and st["records"] <= st["chains"] + st["singletons"]
    text = s.text()
    assert text == want_text and b"\n\n" not in text
    assert s.segments() == want_rows
    return s, text, st


@pytest.fixture(scope="module")
def built(ctx):
    """per k: the graph, the oracle's edges under its ids and the constructed chains (scaffolds_cases.constructed), made once"""
    cache = {}

    def get(k):
        if k not in cache:
            reads = small_pairs(100 + k, k)
            g, vm = device_graph(ctx, k, reads)
            edges, ids = named_edges(g, k, reads)
            chains, gaps = SC.constructed(SC.oracle_edges(k, reads), k)
            cache[k] = (reads, g, vm, edges, [[ids[key] for key in c] for c in chains], gaps)
        return cache[k]

    yield get
    for _reads, g, vm, *_ in cache.values():
        vm.close(); g.close()


# ---- 1. the chains the links give ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 31])
def test_chains_from_the_links(ctx, built, k):
    reads, g, vm, edges, _, _ = built(k)
    S = settings(k)
    links, _ = link(g, vm, reads, min_len=S["min_len"], max_span=S["max_span"])
    joins, jst = links.joins(S["support"])
    assert jst["joins"] == TABLE[(k, 0.0)][3]
    chains = scaffoldChains(joins[0], joins[1])
    gaps = scaffoldGaps(chains, joins, 90)
    assert all(len(gp) == len(c) - 1 for c, gp in zip(chains, gaps)) and sum(len(c) - 1 for c in chains) == jst["joins"]
    _, st, _ = SR.scaffolds(edges, chains, gaps, strands=2, min_len=S["min_len"])
    assert st["adjacent"] > 0 and st["gapped"] > 0 and st["clamped"] > 0 and st["singletons"] > 0
    assert st["chain_forward"] == st["chain_reverse"] > 0                 # an unedited graph: every chain comes with its twin chain
    fp = g.idFingerprint()
    for strands in (1, 2):
        for singletons in (False, True):
            for lw in (0, 1, 7, 60, 61):
                s, text, got = compare(g, edges, chains, gaps, min_len=S["min_len"], line_width=lw, strands=strands, singletons=singletons)
                assert got["records"] == (got["chain_forward"] + got["chain_self_twin"] if strands == 1 else got["chains"]) + got["singletons"]
                assert (got["singletons"] > 0) == singletons
                s.close()
    assert g.idFingerprint() == fp
    links.close()


# ---- 2. every key width, constructed chains ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 31, 34, 47, 64])
def test_every_key_width_with_constructed_chains(built, k):
    """one word (21, 31), four bits of the high word (34), two words (47, 64): adjacent junctions by construction, every gap of
    GAPS at a gapped one (1000: an N run longer than the 512 bytes a wave writes), a chain of one member, a chain with its exact
    twin chain, an edge followed by its own twin"""
    _reads, g, _vm, edges, chains, gaps = built(k)
    used = {x for c, gp in zip(chains, gaps) for a, b, x in zip(c, c[1:], gp) if SR.junction(edges, None, a, b) == "gapped"}
    assert used == set(SC.GAPS) and any(len(c) == 1 for c in chains)
    _, st, _ = SR.scaffolds(edges, chains, gaps, strands=2)
    assert st["adjacent"] > 0 and st["gapped"] > st["clamped"] > 0 and st["n_bases"] >= 1000 and st["chain_self_twin"] == 1
    assert st["chain_forward"] > 0 and st["chain_reverse"] > 0
    a, b = (SR.classify(SR.assemble(edges, chains[i], gaps[i], 10)[0]) for i in (0, 1))
    assert {a, b} == {"forward", "reverse"}                                # the chain and its twin chain
    fp = g.idFingerprint()
    for strands in (1, 2):
        for singletons in (False, True):
            s, text, got = compare(g, edges, chains, gaps, strands=strands, singletons=singletons)
            # 7. independent of the restatement's assembly: the members' paths lie in the record in order and cover what is not N
            recs = SR.parse(text)
            assert len(recs) == got["records"]
            for name, _n, seq in recs:
                if name[0] == "s":
                    assert SC.covered([edges[e][0] + edges[e][2] for e in chains[int(name[1:])]], seq), name
                else:
                    assert seq == edges[int(name[1:])][0] + edges[int(name[1:])][2]
            s.close()
    one, text1, _ = compare(g, edges, chains, gaps, strands=1, singletons=False, min_gap=1, line_width=0)
    assert text1.count(b">s0 ") + text1.count(b">s1 ") == 1
    one.close()
    assert g.idFingerprint() == fp


# ---- 3. chunks, offsets, the file ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [8, 24, 4096])
def test_chunks_and_unaligned_reads(ctx, built, chunk, tmp_path):
    _reads, g, _vm, edges, chains, gaps = built(31)
    want, st, _ = SR.scaffolds(edges, chains, gaps, strands=2, line_width=60)
    assert len(want) > 2 * 4096 and st["n_bases"] >= 1000
    ctx.set_option("contigs_chunk_bytes", chunk)
    try:
        s, text, _ = compare(g, edges, chains, gaps, strands=2, line_width=60)
        path = tmp_path / "s.fa"
        s.write(path)
        assert path.read_bytes() == text and not os.path.exists(str(path) + ".tmp")
        ms = s.last_ms()
        assert ms["emit_kernels"] > 0 and ms["total"] > 0
        first_n = text.index(b"N")
        for start in (0, text.index(b"\n") - 3, first_n - 5, text.index(b">", 1) - 9, len(text) - 40):
            for off in range(start, start + 8):                         # every offset mod 8
                for n in (1, 5, 13, 30):                                 # lengths that end inside a word
                    assert s.read(off, n) == text[off:off + n], (off, n)
        assert s.read(len(text), 4) == b"" and s.read(3, 0) == b"" and s.read(1, len(text)) == text[1:]
        s.close()
    finally:
        ctx.set_option("contigs_chunk_bytes", 0)


# ---- 4. small launch grids -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [1, 3])
def test_small_launch_grids(ctx, built, grid):
    """1 and 3 workgroups per launch: four waves take fourteen chains and sixty edges, a 10 KB text goes out in several trips"""
    _reads, g, _vm, edges, chains, gaps = built(31)
    assert len(chains) > 3 * 4 and len(edges) > 3 * 4
    ctx.set_option("test_max_grid", grid)
    ctx.set_option("contigs_chunk_bytes", 4096)
    try:
        uses = ctx.grid_cap_uses()
        for strands in (1, 2):
            compare(g, edges, chains, gaps, strands=strands, line_width=7)[0].close()
        assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)
        ctx.set_option("contigs_chunk_bytes", 0)


# ---- 5. no chains --------------------------------------------------------------------------------------------------------------

def test_no_chains_is_the_contig_text(built):
    _reads, g, _vm, edges, _, _ = built(31)
    for strands in (1, 2):
        for min_len, lw in ((0, 60), (80, 0), (80, 7)):
            c = g.contigs(min_len=min_len, line_width=lw, strands=strands)
            s, text, st = compare(g, edges, [], [], min_len=min_len, line_width=lw, strands=strands)
            assert text == c.text() and len(text) > 1000
            assert st["records"] == st["singletons"] == c.stats()["records"] and st["bases"] == c.stats()["bases"] and st["chains"] == 0
            s.close(); c.close()
    s = g.scaffolds([], [], singletons=False)
    assert s.text() == b"" and s.stats() == dict.fromkeys(SCAFFOLD_STATS, 0) and s.segments() == []
    s.close()


# ---- 6. errors, stale plans, a loaded graph ------------------------------------------------------------------------------------

def raw_plan(g, members, off, gap, min_gap=10, min_len=0, line_width=60, strands=1, singletons=1, handle=True, null=()):
    """the C call itself -> (return code, *out), which starts as a pattern"""
    m, o, gp = np.array(members, np.uint32), np.array(off, np.uint64), np.array(gap, np.int64)
    h = L.vp(0x1234)
    rc = L.lib().gk_graph_scaffolds_plan(g.h if handle else None, None if "members" in null else L.ptr(m, C.c_uint32),
                                         None if "off" in null else L.ptr(o, C.c_uint64), len(off) - 1, None if "gap" in null else L.ptr(gp, C.c_int64),
                                         min_gap, min_len, line_width, strands, singletons, C.byref(h))
    return rc, h.value


def test_errors_leave_out_null_and_the_graph_alone(ctx, built, tmp_path):
    k = 31
    reads, g0, _vm, edges0, _, _ = built(k)
    g, vm = device_graph(ctx, k, reads)
    vm.close()
    edges, _ = named_edges(g, k, reads)
    assert edges == edges0                                               # (the same build twice gives the same ids)
    ids = sorted(edges)
    far = lambda a: next(b for b in ids if b != a and edges[b][0] != edges[a][1] and edges[a][0] != edges[b][1])
    a = ids[0]
    b = far(a)
    c = next(x for x in ids if x not in (a, b) and edges[x][0] != edges[b][1] and edges[x][0] != edges[a][1])
    near = next((x, y) for x in ids for y in ids if x != y and not {x, y} & {a, b, c} and edges[x][1] == edges[y][0])
    bound = g.idBounds()[1]
    fp = g.idFingerprint()
    bad = L.GK_E_INVALID
    cases = [
        (dict(members=[a, bound], off=[0, 2], gap=[0, 0]), bad),                        # an id at the bound
        (dict(members=[a, 0xfffffffe], off=[0, 2], gap=[0, 0]), bad),
        (dict(members=[a, b, a], off=[0, 3], gap=[0, 0, 0]), bad),                      # twice in one chain
        (dict(members=[a, b, c, a], off=[0, 2, 4], gap=[0] * 4), bad),                  # twice in two chains
        (dict(members=[a, b], off=[0, 2, 2], gap=[0, 0]), bad),                         # an empty chain
        (dict(members=[a, b], off=[0, 0, 2], gap=[0, 0]), bad),
        (dict(members=[a, b, c], off=[0, 3, 2], gap=[0, 0, 0]), bad),                   # chain_off does not ascend
        (dict(members=[a, b], off=[1, 2], gap=[0, 0]), bad),                            # does not start at 0
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], min_gap=0), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], min_gap=-3), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], min_gap=I31 + 1), bad),
        (dict(members=[a, b], off=[0, 2], gap=[I31 + 1, 0]), bad),                      # a used gap above 2^31-1
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], strands=0), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], strands=3), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], line_width=I31 + 1), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], handle=False), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], null=("members",)), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], null=("gap",)), bad),
        (dict(members=[a, b], off=[0, 2], gap=[0, 0], null=("off",)), bad),
        (dict(members=[a, b, c], off=[0, 3], gap=[I31, I31, 0], strands=2), L.GK_E_CAPACITY),      # 2^32 - 2 bases N and three paths
    ]
    for kw, code in cases:
        rc, h = raw_plan(g, **kw)
        assert (rc, h) == (code, None), kw
        assert g.idFingerprint() == fp
    assert L.lib().gk_graph_scaffolds_plan(g.h, None, None, 0, None, 10, 0, 60, 1, 1, None) == bad
    # what is NOT an error: the largest gap where none is used (the last member, an adjacent junction), min_gap at its bounds
    for kw in (dict(members=[a, b], off=[0, 2], gap=[5, I31 + 1]), dict(members=list(near), off=[0, 2], gap=[I31 + 1, 0]),
               dict(members=[a, b], off=[0, 2], gap=[0, 0], min_gap=1), dict(members=[a], off=[0, 1], gap=[0], min_gap=I31)):
        rc, h = raw_plan(g, **kw)
        assert rc == L.GK_OK and h, kw
        L.lib().gk_scaffolds_destroy(h)
    lib = L.lib()
    n, st13 = C.c_uint64(7), np.zeros(13, np.uint64)
    assert lib.gk_scaffolds_stats(None, L.ptr(st13, C.c_uint64)) == bad and lib.gk_scaffolds_read(None, 0, None, 0, C.byref(n)) == bad
    assert lib.gk_scaffolds_write(None, b"/dev/null") == bad and lib.gk_scaffolds_segments(None, None, None, None, None, None, 0, C.byref(n)) == bad
    lib.gk_scaffolds_destroy(None)
    # segments with less room than needed: *n set, nothing copied
    chains, gaps = [[a, b], list(near)], [[-4], [0]]
    s, text, st = compare(g, edges, chains, gaps, strands=2)
    rows = st["members"] + st["singletons"]
    assert lib.gk_scaffolds_segments(s.h, None, None, None, None, None, rows - 1, C.byref(n)) == L.GK_E_CAPACITY and n.value == rows
    assert lib.gk_scaffolds_stats(s.h, None) == bad and lib.gk_scaffolds_write(s.h, None) == bad
    with pytest.raises(L.GkError) as err:
        s.read(len(text) + 1, 1)
    assert err.value.code == bad
    with pytest.raises(L.GkError) as err:
        s.write(tmp_path / "no_such_dir" / "s.fa")
    assert err.value.code == bad and "no_such_dir" in str(err.value)
    # a loaded graph gives the saved graph's text
    g.save(tmp_path / "g.gkg")
    loaded = loadGraph(ctx, tmp_path / "g.gkg")
    s2, text2, _ = compare(loaded, edges, chains, gaps, strands=2)
    assert text2 == text
    s2.close(); loaded.close()
    # a dead member; the plan made before the edit is stale and its numbers still answer
    assert g.removeEdgesById([c]) == 1
    for call in (lambda: s.read(0, 10), s.text, lambda: s.write(tmp_path / "stale.fa")):
        with pytest.raises(L.GkError) as err:
            call()
        assert err.value.code == L.GK_E_STATE
    assert s.stats() == st and len(s.segments()) == rows and not os.path.exists(tmp_path / "stale.fa") and not os.path.exists(tmp_path / "stale.fa.tmp")
    s.close()
    fp = g.idFingerprint()
    assert raw_plan(g, members=[a, c], off=[0, 2], gap=[0, 0]) == (bad, None) and g.idFingerprint() == fp
    del edges[c]
    compare(g, edges, chains, gaps, strands=1)[0].close()
    g.close()
    assert g0.h                                                          # (the shared graph was not the one edited)
