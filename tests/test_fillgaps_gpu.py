"""gk_graph_fill_gaps on the device (-m gpu) against the restatement (tests/fillgaps_ref.py, held to hand-computed cases by
tests/test_fillgaps_cpu.py): the filled chains, their gaps, the class and length of every junction and all ten stats.  Graphs:
the device graph of insert_cases.small_pairs with the point edits of tests/fillgaps_cases.py applied (the unedited graph holds
no bubble and no cycle); the restatement works on the ids, nodes and lengths read back through edgesById.  That the cases hold
every class is asserted without a GPU, in tests/test_fillgaps_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd.dnamap import Context
from genome_amd.graph import FILL_CLASSES, FILL_STATS, loadGraph
from insert_cases import small_pairs
import fillgaps_cases as FC
import fillgaps_ref as FR
import scaffolds_cases as SC
import scaffolds_ref as SR
from test_links_gpu import device_graph, edge_keys

pytestmark = pytest.mark.gpu
assert FILL_STATS == FR.STATS and FILL_CLASSES == FR.CLASSES
I31 = (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def by_id(g):
    """{edge id: (start node id, end node id, len)} of the live edges, as the device holds them now"""
    ids = np.arange(g.idBounds()[1], dtype=np.uint32)
    info = g.edgesById(ids)
    return {int(e): (int(info["start"][e]), int(info["end"][e]), int(info["len"][e])) for e in ids if info["alive"][e]}


def edit(g, k, edits, ids):
    """fillgaps_cases' edits on the device; an added node's k-mer is of no interest to the rule"""
    new = {}
    for op, *a in edits:
        if op == "node":
            new[("new", a[0])] = g.addNode("A" * k)
        elif op == "start":
            g.replaceStart(ids[a[0]], new[a[1]])
        elif op == "end":
            g.replaceEnd(ids[a[0]], new[a[1]])


@pytest.fixture(scope="module")
def planted(ctx):
    cache = {}

    def get(k):
        if k not in cache:
            g, vm = device_graph(ctx, k, small_pairs(100 + k, k))
            vm.close()
            ids = {key: i for i, key in edge_keys(g).items()}
            edits, chains, exact, kinds = FC.planted(k)
            edit(g, k, edits, ids)
            cache[k] = (g, [[ids[x] for x in c] for c in chains], exact, kinds)
        return cache[k]

    yield get
    for g, *_ in cache.values():
        g.close()


def compare(g, edges, chains, gaps, tol, me, mp, displaced=()):
    want = FR.fill(edges, g.k, chains, gaps, tol, me, mp, displaced=displaced)
    got = g.fillGaps(chains, gaps, tol, max_edges=me, max_paths=mp)
    assert got == want, (tol, me, mp)
    assert got[2]["junctions"] == sum(got[2][n] for n in FR.STATS[1:7])
    return got


@pytest.mark.parametrize("k", FC.KS)
def test_the_device_equals_the_restatement(planted, k):
    """two key widths and every parameter of fillgaps_cases.sweep: max_paths 1, 4, 64 and GK_FILL_MAX_PATHS, max_edges 1, 3, 8,
    every gap at L - tol - 1, L - tol, L, L + tol, L + tol + 1"""
    g, chains, exact, kinds = planted(k)
    edges = by_id(g)
    fp = g.idFingerprint()
    filled = back = 0
    for tol, mp, me, d in FC.sweep():
        rep = compare(g, edges, chains, FC.gaps(exact, d), tol, me, mp)[2]
        filled += rep["filled"]; back += rep["searched_backward"]
    assert filled > 0 and back > 0 and g.idFingerprint() == fp
    # the wide gadget alone: a frontier of several trips of a wave, a tree over 64 and within GK_FILL_MAX_PATHS, and paths of up to
    # eight edges unwound (five times one loop and out; what class that is, the restatement says)
    (c, j, (lp, lq, ly)), = kinds[FC.WIDE]
    for G in (exact[c][j], 5 * lp + ly - k, 5 * lq + ly - k, 3 * lp + 4 * lq + ly - k):
        for mp in (64, 764, 765, 1024):
            compare(g, edges, [chains[c]], [[G]], 0, 8, mp)
    # the first line alone: five edges unwound and written
    c, j, m = kinds["line"][0]
    got = compare(g, edges, [chains[c]], [exact[c]], 0, 8, 1024)
    assert m == 5 and len(got[0][0]) == 7 and got[2]["filled"] == 1 and compare(g, edges, [chains[c]], [exact[c]], 0, 4, 1024)[2]["none"] == 1
    assert max(sum(1 for v in edges.values() if v[1] == n) for n in {v[1] for v in edges.values()}) > 4      # an in-list longer than four


@pytest.mark.parametrize("grid", [1, 3])
def test_small_launch_grids(ctx, planted, grid):
    g, chains, exact, _ = planted(31)
    edges = by_id(g)
    assert len(chains) > 3 * 4
    ctx.set_option("test_max_grid", grid)
    try:
        uses = ctx.grid_cap_uses()
        for tol, mp, me, d in ((0, 1024, 8, 0), (12, 4, 3, 12), (3, 1, 8, -3)):
            compare(g, edges, chains, FC.gaps(exact, d), tol, me, mp)
        assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)


def test_a_removed_filler_edge(ctx):
    """a graph of its own: the planted edits, then a filler edge is removed (the file format refuses the planted graph: its added
    nodes' k-mers are not their edges'; test_filled_scaffolds_hold_no_n loads a saved graph)"""
    k = 21
    g, vm = device_graph(ctx, k, small_pairs(100 + k, k))
    vm.close()
    ids = {key: i for i, key in edge_keys(g).items()}
    edits, chains, exact, kinds = FC.planted(k)
    edit(g, k, edits, ids)
    chains = [[ids[x] for x in c] for c in chains]
    gaps = FC.gaps(exact, 0)
    before = compare(g, by_id(g), chains, gaps, 0, 8, 1024)
    c, j, _ = kinds["line"][0]
    assert before[2]["classes"][c][j] == "filled" and len(before[0][c]) == 7
    assert g.removeEdgesById([before[0][c][3]]) == 1            # the middle filler of the line
    edges = by_id(g)
    fp = g.idFingerprint()
    after = compare(g, edges, chains, gaps, 0, 8, 1024)
    assert after[2]["classes"][c][j] == "none" and after[2]["filled"] == before[2]["filled"] - 1 and g.idFingerprint() == fp
    # a displaced edge: another edge of the same first base takes the fan's filler's place in its start node's out-edge word.  The
    # filler stays live and keeps its start node, and is on no path: not forward (the word names the other edge) and not backward
    c, j, _ = kinds["fan"][0]
    x = after[0][c][1]
    assert after[2]["classes"][c][j] == "filled" and compare(g, edges, [chains[c]], [gaps[c]], 60, 8, 1)[2]["searched_backward"] == 1
    info = g.edgesById(np.arange(g.idBounds()[1], dtype=np.uint32))
    z = next(e for e in sorted(edges) if e != x and info["first"][e] == info["first"][x] and e not in after[0][c] and edges[e][0] != edges[x][0])
    g.replaceStart(z, edges[x][0])
    edges = by_id(g)
    assert edges[x][0] == edges[z][0]
    for mp in (1, 1024):                                     # (tol = 60: the fan's other edge fits the bound, so the forward tree is over 1)
        assert compare(g, edges, [chains[c]], [gaps[c]], 60, 8, mp, displaced={x})[2]["none"] == 1
    assert compare(g, edges, chains, gaps, 0, 8, 1024, displaced={x})[2]["filled"] == after[2]["filled"] - 1
    g.close()


def raw(g, members, off, gap, tol=0, me=16, mp=256, cap=None, handle=True, null=()):
    """the C call itself -> (return code, the outputs, which start as patterns)"""
    m, o, gp = np.array(members, np.uint32), np.array(off, np.uint64), np.array(gap, np.int64)
    cap = g.idBounds()[1] if cap is None else cap
    out = dict(members=np.full(max(cap, 1), 0xabababab, np.uint32), gap=np.full(max(cap, 1), -77, np.int64), off=np.full(len(off), 0xcd, np.uint64),
               jclass=np.full(max(len(m), 1), 0xee, np.uint8), jlen=np.full(max(len(m), 1), -55, np.int64), n=np.full(1, 12345, np.uint64),
               stats=np.full(10, 999, np.uint64))
    p = lambda name, a, t: None if name in null else L.ptr(a, t)
    rc = L.lib().gk_graph_fill_gaps(g.h if handle else None, p("in_members", m, C.c_uint32), p("in_off", o, C.c_uint64), len(off) - 1, p("in_gap", gp, C.c_int64),
                                    tol, me, mp, p("members", out["members"], C.c_uint32), p("gap", out["gap"], C.c_int64), cap, p("off", out["off"], C.c_uint64),
                                    p("jclass", out["jclass"], C.c_uint8), p("jlen", out["jlen"], C.c_int64), p("n", out["n"], C.c_uint64),
                                    p("stats", out["stats"], C.c_uint64))
    return rc, {name: a.tolist() for name, a in out.items()}


PATTERN = dict(members=0xabababab, gap=-77, off=0xcd, jclass=0xee, jlen=-55, n=12345, stats=999)


def pristine(out, names=tuple(PATTERN)):
    return all(set(out[name]) == {PATTERN[name]} for name in names)


def test_errors_write_nothing_and_leave_the_graph_alone(planted):
    g, chains, exact, kinds = planted(31)
    edges = by_id(g)
    (a, b), (c, d) = chains[kinds["fan"][0][0]], chains[kinds["line"][0][0]]
    bound = g.idBounds()[1]
    dead = next(i for i in range(bound + 1) if i not in edges)
    fp = g.idFingerprint()
    ok = dict(members=[a, b], off=[0, 2], gap=[0, 0])
    cases = [dict(ok, members=[a, bound]), dict(ok, members=[a, 0xfffffffe]), dict(ok, members=[a, dead]), dict(members=[a, b, a], off=[0, 3], gap=[0] * 3),
             dict(members=[a, b, c, a], off=[0, 2, 4], gap=[0] * 4), dict(ok, off=[0, 2, 2]), dict(ok, off=[0, 0, 2]), dict(members=[a, b, c], off=[0, 3, 2], gap=[0] * 3),
             dict(ok, off=[1, 2]), dict(ok, tol=I31 + 1), dict(ok, me=0), dict(ok, me=FR.MAX_EDGES + 1), dict(ok, mp=0), dict(ok, mp=FR.MAX_PATHS + 1),
             dict(ok, gap=[I31 + 1, 0]), dict(ok, gap=[-I31 - 1, 0]), dict(ok, handle=False), dict(ok, null=("in_members",)), dict(ok, null=("in_gap",)),
             dict(ok, null=("in_off",)), dict(ok, null=("off",)), dict(ok, null=("jclass",)), dict(ok, null=("jlen",)), dict(ok, null=("n",)), dict(ok, null=("stats",)),
             dict(ok, null=("members",)), dict(ok, null=("gap",))]
    for kw in cases:
        rc, out = raw(g, **kw)
        assert rc == L.GK_E_INVALID, kw
        assert pristine(out) and g.idFingerprint() == fp, kw
    # what is no error: the largest gap where none is used, the parameters at their bounds
    for kw in (dict(ok, gap=[5, I31 + 1]), dict(ok, gap=[I31, 0], tol=I31), dict(ok, gap=[-I31, 0], me=FR.MAX_EDGES, mp=FR.MAX_PATHS), dict(ok, me=1, mp=1)):
        assert raw(g, **kw)[0] == L.GK_OK, kw
    # less room than needed: the size and the stats, nothing copied
    L0 = exact[kinds["line"][0][0]][0]
    rc, out = raw(g, [c, d], [0, 2], [L0, 0], me=8, cap=6)
    assert rc == L.GK_E_CAPACITY and out["n"] == [7] and out["stats"] == [1, 0, 0, 0, 0, 0, 1, 5, L0 + 31, 0]
    assert pristine(out, ("members", "gap", "off", "jclass", "jlen"))
    rc, out = raw(g, [c, d], [0, 2], [L0, 0], me=8, cap=7)
    assert rc == L.GK_OK and out["n"] == [7] and out["off"] == [0, 7] and out["gap"][:6] == [-31] * 6 and out["jclass"][:2] == [6, 0] and out["jlen"][0] == L0
    assert raw(g, [], [0], [])[0] == L.GK_OK and g.idFingerprint() == fp


def test_filled_scaffolds_hold_no_n(ctx, tmp_path):
    """end to end on the unedited graph: fillGaps -> scaffolds -> text, against the scaffold restatement on the filled chains; a
    chain and its twin chain, so that one record is written and spells the path.  The same from the graph saved and loaded."""
    k = 47
    reads = small_pairs(100 + k, k)
    g, vm = device_graph(ctx, k, reads)
    vm.close()
    oe = SC.oracle_edges(k, reads)
    twin = SC.twins(oe)
    ids = {key: i for i, key in edge_keys(g).items()}
    outs = {}
    for key in sorted(oe):
        outs.setdefault(oe[key][0], []).append(key)
    e, x, f = next((e, x, f) for e in sorted(oe) for x in outs.get(oe[e][1], []) for f in outs.get(oe[x][1], [])
                   if len({e, x, f, twin[e], twin[x], twin[f]}) == 6 and len(oe[x][2]) >= k + 10)
    named = {ids[key]: v for key, v in oe.items()}
    chains = [[ids[e], ids[f]], [ids[twin[f]], ids[twin[e]]]]
    L0 = len(oe[x][2]) - k
    gaps = [[L0 + 2], [L0 + 2]]
    fc, fg, rep = g.fillGaps(chains, gaps, 2)
    assert (fc, fg, rep) == FR.fill(by_id(g), k, chains, gaps, 2) and rep["filled"] == 2
    assert fc == [[ids[e], ids[x], ids[f]], [ids[twin[f]], ids[twin[x]], ids[twin[e]]]] and fg == [[-k, -k]] * 2
    fp = g.idFingerprint()
    g.save(tmp_path / "g.gkg")
    loaded = loadGraph(ctx, tmp_path / "g.gkg")
    assert by_id(loaded) == by_id(g) and loaded.fillGaps(chains, gaps, 2) == (fc, fg, rep) and loaded.idFingerprint() == fp == g.idFingerprint()
    # more classes on the loaded graph: a pair that meets in a node, unrelated pairs, the same junction out of tolerance and over max_paths
    used = {e, x, f, twin[e], twin[x], twin[f]}
    a, b = next((a, b) for a in sorted(oe) for b in outs.get(oe[a][1], []) if not {a, b} & used and a != b)
    rest = [y for y in sorted(oe) if y not in used | {a, b}]
    more = chains + [[ids[a], ids[b]], [ids[rest[0]], ids[rest[5]]], [ids[rest[1]], ids[rest[7]], ids[rest[3]]]]
    for tol, me, mp, G in ((2, 16, 256, L0 + 2), (1, 16, 256, L0 + 2), (2, 16, 1, L0), (2, 1, 256, L0)):
        more_gaps = [[G], [G], [7], [25], [0, 300]]
        got = loaded.fillGaps(more, more_gaps, tol, max_edges=me, max_paths=mp)
        assert got == g.fillGaps(more, more_gaps, tol, max_edges=me, max_paths=mp) == FR.fill(by_id(g), k, more, more_gaps, tol, me, mp)
        assert got[2]["adjacent"] >= 1 and got[2]["junctions"] == 6
    loaded.close()
    plain, filled = g.scaffolds(chains, gaps, singletons=False), g.scaffolds(fc, fg, singletons=False)
    want, st, _ = SR.scaffolds(named, fc, fg, singletons=False)
    text = filled.text()
    assert text == want and filled.stats() == st and st["chain_forward"] == st["chain_reverse"] == 1 and st["n_bases"] == 0 and b"N" not in text.split(b"\n", 1)[1]
    (name, n, seq), = SR.parse(text)
    assert SC.covered([oe[y][0] + oe[y][2] for y in ((e, x, f) if name == "s0" else (twin[f], twin[x], twin[e]))], seq)
    assert text.split(b"\n", 1)[0].endswith(b" contigs=3 gaps=0") and plain.text().split(b"\n", 1)[0].endswith(b" contigs=2 gaps=%d" % (L0 + 2))
    (_, n0, seq0), = SR.parse(plain.text())
    assert seq0.count("N") == plain.stats()["n_bases"] == L0 + 2 and n == n0 - 2       # the path's L bases stand where L + 2 bases N stood
    plain.close(); filled.close(); g.close()
