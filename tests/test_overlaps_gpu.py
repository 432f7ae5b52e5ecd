"""gk_graph_overlap_gaps, gk_graph_scaffolds_plan_overlaps and gk_scaffolds_overlap_stats on the device (-m gpu) against the
restatement (tests/overlaps_ref.py, held to hand-computed cases by tests/test_overlaps_cpu.py): overlap, jclass and all seven
stats of the stage; text, stats13, the two overlap stats and the segment rows of the plan.  Graphs: tests/overlaps_cases.py (dips,
planted starts, a periodic end, 300 short genomes in one graph, a 6 kb genome with three dips); the restatement works on the
device's own ids, nodes and sequences (`model`).  That the cases hold every class is asserted without a GPU."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context
from genome_amd.graph import OVERLAP_CLASSES, OVERLAP_STATS, HipLinks, Scaffolds, scaffoldChains, scaffoldGaps
from insert_cases import small_pairs
from pairs_ref import make_pairs
from thread_cases import device_graph as graph_by_id
from thread_ref import twin_edges
import overlaps_cases as OC
import overlaps_ref as OR
import scaffolds_cases as SC
import scaffolds_ref as SR
from test_links_gpu import device_graph, edge_keys

pytestmark = pytest.mark.gpu
assert OVERLAP_STATS == OR.STATS and OVERLAP_CLASSES == OR.CLASSES
I31 = (1 << 31) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def model(g):
    """the device graph as the restatement takes it: {edge id: (start k-mer, end k-mer, seq)} and {edge id: (start node id, end node id)}"""
    k = g.k
    nn, ne = g.idBounds()
    ninfo, einfo = g.nodesById(np.arange(nn, dtype=np.uint32)), g.edgesById(np.arange(ne, dtype=np.uint32))
    kmer = lambda n: dna.unpack(int(ninfo["lo"][n]), int(ninfo["hi"][n]), k)
    seqs = {}
    for s, _t, q in g.canonical()[1]:
        assert (s, q[0]) not in seqs
        seqs[(s, q[0])] = q
    edges, ids = {}, {}
    for e in range(ne):
        if einfo["alive"][e]:
            s, t = int(einfo["start"][e]), int(einfo["end"][e])
            q = seqs[(kmer(s), dna.BASES[int(einfo["first"][e])])]
            assert len(q) == int(einfo["len"][e])
            edges[e], ids[e] = (kmer(s), kmer(t), q), (s, t)
    return edges, ids


def built(ctx, k, reads):
    g, vm = device_graph(ctx, k, reads)
    vm.close()
    return (g, *model(g))


def stage(g, edges, ids, chains, gaps, tol, mn=OC.MIN_OVERLAP, mx=None):
    want = OR.overlaps(edges, chains, gaps, tol, mn, mx, node_ids=ids)
    got = g.overlapGaps(chains, gaps, tol, min_overlap=mn, max_overlap=mx)
    assert got == want, (gaps, tol, mn, mx)
    assert got[1]["junctions"] == sum(got[1][n] for n in OR.STATS[1:6]) == sum(len(c) - 1 for c in chains)
    return got


def plan(g, edges, ids, chains, gaps, ov, **kw):
    """the device's text, stats, overlap stats and segments == the restatement's -> (text, stats, overlap stats)"""
    want_text, want_st, want_rows, want_ost = OR.scaffolds(edges, chains, gaps, ov, node_ids=ids, **kw)
    s = g.scaffolds(chains, gaps, overlaps=ov, **kw)
    st, ost, text, rows = s.stats(), s.overlapStats(), s.text(), s.segments()
    s.close()
    assert st == want_st and ost == want_ost and text == want_text and rows == want_rows
    assert st["adjacent"] + st["gapped"] + ost["overlapped"] == st["members"] - (st["records"] - st["singletons"])
    return text, st, ost


# ---- 1. dip graphs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", OC.KS)
def test_dip_graphs(ctx, k):
    """w missing k-mers: o = k - 1 - w at 1, min_overlap - 1, min_overlap and k - 2; every gap at which the range gains and loses o,
    tol 0, 3 and 35; the chain and its twin chain"""
    found = 0
    for o in OC.dip_overlaps(k):
        reads, left, right, _ = OC.dip(1000 * k + o, k, o)
        g, edges, ids = built(ctx, k, reads)
        assert len(edges) == 4
        chains = [[OC.find(edges, left), OC.find(edges, right)], [OC.find(edges, SR.rev_comp(right)), OC.find(edges, SR.rev_comp(left))]]
        fp = g.idFingerprint()
        for tol in OC.TOLS:
            for G in OC.sweep(o, tol):
                ov, rep = stage(g, edges, ids, chains, [[G], [G]], tol)
                inside = abs(G + o) <= tol and o >= OC.MIN_OVERLAP
                assert ov == [[o if inside else 0]] * 2 and rep["classes"][0] == rep["classes"][1] and rep["overlap"] == 2 * inside
                found += inside
        # below min_overlap the stage finds it once asked to; the plan takes it either way
        ov, rep = stage(g, edges, ids, chains, [[-o], [-o]], 0, mn=1)
        assert ov == [[o], [o]]
        for strands in (1, 2):
            text, st, ost = plan(g, edges, ids, chains, [[-o], [-o]], ov, strands=strands, singletons=False)
            assert ost == dict(overlapped=strands, dropped=strands * o) and st["n_bases"] == st["gapped"] == 0 and st["records"] == strands
            seqs = [r[2] for r in SR.parse(text)]
            assert seqs[0] in (left + right[o:], SR.rev_comp(left + right[o:])) and (strands == 1 or seqs[1] == SR.rev_comp(seqs[0]))
        assert g.idFingerprint() == fp
        g.close()
    assert found > 0


# ---- 2. planted starts, the periodic end -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,d", [(21, -1), (21, 0), (21, 1), (21, 20), (31, -1), (31, 0), (31, 1), (31, 30), (64, -1), (64, 0), (64, 1), (64, 20), (64, 62), (64, 63)])
def test_planted_starts(ctx, k, d):
    """o = k - 1, k, k + 1 .. 2k - 1 through an added node as f's start; 127 at k = 64 is GK_OVERLAP_MAX.  tol = 63 around -64 gives
    118 candidates: both rounds of the lane loop, the hit in the second one from o = 74"""
    reads, pe, head, X = OC.planted(7 * k + d, k, d)
    g, edges, ids = built(ctx, k, reads)
    e, f = OC.find(edges, pe), OC.find(edges, head, head=True)
    node = g.addNode(X)
    g.replaceStart(f, node)
    edges, ids = OC.plant(edges, ids, f, X, node)
    assert model(g) == (edges, ids)
    o = k + d
    chains = [[e, f]]
    fp = g.idFingerprint()
    for G, tol, mx in ((-o, 0, OR.OVERLAP_MAX), (-o, 0, o), (-64, 63, OR.OVERLAP_MAX), (-o - 2, 3, OR.OVERLAP_MAX)):
        ov, rep = stage(g, edges, ids, chains, [[G]], tol, mx=mx)
        assert ov == [[o]] and rep["overlap"] == 1 and rep["overlap_bases"] == o
    ov, rep = stage(g, edges, ids, chains, [[-o]], 3, mx=o - 1)                 # max_overlap below the true overlap
    assert ov == [[0]] and rep["none"] == 1
    if o > k:
        assert stage(g, edges, ids, chains, [[-o]], 0)[1]["out_of_range"] == 1   # max_overlap = k by default
    text, st, ost = plan(g, edges, ids, chains, [[-o]], [[o]], strands=2, singletons=False)
    assert ost == dict(overlapped=1, dropped=o) and SR.parse(text)[0][2] == pe + (edges[f][0] + edges[f][2])[o:]
    assert g.idFingerprint() == fp
    g.close()


def test_a_periodic_end_is_ambiguous(ctx):
    k = 31
    reads, pe, head, X = OC.periodic(5, k)
    g, edges, ids = built(ctx, k, reads)
    e, f = OC.find(edges, pe), OC.find(edges, head, head=True)
    node = g.addNode(X)
    g.replaceStart(f, node)
    edges, ids = OC.plant(edges, ids, f, X, node)
    for G, tol, cls, o in ((-13, 1, "ambiguous", 0), (-12, 0, "overlap", 12), (-14, 0, "overlap", 14), (-13, 0, "none", 0), (-12, 2, "ambiguous", 0), (-15, 1, "overlap", 14)):
        ov, rep = stage(g, edges, ids, [[e, f]], [[G]], tol)
        assert (rep["classes"], ov) == ([[cls]], [[o]])
    text, st, ost = plan(g, edges, ids, [[e, f]], [[-13]], [[0]], strands=2, singletons=False)      # it stays N
    assert st["clamped"] == 1 and st["n_bases"] == 10 and ost == dict(overlapped=0, dropped=0)
    g.close()


# ---- 3. many junctions: launch grids, strand symmetry ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many(ctx):
    """300 short genomes with a dip each in one graph: the chains [left, right] and, found with thread_ref.twin_edges, [twin right,
    twin left]; the gaps are off by -2 .. 2 in turn"""
    k = 31
    reads, pairs = OC.many(9, k)
    g, edges, ids = built(ctx, k, reads)
    nodes, by_rank, _keys = graph_by_id(g)
    assert sorted(edges) == list(range(len(edges))) and len(edges) == 4 * len(pairs)      # every id is live: a rank is an id
    twin = twin_edges(k, nodes, by_rank)
    by_path = {s + q: e for e, (s, _t, q) in edges.items()}
    chains, gaps = [], []
    for i, (left, right, o) in enumerate(pairs):
        e, f = by_path[left], by_path[right]
        chains += [[e, f], [twin[f], twin[e]]]
        gaps += [[-o + i % 5 - 2]] * 2
    yield g, edges, ids, chains, gaps
    g.close()


def test_both_strands_chains_are_mirrored(many):
    g, edges, ids, chains, gaps = many
    ov, rep = stage(g, edges, ids, chains, gaps, 1, mn=3)
    assert rep["overlap"] > 100 and rep["none"] > 100 and rep["out_of_range"] > 0
    assert all(ov[i] == ov[i + 1] and rep["classes"][i] == rep["classes"][i + 1] for i in range(0, len(chains), 2))
    text1, st1, ost1 = plan(g, edges, ids, chains, gaps, ov, strands=1, singletons=False, line_width=0)
    text2, st2, ost2 = plan(g, edges, ids, chains, gaps, ov, strands=2, singletons=False, line_width=0)
    assert st1["records"] == len(chains) // 2 and st1["chain_forward"] == st1["chain_reverse"] == len(chains) // 2
    assert (2 * ost1["overlapped"], 2 * ost1["dropped"]) == (ost2["overlapped"], ost2["dropped"]) == (rep["overlap"], rep["overlap_bases"])
    seqs = {name: seq for name, _n, seq in SR.parse(text2)}
    assert all(seqs["s%d" % (i + 1)] == SR.rev_comp(seqs["s%d" % i]) for i in range(0, len(chains), 2))
    assert sorted(name for name, _n, _s in SR.parse(text1)) == sorted(min(("s%d" % i, "s%d" % (i + 1)), key=lambda n: [SR.CODE[c] for c in seqs[n]])
                                                                         for i in range(0, len(chains), 2))


@pytest.mark.parametrize("grid", [1, 3])
def test_small_launch_grids(ctx, many, grid):
    """1 and 3 workgroups per launch: four (twelve) waves take 600 junctions to search"""
    g, edges, ids, chains, gaps = many
    ctx.set_option("test_max_grid", grid)
    try:
        uses = ctx.grid_cap_uses()
        for tol, mn in ((1, 3), (0, 1), (35, 10)):
            ov, rep = stage(g, edges, ids, chains, gaps, tol, mn=mn)
            assert rep["junctions"] == len(chains) > 3 * 4 * 16
        plan(g, edges, ids, chains, gaps, ov, strands=2, singletons=False)
        assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)


# ---- 4. unchanged behaviour ------------------------------------------------------------------------------------------------------

def raw_plan(g, members, off, gap, overlap, min_gap=10, min_len=0, line_width=60, strands=1, singletons=1):
    """gk_graph_scaffolds_plan_overlaps itself -> (return code, *out), which starts as a pattern; overlap None: NULL"""
    m, o, gp = np.array(members, np.uint32), np.array(off, np.uint64), np.array(gap, np.int64)
    ov = None if overlap is None else np.array(overlap, np.uint32)
    h = L.vp(0x1234)
    rc = L.lib().gk_graph_scaffolds_plan_overlaps(g.h, L.ptr(m, C.c_uint32), L.ptr(o, C.c_uint64), len(off) - 1, L.ptr(gp, C.c_int64), L.ptr(ov, C.c_uint32), min_gap,
                                                  min_len, line_width, strands, singletons, C.byref(h))
    return rc, h.value


def flat(chains, per_junction, last=0):
    members = [e for c in chains for e in c]
    off = [0] + list(np.cumsum([len(c) for c in chains]))
    return members, off, [x for c, v in zip(chains, per_junction) for x in list(v)[:len(c) - 1] + [last]]


def test_null_and_zero_overlaps_are_the_plan(ctx):
    """on scaffolds_cases.constructed: gk_graph_scaffolds_plan's bytes, stats13 and segments, with overlap NULL and all zeros"""
    k = 31
    reads = small_pairs(100 + k, k)
    g, vm = device_graph(ctx, k, reads)
    vm.close()
    ids = {key: i for i, key in edge_keys(g).items()}
    chains, gaps = SC.constructed(SC.oracle_edges(k, reads), k)
    chains = [[ids[key] for key in c] for c in chains]
    members, off, gap = flat(chains, gaps)
    for strands in (1, 2):
        for singletons in (0, 1):
            base = g.scaffolds(chains, gaps, strands=strands, singletons=bool(singletons), line_width=7)
            want = base.text(), base.stats(), base.segments()
            assert want[1]["adjacent"] > 0 and want[1]["clamped"] > 0
            for ov in (None, [0] * len(members), [0] * (len(members) - 1) + [99]):       # (the entry at a chain's last member is ignored)
                rc, h = raw_plan(g, members, off, gap, ov, strands=strands, singletons=singletons, line_width=7)
                assert rc == L.GK_OK and h
                s = Scaffolds(g, L.vp(h))
                assert (s.text(), s.stats(), s.segments()) == want and s.overlapStats() == dict(overlapped=0, dropped=0)
                s.close()
            assert base.overlapStats() == dict(overlapped=0, dropped=0)
            base.close()
    g.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------

def raw_stage(g, members, off, gap, tol=0, mn=10, mx=31, handle=True, null=()):
    """gk_graph_overlap_gaps itself -> (return code, the outputs, which start as patterns)"""
    m, o, gp = np.array(members, np.uint32), np.array(off, np.uint64), np.array(gap, np.int64)
    out = dict(overlap=np.full(max(len(m), 1), 0xabababab, np.uint32), jclass=np.full(max(len(m), 1), 0xee, np.uint8), stats=np.full(7, 999, np.uint64))
    p = lambda name, a, t: None if name in null else L.ptr(a, t)
    rc = L.lib().gk_graph_overlap_gaps(g.h if handle else None, p("members", m, C.c_uint32), p("off", o, C.c_uint64), len(off) - 1, p("gap", gp, C.c_int64), tol, mn, mx,
                                       p("overlap", out["overlap"], C.c_uint32), p("jclass", out["jclass"], C.c_uint8), p("stats", out["stats"], C.c_uint64))
    return rc, {name: a.tolist() for name, a in out.items()}


PATTERN = dict(overlap=0xabababab, jclass=0xee, stats=999)


def test_errors_write_nothing_and_leave_the_graph_alone(ctx):
    k, d = 31, 30
    reads, pe, head, X = OC.planted(7 * k + d, k, d)
    g, edges, ids = built(ctx, k, reads)
    e, f = OC.find(edges, pe), OC.find(edges, head, head=True)
    node = g.addNode(X)
    g.replaceStart(f, node)
    edges, ids = OC.plant(edges, ids, f, X, node)
    h = next(x for x in edges if ids[x][0] == ids[e][1])                        # leaves e's end node: (e, h) is adjacent
    c = next(x for x in sorted(edges) if x not in (e, f, h))
    bound = g.idBounds()[1]
    fp = g.idFingerprint()
    o = k + d
    ok = dict(members=[e, f], off=[0, 2], gap=[-o, 0], mx=OR.OVERLAP_MAX)
    rc, out = raw_stage(g, **ok)
    assert rc == L.GK_OK and out == dict(overlap=[o, 0], jclass=[5, 0], stats=[1, 0, 0, 0, 0, 1, o])
    cases = [dict(ok, members=[e, bound]), dict(ok, members=[e, 0xfffffffe]), dict(members=[e, f, e], off=[0, 3], gap=[0] * 3), dict(members=[e, f, c, e], off=[0, 2, 4], gap=[0] * 4),
             dict(ok, off=[0, 2, 2]), dict(ok, off=[0, 0, 2]), dict(members=[e, f, c], off=[0, 3, 2], gap=[0] * 3), dict(ok, off=[1, 2]), dict(ok, tol=I31 + 1),
             dict(ok, mn=0), dict(ok, mn=128, mx=128), dict(ok, mx=128), dict(ok, mn=11, mx=10), dict(ok, mx=0), dict(ok, gap=[I31 + 1, 0]), dict(ok, gap=[-I31 - 1, 0]),
             dict(ok, handle=False), dict(ok, null=("members",)), dict(ok, null=("gap",)), dict(ok, null=("off",)), dict(ok, null=("overlap",)), dict(ok, null=("jclass",)),
             dict(ok, null=("stats",))]
    for kw in cases:
        rc, out = raw_stage(g, **kw)
        assert rc == L.GK_E_INVALID, kw
        assert all(set(out[name]) == {PATTERN[name]} for name in PATTERN) and g.idFingerprint() == fp, kw
    # what is no error: the parameters at their bounds, the largest gap where none is used (an adjacent junction, a last member)
    for kw in (dict(ok, tol=I31), dict(ok, mn=1, mx=1), dict(ok, mn=127, mx=127), dict(ok, gap=[I31, 0]), dict(ok, gap=[-I31, 0], tol=I31), dict(ok, gap=[-o, I31 + 1]),
               dict(ok, members=[e, h], gap=[I31 + 1, 0])):
        assert raw_stage(g, **kw)[0] == L.GK_OK, kw
    assert raw_stage(g, [], [0], [])[0:2] == (L.GK_OK, dict(overlap=[PATTERN["overlap"]], jclass=[PATTERN["jclass"]], stats=[0] * 7))
    # the plan does not trust the array
    two = dict(members=[e, f], off=[0, 2], gap=[-o, 0])
    assert len(edges[f][0] + edges[f][2]) == 2 * k
    for kw in (dict(two, overlap=[128, 0]), dict(two, overlap=[2 * k, 0]), dict(two, overlap=[o - 1, 0]), dict(two, overlap=[1 << 31, 0]),
               dict(members=[e, h], off=[0, 2], gap=[0, 0], overlap=[5, 0])):
        assert raw_plan(g, **kw) == (L.GK_E_INVALID, None) and g.idFingerprint() == fp, kw
    for kw in (dict(two, overlap=[o, 0]), dict(two, overlap=[0, 0]), dict(two, overlap=[o, 77]), dict(members=[e, h], off=[0, 2], gap=[0, 0], overlap=[0, 5])):
        rc, s = raw_plan(g, **kw)
        assert rc == L.GK_OK and s, kw
        L.lib().gk_scaffolds_destroy(s)
    st2 = np.zeros(2, np.uint64)
    assert L.lib().gk_scaffolds_overlap_stats(None, L.ptr(st2, C.c_uint64)) == L.GK_E_INVALID
    # bases that differ in the last position only: f's start is e's end k-mer but for its last base
    g.close()
    reads, pe, head, X = OC.planted(7 * k, k, 0)
    g, edges, ids = built(ctx, k, reads)
    e, f = OC.find(edges, pe), OC.find(edges, head, head=True)
    g.replaceStart(f, g.addNode(X[:-1] + OC.OTHER[X[-1]]))
    fp = g.idFingerprint()
    two = dict(members=[e, f], off=[0, 2], gap=[-k, 0])
    assert raw_plan(g, **dict(two, overlap=[k, 0])) == (L.GK_E_INVALID, None) and g.idFingerprint() == fp
    assert raw_stage(g, **dict(two, tol=0))[1]["jclass"] == [3, 0]                  # none
    g.replaceStart(f, g.addNode(X))
    rc, s = raw_plan(g, **dict(two, overlap=[k, 0]))
    assert rc == L.GK_OK and s
    L.lib().gk_scaffolds_destroy(s)
    # a dead member
    assert g.removeEdgesById([f]) == 1
    fp = g.idFingerprint()
    rc, out = raw_stage(g, **two)
    assert rc == L.GK_E_INVALID and all(set(out[name]) == {PATTERN[name]} for name in PATTERN) and g.idFingerprint() == fp
    g.close()


def test_the_three_entries_hold_one_chain_list_contract(ctx):
    """the plan, gap filling and overlap detection give the same malformed chain list the same error code and write nothing; the
    one difference is a gap of -(2^31) at a junction that is not adjacent, which the plan clamps and the other two refuse"""
    from test_fillgaps_gpu import pristine as fill_pristine, raw as raw_fill
    g, edges, ids = built(ctx, 31, small_pairs(100 + 31, 31))
    x, y = next((a, b) for a in sorted(edges) for b in sorted(edges) if a != b and ids[a][1] != ids[b][0])        # not adjacent
    z, w = [a for a in sorted(edges) if a not in (x, y)][:2]
    fp = g.idFingerprint()

    def codes(members, off, gap):
        rc_plan, s = raw_plan(g, members, off, gap, None)
        rc_fill, out_fill = raw_fill(g, members, off, gap)
        rc_ovl, out_ovl = raw_stage(g, members, off, gap)
        if rc_plan == L.GK_OK:
            L.lib().gk_scaffolds_destroy(s)
        assert (s is None) == (rc_plan != L.GK_OK) and g.idFingerprint() == fp
        assert rc_fill == L.GK_OK or fill_pristine(out_fill)
        assert rc_ovl == L.GK_OK or all(set(out_ovl[name]) == {PATTERN[name]} for name in PATTERN)
        return rc_plan, rc_fill, rc_ovl

    assert codes([x, y, z, w], [0, 2, 4], [5, 0, 5, 0]) == (L.GK_OK,) * 3
    for kw in (dict(members=[x, g.idBounds()[1]], off=[0, 2], gap=[0] * 2),                 # an id at the bound
               dict(members=[x, y, z, x], off=[0, 2, 4], gap=[0] * 4),                      # a duplicate across two chains
               dict(members=[x, y], off=[0, 2, 2], gap=[0] * 2),                            # an empty chain
               dict(members=[x, y], off=[1, 2], gap=[0] * 2),                               # a chain_off that does not start at 0
               dict(members=[x, y, z], off=[0, 3, 2], gap=[0] * 3)):                        # a chain_off that descends
        assert codes(**kw) == (L.GK_E_INVALID,) * 3, kw
    assert codes([x, y], [0, 2], [-I31 - 1, 0]) == (L.GK_OK, L.GK_E_INVALID, L.GK_E_INVALID)
    g.close()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------

def test_three_dips_end_to_end(ctx):
    """pairs -> pairLinks -> joins -> scaffoldChains -> scaffoldGaps -> overlapGaps -> scaffolds: one record, the genome"""
    E = OC.E2E
    k = E["k"]
    g, vm = device_graph(ctx, k, OC.e2e_pieces())
    reads = make_pairs(E["seed"], k, glen=E["glen"], nrep=0, L=k + 9, npairs=E["npairs"], ins=E["ins"])
    links = HipLinks(ctx)
    g.pairLinks(vm, (dna.reads_to_bin(reads), len(reads) // 2), links, min_len=0, max_span=E["ins"][1] + k)
    joins, _ = links.joins(E["support"])
    chains = scaffoldChains(joins[0], joins[1])
    gaps = scaffoldGaps(chains, joins, E["mid"])
    assert [len(c) for c in chains] == [4, 4]
    edges, ids = model(g)
    ov, rep = stage(g, edges, ids, chains, gaps, E["tol"])
    assert rep["overlap"] == 6 and rep["ambiguous"] == 0 and sorted(ov[0]) == sorted(k - 1 - w for _p, w in E["dips"])
    text, st, ost = plan(g, edges, ids, chains, gaps, ov, singletons=False)
    (name, n, seq), = SR.parse(text)
    G = OC.e2e_genome()
    assert text.split(b"\n", 1)[0].endswith(b" contigs=4 gaps=0") and "N" not in seq and seq in (G, SR.rev_comp(G))
    assert ost == dict(overlapped=3, dropped=sum(k - 1 - w for _p, w in E["dips"]))
    # the same run without the stage
    plain = g.scaffolds(chains, gaps, singletons=False)
    assert plain.stats()["clamped"] == 3 and plain.overlapStats() == dict(overlapped=0, dropped=0)
    plain.close(); links.close(); vm.close(); g.close()
