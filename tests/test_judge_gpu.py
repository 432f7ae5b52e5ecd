"""gk_placements_* and gk_scaffolds_judge on the device (-m gpu) against the restatement (tests/judge_ref.py, held to hand-written
answers by tests/test_judge_cpu.py): every per-edge array, every junction array and every stat, exactly.  Set-ups:
tests/judge_cases.py (two reference records, contigs known by their paths, every junction class planted by a hand-written chain
list, reference variants, planted repeats); the restatement works on the device's own ids (`model`)."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import check as GC
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Placements, buildGraph
import judge_cases as JC
import judge_ref as JR
import overlaps_cases as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def device_graph(ctx, k, reads):
    """the graph of the reads and its position map"""
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    g = buildGraph(k, m)
    m.close()
    return g, g.getGraphMap()


def model(g):
    """the device graph as the restatement takes it: {node id: k-mer}, {edge id: (start k-mer, seq)}, {edge id: (start node id, end
    node id)}, {edge id: path}"""
    k = g.k
    nn, ne = g.idBounds()
    ninfo, einfo = g.nodesById(np.arange(nn, dtype=np.uint32)), g.edgesById(np.arange(ne, dtype=np.uint32))
    kmer = lambda n: dna.unpack(int(ninfo["lo"][n]), int(ninfo["hi"][n]), k)
    nodes = {n: kmer(n) for n in range(nn) if ninfo["alive"][n]}
    seqs = {(s, q[0]): q for s, _t, q in g.canonical()[1]}
    edges, ends = {}, {}
    for e in range(ne):
        if einfo["alive"][e]:
            s, t = int(einfo["start"][e]), int(einfo["end"][e])
            edges[e], ends[e] = (kmer(s), seqs[(kmer(s), dna.BASES[int(einfo["first"][e])])]), (s, t)
    return nodes, edges, ends, ne


def finder(edges):
    by_path = {s + q: e for e, (s, q) in edges.items()}
    assert len(by_path) == len(edges)
    return lambda path: by_path[path]


def placed_equal(g, vm, records, nodes, edges, ne):
    """the device's stats and per-edge arrays == the restatement's -> (Placements, the restatement's per-edge dict)"""
    want_st, want = JR.place(g.k, nodes, edges, records, id_bound=ne)
    pl = g.place(vm, records)
    st, ed = pl.stats(), pl.edges()
    got = {e: (ed["cls"][e], ed["record"][e], ed["pos"][e], ed["windows_fwd"][e], ed["windows_rev"][e]) for e in range(ne)}
    assert st == want_st
    assert got == want
    JR.identities(pst=st, live_edges=len(edges))
    return pl, want


def judged_equal(s, pl, ends, want_placed, tol, nchains):
    want = JR.judge(s.segments(), ends, want_placed, tol, chain_records=nchains)
    got = s.judge(pl, tol)
    assert (got["classes"], got["err"], got["stats"]) == want
    JR.identities(jst=got["stats"])
    return got


@pytest.fixture(scope="module", params=JC.KS)
def setup(request, ctx):
    k = request.param
    case = JC.main(k)
    g, vm = device_graph(ctx, k, case["reads"])
    yield dict(k=k, case=case, g=g, vm=vm, model=model(g))
    vm.close()
    g.close()


def test_planted_junction_classes(setup):
    """every class by a hand-written chain list: adjacent, gapped and overlapped correct joins (the overlap from overlapGaps on the
    coverage dip), wrong order, an inversion, a join across the two records, a chain on the reverse strand, an unjudged join; the
    gap estimate off by tol and by tol + 1"""
    k, case, g, vm = setup["k"], setup["case"], setup["g"], setup["vm"]
    nodes, edges, ends, ne = setup["model"]
    find = finder(edges)
    pl, want_placed = placed_equal(g, vm, case["records"], nodes, edges, ne)
    for name, (r, x) in JC.coords(k).items():
        path = case["paths"][name]
        assert want_placed[find(path)][:3] == ("forward", r, x) and want_placed[find(JC.rc(path))][:3] == ("reverse", r, x + len(path) - 1)
    for tol, delta in ((3, 3), (3, 4), (0, 0), (5, -5), (5, -6)):
        chains, gaps = JC.chains(find, case["paths"], k, delta)
        ov, rep = g.overlapGaps(chains, gaps, tol=8)
        assert ov[0] == [0, 0, JC.OVERLAP] and rep["overlap"] == 1
        s = g.scaffolds(chains, gaps, strands=2, overlaps=ov)
        got = judged_equal(s, pl, ends, want_placed, tol, len(chains))
        want_c, want_e = JC.expected(tol, delta)
        assert got["classes"] == want_c and all(w is None or w == e for w, e in zip(want_e, got["err"]))
        assert got["stats"]["adjacent_correct"] == 2 and got["stats"]["overlapped_correct"] == 1 and got["stats"]["records_judged"] == 5
        s.close()
    pl.close()


def test_strands_1_judges_the_written_chains(setup):
    """strands = 1 writes one chain of a twin pair; its pieces are still P(edge) forward, and the same rule judges them"""
    k, case, g, vm = setup["k"], setup["case"], setup["g"], setup["vm"]
    nodes, edges, ends, ne = setup["model"]
    find = finder(edges)
    chains, gaps = JC.chains(find, case["paths"], k, 0)
    with g.place(vm, case["records"]) as pl:
        want_placed = JR.place(k, nodes, edges, case["records"], id_bound=ne)[1]
        s = g.scaffolds(chains, gaps, strands=1, singletons=False)
        nrec = s.stats()["records"]
        assert 0 < nrec <= len(chains)
        judged_equal(s, pl, ends, want_placed, 3, nrec)
        s.close()


def test_reference_variants(setup):
    """an N, a lowercase run and a substituted base inside contigs: one diagonal, fewer windows; a deleted base: scattered"""
    k, case, g, vm = setup["k"], setup["case"], setup["g"], setup["vm"]
    nodes, edges, ends, ne = setup["model"]
    find = finder(edges)
    clean = JR.place(k, nodes, edges, case["records"], id_bound=ne)[1]
    pl, marks = placed_equal(g, vm, JC.variant_marks(case["records"], k), nodes, edges, ne)
    c0a, c3, d1 = (find(case["paths"][n]) for n in ("c0a", "c3", "d1"))
    assert marks[c3][:3] == ("forward", 0, 1760) and marks[c3][3] == clean[c3][3] - k
    assert marks[c0a][:3] == ("forward", 0, 0) and marks[c0a][3] < clean[c0a][3]
    pl.close()
    pl, dele = placed_equal(g, vm, JC.variant_deletion(case["records"]), nodes, edges, ne)
    assert dele[d1][0] == "scattered"
    chains, gaps = JC.chains(find, case["paths"], k, 0)
    s = g.scaffolds(chains, gaps, strands=2)
    got = judged_equal(s, pl, ends, dele, 3, len(chains))
    assert got["classes"][3] == "unjudged"                      # the join [d1, d0] has lost its judge
    s.close()
    pl.close()


def test_slices_give_the_unsliced_answers(setup, ctx):
    """slices of 1 (all halo), 257 and 4097 characters: every boundary falls inside a contig.  No record here is longer than 2400
    bases, so 4097 is the whole record in one slice and every launch is one workgroup; the slices that pass a workgroup's tile
    are test_long_record_slices'."""
    k, case, g, vm = setup["k"], setup["case"], setup["g"], setup["vm"]
    nodes, edges, ends, ne = setup["model"]
    recs = JC.variant_marks(case["records"], k)
    try:
        for sl in (1, 257, 4097):
            ctx.set_option("test_place_slice", sl)
            placed_equal(g, vm, recs, nodes, edges, ne)[0].close()
    finally:
        ctx.set_option("test_place_slice", 0)


# ---- a record of several workgroups' tiles (JC.long_record; the inputs are held to hand-written answers by test_judge_cpu.py) ----------
@pytest.fixture(scope="module", params=JC.LONG_KS)
def long_setup(request, ctx):
    k = request.param
    case = JC.long_record(k)
    g, vm = device_graph(ctx, k, case["reads"])
    yield dict(k=k, case=case, g=g, vm=vm, model=model(g))
    vm.close()
    g.close()


def test_long_record_over_four_tiles(long_setup):
    """contigs across the first two tile boundaries, a break between two edges exactly on the third, a contig in the last, partly
    filled tile; invalid characters on, just before and k - 1 after a boundary; records of T - 1, T and T + 1 windows"""
    k, case, g, vm = long_setup["k"], long_setup["case"], long_setup["g"], long_setup["vm"]
    nodes, edges, _ends, ne = long_setup["model"]
    find = finder(edges)
    rec = case["record"]
    pl, want = placed_equal(g, vm, [rec], nodes, edges, ne)
    for name, x in JC.long_coords(k).items():
        path = case["paths"][name]
        assert want[find(path)] == ("forward", 0, x, len(path) - k - 1, 0) and want[find(JC.rc(path))] == ("reverse", 0, x + len(path) - 1, 0, len(path) - k - 1)
    pl.close()
    pl, marks = placed_equal(g, vm, [JC.long_marks(rec, k)], nodes, edges, ne)
    a, b = (find(case["paths"][n]) for n in ("a", "b"))
    assert marks[a] == want[a][:3] + (want[a][3] - k, 0) and marks[b] == want[b][:3] + (want[b][3] - (k + 3), 0)
    pl.close()
    for cut, windows in zip(JC.long_truncations(rec, k), (JC.T - 1, JC.T, JC.T + 1)):
        pl, _ = placed_equal(g, vm, [cut], nodes, edges, ne)
        assert pl.stats()["windows"] == windows
        pl.close()


def test_long_record_slices(long_setup, ctx):
    """device slices of T, T + 1, T + k - 1 and 2T characters of the marked record: a later slice starts its halo early, so its tile
    boundaries are not the unsliced ones.  (A run with test_max_grid = 1 is left out: k_place_windows' grid is the number of tiles
    of the slice and does not go through the cap, so gk_test_grid_cap_uses would not move.)"""
    k, case, g, vm = long_setup["k"], long_setup["case"], long_setup["g"], long_setup["vm"]
    nodes, edges, _ends, ne = long_setup["model"]
    recs = [JC.long_marks(case["record"], k)]
    try:
        for sl in (JC.T, JC.T + 1, JC.T + k - 1, 2 * JC.T):
            ctx.set_option("test_place_slice", sl)
            placed_equal(g, vm, recs, nodes, edges, ne)[0].close()
    finally:
        ctx.set_option("test_place_slice", 0)


def test_long_record_as_the_second_record(long_setup):
    """behind a record that hits nothing: record = 1 travels in the high bits of the min and max words of every tile's triples"""
    k, case, g, vm = long_setup["k"], long_setup["case"], long_setup["g"], long_setup["vm"]
    nodes, edges, _ends, ne = long_setup["model"]
    find = finder(edges)
    pl, want = placed_equal(g, vm, [JC.main(k)["records"][1], case["record"]], nodes, edges, ne)
    for name, x in JC.long_coords(k).items():
        assert want[find(case["paths"][name])][:3] == ("forward", 1, x)
    assert pl.stats()["records"] == 2 and pl.stats()["forward"] == pl.stats()["reverse"] == 5
    pl.close()


def test_repeats(ctx):
    """an exact repeat and an inverted repeat longer than k"""
    for k in JC.KS:
        case = JC.repeats(k)
        g, vm = device_graph(ctx, k, case["reads"])
        nodes, edges, _ends, ne = model(g)
        pl, placed = placed_equal(g, vm, case["records"], nodes, edges, ne)
        st = pl.stats()
        assert st["scattered"] >= 2 and st["both_strands"] >= 2 and st["forward"] == st["reverse"] > 0
        pl.close(); vm.close(); g.close()


def test_many_records_one_workgroup(ctx):
    """300 reference records and 600 junction-bearing segments with every grid-stride launch held to one workgroup"""
    k = 21
    reads, pairs = OC.many(77, k, n=300)
    g, vm = device_graph(ctx, k, reads)
    nodes, edges, ends, ne = model(g)
    find = finder(edges)
    records = [left + right[o:] for left, right, o in pairs]
    chains = [[find(left), find(right)] for left, right, _o in pairs]
    gaps = [[-o + (i % 3)] for i, (_l, _r, o) in enumerate(pairs)]
    ov = [[o if o >= 10 else 0] for _l, _r, o in pairs]
    try:
        ctx.set_option("test_max_grid", 1)
        pl, placed = placed_equal(g, vm, records, nodes, edges, ne)
        s = g.scaffolds(chains, gaps, strands=2, overlaps=ov)
        got = judged_equal(s, pl, ends, placed, 1, len(chains))
    finally:
        ctx.set_option("test_max_grid", 0)
    assert got["stats"]["junctions"] == 300 and got["stats"]["overlapped_correct"] > 0 and got["stats"]["gapped_distance"] > 0
    assert max(placed[e][1] for e in placed) == 299
    ns = GC.scaffold_n50s(s.segments(), got["classes"])
    assert ns["n50_broken"] <= ns["n50"] and ns["pieces"] == ns["records"] + sum(got["stats"][c] for c in JR.MISJOINS)
    s.close(); pl.close(); vm.close(); g.close()


def test_errors(setup, ctx):
    k, case, g0, vm0 = setup["k"], setup["case"], setup["g"], setup["vm"]
    lib = L.lib()
    # a position map of another k
    other = 31 if k != 31 else 21
    g2, vm2 = device_graph(ctx, other, JC.main(other)["reads"])
    with pytest.raises(L.GkError) as ei:
        Placements(g0, vm2)
    assert ei.value.code == L.GK_E_KLEN
    vm2.close(); g2.close()
    # a graph of its own: it is edited below
    g, vm = device_graph(ctx, k, case["reads"])
    nodes, edges, ends, ne = model(g)
    find = finder(edges)
    chains, gaps = JC.chains(find, case["paths"], k, 0)
    pl = g.place(vm, case["records"])
    s = g.scaffolds(chains, gaps, strands=2, overlaps=JC.overlaps())
    # an edge id at the bound: nothing written
    ids = np.array([0, ne], np.uint32)
    cls = np.full(2, 77, np.uint8)
    assert lib.gk_placements_edges(pl.h, L.ptr(ids, C.c_uint32), 2, L.ptr(cls, C.c_uint8), None, None, None, None) == L.GK_E_INVALID
    assert cls.tolist() == [77, 77]
    # a short cap: *n and the stats are set, nothing is copied
    n, st = C.c_uint64(), np.zeros(len(JR.JUDGE_STATS), np.uint64)
    jc, je = np.full(9, 77, np.uint8), np.full(9, 77, np.int64)
    assert lib.gk_scaffolds_judge(s.h, pl.h, 3, L.ptr(jc, C.c_uint8), L.ptr(je, C.c_int64), 8, C.byref(n), L.ptr(st, C.c_uint64)) == L.GK_E_CAPACITY
    assert n.value == 9 and int(st[0]) == 9 and jc.tolist() == [77] * 9 and je.tolist() == [77] * 9
    assert lib.gk_scaffolds_judge(s.h, pl.h, 3, L.ptr(jc, C.c_uint8), L.ptr(je, C.c_int64), 9, C.byref(n), L.ptr(st, C.c_uint64)) == L.GK_OK
    assert [JR.JUDGE_CLASSES[x] for x in jc] == JC.expected(3, 0)[0]
    # a plan and placements of different graphs
    pl0 = g0.place(vm0, case["records"])
    assert lib.gk_scaffolds_judge(s.h, pl0.h, 3, L.ptr(jc, C.c_uint8), L.ptr(je, C.c_int64), 9, C.byref(n), L.ptr(st, C.c_uint64)) == L.GK_E_INVALID
    pl0.close()
    assert lib.gk_scaffolds_judge(None, pl.h, 3, None, None, 0, C.byref(n), L.ptr(st, C.c_uint64)) == L.GK_E_INVALID
    assert lib.gk_scaffolds_judge(s.h, None, 3, None, None, 0, C.byref(n), L.ptr(st, C.c_uint64)) == L.GK_E_INVALID
    # a stale position map: the graph is edited, a new Placements over the old map must refuse the first record
    assert g.removeEdgesById([find(case["paths"]["c3"])]) == 1
    for call in (lambda: pl.stats(), lambda: pl.edges(), lambda: pl.add("ACGT"), lambda: s.judge(pl, 3)):
        with pytest.raises(L.GkError) as ei:
            call()
        assert ei.value.code == L.GK_E_STATE
    stale = Placements(g, vm)
    with pytest.raises(L.GkError) as ei:
        stale.add(case["records"][0])
    assert ei.value.code == L.GK_E_STATE
    with pytest.raises(L.GkError) as ei:                       # after a failed add_record the handle refuses further records
        stale.add("ACGT")
    assert ei.value.code == L.GK_E_STATE
    stale.close(); s.close(); pl.close(); vm.close(); g.close()


def test_judge_scaffolds_reads_fasta(setup, tmp_path):
    """genome_amd.check.judge_scaffolds over a FASTA file (plain and .gz) == the pieces called by hand"""
    import gzip
    k, case, g, vm = setup["k"], setup["case"], setup["g"], setup["vm"]
    nodes, edges, ends, ne = setup["model"]
    chains, gaps = JC.chains(finder(edges), case["paths"], k, 4)
    s = g.scaffolds(chains, gaps, strands=2)
    text = JC.fasta(case["records"])
    (tmp_path / "ref.fa").write_bytes(text)
    with gzip.open(tmp_path / "ref.fa.gz", "wb") as f:
        f.write(text)
    with g.place(vm, case["records"]) as pl:
        want = s.judge(pl, 3)
        want_pst = pl.stats()
    for src in (tmp_path / "ref.fa", tmp_path / "ref.fa.gz", text):
        out = GC.judge_scaffolds(g, src, s, 3)
        assert (out["classes"], out["err"], out["stats"], out["placements"]) == (want["classes"], want["err"], want["stats"], want_pst)
        assert out["n50_broken"] < out["n50"]
    s.close()
