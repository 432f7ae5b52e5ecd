"""gk_blocks_* on the device (-m gpu) against the restatement (tests/blocks_ref.py, held to hand-written answers and to the
placements by tests/test_blocks_cpu.py): every row, class, shift, per-edge array, piece and stat, exactly.  Set-ups:
tests/blocks_cases.py and tests/judge_cases.py; the restatement works on the device's own ids (test_judge_gpu.model)."""
import ctypes as C

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import check as GC
from genome_amd.dnamap import Context
from genome_amd.graph import BLOCK_CLASSES, Blocks
import blocks_cases as BC
import blocks_ref as BR
import folded_cases as F
import judge_cases as JC
import overlaps_cases as OC
import test_folded_gpu as FG
import test_spans_gpu as SG
from test_judge_gpu import device_graph, finder, model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def read_all(b, ne):
    ed = b.edges()
    return dict(rows=b.rows(), edges={e: (ed["cls"][e], ed["full"][e], ed["first_row"][e], ed["nrows"][e]) for e in range(ne)}, pieces=b.pieces(),
                stats=b.stats(), **b.na50())


def blocks_equal(g, vm, records, nodes, edges, ne, tol=BC.TOL, keep=False):
    """the device's rows, per-edge arrays, pieces, stats, NA50 and NGA50 == the restatement's -> the restatement's result (and the
    open Blocks with keep)"""
    want = BR.align(g.k, nodes, edges, records, tol, id_bound=ne)
    b = g.alignBlocks(vm, records, tol)
    got = read_all(b, ne)
    assert got["stats"] == want["stats"]
    assert got["rows"] == want["rows"]
    assert got == want
    BR.identities(got["stats"], live_edges=len(edges))
    if keep:
        return want, b
    b.close()
    return want


@pytest.fixture(scope="module", params=JC.KS)
def chim(request, ctx):
    k = request.param
    case = BC.chimeras(k)
    g, vm = device_graph(ctx, k, case["reads"])
    yield dict(k=k, case=case, g=g, vm=vm, model=model(g))
    vm.close()
    g.close()


@pytest.fixture(scope="module", params=JC.KS)
def main(request, ctx):
    k = request.param
    case = JC.main(k)
    g, vm = device_graph(ctx, k, case["reads"])
    yield dict(k=k, case=case, g=g, vm=vm, model=model(g))
    vm.close()
    g.close()


def test_planted_contigs(chim):
    """every breakpoint class and edge class by a planted contig; a record shorter than k, an empty one, one of exactly k; then
    a second finish with another tol, without feeding again"""
    k, case, g, vm = chim["k"], chim["case"], chim["g"], chim["vm"]
    nodes, edges, _ends, ne = chim["model"]
    find = finder(edges)
    want, b = blocks_equal(g, vm, case["records"], nodes, edges, ne, keep=True)
    for name, (cls, full) in case["classes"].items():
        assert want["edges"][find(case["paths"][name])][:2] == (cls, full) and want["edges"][find(JC.rc(case["paths"][name]))][:2] == (cls, full)
    for tol in (BC.TOL - 1, 0, 10 ** 6, BC.TOL):
        b.finish(tol)
        assert read_all(b, ne) == BR.align(k, nodes, edges, case["records"], tol, id_bound=ne)
    b.close()
    blocks_equal(g, vm, BC.marked(case["records"], k), nodes, edges, ne)


def test_main_case_and_its_variants(main):
    k, case, g, vm = main["k"], main["case"], main["g"], main["vm"]
    nodes, edges, _ends, ne = main["model"]
    find = finder(edges)
    want = blocks_equal(g, vm, case["records"], nodes, edges, ne)
    assert all(want["edges"][find(case["paths"][n])][:2] == ("exact", 1) for n in JC.coords(k))
    want = blocks_equal(g, vm, JC.variant_marks(case["records"], k), nodes, edges, ne)
    assert want["edges"][find(case["paths"]["c0a"])][0] == "colinear" and want["edges"][find(case["paths"]["c3"])][0] == "colinear"
    want = blocks_equal(g, vm, JC.variant_deletion(case["records"]), nodes, edges, ne)
    assert want["edges"][find(case["paths"]["d1"])][0] == "indel" and want["stats"]["indel_shift_max"] == 1


def test_slices_give_the_unsliced_answers(main, ctx):
    """slice boundaries inside a run, on a run's first start and on its last, k - 1 and k characters behind an invalid character"""
    k, case, g, vm = main["k"], main["case"], main["g"], main["vm"]
    nodes, edges, _ends, ne = main["model"]
    recs = JC.variant_marks(case["records"], k)
    try:
        for sl in BC.slice_values(k):
            ctx.set_option("test_place_slice", sl)
            blocks_equal(g, vm, recs, nodes, edges, ne)
    finally:
        ctx.set_option("test_place_slice", 0)


def test_slices_shorter_than_k_plus_1(main, ctx):
    """every slice is all halo: 1, k - 1 and k characters, over the first 400 bases with the N and the lowercase run"""
    k, case, g, vm = main["k"], main["case"], main["g"], main["vm"]
    nodes, edges, _ends, ne = main["model"]
    recs = [JC.variant_marks(case["records"], k)[0][:400], "ACGT"]
    try:
        for sl in BC.short_slices(k):
            ctx.set_option("test_place_slice", sl)
            blocks_equal(g, vm, recs, nodes, edges, ne)
    finally:
        ctx.set_option("test_place_slice", 0)


def test_repeats(ctx):
    """an exact repeat and an inverted repeat longer than k"""
    for k in JC.KS:
        case = JC.repeats(k)
        g, vm = device_graph(ctx, k, case["reads"])
        nodes, edges, _ends, ne = model(g)
        want = blocks_equal(g, vm, case["records"], nodes, edges, ne)
        assert want["stats"]["edges_repeat"] >= 2 and want["stats"]["brk_overlap"] >= 2
        vm.close(); g.close()


# ---- a record of several workgroups' tiles -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=JC.LONG_KS)
def long_setup(request, ctx):
    k = request.param
    case = JC.long_record(k)
    g, vm = device_graph(ctx, k, case["reads"])
    yield dict(k=k, case=case, g=g, vm=vm, model=model(g))
    vm.close()
    g.close()


def test_long_record_over_four_tiles(long_setup):
    """runs across a lane's 16 starts, a wave's 1024 and the first two tile boundaries; a run that ends on the last start of the
    third tile; invalid characters on, just before and k - 1 after a boundary; records of T - 1, T and T + 1 windows; the long
    record as the second record"""
    k, case, g, vm = long_setup["k"], long_setup["case"], long_setup["g"], long_setup["vm"]
    nodes, edges, _ends, ne = long_setup["model"]
    rec = case["record"]
    want = blocks_equal(g, vm, [rec], nodes, edges, ne)
    assert want["stats"]["edges_exact"] == 10 and want["stats"]["full_edges"] == 10
    want = blocks_equal(g, vm, [JC.long_marks(rec, k)], nodes, edges, ne)
    assert want["stats"]["edges_colinear"] == 2
    for cut, windows in zip(JC.long_truncations(rec, k), (JC.T - 1, JC.T, JC.T + 1)):
        assert blocks_equal(g, vm, [cut], nodes, edges, ne)["stats"]["windows"] == windows
    want = blocks_equal(g, vm, [JC.main(k)["records"][1], rec], nodes, edges, ne)
    assert {r[2] for r in want["rows"]} == {1}


def test_long_record_slices(long_setup, ctx):
    """device slices of T, T + 1, T + k - 1, T + k and 2T characters of the marked record: a later slice starts its halo early, so its
    tile boundaries are not the unsliced ones"""
    k, case, g, vm = long_setup["k"], long_setup["case"], long_setup["g"], long_setup["vm"]
    nodes, edges, _ends, ne = long_setup["model"]
    recs = [JC.long_marks(case["record"], k)]
    try:
        for sl in (JC.T, JC.T + 1, JC.T + k - 1, JC.T + k, 2 * JC.T):
            ctx.set_option("test_place_slice", sl)
            blocks_equal(g, vm, recs, nodes, edges, ne)
    finally:
        ctx.set_option("test_place_slice", 0)


def test_many_records_and_capped_grids(ctx):
    """300 short reference records in one handle; the finish kernels under test_max_grid = 1 and 3"""
    k = 21
    reads, pairs = OC.many(77, k, n=300)
    g, vm = device_graph(ctx, k, reads)
    nodes, edges, _ends, ne = model(g)
    records = [left + right[o:] for left, right, o in pairs]
    want = blocks_equal(g, vm, records, nodes, edges, ne)
    assert max(r[2] for r in want["rows"]) == 299
    try:
        for cap in (1, 3):
            ctx.set_option("test_max_grid", cap)
            uses = ctx.grid_cap_uses()
            blocks_equal(g, vm, records, nodes, edges, ne)
            assert ctx.grid_cap_uses() > uses
    finally:
        ctx.set_option("test_max_grid", 0)
    vm.close(); g.close()


@pytest.mark.parametrize("k", F.KS)
def test_folded_graph(ctx, k):
    """tandem and inverted repeats, a hairpin and, at even k, the palindromic node: the genome as one record and cut in two"""
    c = F.case(k, F.SEEDS[k], "clean")
    m, g, vm = FG.build(ctx, c)
    nodes, bid = SG.by_id(g)
    ln, le = FG.live(nodes, bid)
    at, n = F.where(F.SEEDS[k], k, "inverted")
    for records in ([c.genome], [c.genome[:at + n // 2], c.genome[at + n // 2:]]):
        want = blocks_equal(g, vm, records, ln, le, len(bid), tol=5)
        assert want["stats"]["rows"] > 0 and (len(records) > 1 or want["stats"]["edges_repeat"] > 0)
    for x in (vm, g, m):
        x.close()


def test_after_simplify_and_an_edit(main, ctx):
    """a graph after simplifyGraph gives the restatement's answers on its own ids; an edit makes every call but close GK_E_STATE"""
    k, case = main["k"], main["case"]
    g, vm0 = device_graph(ctx, k, case["reads"])
    vm0.close()
    g.simplifyGraph()
    vm = g.getGraphMap()
    nodes, edges, _ends, ne = model(g)
    _want, b = blocks_equal(g, vm, case["records"], nodes, edges, ne, keep=True)
    assert g.removeEdgesById([finder(edges)(case["paths"]["c3"])]) == 1
    for call in (b.stats, b.rows, b.edges, b.pieces, lambda: b.finish(3), lambda: b.add_record("ACGT")):
        with pytest.raises(L.GkError) as ei:
            call()
        assert ei.value.code == L.GK_E_STATE
    b.close()
    # a stale map: a new handle over the old map refuses the first record that reaches the removed edge, and every record after it
    stale = Blocks(g, vm)
    with pytest.raises(L.GkError) as ei:
        stale.add_record(case["records"][0])
    assert ei.value.code == L.GK_E_STATE
    with pytest.raises(L.GkError) as ei:
        stale.add_record("ACGT")
    assert ei.value.code == L.GK_E_STATE
    stale.close(); vm.close(); g.close()


def test_errors(main, ctx):
    k, case, g, vm = main["k"], main["case"], main["g"], main["vm"]
    nodes, edges, _ends, ne = main["model"]
    lib = L.lib()
    other = 31 if k != 31 else 21
    g2, vm2 = device_graph(ctx, other, JC.main(other)["reads"])
    with pytest.raises(L.GkError) as ei:
        Blocks(g, vm2)
    assert ei.value.code == L.GK_E_KLEN
    vm2.close(); g2.close()
    h, n, st = L.vp(), C.c_uint64(7), np.zeros(len(BR.STATS), np.uint64)
    assert lib.gk_blocks_create(None, vm.h, C.byref(h)) == L.GK_E_INVALID and lib.gk_blocks_create(g.h, None, C.byref(h)) == L.GK_E_INVALID
    assert lib.gk_blocks_create(g.h, vm.h, None) == L.GK_E_INVALID
    assert lib.gk_blocks_add_record(None, b"ACGT", 4) == L.GK_E_INVALID and lib.gk_blocks_finish(None, 3) == L.GK_E_INVALID
    assert lib.gk_blocks_stats(None, L.ptr(st, C.c_uint64)) == L.GK_E_INVALID and lib.gk_blocks_last_ms(None, None) == L.GK_E_INVALID
    assert lib.gk_blocks_rows(None, None, None, None, None, None, None, None, None, 0, C.byref(n)) == L.GK_E_INVALID and n.value == 0
    lib.gk_blocks_destroy(None)
    b = Blocks(g, vm)
    for r in case["records"]:
        b.add_record(r)
    # before the first finish
    for call in (b.stats, b.rows, b.edges, b.pieces):
        with pytest.raises(L.GkError) as ei:
            call()
        assert ei.value.code == L.GK_E_STATE
    assert lib.gk_blocks_add_record(b.h, None, 4) == L.GK_E_INVALID
    b.finish(BC.TOL)
    with pytest.raises(L.GkError) as ei:
        b.add_record("ACGT")
    assert ei.value.code == L.GK_E_STATE
    want = BR.align(k, nodes, edges, case["records"], BC.TOL, id_bound=ne)
    # a short cap: *n is set, nothing is copied; any array may be NULL
    nr = len(want["rows"])
    edge = np.full(nr, 77, np.uint32)
    assert lib.gk_blocks_rows(b.h, L.ptr(edge, C.c_uint32), None, None, None, None, None, None, None, nr - 1, C.byref(n)) == L.GK_E_CAPACITY
    assert n.value == nr and set(edge.tolist()) == {77}
    assert lib.gk_blocks_rows(b.h, L.ptr(edge, C.c_uint32), None, None, None, None, None, None, None, nr, C.byref(n)) == L.GK_OK
    assert edge.tolist() == [r[0] for r in want["rows"]]
    ln = np.full(len(want["pieces"]), 77, np.uint64)
    assert lib.gk_blocks_pieces(b.h, L.ptr(ln, C.c_uint64), None, len(ln) - 1, C.byref(n)) == L.GK_E_CAPACITY and n.value == len(ln) and set(ln.tolist()) == {77}
    assert lib.gk_blocks_pieces(b.h, L.ptr(ln, C.c_uint64), None, len(ln), C.byref(n)) == L.GK_OK and ln.tolist() == [p[0] for p in want["pieces"]]
    assert lib.gk_blocks_rows(b.h, None, None, None, None, None, None, None, None, nr, None) == L.GK_E_INVALID
    # an edge id at the bound: nothing written
    ids, cls = np.array([0, ne], np.uint32), np.full(2, 77, np.uint8)
    assert lib.gk_blocks_edges(b.h, L.ptr(ids, C.c_uint32), 2, L.ptr(cls, C.c_uint8), None, None, None) == L.GK_E_INVALID and cls.tolist() == [77, 77]
    assert lib.gk_blocks_edges(b.h, L.ptr(ids, C.c_uint32), 1, L.ptr(cls, C.c_uint8), None, None, None) == L.GK_OK and BLOCK_CLASSES[cls[0]] == want["edges"][0][0]
    assert set(b.last_ms()) == {"upload", "count_kernels", "emit_kernels", "total", "finish_kernels", "finish_total"}
    b.close()


def test_align_contigs_reads_fasta(chim, tmp_path):
    """genome_amd.check.align_contigs over a FASTA file (plain and .gz) and over bytes == the restatement"""
    import gzip
    k, case, g = chim["k"], chim["case"], chim["g"]
    nodes, edges, _ends, ne = chim["model"]
    records = [r for r in case["records"] if r]                     # (FASTA cannot tell an empty record's lines from none: it still counts)
    text = JC.fasta(records)
    (tmp_path / "ref.fa").write_bytes(text)
    with gzip.open(tmp_path / "ref.fa.gz", "wb") as f:
        f.write(text)
    want = BR.align(k, nodes, edges, records, BC.TOL, id_bound=ne)
    for src in (tmp_path / "ref.fa", tmp_path / "ref.fa.gz", text):
        out = GC.align_contigs(g, src, BC.TOL)
        assert (out["stats"], out["rows"], out["pieces"], out["na50"], out["nga50"]) == (want["stats"], want["rows"], want["pieces"], want["na50"], want["nga50"])
        assert out["genome_fraction"] == want["stats"]["covered"] / want["stats"]["windows"]
