"""The slot -> rank structure of the pointer-jumping unitig build (gk_graph.hip: k_rank_masks, k_rank_scan, k_rank_fill) on tables
of more than 1024 rank chunks, where the single workgroup of k_rank_scan gives every thread per = ceil(nchunks / 1024) > 1 chunks
— every table beyond 1024 * 16384 = 16.8 M slots, which the production tables all are and no other test's table is.

Direct: the test-build hook gk_test_slot_ranks hands back (mask, base) per 64 slots of a map's table, made by the function the
build calls; base must be the exclusive cumulative popcount of the masks (numpy) and the total the map's size.
End to end: gk_graph_build under "graph_unitigs" = 2 on tables of that many slots — the read sets of
test_graph_gpu.py::test_unitig_construction_modes_agree_with_oracle against the oracle, and the error-free 300 kbp genome of
test_long_unitig_is_fast_and_exact against the genome.  A filter call would compact the table under the bound, so the tables here
are never filtered on the device: the oracle's filtered keys go into a table from gk_map_create_for_graph (gk_map_add_counts),
the genome's reads are counted into a table created that large."""
import ctypes as C
import random
from contextlib import contextmanager

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import oracle as O
from oracle import pyref as R
from test_graph_gpu import _reads, oracle_canonical

pytestmark = pytest.mark.gpu

RANK_CHUNK_SLOTS = 256 * 64                  # gk_graph.hip: RANK_CHUNK blocks of 64 slots
BOUND = 1024 * RANK_CHUNK_SLOTS              # tables of more slots have more than 1024 chunks: per > 1 in k_rank_scan
# The smallest hints whose table passes BOUND.  gk_map_create sizes for a load of 0.65: hint / 0.65 + 1 slots, rounded up to whole
# L1 buckets of segments (a granule BOUND is a multiple of), so the first hint with more than BOUND slots wanted;
# gk_map_create_for_graph sizes for a load of 0.25 while the table is small beside the device's memory: BOUND / 4 keys.
HINT = 10905191
HINT_FOR_GRAPH = BOUND // 4
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@contextmanager
def options(ctx, **opts):
    """test-build switches for the block; 0 (their default) afterwards"""
    try:
        for name, v in opts.items():
            ctx.set_option(name, v)
        yield
    finally:
        for name in opts:
            ctx.set_option(name, 0)


def slot_ranks(m):
    """-> (masks, bases, total) of the map's table as gk_graph_build would rank it"""
    cap = (m.slots() + 63) // 64
    masks, bases = np.full(cap, 0x55, np.uint64), np.full(cap, 0x55, np.uint64)
    nblk, total = C.c_uint64(), C.c_uint64(1 << 60)
    L.check(L.test_hook("gk_test_slot_ranks")(m.h, L.ptr(masks, C.c_uint64), L.ptr(bases, C.c_uint64), cap, C.byref(nblk), C.byref(total)), m.ctx.h)
    assert nblk.value == cap == (m.slots() + 63) // 64, "the table changed its size on the way into the graph layout"
    return masks, bases, total.value


def check_ranks(m, masks, bases, total):
    slots = m.slots()
    pop = POP8[masks.view(np.uint8)].reshape(-1, 8).sum(axis=1)
    assert total == m.size()
    assert int(pop.sum()) == total
    want = np.zeros(len(pop), np.uint64)
    np.cumsum(pop[:-1], dtype=np.uint64, out=want[1:])
    bad = np.flatnonzero(bases != want)
    assert bad.size == 0, f"{bad.size} bases differ, the first at block {int(bad[0])} (chunk {int(bad[0]) // 256}): {int(bases[bad[0]])} != {int(want[bad[0]])}"
    if slots % 64:
        assert int(masks[-1]) >> (slots % 64) == 0, "live bits beyond the table's last slot"


def filled(ctx, k, hint, genome_len=300_000, nreads=20_000, config_id=21):
    """a map created for `hint` keys holding the k-mers of error-free 150-base reads over a synthetic genome; never filtered"""
    m = HipDNAMap(ctx, k, hint)
    d = ctx.alloc(nreads * synth.record_stride(150) + 64)
    ctx.synth_reads(d, nreads, 150, "G", config_id, 0, genome_len, 0.0)
    m.count_reads_dev(d, nreads, 150)
    ctx.free(d)
    return m


@pytest.mark.parametrize("k", [31, 47])
def test_the_hints_are_the_smallest_that_pass_1024_chunks(ctx, k):
    for hint, for_graph in ((HINT, False), (HINT_FOR_GRAPH, True)):
        below, at = HipDNAMap(ctx, k, hint - 1, for_graph=for_graph), HipDNAMap(ctx, k, hint, for_graph=for_graph)
        assert below.slots() == BOUND < at.slots() <= BOUND + BOUND // 16, (hint, for_graph, below.slots(), at.slots())
        below.close(); at.close()


@pytest.mark.parametrize("k", [31, 47])
def test_ranks_of_a_table_beyond_1024_chunks(ctx, k):
    m = filled(ctx, k, HINT)
    assert m.slots() > BOUND, "the sizing policy changed: this table has per == 1 again"
    assert m.size() > 200_000
    masks, bases, total = slot_ranks(m)
    assert m.slots() > BOUND and (len(masks) + 255) // 256 > 1024
    assert m.stats()["slot_bytes"] == (16 if k == 31 else 24)
    check_ranks(m, masks, bases, total)
    # the live slots are spread by the hash: no quarter of the chunks may be empty (a scan that skipped a share would still pass
    # the cumulative check if the share held nothing)
    pop = POP8[masks.view(np.uint8)].reshape(-1, 8).sum(axis=1)
    assert all(int(q.sum()) > total // 8 for q in np.array_split(pop, 4))
    m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_ranks_of_an_empty_table_beyond_1024_chunks(ctx, k):
    m = HipDNAMap(ctx, k, HINT)
    assert m.slots() > BOUND and m.size() == 0
    masks, bases, total = slot_ranks(m)
    assert total == 0 and not masks.any() and not bases.any()
    m.close()


@pytest.mark.parametrize("k,hint,nreads,nchunks", [(31, 10000, 25, 1), (31, 12000, 50, 2), (47, 10000, 25, 1), (47, 12000, 50, 2)])
def test_ranks_of_small_tables(ctx, k, hint, nreads, nchunks):
    """one chunk (16384 slots) and two (32768): the reads' windows fit the table as created and fill less than a quarter of it,
    so neither the count nor the way into the graph layout changes its slots"""
    m = filled(ctx, k, hint, genome_len=5000, nreads=nreads)
    assert m.slots() == nchunks * RANK_CHUNK_SLOTS
    masks, bases, total = slot_ranks(m)
    assert (len(masks) + 255) // 256 == nchunks, m.slots()
    assert total > 1500
    check_ranks(m, masks, bases, total)
    m.close()


def test_null_arguments_are_invalid(ctx):
    f = L.test_hook("gk_test_slot_ranks")
    m = HipDNAMap(ctx, 31)
    a, n = np.zeros(64, np.uint64), C.c_uint64()
    p = L.ptr(a, C.c_uint64)
    assert f(None, p, p, 64, C.byref(n), C.byref(n)) == L.GK_E_INVALID
    assert f(m.h, None, p, 64, C.byref(n), C.byref(n)) == L.GK_E_INVALID
    assert f(m.h, p, None, 64, C.byref(n), C.byref(n)) == L.GK_E_INVALID
    assert f(m.h, p, p, 64, None, C.byref(n)) == L.GK_E_INVALID
    assert f(m.h, p, p, 64, C.byref(n), None) == L.GK_E_INVALID
    assert f(m.h, p, p, 1, C.byref(n), C.byref(n)) == L.GK_E_CAPACITY and n.value == m.slots() // 64
    m.close()


# ---- end to end: gk_graph_build by pointer jumping over more than 1024 rank chunks ---------------------------------------------

def oracle_cases(k, seed, hap):
    """the two read sets of test_unitig_construction_modes_agree_with_oracle[k-seed-hap], counted and filtered by the oracle"""
    rnd = random.Random(seed)
    for err, nreads in ((0.01, 700), (0.0, 400)):
        reads = _reads(rnd, nreads, k + 5, min(255, k + 90), 1500, err, hap)
        ref = O.PMap(k, 1)
        ref.count_reads(dna.reads_to_bin(reads), len(reads))
        ref.delete_lt(2)
        yield ref


@pytest.mark.parametrize("max_grid", [0, 3])
@pytest.mark.parametrize("k,seed,hap", [(31, 5, 2), (35, 6, 2)])
def test_pointer_jumping_beyond_1024_chunks_gives_the_oracles_graph(ctx, k, seed, hap, max_grid):
    for ref in oracle_cases(k, seed, hap):
        lo, hi, cnt = ref.export_sorted()
        m = HipDNAMap(ctx, k, HINT_FOR_GRAPH, for_graph=True)
        m.add_counts(lo, hi, cnt)
        assert m.size() == ref.size() > 0
        with options(ctx, graph_unitigs=2, test_max_grid=max_grid):
            before = ctx.grid_cap_uses()
            assert m.slots() > BOUND, "the sizing policy changed: this table has per == 1 again"
            g = buildGraph(k, m)
            assert (ctx.grid_cap_uses() > before) == (max_grid > 0)
        assert m.slots() > BOUND
        assert g.buildStats()["pointer_jumping"]
        assert g.canonical() == oracle_canonical(O.Graph(ref))
        g.close(); m.close()


def test_long_unitig_beyond_1024_chunks_is_the_genome(ctx):
    n, L_, k, G = 60000, 150, 31, 300_000
    m = filled(ctx, k, HINT, genome_len=G, nreads=n, config_id=12)
    with options(ctx, graph_unitigs=2):
        assert m.slots() > BOUND, "the sizing policy changed: this table has per == 1 again"
        g = buildGraph(k, m)
    assert m.slots() > BOUND
    assert g.buildStats()["pointer_jumping"]
    nodes, edges = g.canonical()
    genome = synth.bases_to_str(synth.genome_bases(G, 12))
    rc = R.rev_comp(genome)
    assert len(nodes) % 2 == 0 and sum(len(q) for _, _, q in edges) == g.counts()[2]
    for s, t_, q in edges:
        w = s + q
        assert (w in genome) or (w in rc)
        assert w.endswith(t_)
    assert max(len(q) for _, _, q in edges) > 20000
    g.close(); m.close()
