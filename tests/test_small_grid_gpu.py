"""The graph phase's grid-stride loops, the per-workgroup LDS component table's overflow and scan_counts over several chunks, at a
size the oracle can follow (-m gpu).

Every graph-phase launch takes at most cu_count * 8 workgroups of BLOCK threads, so at any size the oracle and the restatements
can follow every `for (i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)` makes ONE trip.  The test build's
"test_max_grid" (include/genome_amd_test.h) caps those grids: G = 1 makes one workgroup walk everything — and see every root, so
that its 1024-entry component table overflows — G = 3 gives a stride that is no power of two and a last trip that differs per
workgroup.  Everything here runs under forced(ctx, test_max_grid=G) and is compared with the oracle or a restatement, never with
another run of the device; where it is cheap the same call is made once more at the default grid on the same handle.

The inputs (tests/small_grid_cases.py) were sized on the CPU oracle; every case asserts on the reference side what it relies on:
more than 2 * G * BLOCK nodes and edges, neither a multiple of 64 (a second trip, and a last one with a partly filled wave), more
components than 1024 / 0.6, more nodes than one SCAN_CHUNK.  As measured there:
  reads, k = 11:  1886 nodes, 2741 edges;  k = 35: 2012 nodes, 2330 edges;  k = 64: 2068 nodes, 1924 edges
  (their components at build are compared too: 14 with one of 1860 nodes, 128 up to 196 nodes, 330 up to 66 nodes)
  planted, k = 31 and k = 34:  4682 nodes, 2530 edges, 2224 components, 18 of them tied for largest at 15 nodes; one round of the
  tip rule removes 54 edges, one of the bubble rule 54 more (72 pairs compared)
  (d): the k = 11 graph again (19504 position-map entries; merged: 1389 edges, 46 of them longer than 64 bases); 2500 pairs per
  walkPairs call; a spectrum table of more than 2048 slots; 197 records to correct
Every block under the cap also asks the switch's echo (gk_test_grid_cap_uses) that launches in it were sized by the cap.
"""
from contextlib import contextmanager

import numpy as np
import pytest

from genome_amd import dna
from genome_amd.dnamap import HipDNAMap
from genome_amd.graph import buildGraph, loadGraph
from oracle import oracle as O

import bubbles_ref as B
import components_ref as CR
import small_grid_cases as S
import test_checkgraph_gpu as checkgraph_cases
import test_correct_gpu as correct_cases
import test_pairs_gpu as pairs_cases
import test_spectrum_gpu as spectrum_cases
import test_vmap_gpu as vmap_cases
import tips_ref as T
from small_grid_cases import BLOCK, CC_TAB, SCAN_CHUNK      # gk_tile.h (through gk_internal.h), gk_graph_ops.hip, gk_scan.h
from test_fuzz_gpu import _oracle_graph
from test_graph_file_gpu import same_graph
from test_variants_gpu import ctx, forced  # noqa: F401 (the module-scoped context fixture)

pytestmark = pytest.mark.gpu
GRIDS = (1, 3)


def two_trips(n, G):
    """a grid of G workgroups of BLOCK lanes takes a second trip over n items, and the last wave of the last trip is partly filled"""
    return n > 2 * G * BLOCK and n % 64 != 0


@contextmanager
def unitigs(ctx, mode):
    """the unitig construction of gk_graph_build: lanes fed from a queue, one edge per lane, pointer jumping, or the first on a
    minimizer-bucketed copy of the table"""
    try:
        ctx.set_option("graph_unitigs", {"walk": 1, "walk1": 1, "pj": 2, "mbt": 0}[mode])
        ctx.set_option("graph_walk_queue", 0 if mode == "walk1" else -1)
        ctx.set_option("graph_mbt", 1 if mode == "mbt" else -1)
        yield
    finally:
        ctx.set_option("graph_unitigs", 0)
        ctx.set_option("graph_walk_queue", -1)
        ctx.set_option("graph_mbt", -1)


@contextmanager
def capped(ctx, G):
    """forced(ctx, test_max_grid=G), and the switch's echo: launches inside the block were sized under the cap"""
    with forced(ctx, test_max_grid=G):
        before = ctx.grid_cap_uses()
        yield
        assert ctx.grid_cap_uses() > before, "no launch consulted test_max_grid"


def test_the_switch_refuses_a_negative_grid(ctx):
    from genome_amd import _lib as L
    with pytest.raises(L.GkError) as e:
        ctx.set_option("test_max_grid", -1)
    assert e.value.code == L.GK_E_INVALID
    for ok in (1, 3, 1 << 20, 0):
        ctx.set_option("test_max_grid", ok)
    # the echo counts launches under the cap only
    m = HipDNAMap(ctx, 21, 1 << 10)
    m.count_reads(dna.reads_to_bin(["AGCT" * 10]), 1)
    before = ctx.grid_cap_uses()
    m.spectrum(16)
    assert ctx.grid_cap_uses() == before
    with forced(ctx, test_max_grid=2):
        m.spectrum(16)
    assert ctx.grid_cap_uses() == before + 1
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) build -> removeBubbles -> simplifyGraph -> removeEdges -> simplifyGraph -> retainLargest against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
_FLOW = {}


def _sample(nodes):
    return nodes[::max(1, len(nodes) // 48)]


def _flow_reference(k):
    """the oracle's graph after every step: (canonical, out_order of a sample of its nodes), computed once per k"""
    if k in _FLOW:
        return _FLOW[k]
    reads = S.reads_case(k)
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, len(reads))
    ref.delete_lt(2)
    og = O.Graph(ref)
    steps = []

    def snap():
        nodes, edges = _oracle_graph(og, k)
        steps.append((nodes, edges, {s: og.out_order(*dna.pack(s)) for s in _sample(nodes)}))
    snap()
    sizes = (og.num_nodes(), og.num_edges())
    stats, hist = CR.stats(*steps[0][:2]), CR.histograms(*steps[0][:2])
    assert len(stats) == og.num_components()
    og.remove_bubbles(); snap()
    og.simplify(); snap()
    victims = [(s, q[0]) for i, (s, _e, q) in enumerate(steps[-1][1]) if i % 3 == 0]
    for s, b in victims:
        assert og.remove_edge(*dna.pack(s), "AGCT".index(b))
    snap()
    og.simplify(); snap()
    comps = og.num_components()
    kept = og.retain_largest(); snap()
    _FLOW[k] = dict(binb=binb, n=len(reads), occ=occ, keys=ref.size(), steps=steps, sizes=sizes, stats=stats, hist=hist, victims=victims, comps=comps, kept=kept)
    og.close(); ref.close()
    return _FLOW[k]


def _same(g, step):
    nodes, edges, orders = step
    assert g.canonical() == (nodes, edges)
    for s, want in orders.items():
        assert g.out_order(s) == want, s


def _run_flow(ctx, k, mode, F):
    m = HipDNAMap(ctx, k)
    assert m.count_reads(F["binb"], F["n"]) == F["occ"]
    m.deleteAll_lt(2)
    with unitigs(ctx, mode):
        g = buildGraph(k, m)
    if mode == "mbt":       # (graph_build_entry: tables below 4096 keys and k = 64's tagged slots are read in place)
        assert F["keys"] >= 4096 and (g.buildStats()["bucketed_table"]["slots"] > 0) == (k != 64)
    if mode == "pj":
        assert g.buildStats()["pointer_jumping"]
    steps = F["steps"]
    _same(g, steps[0])
    nodes_pc, len_pc = g.componentStats()               # components of hundreds of nodes: one root, many waves and trips
    assert sorted(zip((int(x) for x in nodes_pc), (int(x) for x in len_pc))) == F["stats"]
    assert g.componentHistograms() == F["hist"]
    g.removeBubbles(); _same(g, steps[1])
    g.simplifyGraph(); _same(g, steps[2])
    assert g.removeEdges(F["victims"]) == len(F["victims"]); _same(g, steps[3])
    g.simplifyGraph(); _same(g, steps[4])
    assert g.retainLargest() == (F["kept"], F["comps"]); _same(g, steps[5])
    assert g.counts()[0] == F["kept"]
    g.close(); m.close()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("mode", ["walk", "walk1", "pj", "mbt"])
@pytest.mark.parametrize("k", [11, 35, 64])
def test_build_to_retain_against_the_oracle(ctx, k, mode, G):
    F = _flow_reference(k)
    nodes, edges = F["sizes"]
    assert two_trips(nodes, G) and two_trips(edges, G), (nodes, edges)
    assert len(F["victims"]) > 64 and F["comps"] > 1 and 0 < F["kept"] < len(F["steps"][4][0])
    assert F["stats"][-1][0] > (BLOCK if k == 11 else 8) and len(set(F["stats"])) > 3     # the largest component, at build
    with capped(ctx, G):
        _run_flow(ctx, k, mode, F)
    if G == GRIDS[0]:       # the same at the default grid
        _run_flow(ctx, k, mode, F)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) components, per component
# ---------------------------------------------------------------------------------------------------------------------------
_PLANTED = {}


def _planted_reference(k):
    if k in _PLANTED:
        return _PLANTED[k]
    counts = S.planted_case(k)
    ref = O.PMap(k, 1)
    for key in counts:
        ref.update_inc(*dna.pack(key))
    og = O.Graph(ref)
    nodes, edges = _oracle_graph(og, k)
    comps = og.num_components()
    kept = og.retain_largest()
    _PLANTED[k] = dict(counts=counts, nodes=nodes, edges=edges, comps=comps, kept=kept, retained=_oracle_graph(og, k),
                       stats=CR.stats(nodes, edges), hist=CR.histograms(nodes, edges), tied=CR.tied_for_largest(nodes, edges))
    og.close(); ref.close()
    return _PLANTED[k]


def fill(ctx, k, counts):
    m = HipDNAMap(ctx, k, 2 * len(counts) + 64)
    lo, hi = dna.pack_many(list(counts))
    m.add_counts(lo, hi, np.array(list(counts.values()), np.int32))
    return m


def _check_components(g, P):
    nodes_pc, len_pc = g.componentStats()
    assert sorted(zip((int(x) for x in nodes_pc), (int(x) for x in len_pc))) == P["stats"]
    assert g.componentHistograms() == P["hist"]


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("k", [31, 34])
def test_components_per_component(ctx, k, G):
    P = _planted_reference(k)
    nodes, edges, tied = P["nodes"], P["edges"], P["tied"]
    # the reference side of what this case is for
    assert two_trips(len(nodes), G) and two_trips(len(edges), G)
    assert len(P["stats"]) == P["comps"] > CC_TAB / 0.6                   # one workgroup's LDS table overflows at G = 1
    assert len(nodes) > SCAN_CHUNK and len(nodes) % SCAN_CHUNK != 0
    assert len(tied) >= (17 if k == 34 else 2) and all(len(ms) == P["kept"] for ms in tied)
    assert len(set(P["stats"])) >= 10                                      # a length on the wrong root changes the multiset
    assert CR.retained(nodes, edges) == P["retained"]                      # the restatement and the oracle keep the same component
    keys = [[CR.kmer_key(s) for s in ms] for ms in tied]
    if k == 34:
        # both stages of k_cc_pick decide: several tied components hold a k-mer of the minimal high word, and the smallest
        # low word of all sits in a component that does not win
        min_hi = min(hi for ks in keys for hi, _lo in ks)
        assert sum(1 for ks in keys if any(hi == min_hi for hi, _lo in ks)) >= 2
        winner = min(range(len(tied)), key=lambda i: min(keys[i]))
        lowest = min(range(len(tied)), key=lambda i: min(lo for _hi, lo in keys[i]))
        assert winner != lowest and set(tied[winner]) == set(P["retained"][0])
    m = fill(ctx, k, P["counts"])
    with capped(ctx, G):
        g = buildGraph(k, m)
        assert g.canonical() == (nodes, edges)
        _check_components(g, P)
        if G == 1:
            for find in (0, 1, 2, 3):
                with forced(ctx, cc_find=find):
                    _check_components(g, P)
    _check_components(g, P)                                                # the default grid, the same handle
    with capped(ctx, G):
        assert g.retainLargest() == (P["kept"], P["comps"])
        assert g.canonical() == P["retained"]
    g.close(); m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (c) coverage, tips, bubbles, distance on the graph of (b)
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_ids(g, edges):
    ids = np.array([g.nodeId(s, q[0])[1] for s, _e, q in edges], np.uint32)
    assert len(set(ids.tolist())) == len(edges)
    return ids


def _beyond_first_chunk(g, edges, removed):
    """an edge of `removed` leaves a node whose id is beyond the first SCAN_CHUNK of the node arrays"""
    return any(g.nodeId(edges[i][0])[0] >= SCAN_CHUNK for i in removed)


@pytest.mark.parametrize("G", GRIDS)
def test_coverage_tips_bubbles_distance(ctx, G):
    k = 31
    P = _planted_reference(k)
    counts, edges = P["counts"], sorted(P["edges"])
    assert two_trips(len(P["nodes"]), G) and two_trips(len(edges), G) and len(P["nodes"]) > SCAN_CHUNK
    want_cov, missing = T.coverage(counts, edges)
    assert missing == 0 and any(c[0] > 64 for c in want_cov) and any(c[0] <= 64 for c in want_cov)      # both coverage kernels
    tips = T.tips(counts, edges, 2 * k)
    left = [e for i, e in enumerate(edges) if i not in tips]
    popped, compared = B.pop(counts, left, 2 * k, 3)
    assert len(tips) >= 10 and len(popped) >= 10 and compared > len(popped) // 2
    # pairs for the distance: the parallel ones, and neighbours in the sorted edge list
    pairs = B.parallel_pairs(edges, 2 * k) + [(i, (i * 7 + 1) % len(edges)) for i in range(len(edges))]
    pairs = pairs[:2 * max(GRIDS) * BLOCK + 70]
    assert len(pairs) >= 2 * G * BLOCK and len(pairs) % 4 != 0            # (a workgroup is four waves, a wave takes one pair)
    want_dist = [B.distance(edges[i][2], edges[j][2], 3) for i, j in pairs]
    assert {0, 1, 2, 3, 4} <= set(want_dist)                             # every answer the call can give at max_diff = 3
    m = fill(ctx, k, counts)

    def coverage_is_right(g, ids):
        cov = g.edgeCoverage(m, ids)
        got = list(zip(cov["kmers"].tolist(), cov["sum"].tolist(), cov["min"].tolist(), cov["max"].tolist()))
        assert got == want_cov and cov["missing"] == 0

    with capped(ctx, G):
        g = buildGraph(k, m)
        assert sorted(g.canonical()[1]) == edges
        ids = _edge_ids(g, edges)
        coverage_is_right(g, ids)
        pe, pf = ids[[i for i, _ in pairs]], ids[[j for _, j in pairs]]
        assert g.edgeDistance(pe, pf, 3).tolist() == want_dist
    coverage_is_right(g, ids)                                              # the default grid, the same handle
    assert g.edgeDistance(pe, pf, 3).tolist() == want_dist
    with capped(ctx, G):
        assert _beyond_first_chunk(g, edges, tips)
        assert g.clipTips(m) == len(tips)
        assert sorted(g.canonical()[1]) == left
        assert _beyond_first_chunk(g, left, popped)
        assert g.popBubbles(m) == (len(popped), compared)
        assert sorted(g.canonical()[1]) == [e for i, e in enumerate(left) if i not in popped]
    g.close(); m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the remaining capped launch sites, one case each under G = 1, against the reference their own modules use.  Each asserts on
# the reference side the counts that make its kernels take several trips.
# ---------------------------------------------------------------------------------------------------------------------------
def _k11_pair(ctx):
    """the k = 11 reads graph of (a), freshly built on the device and in the oracle (the oracle's stays open for the caller)"""
    k = 11
    F = _flow_reference(k)
    assert two_trips(F["sizes"][0], 1) and two_trips(F["sizes"][1], 1), F["sizes"]       # 1886 nodes, 2741 edges
    m, ref = HipDNAMap(ctx, k), O.PMap(k, 1)
    assert m.count_reads(F["binb"], F["n"]) == ref.count_reads(F["binb"], F["n"]) == F["occ"]
    m.deleteAll_lt(2); ref.delete_lt(2)
    g, og = buildGraph(k, m), O.Graph(ref)
    assert (og.num_nodes(), og.num_edges()) == F["sizes"]
    return k, F, m, ref, g, og


def test_graph_file_round_trip(ctx, tmp_path):
    k, F, m, ref, g, og = _k11_pair(ctx)
    with capped(ctx, 1):
        g.save(tmp_path / "g.gkg")
        h = loadGraph(ctx, tmp_path / "g.gkg")
        same_graph(g, h)                                                   # ids, fingerprint, checksum, every node's order
        assert h.canonical() == F["steps"][0][:2]
        h.save(tmp_path / "h.gkg")
    g.save(tmp_path / "g0.gkg")                                            # the default grid writes the same bytes
    assert (tmp_path / "g.gkg").read_bytes() == (tmp_path / "h.gkg").read_bytes() == (tmp_path / "g0.gkg").read_bytes()
    h.close(); g.close(); m.close(); og.close(); ref.close()


@pytest.mark.parametrize("simplified", [False, True])
def test_graph_map_against_the_oracles_put_new(ctx, simplified):
    """k_pos_reserve / k_pos_nodes / k_pos_fill / k_pos_fill_long, the value map's kernels and the by-id reads of the comparison"""
    k, F, m, ref, g, og = _k11_pair(ctx)
    if simplified:                                       # long edges: k_pos_fill_long, one edge per workgroup at a time
        g.removeBubbles(); og.remove_bubbles(); g.simplifyGraph(); og.simplify()
        lens = og.edges()["len"]
        assert sum(1 for x in lens if x - 1 > 64) > 2 and og.num_edges() > 2 * BLOCK and og.num_edges() % 64 != 0
    entries = og.total_edge_len() + og.num_nodes() - og.num_edges()
    assert two_trips(entries, 1)
    with capped(ctx, 1):
        vmap_cases.check_graph_map(g, og, k, seed=1)
    g.close(); m.close(); og.close(); ref.close()


def test_contig_stats(ctx):
    """k_contig_reduce and k_contig_hist over 2741 edges, and over the merged graph's"""
    k, F, m, ref, g, og = _k11_pair(ctx)
    with capped(ctx, 1):
        lengths = checkgraph_cases.check_contigs(g, og.edges()["len"])
        assert two_trips(len(lengths), 1)
        g.removeBubbles(); og.remove_bubbles(); g.simplifyGraph(); og.simplify()
        merged = checkgraph_cases.check_contigs(g, og.edges()["len"])
        assert max(merged) > 100 and len(merged) > 2 * BLOCK             # 1389 edges, the longest 175 bases
    assert g.contigStats(100) == checkgraph_cases.ref.contig_stats(merged, 100)           # the default grid, the same handle
    g.close(); m.close(); og.close(); ref.close()


def test_walk_pairs_support(ctx):
    """k_walk_pairs: a wave per pair orientation, 2 * G workgroups of four waves (the smallest case of tests/test_pairs_gpu.py; its
    graph is a dozen nodes, so only the walks and the position lookups of the pairs take several trips here)"""
    case = (21, 1, 0.0, (60, 95))
    npairs = len(pairs_cases.make_pairs(case[1], case[0], err=case[2])) // 2
    assert two_trips(npairs // 2, 1) and 2 * (npairs // 2) > 2 * 2 * (BLOCK // 64)        # per call of the two: 2500 pairs, 5000 orientations
    with capped(ctx, 1):
        pairs_cases.test_walk_pairs_support_and_split_vs_oracle(ctx, *case)


def test_spectrum(ctx):
    """k_spectrum: 4 * BLOCK slots per workgroup and trip, over 12-byte count slots and the 16-byte slots deleteAll leaves"""
    k = 21
    reads = spectrum_cases._ragged_reads(k)
    counts, occ = spectrum_cases._oracle_counts(k)
    m = HipDNAMap(ctx, k, 1 << 13)
    assert m.count_reads(dna.reads_to_bin(reads), len(reads)) == occ
    assert m.slots() > 2 * 4 * BLOCK and len(counts) > 2 * BLOCK
    with capped(ctx, 1):
        spectrum_cases._check(m, counts)
        m.deleteAll_lt(2)
        assert m.slots() > 2 * 4 * BLOCK
        spectrum_cases._check(m, spectrum_cases._oracle_counts(k, 2)[0])
    spectrum_cases._check(m, spectrum_cases._oracle_counts(k, 2)[0])                       # the default grid, the same handle
    m.close()


def test_correct_reads_dev(ctx):
    """k_correct_reads: a tile of 64 records per workgroup at a time; 64 * 3 + 5 records of stride 26 are four tiles, the last of five
    records, out of place and in place"""
    k, tile = 31, 64                                                       # gk_tile.h: TILE_READS
    reads, counts, _raw = correct_cases.run_of(k)
    mine = [r[:99] if i % 7 else r[:i % 99] for i, r in enumerate(reads[:tile * 3 + 5])]
    assert len(mine) > 2 * tile and len(mine) % tile != 0
    rec = correct_cases.fixed_records(mine, 99)
    want, want_st = correct_cases.expected_fixed(counts, rec, mine, k, 3)
    assert want_st["corrected"] > 0 and want_st["short"] > 0 and (want != rec).any()
    assert (want[2 * tile:] != rec[2 * tile:]).any()                       # something to correct beyond the second tile
    m = correct_cases.table_of(ctx, k, "counted", 0)
    d_in, d_out = ctx.alloc(rec.size + 64), ctx.alloc(rec.size + 64)
    ctx.upload(d_in, rec.reshape(-1))
    with capped(ctx, 1):
        correct_cases.check_stats(m.correct_reads_dev(d_in, len(mine), 99, 3, d_out), want_st)
        assert (ctx.download(d_out, rec.size).reshape(rec.shape) == want).all()
        assert (ctx.download(d_in, rec.size).reshape(rec.shape) == rec).all()
        correct_cases.check_stats(m.correct_reads_dev(d_in, len(mine), 99, 3), want_st)
        assert (ctx.download(d_in, rec.size).reshape(rec.shape) == want).all()
    ctx.upload(d_in, rec.reshape(-1))
    correct_cases.check_stats(m.correct_reads_dev(d_in, len(mine), 99, 3), want_st)        # the default grid
    assert (ctx.download(d_in, rec.size).reshape(rec.shape) == want).all()
    ctx.free(d_in); ctx.free(d_out); m.close()
