"""gk_graph_remove_weak_edges on the device against its restatement (tests/weak_ref.py) (-m gpu): the hand-written graphs of
tests/weak_cases.py built on the device from their counts, two random cases where the restatement reads the oracle's table and
graph, the same under a capped grid, the refusals, and a graph with a node copy.

The random inputs are synth.reads_mode_g(3000, 100, 2000, 0.01, config_id=...) with the k-mers seen once dropped, as in
tests/test_tips_gpu.py.  The config ids were searched on the CPU, with the oracle and the restatement alone, from 0 upwards for
the first at which, at ratio 5 and max_len 2k, rule (A) removes at least 5 edges and keeps at least one candidate (both asserted
below).  Found there, at 3000 reads:
  k = 21: config_id 0 — 2156 edges, 712 candidates, 272 removed
  k = 55: config_id 7 —  624 edges,  64 candidates,   6 removed (ids 0..6 remove 0 to 4)
"""
import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import WEAK_STATS, buildGraph
from oracle import oracle as O

import tips_ref as T
import weak_cases as WC
import weak_ref as W
from test_tips_gpu import fill, oracle_graph_edges

pytestmark = pytest.mark.gpu
CASES = WC.cases()
BY = {c["name"]: c for c in CASES}
RANDOM = {21: 0, 55: 7}           # k -> config_id of synth.reads_mode_g
READS = 3000
ZERO = dict.fromkeys(W.STATS, 0)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_option("test_max_grid", 0)
    c.close()


def test_the_binding_names_the_stats_as_the_restatement_does():
    assert WEAK_STATS == W.STATS == WC.STATS


def left_of(edges, removed):
    return sorted(e for i, e in enumerate(edges) if i not in removed)


def check_hand_case(ctx, case):
    """build, the calls that remove nothing, the call, a second call: all against the restatement; -> the first call's result"""
    counts, edges = case["counts"], sorted(case["edges"])
    max_len, ratio, floor = case["max_len"], case["ratio"], case["floor"]
    m = fill(ctx, WC.K, counts)
    g = buildGraph(WC.K, m)
    assert sorted(g.canonical()[1]) == edges
    nodes, fp = g.counts()[0], g.idFingerprint()
    want_rm, want = W.weak(counts, edges, max_len, ratio, floor)
    assert {edges[i] for i in want_rm} == case["removed"] and want == case["stats"]                 # the hand-computed answer
    assert g.removeWeakEdges(m, 0, max(ratio, 1), 1000) == ZERO and g.idFingerprint() == fp          # max_len = 0 removes nothing
    off = g.removeWeakEdges(m, max_len, 0, 0)                                                        # ratio = floor = 0 neither
    assert off == dict(ZERO, candidates=W.weak(counts, edges, max_len, 0, 0)[1]["candidates"]) and g.idFingerprint() == fp
    got = g.removeWeakEdges(m, max_len, ratio, floor)
    assert got == want
    left = left_of(edges, want_rm)
    assert sorted(g.canonical()[1]) == left
    assert g.counts()[0] == nodes                                                                    # nodes stay
    rm2, want2 = W.weak(counts, left, max_len, ratio, floor)                                         # a second call: the new state
    assert g.removeWeakEdges(m, max_len, ratio, floor) == want2
    assert sorted(g.canonical()[1]) == left_of(left, rm2)
    g.close(); m.close()
    return got, left


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_graphs(ctx, case):
    check_hand_case(ctx, case)


def test_default_arguments_are_2k_ratio_5_floor_0(ctx):
    case = BY["chimeric_bridge"]
    assert (case["max_len"], case["ratio"], case["floor"]) == (2 * WC.K, 5, 0)
    m = fill(ctx, WC.K, case["counts"])
    g = buildGraph(WC.K, m)
    assert g.removeWeakEdges(m) == case["stats"]
    g.close(); m.close()


@pytest.fixture(scope="module")
def random_case(ctx):
    """per k: the device's table, with the oracle's table and graph (computed once)"""
    made = {}

    def get(k):
        if k not in made:
            rec = synth.reads_mode_g(READS, 100, 2000, 0.01, config_id=RANDOM[k])
            ref = O.PMap(k, 1)
            occ = ref.count_reads(rec.tobytes(), READS)
            ref.delete_lt(2)
            lo, hi, cnt = ref.export_sorted()
            counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
            m = HipDNAMap(ctx, k, occ)
            assert m.count_reads(rec.tobytes(), READS) == occ
            m.deleteAll_lt(2)
            made[k] = (m, counts, sorted(oracle_graph_edges(O.Graph(ref))))
        return made[k]

    yield get
    for m, _c, _e in made.values():
        m.close()


def check_random_case(ctx, random_case, k):
    m, counts, edges = random_case(k)
    g = buildGraph(k, m)
    assert sorted(g.canonical()[1]) == edges
    nodes = g.counts()[0]
    rm, want = W.weak(counts, edges, 2 * k, 5, 0)
    # the input qualifies: the rule has work to do, and a reason to hold back
    assert want["removed_ratio"] >= 5 and want["candidates"] > want["removed_ratio"]
    assert g.removeWeakEdges(m) == want                                  # max_len = None: 2k; ratio 5, floor 0
    left = left_of(edges, rm)
    assert sorted(g.canonical()[1]) == left and g.counts()[0] == nodes
    assert T.strand_closed(left)
    # a second round on the merged graph, with a floor this time
    g.simplifyGraph()
    merged = sorted(g.canonical()[1])
    assert len(merged) < len(left) and T.strand_closed(merged)
    rm2, want2 = W.weak(counts, merged, 2 * k, 5, 3)
    assert g.removeWeakEdges(m, 2 * k, 5, 3) == want2
    left2 = left_of(merged, rm2)
    assert sorted(g.canonical()[1]) == left2 and T.strand_closed(left2)
    g.close()
    return want, want2


@pytest.mark.parametrize("k", sorted(RANDOM))
def test_random_reads_against_the_oracle_and_the_restatement(ctx, random_case, k):
    _first, second = check_random_case(ctx, random_case, k)
    if k == 21:
        assert second["removed_floor_only"] >= 1                         # (B) alone had work to do as well


@pytest.mark.parametrize("G", [1, 3])
def test_under_a_capped_grid_the_results_are_the_same(ctx, random_case, G):
    """one workgroup walks every edge (G = 1); a stride that is no power of two (G = 3)"""
    before = ctx.grid_cap_uses()
    try:
        ctx.set_option("test_max_grid", G)
        check_random_case(ctx, random_case, 21)
        check_hand_case(ctx, BY["chimeric_bridge"])
    finally:
        ctx.set_option("test_max_grid", 0)
    assert ctx.grid_cap_uses() > before, "no launch consulted test_max_grid"


def test_a_table_that_lacks_one_kmer_is_refused_and_the_graph_untouched(ctx):
    case = BY["chimeric_bridge"]
    edges = sorted(case["edges"])
    m = fill(ctx, WC.K, case["counts"])
    g = buildGraph(WC.K, m)
    lacking = dict(case["counts"])
    del lacking[WC.R.canon(WC.G[3:3 + WC.K])]                            # a k-mer inside one of G's edges, far from the bridge
    assert T.coverage(lacking, edges)[1] == 2                            # the window and its twin's
    m2 = fill(ctx, WC.K, lacking)
    fp, chk = g.idFingerprint(), g.checksum()
    with pytest.raises(L.GkError) as err:
        g.removeWeakEdges(m2)
    assert err.value.code == L.GK_E_STATE
    assert (g.idFingerprint(), g.checksum()) == (fp, chk) and sorted(g.canonical()[1]) == edges
    assert g.removeWeakEdges(m) == case["stats"]                         # and the handle works on
    g.close(); m.close(); m2.close()


def test_a_ratio_beyond_65535_is_invalid(ctx):
    case = BY["chimeric_bridge"]
    m = fill(ctx, WC.K, case["counts"])
    g = buildGraph(WC.K, m)
    chk = g.checksum()
    with pytest.raises(L.GkError) as err:
        g.removeWeakEdges(m, ratio=W.MAX_RATIO + 1)
    assert err.value.code == L.GK_E_INVALID and g.checksum() == chk
    assert g.removeWeakEdges(m, ratio=W.MAX_RATIO) == dict(case["stats"], removed_ratio=0, removed=0)   # 65535 * 230 is not below 1200
    g.close(); m.close()


def test_competitors_are_found_by_node_id(ctx):
    """the bridge re-attached (by id) to a COPY of its end node: the copy has one way in, so the bridge is no connection any more
    and stays, while its twin, whose nodes are as they were, goes"""
    case = BY["chimeric_bridge"]
    counts, edges = case["counts"], sorted(case["edges"])
    m = fill(ctx, WC.K, counts)
    g = buildGraph(WC.K, m)
    ids = np.array([g.nodeId(s, q[0])[1] for s, _e, q in edges], np.uint32)
    assert len(set(ids.tolist())) == len(edges)
    i = edges.index(WC.edge(WC.bridge(WC.B)[1]))
    copy = g.addNode(edges[i][1])
    g.replaceEnd(int(ids[i]), copy)
    info = g.edgesById(ids)
    assert info["alive"].all() and int(info["end"][i]) == copy
    ends = list(zip(info["start"].tolist(), info["end"].tolist()))
    rm, want = W.weak(counts, edges, 2 * WC.K, 5, 0, ends)
    assert len(rm) == 1 and i not in rm and want == dict(zip(W.STATS, (1, 1, 0, 1)))
    assert len(W.weak(counts, edges, 2 * WC.K, 5, 0)[0]) == 2            # by k-mer the rule would take both
    assert g.removeWeakEdges(m) == want
    assert sorted(g.canonical()[1]) == left_of(edges, rm)
    g.close(); m.close()


def test_multik_assemble_takes_the_step_through_an_opt_in_keyword(ctx):
    """the planted read set of tests/weak_planted.py through genome_amd.multik.assemble: off by default, on with remove_weak"""
    from genome_amd import multik
    import weak_planted as P

    reads = P.reads()
    binb = dna.reads_to_bin(reads)
    got = {}
    for name, kw in (("off", {}), ("defaults", {"remove_weak": {}}), ("floor_alone", {"remove_weak": {"ratio": 0, "floor": 20}}),
                     ("too_short", {"remove_weak": {"max_len": P.K - 1}})):
        m, g, stages = multik.assemble(ctx, binb, len(reads), [P.K], rounds=P.ROUNDS, **kw)
        got[name] = (g.counts()[1], stages[0]["edges"])
        g.close(); m.close()
    assert got == {"off": (10, 10), "defaults": (4, 4), "floor_alone": (4, 4), "too_short": (10, 10)}
