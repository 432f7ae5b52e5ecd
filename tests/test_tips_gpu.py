"""gk_graph_clip_tips on the device against its restatement (tests/tips_ref.py) (-m gpu): the hand-written graphs of
tests/tips_cases.py built on the device from their counts, and two random cases — 3000 reads of 100 bases with 1 % errors over
a 2000-base genome, k-mers seen once dropped — where the restatement reads the oracle's table and graph.

The random inputs were chosen on the CPU, with the oracle and the restatement alone, so that the rule has work to do and a reason
to hold back (asserted below): it removes at least 10 edges, and keeps at least one edge of tip shape (a tie in coverage).
"""
import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import oracle as O

import tips_cases as TC
import tips_ref as T

pytestmark = pytest.mark.gpu
CASES = TC.cases()
RANDOM = {21: 2, 55: 2}           # k -> config_id of synth.reads_mode_g


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def fill(ctx, k, counts):
    m = HipDNAMap(ctx, k, 2 * len(counts) + 64)
    lo, hi = dna.pack_many(list(counts))
    m.add_counts(lo, hi, np.array(list(counts.values()), np.int32))
    return m


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_graphs(ctx, case):
    m = fill(ctx, TC.K, case["counts"])
    g = buildGraph(TC.K, m)
    assert sorted(g.canonical()[1]) == sorted(case["edges"])
    nodes = g.counts()[0]
    assert g.clipTips(m, 0) == 0 and sorted(g.canonical()[1]) == sorted(case["edges"])       # max_len = 0 removes nothing
    removed = g.clipTips(m, case["max_len"])
    assert removed == len(case["removed"])
    assert sorted(g.canonical()[1]) == sorted(e for e in case["edges"] if e not in case["removed"])
    assert g.counts()[0] == nodes                                                            # nodes stay
    assert g.clipTips(m, case["max_len"]) == 0                                               # nothing left of tip shape but ties
    g.close(); m.close()


def tip_shaped(edges):
    """indices of the edges that are out-tips or in-tips by shape alone"""
    outd, ind = {}, {}
    for s, e, _q in edges:
        outd[s] = outd.get(s, 0) + 1
        ind[e] = ind.get(e, 0) + 1
    return {i for i, (s, e, _q) in enumerate(edges)
            if (outd.get(e, 0) == 0 and ind[e] == 1 and outd[s] >= 2) or (ind.get(s, 0) == 0 and outd[s] == 1 and ind[e] >= 2)}


def oracle_graph_edges(og):
    k = og.k
    e = og.edges()
    out = []
    for i in range(len(e["len"])):
        seq = synth.bases_to_str(e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        out.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k), dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k), seq))
    return out


@pytest.fixture(scope="module")
def random_case(ctx):
    """per k: the device's table and a function that builds a fresh graph of it, with the oracle's table and graph (computed once)"""
    made = {}

    def get(k):
        if k not in made:
            rec = synth.reads_mode_g(3000, 100, 2000, 0.01, config_id=RANDOM[k])
            ref = O.PMap(k, 1)
            occ = ref.count_reads(rec.tobytes(), 3000)
            ref.delete_lt(2)
            lo, hi, cnt = ref.export_sorted()
            counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
            m = HipDNAMap(ctx, k, occ)
            assert m.count_reads(rec.tobytes(), 3000) == occ
            m.deleteAll_lt(2)
            made[k] = (m, counts, sorted(oracle_graph_edges(O.Graph(ref))))
        return made[k]

    yield get
    for m, _c, _e in made.values():
        m.close()


@pytest.mark.parametrize("k", sorted(RANDOM))
def test_random_reads_against_the_oracle_and_the_restatement(ctx, random_case, k):
    m, counts, edges = random_case(k)
    g = buildGraph(k, m)
    assert sorted(g.canonical()[1]) == edges
    rm = T.tips(counts, edges, 2 * k)
    # the input is not degenerate: the rule has work to do, and a reason to hold back
    assert len(rm) >= 10
    assert tip_shaped(edges) - rm
    assert g.clipTips(m) == len(rm)                                      # max_len = None: 2k
    left = [e for i, e in enumerate(edges) if i not in rm]
    assert sorted(g.canonical()[1]) == left
    assert T.strand_closed(left)
    # a second round on the merged graph
    g.simplifyGraph()
    merged = sorted(g.canonical()[1])
    assert len(merged) < len(left) and T.strand_closed(merged)
    rm2 = T.tips(counts, merged, 2 * k)
    assert g.clipTips(m, 2 * k) == len(rm2)
    assert sorted(g.canonical()[1]) == [e for i, e in enumerate(merged) if i not in rm2]
    g.close()


def test_foreign_map_is_refused_and_the_graph_untouched(ctx, random_case):
    k = 21
    m, counts, edges = random_case(k)
    g = buildGraph(k, m)
    rec = synth.reads_mode_g(3000, 100, 2000, 0.01, config_id=RANDOM[k] + 100)     # another genome
    foreign = HipDNAMap(ctx, k, 1 << 16)
    foreign.count_reads(rec.tobytes(), 3000)
    fp, chk = g.idFingerprint(), g.checksum()
    with pytest.raises(L.GkError) as err:
        g.clipTips(foreign)
    assert err.value.code == L.GK_E_STATE
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)
    assert sorted(g.canonical()[1]) == edges
    assert g.clipTips(m, 0) == 0 and g.idFingerprint() == fp             # max_len = 0 removes nothing
    assert g.clipTips(m) == len(T.tips(counts, edges, 2 * k))            # and the handle works on
    foreign.close(); g.close()
