"""gk_graph_pop_bubbles on the device against its restatement (tests/bubbles_ref.py) (-m gpu): the hand-written graphs of
tests/bubbles_cases.py built on the device from their counts; a genome with a planted second haplotype per k in {21, 55}
(tests/bubbles_planted.py: haplotype_case); and 3000 reads of 100 bases over a 2000-base genome at k = 21, k-mers seen once
dropped, where the restatement reads the oracle's table and graph and the rounds clip -> pop -> simplify are followed one by one.

The inputs were chosen on the CPU, with the oracle and the restatement alone, so that the rule has work to do and a reason to
hold back; what that means per input is asserted below.
"""
import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import oracle as O

import bubbles_cases as BC
import bubbles_planted as P
import bubbles_ref as B
import tips_ref as T

pytestmark = pytest.mark.gpu
CASES = BC.cases()
ERRS = (0.02, 0.01)               # of the read case: config_id = 3 of synth.reads_mode_g


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


def oracle_graph_edges(og):
    k = og.k
    e = og.edges()
    out = []
    for i in range(len(e["len"])):
        seq = synth.bases_to_str(e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        out.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k), dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k), seq))
    return out


def oracle_edges_of(counts, k):
    ref = O.PMap(k, 1)
    for key in counts:
        ref.update_inc(*dna.pack(key))
    return sorted(oracle_graph_edges(O.Graph(ref)))


def pair_facts(counts, edges, max_len, max_diff):
    """of the parallel pairs within max_len: those tied in coverage, those compared and too far apart, those of unequal lengths"""
    pairs = B.parallel_pairs(edges, max_len)
    cand = sorted({i for p in pairs for i in p})
    cov = dict(zip(cand, T.coverage(counts, [edges[i] for i in cand])[0]))
    tied = [(i, j) for i, j in pairs if not T._weaker(cov[i], cov[j]) and not T._weaker(cov[j], cov[i])]
    far = [(i, j) for i, j in pairs if abs(len(edges[i][2]) - len(edges[j][2])) <= max_diff and B.levenshtein(edges[i][2], edges[j][2]) > max_diff]
    uneven = [(i, j) for i, j in pairs if len(edges[i][2]) != len(edges[j][2])]
    return pairs, tied, far, uneven


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_graphs(ctx, case):
    m = fill(ctx, BC.K, case["counts"])
    g = buildGraph(BC.K, m)
    assert sorted(g.canonical()[1]) == sorted(case["edges"])
    nodes = g.counts()[0]
    fp = g.idFingerprint()
    assert g.popBubbles(m, 0, case["max_diff"]) == (0, 0) and g.idFingerprint() == fp                       # max_len = 0 removes nothing
    assert g.popBubbles(m, case["max_len"], 0) == (0, case["pairs_at_0"]) and g.idFingerprint() == fp       # nor does max_diff = 0
    assert g.popBubbles(m, case["max_len"], case["max_diff"]) == (len(case["removed"]), case["pairs"])
    left = sorted(e for e in case["edges"] if e not in case["removed"])
    assert sorted(g.canonical()[1]) == left and all(e in left for e in case["keep"])
    assert g.counts()[0] == nodes                                                                           # nodes stay
    assert g.popBubbles(m, case["max_len"], case["max_diff"])[0] == 0                                       # a second round removes nothing
    assert sorted(g.canonical()[1]) == left
    g.close(); m.close()


@pytest.mark.parametrize("k", [21, 55])
def test_planted_second_haplotype(ctx, k):
    _g, counts = P.haplotype_case(k, seed=k)
    edges = oracle_edges_of(counts, k)
    rm, compared = B.pop(counts, edges, 2 * k, 3)
    pairs, tied, far, uneven = pair_facts(counts, edges, 2 * k, 3)
    # the input is not degenerate: the rule has work to do, and reasons to hold back
    assert len(rm) >= 10
    assert tied and not any(i in rm or j in rm for i, j in tied)                 # a tie kept
    assert far and any(i not in rm and j not in rm for i, j in far)              # a pair kept for its distance
    assert any(i in rm or j in rm for i, j in uneven)                            # a removed pair of unequal lengths
    assert compared == len(pairs)
    m = fill(ctx, k, counts)
    g = buildGraph(k, m)
    assert sorted(g.canonical()[1]) == edges
    nodes = g.counts()[0]
    assert g.popBubbles(m) == (len(rm), compared)                                # max_len = None: 2k, max_diff = None: 3
    left = [e for i, e in enumerate(edges) if i not in rm]
    assert sorted(g.canonical()[1]) == left and B.strand_closed(left) and g.counts()[0] == nodes
    assert g.popBubbles(m) == (0, B.pop(counts, left, 2 * k, 3)[1])
    # max_diff = 4 takes the four-SNP branches too
    rm4, compared4 = B.pop(counts, left, 2 * k, 4)
    assert rm4 and g.popBubbles(m, max_diff=4) == (len(rm4), compared4)
    assert sorted(g.canonical()[1]) == [e for i, e in enumerate(left) if i not in rm4]
    g.close(); m.close()


@pytest.fixture(scope="module")
def read_case(ctx):
    """per err: the device's table, its contents, the oracle's table and the edges of the oracle's graph (computed once)"""
    made = {}

    def get(err):
        if err not in made:
            k = 21
            rec = synth.reads_mode_g(3000, 100, 2000, err, config_id=3)
            ref = O.PMap(k, 1)
            occ = ref.count_reads(rec.tobytes(), 3000)
            ref.delete_lt(2)
            lo, hi, cnt = ref.export_sorted()
            counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
            m = HipDNAMap(ctx, k, occ)
            assert m.count_reads(rec.tobytes(), 3000) == occ
            m.deleteAll_lt(2)
            made[err] = (m, counts, ref, sorted(oracle_graph_edges(O.Graph(ref))))
        return made[err]

    yield get
    for m, *_ in made.values():
        m.close()


@pytest.mark.parametrize("err", ERRS)
def test_reads_through_the_whole_path(ctx, read_case, err):
    k = 21
    m, counts, _ref, edges = read_case(err)
    g = buildGraph(k, m)
    assert sorted(g.canonical()[1]) == edges
    # the raw graph: a few SNP bubbles (22 against 22 bases, one edit apart)
    rm, compared = B.pop(counts, edges, 2 * k, 3)
    pairs, tied, _far, _uneven = pair_facts(counts, edges, 2 * k, 3)
    assert len(rm) >= 2 and compared == len(pairs) >= 2
    if err == 0.01:
        assert tied and not any(i in rm or j in rm for i, j in tied)             # a tied pair survives
    h = buildGraph(k, m)
    assert h.popBubbles(m) == (len(rm), compared)
    assert sorted(h.canonical()[1]) == [e for i, e in enumerate(edges) if i not in rm]
    h.close()
    if err != 0.01:                                                              # (the rounds on the smaller of the two graphs)
        g.close()
        return
    # clip -> pop -> simplify, round by round, as graph_builder --clip-tips --pop-bubbles does
    rounds = 0
    while rounds < 8:
        rounds += 1
        tips = T.tips(counts, edges, 2 * k)
        assert g.clipTips(m) == len(tips)
        edges = [e for i, e in enumerate(edges) if i not in tips]
        rm, compared = B.pop(counts, edges, 2 * k, 3)
        assert g.popBubbles(m) == (len(rm), compared)
        edges = [e for i, e in enumerate(edges) if i not in rm]
        assert sorted(g.canonical()[1]) == edges and B.strand_closed(edges)
        if not tips and not rm:
            break
        g.simplifyGraph()
        edges = sorted(g.canonical()[1])
        assert B.strand_closed(edges)
    assert rounds >= 2
    g.close()


def test_foreign_map_is_refused_and_the_graph_untouched(ctx, read_case):
    k = 21
    m, counts, _ref, edges = read_case(ERRS[0])
    g = buildGraph(k, m)
    rec = synth.reads_mode_g(3000, 100, 2000, 0.01, config_id=103)               # another genome
    foreign = HipDNAMap(ctx, k, 1 << 16)
    foreign.count_reads(rec.tobytes(), 3000)
    fp, chk = g.idFingerprint(), g.checksum()
    with pytest.raises(L.GkError) as err:
        g.popBubbles(foreign)
    assert err.value.code == L.GK_E_STATE
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)
    assert sorted(g.canonical()[1]) == edges
    wrong_k = HipDNAMap(ctx, 23, 1 << 10)
    for bad in (lambda: g.popBubbles(wrong_k), lambda: g.popBubbles(m, max_diff=32)):
        with pytest.raises(L.GkError) as err:
            bad()
        assert err.value.code == L.GK_E_INVALID
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)
    assert g.popBubbles(m) == (len(B.pop(counts, edges, 2 * k, 3)[0]), B.pop(counts, edges, 2 * k, 3)[1])      # and the handle works on
    wrong_k.close(); foreign.close(); g.close()


def test_remove_bubbles_is_still_the_references_rule(ctx, read_case):
    k = 21
    m, _counts, ref, edges = read_case(ERRS[0])
    g = buildGraph(k, m)
    og = O.Graph(ref)
    og.remove_bubbles()
    want = sorted(oracle_graph_edges(og))
    assert len(want) < len(edges)                                                # it had something to remove
    g.removeBubbles()
    assert sorted(g.canonical()[1]) == want
    g.close()
