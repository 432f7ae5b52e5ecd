"""gk_graph_edge_distance on the device against its restatement (tests/bubbles_ref.py) (-m gpu): graphs of planted bubbles at
k = 11 and k = 35 (tests/bubbles_planted.py: distance_plan), every ordered pair of their edges, parallel or not, at
max_diff = 0, 1, 3, 31 — and the ids the rule names: the same edge twice, a dead one, one beyond the bound, none at all, and a
max_diff the band of one wave cannot hold.

The lengths 1..5, 31..33, 63..65 and about 200 (the byte, the 32-base chunk and the wave's 64 lanes, and many chunks) are
asserted to be among the edges compared, and so are, per max_diff, a pair at exactly that distance and one at one more, and
lengths that differ by exactly max_diff and by one more.
"""
import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

import bubbles_planted as P
import bubbles_ref as B

pytestmark = pytest.mark.gpu
DIFFS = (0, 1, 3, 31)
INVALID = 0xffffffff


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planted(ctx):
    """per k: the graph, the ids and sequences of its edges, and the Levenshtein distance of every unordered pair whose lengths
    are within 31 of each other (computed once)"""
    made = {}

    def get(k):
        if k not in made:
            _g, counts = P.planted(k, P.distance_plan(k), seed=1)
            m = HipDNAMap(ctx, k, 2 * len(counts) + 64)
            lo, hi = dna.pack_many(list(counts))
            m.add_counts(lo, hi, np.array(list(counts.values()), np.int32))
            g = buildGraph(k, m)
            edges = g.canonical()[1]
            ids = np.array([g.nodeId(s, q[0])[1] for s, _e, q in edges], np.uint32)
            assert len(set(ids.tolist())) == len(edges)
            seqs = [q for _s, _e, q in edges]
            lev = {}
            for i in range(len(seqs)):
                js = [j for j in range(i + 1, len(seqs)) if abs(len(seqs[i]) - len(seqs[j])) <= max(DIFFS)]
                lev.update(zip(((i, j) for j in js), B.levenshtein_many(seqs[i], [seqs[j] for j in js])))
            made[k] = (m, g, ids, seqs, lev)
        return made[k]

    yield get
    for m, g, *_ in made.values():
        g.close(); m.close()


@pytest.mark.parametrize("k", [11, 35])
def test_planted_lengths_and_edits_are_among_the_edges(planted, k):
    _m, _g, ids, seqs, lev = planted(k)
    assert 100 <= len(ids) <= 500
    lens = {len(q) for q in seqs}
    assert {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65} <= lens and any(195 <= n <= 205 for n in lens), sorted(lens)
    gaps = {abs(len(seqs[i]) - len(seqs[j])) for i, j in lev}
    for d in DIFFS:
        assert d in gaps and any(abs(len(a) - len(b)) == d + 1 for a in seqs for b in seqs)
        assert d == 0 or (d in lev.values() and d + 1 in lev.values())
    # a pair that differs in its last base only, one that is the other without its last base, one with a base more after the first
    pairs = [(seqs[i], seqs[j]) for (i, j), n in lev.items() if n <= 2]
    assert any(len(a) == len(b) and a[1:-1] == b[1:-1] and a[-1] != b[-1] for a, b in pairs)
    assert any(abs(len(a) - len(b)) == 1 and min(a, b, key=len)[1:] == max(a, b, key=len)[1:-1] for a, b in pairs)
    assert any(abs(len(a) - len(b)) == 1 and min(a, b, key=len)[1:] == max(a, b, key=len)[2:] for a, b in pairs)


@pytest.mark.parametrize("max_diff", DIFFS)
@pytest.mark.parametrize("k", [11, 35])
def test_every_ordered_pair_against_the_restatement(planted, k, max_diff):
    _m, g, ids, seqs, lev = planted(k)
    n = len(ids)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    gap = np.abs(np.array([len(q) for q in seqs])[i] - np.array([len(q) for q in seqs])[j])
    full = np.array([0 if a == b else lev.get((min(a, b), max(a, b)), max(DIFFS) + 1) for a, b in zip(i.tolist(), j.tolist())])
    want = np.where(gap > max_diff, max_diff + 1, np.minimum(full, max_diff + 1)).astype(np.uint32)
    got = g.edgeDistance(ids[i], ids[j], max_diff)
    assert got.dtype == np.uint32
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(seqs[i[b]], seqs[j[b]], int(got[b]), int(want[b])) for b in bad[:5]]
    # the array is the restatement's function, spot-checked where it decides
    for b in np.nonzero(gap <= max_diff)[0][::97]:
        assert want[b] == B.distance(seqs[i[b]], seqs[j[b]], max_diff)


def test_ids_the_rule_names(planted):
    _m, g, ids, seqs, _lev = planted(11)
    fp, chk = g.idFingerprint(), g.checksum()
    assert g.edgeDistance([], [], 3).shape == (0,)                                       # n = 0
    assert g.edgeDistance(ids, ids, 0).tolist() == [0] * len(ids)                        # e == f
    bound = g.idBounds()[1]
    got = g.edgeDistance([ids[0], bound, ids[1], INVALID], [bound, ids[0], bound + 7, ids[2]], 31)
    assert got.tolist() == [INVALID] * 4                                                 # an id beyond the bound, on either side
    with pytest.raises(L.GkError) as err:
        g.edgeDistance(ids[:2], ids[:2], 32)
    assert err.value.code == L.GK_E_INVALID
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)                                # the graph is not changed
    # a dead id: its own graph, so that the module's one stays whole
    m = planted(11)[0]
    h = buildGraph(11, m)
    edges = h.canonical()[1]
    hid = np.array([h.nodeId(s, q[0])[1] for s, _e, q in edges[:3]], np.uint32)
    assert h.removeEdgesById(hid[:1]) == 1
    got = h.edgeDistance([hid[0], hid[1], hid[0], hid[1]], [hid[1], hid[0], hid[0], hid[2]], 3)
    assert got.tolist() == [INVALID, INVALID, INVALID, B.distance(edges[1][2], edges[2][2], 3)]
    h.close()
