"""gk_graph_edge_coverage on the device against its restatement (tests/tips_ref.py), exact on all four numbers (-m gpu).

The tables are filled with known counts through gk_map_add_counts (no reads): the k-mers of a random 400-base sequence at count 10
and a 12-base branch at count 2, for every key width and slot layout; at k = 31 and 47 also an edge of thousands of windows
(the long form of the kernel, with position-dependent counts so that a skipped, repeated or shifted window shows), a count
table in the 12-byte layout that the graph was not built from, a table of verbatim non-canonical keys, graphs after
simplifyGraph and after a node split's edits, missing k-mers, dead and foreign ids, and a table of another k.
"""
import ctypes as C
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import pyref as R

import tips_ref as T

pytestmark = pytest.mark.gpu
KS = [5, 21, 31, 34, 47, 63, 64]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def branch_counts(k, seed=1):
    """canonical k-mer -> count: a random 400-base sequence at 10 and a branch of 12 windows leaving it at 2"""
    rnd = random.Random(1000 * seed + k)
    s = rand_seq(rnd, 400)
    j = 200
    piece = s[j - k + 1:j] + [b for b in "AGCT" if b != s[j]][0] + rand_seq(rnd, 11)
    counts = {}
    for i in range(len(s) - k + 1):
        counts[R.canon(s[i:i + k])] = 10
    for i in range(len(piece) - k + 1):
        key = R.canon(piece[i:i + k])
        counts[key] = counts.get(key, 0) + 2
    return counts


def fill(ctx, k, counts):
    """a table holding exactly `counts` (stored k-mer string -> count), keys verbatim"""
    m = HipDNAMap(ctx, k, 2 * len(counts) + 64)
    lo, hi = dna.pack_many(list(counts))
    m.add_counts(lo, hi, np.array(list(counts.values()), np.int32))
    assert m.size() == len(counts)
    return m


def edges_with_ids(g):
    """canonical() edges and, for each, its id: an edge is named by its start k-mer and first base"""
    ne = g.idBounds()[1]
    ids = np.arange(ne, dtype=np.uint32)
    e = g.edgesById(ids)
    nodes = g.nodesById(e["start"][e["alive"]])
    by_start = {}
    for i, lo, hi in zip(ids[e["alive"]], nodes["lo"], nodes["hi"]):
        key = (dna.unpack(int(lo), int(hi), g.k), dna.BASES[int(e["first"][i])])
        assert key not in by_start
        by_start[key] = int(i)
    edges = g.canonical()[1]
    assert len(edges) == len(by_start)
    return edges, [by_start[(s, q[0])] for s, _e, q in edges]


def check(g, m, counts):
    """edgeCoverage of every live edge (asked by id, in canonical order) == the restatement; -> (edges, ids, coverage)"""
    edges, ids = edges_with_ids(g)
    want, missing = T.coverage(counts, edges)
    got = g.edgeCoverage(m, ids)
    rows = list(zip(got["kmers"].tolist(), got["sum"].tolist(), got["min"].tolist(), got["max"].tolist()))
    assert rows == want
    assert got["missing"] == missing
    return edges, ids, want


@pytest.mark.parametrize("k", KS)
def test_branch_graph_every_key_width(ctx, k):
    counts = branch_counts(k)
    m = fill(ctx, k, counts)
    g = buildGraph(k, m)
    fp, chk = g.idFingerprint(), g.checksum()
    edges, ids, want = check(g, m, counts)
    assert len(edges) >= 6 and any(r[2] == 2 for r in want) and any(r[2] == 10 for r in want)
    # the default: every id below the bound, dead ones included (none yet); twins read the same numbers
    allc = g.edgeCoverage(m)
    assert len(allc["ids"]) == g.idBounds()[1] and allc["missing"] == 0
    by_edge = dict(zip(edges, want))
    for s, e, q in edges:
        rp = R.rev_comp(s + q)
        assert by_edge[(rp[:k], rp[len(q):], rp[k:])] == by_edge[(s, e, q)]
    assert (g.idFingerprint(), g.checksum()) == (fp, chk)                # stateless: the graph is as it was
    g.close(); m.close()


def long_counts(k, n=6000):
    """an error-free sequence of n bases: one edge (and its twin) of n - k windows; counts depend on the position"""
    rnd = random.Random(77 + k)
    s = rand_seq(rnd, n)
    counts = {}
    for i in range(n - k + 1):
        counts[R.canon(s[i:i + k])] = 3 + (i * 7919) % 97
    assert len(counts) == n - k + 1
    return counts


@pytest.mark.parametrize("k", [31, 47])
def test_edge_of_thousands_of_windows(ctx, k):
    """6000 - k + 1 windows: more than one workgroup pass of 256 runs of 16, the last pass partial, the last run cut short"""
    counts = long_counts(k)
    m = fill(ctx, k, counts)
    g = buildGraph(k, m)
    edges, ids, want = check(g, m, counts)
    assert len(edges) == 2 and want[0][0] == 6000 - k + 1 and want[0][0] % 16 != 0 and want[0][0] > 4096
    assert want[0][2] == 3 and want[0][3] == 99
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_other_tables_of_the_same_kmers(ctx, k):
    """The graph is built from one table; coverage is asked of others: an unfiltered table counted from reads in the layout
    counting leaves (12-byte slots at k = 31), and one filled with verbatim keys in the other orientation (some in both)."""
    counts = branch_counts(k)
    built_from = fill(ctx, k, counts)
    g = buildGraph(k, built_from)
    # reads: every window of the graph's k-mers is in them, with multiplicities of their own
    rnd = random.Random(k)
    keys = list(counts)
    reads = [s if rnd.random() < 0.5 else R.rev_comp(s) for s in keys for _ in range(rnd.randint(1, 4))]
    read_counts = {}
    for s in reads:
        read_counts[R.canon(s)] = read_counts.get(R.canon(s), 0) + 1
    m = HipDNAMap(ctx, k, 0)
    m.set_insert_path("partitioned")
    assert m.count_reads(dna.reads_to_bin(reads), len(reads)) == len(reads)
    st = m.stats()
    assert st["slot_bytes"] == (12 if k <= 31 else 24)
    if st["retries_direct"] == 0:
        assert st["last_slot"] == ("count12" if k <= 31 else "slot24")
    check(g, m, read_counts)
    m.close()
    # verbatim keys: the reverse complement of every canonical key, and for every 5th k-mer the canonical one too
    items = [(R.rev_comp(s), c) for s, c in counts.items()] + [(s, 7) for s in keys[::5]]
    dirty = HipDNAMap(ctx, k, 4 * len(items))
    lo, hi = dna.pack_many([s for s, _ in items])
    dirty.add_counts(lo, hi, np.array([c for _, c in items], np.int32))
    assert dirty.stats()["noncanonical_keys"] is True and dirty.size() == len(items)
    check(g, dirty, T.canonical_counts(items))
    dirty.close(); g.close(); built_from.close()


@pytest.mark.parametrize("k", [31, 47])
def test_after_simplify_and_after_point_edits(ctx, k):
    """merged edges (simplifyGraph) and a node copy (addNode + replaceEnd, what a node split does): the windows are the same"""
    rnd = random.Random(5 * k)
    counts = {key: 1 + rnd.randrange(40) for key in branch_counts(k)}
    m = fill(ctx, k, counts)
    g = buildGraph(k, m)
    before = g.counts()[1]
    # drop the branch on both strands, so that simplifyGraph has something to merge
    edges, ids, _ = check(g, m, counts)
    arm = [i for (s, e, q), i in zip(edges, ids) if len(q) == 12]
    assert len(arm) == 2 and g.removeEdgesById(arm) == 2
    g.simplifyGraph()
    assert g.counts()[1] < before - 2
    edges, ids, want = check(g, m, counts)
    dead = g.edgeCoverage(m, arm)
    assert not dead["kmers"].any() and not dead["sum"].any() and not dead["max"].any() and dead["missing"] == 0
    # a copy of an edge's end node takes the edge over
    s, e, q = edges[0]
    copy = g.addNode(e)
    g.replaceEnd(ids[0], copy)
    edges2, ids2, want2 = check(g, m, counts)
    assert edges2 == edges and want2 == want
    g.close(); m.close()


@pytest.mark.parametrize("k", [31, 47])
def test_missing_kmers_dead_ids_and_errors(ctx, k):
    counts = long_counts(k, 1500)
    m = fill(ctx, k, counts)
    g = buildGraph(k, m)
    edges, ids, want = check(g, m, counts)
    s, e, q = edges[0]
    path = s + q
    gone = [R.canon(path[d:d + k]) for d in (1, 700, len(q) - 1)]        # inside the edge, not its end nodes
    fewer = {key: c for key, c in counts.items() if key not in gone}
    lacking = fill(ctx, k, fewer)
    got = g.edgeCoverage(lacking, [ids[0]])
    assert got["missing"] == 3 and got["min"][0] == 0
    assert got["kmers"][0] == want[0][0] and got["sum"][0] == want[0][1] - sum(counts[x] for x in gone)
    check(g, lacking, fewer)                                             # both strands: 6 missing, as the restatement says
    # an id asked twice answers twice; a dead and an out-of-range id read zeros
    ne = g.idBounds()[1]
    assert g.removeEdgesById([ids[1]]) == 1
    got = g.edgeCoverage(m, [ids[0], ids[1], ne, 0xfffffffe, ids[0]])
    assert got["kmers"].tolist() == [want[0][0], 0, 0, 0, want[0][0]] and got["sum"].tolist() == [want[0][1], 0, 0, 0, want[0][1]]
    assert got["min"].tolist() == [want[0][2], 0, 0, 0, want[0][2]] and got["max"].tolist() == [want[0][3], 0, 0, 0, want[0][3]]
    assert g.edgeCoverage(m, [])["missing"] == 0
    # another k, a NULL handle
    other = HipDNAMap(ctx, k - 2, 64)
    with pytest.raises(L.GkError) as err:
        g.edgeCoverage(other)
    assert err.value.code == L.GK_E_INVALID
    with pytest.raises(L.GkError) as err:
        g.clipTips(other)
    assert err.value.code == L.GK_E_INVALID
    n = C.c_uint64()
    assert L.lib().gk_graph_edge_coverage(g.h, None, None, 0, None, None, None, None, C.byref(n)) == L.GK_E_INVALID
    assert L.lib().gk_graph_edge_coverage(None, m.h, None, 0, None, None, None, None, None) == L.GK_E_INVALID
    # any output may be NULL
    one = np.array([ids[0]], np.uint32)
    total = np.zeros(1, np.uint64)
    L.check(L.lib().gk_graph_edge_coverage(g.h, m.h, L.ptr(one, C.c_uint32), 1, None, L.ptr(total, C.c_uint64), None, None, None), ctx.h)
    assert int(total[0]) == want[0][1]
    other.close(); lacking.close(); g.close(); m.close()
