"""The three device-computed 64-bit values the suite compares tables and graphs by -- gk_map_verify's checksum (k_verify),
gk_graph_checksum (k_graph_checksum) and gk_graph_id_fingerprint (k_graph_id_fingerprint and its bounds term) -- against the plain
restatement of tests/checksum_ref.py.  Exact equality everywhere.  -m gpu.

Where the oracle can follow, the restatement is taken over the ORACLE's table or graph of the same reads (reads -> oracle ->
restatement against reads -> device -> kernel), and the device's content is compared with the oracle's beside it.  The device's own
exports enter only where the oracle cannot follow: ids (the fingerprint is always restated from nodesById / edgesById / idBounds,
whose k-mers and lengths are then checked against the content), node copies and span copies.  For k <= 31 the restatement takes
hi = 0 whatever the device exports.

tests/test_checksum_cpu.py asserts on the oracle alone what the inputs hold (which graphs removeBubbles + simplifyGraph changes,
the edge lengths mod 4, the long edges); each test here asserts the rest on its reference side.
"""
import json
import os
import random
import re
from contextlib import contextmanager

import numpy as np
import pytest

import checksum_ref as CS
import components_ref as CR
import small_grid_cases as S
from folded_cases import SEEDS, case as folded_case
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph, loadGraph
from genome_amd.partitioned import PartitionedDNAMap
from oracle import oracle as O
from oracle import pyref as R
from small_grid_cases import BLOCK
from test_fuzz_gpu import _oracle_graph
from test_pairs_gpu import make_pairs
from test_spans_gpu import graph_of, pieces, spans_of, strands
from test_variants_gpu import ctx, forced  # noqa: F401 (the module-scoped context fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 1 << 64
GRIDS = (1, 3)


@contextmanager
def capped(ctx, G):
    """forced(ctx, test_max_grid=G), and the switch's echo: launches inside the block were sized under the cap"""
    with forced(ctx, test_max_grid=G):
        before = ctx.grid_cap_uses()
        yield
        assert ctx.grid_cap_uses() > before, "no launch consulted test_max_grid"


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
TABLE_KS = (2, 5, 21, 31, 34, 47, 63, 64)


def max_count():
    """the largest count gk_map_add_counts admits: "Counts are int32" (include/genome_amd.h, the conventions at its top, and the
    int32_t array of the prototype)"""
    text = open(os.path.join(ROOT, "include", "genome_amd.h")).read()
    assert "Counts are int32" in text
    assert re.search(r"int gk_map_add_counts\(gk_map \*m, const uint64_t \*lo, const uint64_t \*hi, const int32_t \*counts, uint64_t n\);", text)
    return 2 ** 31 - 1


COUNTS = (1, 2, 255, 256, 65535, 65536)


def hand_table(k, n=1500, seed=0):
    """{k-mer: count}: n distinct random k-mers (fewer where 4^k is small), the counts 1, 2, 255, 256, 65 535, 65 536 and the
    largest int32 in turn"""
    rnd = random.Random(100 * k + seed)
    n = min(n, 4 ** k * 5 // 8)
    keys = set()
    while len(keys) < n:
        keys.add("".join(rnd.choice("AGCT") for _ in range(k)))
    counts = COUNTS + (max_count(),)
    return {s: counts[i % len(counts)] for i, s in enumerate(sorted(keys))}


def fill(ctx, k, table, hint, for_graph=False):
    return put(HipDNAMap(ctx, k, hint, for_graph=for_graph), table)


def put(m, table):
    lo, hi = dna.pack_many(list(table))
    m.add_counts(lo, hi, np.array(list(table.values()), np.int32))
    # the stored counts are the ones given, before anything is said about a checksum
    assert m.apply_batch((lo, hi)).tolist() == list(table.values())
    return m


def check_table(m, table):
    """(live, bad, sum, checksum) of the device against the dict"""
    assert m.verify_checksum() == (len(table), 0, sum(table.values()), CS.table_checksum_of(table))


def oracle_table(ref):
    lo, hi, c = ref.export_sorted()
    return {dna.unpack(int(a), int(b), ref.k): int(x) for a, b, x in zip(lo, hi, c)}


@pytest.mark.parametrize("for_graph", [False, True])
@pytest.mark.parametrize("k", TABLE_KS)
def test_table_states(ctx, k, for_graph):
    """hand_table(k) through add_counts: 1500 keys (10 at k = 2, 640 at k = 5) holding every count of COUNTS and 2^31 - 1, in a
    table that fits them and (the count table only, k >= 21) 3000 keys in a table made for 16, which has to grow; then
    deleteAll_lt(2), which leaves dead slots and the 16-byte layout at k <= 31; then clear().  Both maps of slot_ref.KS: 12-byte
    count slots / 24-byte / tagged, and gk_map_create_for_graph's 16-byte slots."""
    W = 1 if k <= 31 else 2
    for grow in ([False] if for_graph or k < 21 else [False, True]):
        table = hand_table(k, 3000 if grow else 1500)
        assert set(table.values()) == set(COUNTS) | {2 ** 31 - 1} and len(table) == min(3000 if grow else 1500, 4 ** k * 5 // 8)
        m = HipDNAMap(ctx, k, 16 if grow else 2 * len(table), for_graph=for_graph)
        slots0 = m.slots()
        put(m, table)
        assert m.stats()["slot_bytes"] == (24 if W == 2 else 16 if for_graph else 12)
        if grow:
            assert len(table) > slots0 and m.slots() > slots0 and m.stats()["grows"] > 0          # past the capacity hint
        check_table(m, table)
        m.deleteAll_lt(2)
        left = {s: c for s, c in table.items() if c >= 2}
        assert 0 < len(left) < len(table)
        assert m.stats()["slot_bytes"] == (24 if W == 2 else 16)
        check_table(m, left)
        m.clear()
        assert m.verify_checksum() == (0, 0, 0, 0)
        m.add_counts(*dna.pack_many(list(left)), np.array(list(left.values()), np.int32))     # ... and the table is usable again
        check_table(m, left)
        m.close()


def reads_for(k, seed=0):
    """150 reads of 100 bases from both strands of a 1200-base genome, 1 % substitutions"""
    rnd = random.Random(7 * k + seed)
    g = "".join(rnd.choice("AGCT") for _ in range(1200))
    out = []
    for _ in range(150):
        s = rnd.randrange(0, len(g) - 100)
        r = g[s:s + 100]
        if rnd.random() < 0.5:
            r = R.rev_comp(r)
        out.append("".join(c if rnd.random() >= 0.01 else rnd.choice([x for x in "AGCT" if x != c]) for c in r))
    return out


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k", TABLE_KS)
def test_table_counted_from_reads_against_the_oracles(ctx, k, path):
    """reads_for(k): a few thousand distinct k-mers (16 and 512 at k = 2 and 5), most seen several times, errors seen once; the
    oracle's table of the reads, and after delete_lt(2), restated"""
    reads = reads_for(k)
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, len(reads))
    want = oracle_table(ref)
    assert len(want) == ref.size() >= (10 if k == 2 else 500) and max(want.values()) > 2
    assert k < 21 or min(want.values()) == 1
    m = HipDNAMap(ctx, k, 256)
    m.set_insert_path(path)
    assert m.count_reads(binb, len(reads)) == occ
    st = m.stats()
    assert (st["partitioned_launches"] > 0) == (path == "partitioned"), st
    check_table(m, want)
    ref.delete_lt(2); m.deleteAll_lt(2)
    left = oracle_table(ref)
    assert k < 21 or 0 < len(left) < len(want)
    check_table(m, left)
    assert m.count_reads(binb, len(reads)) == occ                          # on top of the filtered table, dead slots under it
    for s, c in want.items():
        left[s] = left.get(s, 0) + c
    check_table(m, left)
    m.close(); ref.close()


@pytest.mark.parametrize("k", [21, 35, 64])
def test_partitions_add_up_to_the_oracles_table(ctx, k):
    """PartitionedDNAMap, P = 3, of reads_for(k): the partitions' checksums sum to the restatement over the oracle's WHOLE table,
    each partition's is the restatement over what it holds, and none is empty"""
    reads = reads_for(k, 1)
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 3)
    occ = ref.count_reads(binb, len(reads))
    want = oracle_table(ref)
    pm = PartitionedDNAMap(ctx, k, 3)
    assert pm.count_reads(binb, len(reads)) == occ
    assert pm.verify() == (len(want), 0, occ, CS.table_checksum_of(want))
    total, seen = 0, {}
    for part in pm.parts:
        lo, hi, c = part.items()
        mine = {dna.unpack(int(a), int(b), k): int(x) for a, b, x in zip(lo, hi, c)}
        assert mine and not set(mine) & set(seen)
        check_table(part, mine)
        seen.update(mine)
        total += part.verify_checksum()[3]
    assert seen == want and total % M == CS.table_checksum_of(want)
    pm.close(); ref.close()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("k", [31, 47])
def test_table_under_a_small_grid(ctx, k, G):
    """hand_table(k) in a table of more than 2 * G * BLOCK slots, not all of them a whole number of trips: k_verify's workgroups
    each take several trips through its loop"""
    table = hand_table(k)
    m = fill(ctx, k, table, 4 * len(table))
    assert m.slots() > 2 * G * BLOCK and len(table) > 2 * G * BLOCK // 2
    with capped(ctx, G):
        check_table(m, table)
        m.deleteAll_lt(256)
        left = {s: c for s, c in table.items() if c >= 256}
        assert m.slots() > 2 * G * BLOCK
        check_table(m, left)
    check_table(m, left)                                                   # the default grid, the same handle
    m.close()


def test_tables_that_differ_in_one_count_or_one_high_word(ctx):
    """k = 47, hand_table: one count raised by 1; one key whose HIGH word alone differs (bit 20 of hi, base 42)"""
    k = 47
    a = hand_table(k, 300)
    key = sorted(a)[17]
    b = dict(a); b[key] += 1
    lo, hi = dna.pack(key)
    other = dna.unpack(lo, hi ^ (1 << 20), k)
    assert other not in a and dna.pack(other)[0] == lo
    c = {(other if s == key else s): v for s, v in a.items()}
    got = []
    for t in (a, b, c):
        m = fill(ctx, k, t, 1024)
        check_table(m, t)
        got.append(m.verify_checksum())
        m.close()
    assert got[0][0] == got[1][0] == got[2][0] and got[0][2] + 1 == got[1][2] and got[0][2] == got[2][2]
    assert len({x[3] for x in got}) == 3
    # one key word: the same two at k = 31 (the count; the top used bit of lo)
    k = 31
    a = hand_table(k, 300)
    key = sorted(a)[17]
    b = dict(a); b[key] -= 1 if b[key] > 1 else -1
    lo, _ = dna.pack(key)
    other = dna.unpack(lo ^ (1 << 61), 0, k)
    assert other not in a
    c = {(other if s == key else s): v for s, v in a.items()}
    got = []
    for t in (a, b, c):
        m = fill(ctx, k, t, 1024)
        check_table(m, t)
        got.append(m.verify_checksum()[3])
        m.close()
    assert len(set(got)) == 3


# ---------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------
def by_id(g):
    """the device's live nodes (id, lo, hi) and live edges (id, start id, end id, first base code, length), and the id bounds"""
    nb, eb = g.idBounds()
    n, e = g.nodesById(np.arange(nb, dtype=np.uint32)), g.edgesById(np.arange(eb, dtype=np.uint32))
    nodes = [(int(i), int(n["lo"][i]), int(n["hi"][i])) for i in np.flatnonzero(n["alive"])]
    edges = [(int(i), int(e["start"][i]), int(e["end"][i]), int(e["first"][i]), int(e["len"][i])) for i in np.flatnonzero(e["alive"])]
    return nodes, edges, nb, eb


def check_graph(g, content=None):
    """the checksum pair against the restatement over `content` (the oracle's (nodes, edges); None: the oracle cannot follow, the
    device's canonical()), the fingerprint against the restatement over the device's ids, and the ids against the content
    -> (checksum pair, fingerprint, restated fingerprint)"""
    k = g.k
    got = g.canonical()
    if content is None:
        content = got
    nodes, edges = sorted(content[0]), sorted(content[1])
    assert (sorted(got[0]), sorted(got[1])) == (nodes, edges)
    assert g.counts() == (len(nodes), len(edges), sum(len(q) for _s, _t, q in edges))
    assert g.checksum() == CS.graph_checksum(nodes, edges)
    ns, es, nb, eb = by_id(g)
    want_fp = CS.id_fingerprint([(i, lo, hi if k >= 34 else 0) for i, lo, hi in ns], es, nb, eb)
    fp = g.idFingerprint()
    assert fp == want_fp
    # the ids name this content
    assert all(hi == 0 for _i, _lo, hi in ns) or k >= 34
    kmer = {i: dna.unpack(lo, hi, k) for i, lo, hi in ns}
    assert sorted(kmer.values()) == nodes and nb > max(kmer) and (not es or eb > max(x[0] for x in es))
    assert sorted((kmer[s], kmer[t], ln, dna.BASES[first]) for _e, s, t, first, ln in es) == sorted((s, t, len(q), q[0]) for s, t, q in edges)
    return g.checksum(), fp, want_fp


def check_loaded(g, tmp_path, content, name="g.gkg"):
    """save, load in a FRESH context, the same three values there"""
    p = tmp_path / name
    g.save(p)
    c2 = Context(0)
    h = loadGraph(c2, p)
    assert check_graph(h, content)[:2] == (g.checksum(), g.idFingerprint())
    h.close(); c2.close()


GRAPH_CASES = ["g_k11_p1", "g_k21_p3", "g_k31_p1", "g_k35_p2", "g_k63_p1", "folded_k64", "reads_k11", "reads_k35", "reads_k64",
               "planted_k31", "planted_k34"]
SIMPLIFY_CHANGES = {"folded_k64", "reads_k11", "reads_k35", "reads_k64", "planted_k31", "planted_k34"}
_REF = {}


def graph_input(name):
    """-> (k, what fills the table: ("reads", bin, n, rounds) or ("counts", dict))"""
    if name.startswith("g_k"):
        fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
        return fx["k"], ("reads", bytes.fromhex(fx["bin_hex"]), fx["nreads"], fx["rounds"])
    kind, k = name.split("_k")
    k = int(k)
    if kind == "planted":
        return k, ("counts", S.planted_case(k))
    if kind == "folded":
        c = folded_case(k, SEEDS[k], "noisy")
        return k, ("reads", dna.reads_to_bin(c.graph_reads), len(c.graph_reads), c.min_count)
    reads = S.reads_case(k)
    return k, ("reads", dna.reads_to_bin(reads), len(reads), 2)


def oracle_fill(k, src):
    ref = O.PMap(k, 1)
    if src[0] == "reads":
        ref.count_reads(src[1], src[2])
        ref.delete_lt(src[3])
    else:
        for key in src[1]:
            ref.update_inc(*dna.pack(key))
    return ref


def device_fill(ctx, k, src, hint=0):
    if src[0] == "reads":
        m = HipDNAMap(ctx, k, hint)
        m.count_reads(src[1], src[2])
        m.deleteAll_lt(src[3])
        return m
    m = HipDNAMap(ctx, k, hint or 2 * len(src[1]) + 64)
    lo, hi = dna.pack_many(list(src[1]))
    m.add_counts(lo, hi, np.array(list(src[1].values()), np.int32))
    return m


def victims_of(edges):
    """three edges of a sorted content list (all of them where there are fewer), by content"""
    n = len(edges)
    return [edges[i] for i in sorted({0, n // 2, n - 1})]


def graph_reference(name):
    """the oracle's content after every step of the flow, computed once: built; removeBubbles + simplifyGraph; retainLargest;
    three edges removed"""
    if name in _REF:
        return _REF[name]
    k, src = graph_input(name)
    ref = oracle_fill(k, src)
    og = O.Graph(ref)
    steps = {"built": _oracle_graph(og, k)}
    og.remove_bubbles(); og.simplify()
    steps["simplified"] = _oracle_graph(og, k)
    assert (steps["simplified"] != steps["built"]) == (name in SIMPLIFY_CHANGES)
    want = CR.retained(*steps["simplified"])
    comps = og.num_components()
    kept = og.retain_largest()
    steps["retained"] = _oracle_graph(og, k)
    assert (sorted(want[0]), sorted(want[1])) == (sorted(steps["retained"][0]), sorted(steps["retained"][1]))
    assert comps > 1 and 0 < kept == len(steps["retained"][0]) < len(steps["simplified"][0])          # sparse ids after it
    victims = victims_of(sorted(steps["retained"][1]))
    for s, _t, q in victims:
        assert og.remove_edge(*dna.pack(s), dna.BASES.index(q[0]))
    steps["removed"] = _oracle_graph(og, k)
    assert len(steps["removed"][1]) == len(steps["retained"][1]) - len(victims)
    og.close(); ref.close()
    # every state's three values differ from the state's before it (where the state differs): no step is checked in vain
    sums = {s: CS.graph_checksum(*c) for s, c in steps.items()}
    assert sums["retained"] != sums["simplified"] and sums["removed"][1] != sums["retained"][1]
    _REF[name] = dict(k=k, src=src, steps=steps, victims=victims, kept=kept, comps=comps)
    return _REF[name]


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_graph_states_against_the_oracles(ctx, tmp_path, name):
    """The five golden graphs (20 / 4 / 12 / 16 / 4 nodes), the noisy folded k = 64 graph (267 nodes, 223 edges), the reads of
    small_grid_cases at k = 11, 35, 64 (about 2000 nodes and 1900 to 2700 edges each) and its planted k-mer sets at k = 31 and 34
    (4682 nodes, 2530 edges, 2224 components).  Each: built; loaded from a save in a fresh context; after removeBubbles +
    simplifyGraph (merged edges and pool holes in all but the golden five, which it leaves alone: test_checksum_cpu.py);
    after retainLargest (sparse ids); after removeEdgesById of three edges (of the one or two there are, in the smallest golden
    graphs); loaded again.  Content from the oracle at every step."""
    F = graph_reference(name)
    k, steps = F["k"], F["steps"]
    m = device_fill(ctx, k, F["src"])
    g = buildGraph(k, m)
    seen = [check_graph(g, steps["built"])]
    check_loaded(g, tmp_path, steps["built"], "built.gkg")
    if name == "reads_k11":
        # k_graph_checksum and k_graph_id_fingerprint with one and with three workgroups: several trips each, a last one that
        # differs per workgroup, a last wave that is partly filled
        n, e = len(steps["built"][0]), len(steps["built"][1])
        assert n > 2 * 3 * BLOCK and e > 2 * 3 * BLOCK and n % 64 and e % 64
        for G in GRIDS:
            with capped(ctx, G):
                assert check_graph(g, steps["built"]) == seen[0]
    g.removeBubbles(); g.simplifyGraph()
    seen.append(check_graph(g, steps["simplified"]))
    if name in SIMPLIFY_CHANGES:
        nb, eb = g.idBounds()
        assert eb > g.counts()[1] and seen[1][0] != seen[0][0] and seen[1][1] != seen[0][1]       # dead ids under the live ones
    assert g.retainLargest() == (F["kept"], F["comps"])
    seen.append(check_graph(g, steps["retained"]))
    ids = [g.nodeId(s, q[0])[1] for s, _t, q in F["victims"]]
    assert None not in ids and len(set(ids)) == len(ids) == min(3, len(steps["retained"][1]))
    fp = g.idFingerprint()
    assert g.removeEdgesById(np.array(ids, np.uint32)) == len(ids)
    seen.append(check_graph(g, steps["removed"]))
    assert g.idFingerprint() != fp
    # four states, four fingerprints -- but for the golden five, whose second state is their first
    assert (seen[1] == seen[0]) == (name not in SIMPLIFY_CHANGES)
    assert len({s[1] for s in seen}) == (4 if name in SIMPLIFY_CHANGES else 3)
    check_loaded(g, tmp_path, steps["removed"], "removed.gkg")
    g.close(); m.close()


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("name", ["reads_k35", "reads_k64", "planted_k34"])
def test_wide_keys_under_a_small_grid(ctx, name, G):
    """the two-word graphs of small_grid_cases, built and merged, with every launch capped at G workgroups"""
    F = graph_reference(name)
    n, e = len(F["steps"]["built"][0]), len(F["steps"]["built"][1])
    assert n > 2 * G * BLOCK and e > 2 * G * BLOCK
    m = device_fill(ctx, F["k"], F["src"])
    with capped(ctx, G):
        g = buildGraph(F["k"], m)
        a = check_graph(g, F["steps"]["built"])
        g.removeBubbles(); g.simplifyGraph()
        b = check_graph(g, F["steps"]["simplified"])
    assert check_graph(g, F["steps"]["simplified"])[:2] == b[:2] and a[0] != b[0]          # the default grid, the same handle
    g.close(); m.close()


@pytest.mark.parametrize("k", [21, 35])
def test_after_a_node_split(ctx, tmp_path, k):
    """the node split of test_graph_file_gpu.test_graph_states_round_trip (walkPairs + splitBySupport at cutoff 3 over
    make_pairs(seed, k)): nodes that share a k-mer, which the oracle's content export cannot tell apart by id.  Content from the
    device's canonical(); the copies are asserted there."""
    seed, rng = {21: (1, (60, 95)), 35: (4, (50, 80))}[k]
    reads = make_pairs(seed, k)
    binb = dna.reads_to_bin(reads)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(k, m)
    before = check_graph(g)
    vm, sup = g.getGraphMap(), Support(ctx)
    g.walkPairs(vm, sup, binb, len(reads) // 2, *rng)
    assert check_graph(g) == before                                        # the walk edits nothing
    _rm, nn = g.splitBySupport(sup, 3)
    assert nn > 0
    nodes = g.canonical()[0]
    assert len(set(nodes)) < len(nodes)                                    # copies
    after = check_graph(g)
    assert after[0] != before[0] and after[1] != before[1]
    check_loaded(g, tmp_path, None)
    g.simplifyGraph()
    assert check_graph(g)[1] != after[1]
    check_loaded(g, tmp_path, None, "simplified.gkg")
    sup.close(); vm.close(); g.close(); m.close()


@pytest.mark.parametrize("k", [11, 31, 35, 64])
def test_after_a_span_split(ctx, tmp_path, k):
    """A R B R C of tests/test_spans_gpu.py, |R| = k + 60: splitEdgesBySpans copies the repeat's edge, the copies share its pool
    bytes (content from the device); the simplifyGraph after it leaves the genome whole on both strands, which is restated from
    the genome itself"""
    r = k + 60
    A, Rp, B, C_ = pieces(k, k, [300, r, 280, 310], lambda A, Rp, B, C_: [A + Rp + B + Rp + C_])
    gen = A + Rp + B + Rp + C_
    g, reads = graph_of(ctx, k, [gen])
    before = check_graph(g)
    sp, st = spans_of(g, reads)
    assert st["spans"] > 0
    est = g.splitEdgesBySpans(sp, 3)
    assert (est["new_edges"], est["new_nodes"]) == (2, 4)
    nodes, edges = g.canonical()
    assert len(set(nodes)) < len(nodes) and len({q for _s, _t, q in edges}) < len(edges)           # node copies, edge copies
    split = check_graph(g)
    assert split[0] != before[0] and split[1] != before[1]
    check_loaded(g, tmp_path, None, "split.gkg")
    g.simplifyGraph()
    whole = [(x[:k], x[-k:], x[k:]) for x in strands([gen])]
    assert len(gen) - k > 64
    merged = check_graph(g, ([x[:k] for x in strands([gen])] + [x[-k:] for x in strands([gen])], whole))
    assert merged[1] != split[1]
    check_loaded(g, tmp_path, None, "merged.gkg")
    sp.close(); g.close()


@pytest.mark.parametrize("k", [21, 47])
def test_a_snp_in_the_last_partial_byte_of_a_long_edge(ctx, k):
    """two genomes of k + 211 bases that differ in their last base but one: each is one edge of 211 bases per strand (53 bytes, the
    last holds three bases), and on the forward strand the SNP lies in that last, partly filled byte"""
    rnd = random.Random(k)
    a = "".join(rnd.choice("AGCT") for _ in range(k + 211))
    p = len(a) - 2
    b = a[:p] + "AGCT"[("AGCT".index(a[p]) + 1) % 4] + a[p + 1:]
    got = []
    for gen in (a, b):
        reads = [gen[i:i + 100] for i in range(0, len(gen) - 99)]
        binb = dna.reads_to_bin(reads)
        ref = O.PMap(k, 1)
        ref.count_reads(binb, len(reads))
        og = O.Graph(ref)
        content = _oracle_graph(og, k)
        fwd = [e for e in content[1] if e[0] == gen[:k]]
        assert len(content[1]) == 2 and len(fwd) == 1 and fwd[0][2] == gen[k:]
        ln = len(gen) - k
        assert ln > 64 and ln % 4 >= 2 and p - k >= ln - ln % 4                             # the SNP's base is in the last byte
        m = HipDNAMap(ctx, k)
        m.count_reads(binb, len(reads))
        g = buildGraph(k, m)
        got.append(check_graph(g, content))
        g.close(); m.close(); og.close(); ref.close()
    assert got[0][0][1] != got[1][0][1]
    assert CS.pack_bases(a[k:])[:-1] == CS.pack_bases(b[k:])[:-1] and CS.pack_bases(a[k:])[-1] != CS.pack_bases(b[k:])[-1]


@pytest.mark.parametrize("name", ["g_k35_p2", "reads_k11"])
def test_two_builds_of_one_table_at_different_capacities(ctx, name):
    """the oracle's filtered table through add_counts into a table made for its keys and into one made for 2^17: the table and
    content checksums agree; the fingerprints agree exactly if the restatements over each build's own ids do"""
    F = graph_reference(name)
    ref = oracle_fill(F["k"], F["src"])
    table = oracle_table(ref)
    ref.close()
    out = []
    for hint in (len(table), 1 << 17):
        m = fill(ctx, F["k"], table, hint)
        check_table(m, table)
        out.append((m.slots(), m.verify_checksum()))
        g = buildGraph(F["k"], m)
        out[-1] += check_graph(g, F["steps"]["built"])
        g.close(); m.close()
    (s1, t1, c1, f1, w1), (s2, t2, c2, f2, w2) = out
    assert s2 > s1 and t1 == t2 and c1 == c2
    assert (f1 == f2) == (w1 == w2)
