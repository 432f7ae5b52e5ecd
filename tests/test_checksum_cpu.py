"""tests/checksum_ref.py, the plain restatement of gk_map_verify's checksum, gk_graph_checksum and gk_graph_id_fingerprint, held
to values worked out by hand, to its own promises (every field enters, order does not) and to the oracle's tables and graphs of
the golden inputs.  No device: tests/test_checksum_gpu.py holds the kernels to the restatement, and tests/test_graph_file_cpu.py
holds the restatement to the bytes of the committed graph files.

What the oracle says about the inputs the GPU tests take (measured here, asserted below):
  * the five golden inputs: delete_lt(rounds) drops most of each table (605 -> 238, 1107 -> 264, 1847 -> 319, 1704 -> 287,
    1317 -> 264 keys) and with it most of the graph (164 nodes -> 20, 242 -> 4, 308 -> 12, 288 -> 16, 150 -> 4): all three
    restated values change.  But the graph of each FILTERED table is a fixed point of removeBubbles + simplifyGraph: the oracle's
    build already emits maximal unitigs and these inputs hold no bubble.  On them "after simplify" can only show that nothing
    changes, and that is what is asserted, as a fact about the inputs.
  * where simplify does work: the golden SNP inputs (snp_k11_p2: 16 nodes, 20 edges -> 4, 2; snp_k35_p1: 12, 14 -> 4, 2), the
    reads of small_grid_cases (k = 11: 2741 edges -> 1389) and the folded k = 64 graph.  These are what the GPU tests take for the
    state "merged edges, holes in the pool", and the restatement changes there.
  * edge lengths after removeBubbles + simplifyGraph: g_k35_p2 alone holds len % 4 = 0, 1, 2 and 3 and six edges longer than 64
    bases; every golden graph holds an edge longer than 64.
"""
import json
import os
import random

import pytest

import checksum_ref as CS
import small_grid_cases as S
from folded_cases import SEEDS, case as folded_case
from genome_amd import dna
from oracle import oracle as O
from test_fuzz_gpu import _oracle_graph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIVE = ["g_k11_p1", "g_k21_p3", "g_k31_p1", "g_k35_p2", "g_k63_p1"]
M = 2 ** 64


# ---- mix64 ---------------------------------------------------------------------------------------------------------------------
def test_mix64_against_values_worked_out_here():
    # x = 1, step by step
    a = 1 ^ (1 >> 33)
    assert a == 1
    b = (a * 0xff51afd7ed558ccd) % M
    assert b == 0xff51afd7ed558ccd
    c = b ^ (b >> 33)
    assert b >> 33 == 0x7fa8d7eb and c == 0xff51afd792fd5b26
    d = (c * 0xc4ceb9fe1a85ec53) % M
    assert d == 0xb456bcfc6ee99552
    e = d ^ (d >> 33)
    assert d >> 33 == 0x5a2b5e7e and e == 0xb456bcfc34c2cb2c
    assert CS.mix64(1) == e
    # four more, each as one expression of masked arithmetic
    for x in (0, M - 1, CS.G, 0x0123456789abcdef):
        y = x ^ (x >> 33)
        y = (y * 0xff51afd7ed558ccd) & (M - 1)
        y ^= y >> 33
        y = (y * 0xc4ceb9fe1a85ec53) & (M - 1)
        y ^= y >> 33
        assert CS.mix64(x) == y
    assert CS.mix64(0) == 0
    assert CS.mix64(M - 1) == 0x64b5720b4b825f21
    assert CS.mix64(CS.G) == 0x9ca066f1a4ab2eea
    assert CS.mix64(0x0123456789abcdef) == 0x87cbfbfe89022cea
    assert CS.mix64(M + 1) == CS.mix64(1)                                   # the argument is taken mod 2^64
    assert CS.G == 0x9e3779b97f4a7c15


def test_packing_is_the_librarys():
    rnd = random.Random(1)
    for k in (2, 31, 34, 64):
        s = "".join(rnd.choice("AGCT") for _ in range(k))
        assert CS.pack(s) == dna.pack(s)
    assert CS.pack_bases("AGCTT") == bytes([0 | 1 << 2 | 2 << 4 | 3 << 6, 3])
    assert dna.reads_to_bin(["AGCTTGA"])[1:] == CS.pack_bases("AGCTTGA")


def test_one_entry_one_node_one_edge_by_hand():
    """each formula once, spelled out with mix64 alone"""
    m, G = CS.mix64, CS.G
    lo, hi = dna.pack("GATTACA" * 4 + "GAT")                               # k = 31
    assert hi == 0 and lo >> 60
    assert CS.table_checksum(31, [(lo, 0, 7)]) == m((m(lo ^ 0x243f6a8885a308d3) + 7 * G) % M)
    lo2, hi2 = dna.pack("GATTACA" * 5)                                     # k = 35
    assert hi2 != 0
    assert CS.table_checksum(35, [(lo2, hi2, 7)]) == m((m(lo2 ^ m(hi2 ^ 0x13198a2e03707344)) + 7 * G) % M)
    assert CS.nodes_checksum([(lo, 0)]) == m(lo ^ m(0x13198a2e03707344))
    assert CS.nodes_checksum([(lo2, hi2)]) == m(lo2 ^ m(hi2 ^ 0x13198a2e03707344))
    seq = "TTGCA"                                                          # two bytes: T T G C | A
    b0, b1 = 3 | 3 << 2 | 1 << 4 | 2 << 6, 0
    h = (m(lo ^ m(0 ^ 1)) + 3 * m(lo2 ^ m(hi2 ^ 2)) + 5 * m(5)) % M
    h = m(h ^ ((b0 + G * 1) % M))
    h = m(h ^ ((b1 + G * 2) % M))
    assert CS.edge_hash((lo, 0), (lo2, hi2), seq) == h
    fm = lambda a, v: m(a ^ ((v + G) % M))
    want = (m(m(9 ^ 0x626f756e6473) ^ ((4 + G) % M)) + fm(fm(fm(0x6e6f6465, 8), lo2), hi2)
            + fm(fm(fm(fm(fm(0x65646765, 3), 8), 8), 3), 5)) % M
    assert CS.id_fingerprint([(8, lo2, hi2)], [(3, 8, 8, 3, 5)], 9, 4) == want


# ---- every field enters --------------------------------------------------------------------------------------------------------
def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def make_state(k, seed=0):
    """a small table and a small graph by id.  Nodes 0, 1, 2 and 6 carry k-mers of their own, node 4 is a COPY of node 1 (a node
    split leaves such); edge 0 has 45 bases (12 bytes, the last holds one base), edges 2 and 5 have 7 and 10; ids are sparse."""
    rnd = random.Random(1000 * k + seed)
    kmers = [rand_seq(rnd, k) for _ in range(4)]
    assert len(set(kmers)) == 4
    return dict(k=k, table={s: c for s, c in zip([rand_seq(rnd, k) for _ in range(6)], (1, 2, 255, 256, 65535, 65536))},
                nodes={0: kmers[0], 1: kmers[1], 2: kmers[2], 4: kmers[1], 6: kmers[3]},
                edges=[(0, 0, 1, rand_seq(rnd, 45)), (2, 1, 2, rand_seq(rnd, 7)), (5, 2, 6, rand_seq(rnd, 10))], nb=7, eb=6)


def values(st):
    nodes, edges = st["nodes"], st["edges"]
    cn, ce = CS.graph_checksum(list(nodes.values()), [(nodes[s], nodes[t], q) for _e, s, t, q in edges])
    return {"table": CS.table_checksum_of(st["table"]), "nodes": cn, "edges": ce,
            "fp": CS.id_fingerprint_of(nodes, edges, st["nb"], st["eb"])}


def changed(a, b):
    va, vb = values(a), values(b)
    return {name for name in va if va[name] != vb[name]}


def other(c):
    return "AGCT"[("AGCT".index(c) + 1) % 4]


def with_base(seq, i, c=None):
    return seq[:i] + (c or other(seq[i])) + seq[i + 1:]


def copy_of(st):
    return dict(st, table=dict(st["table"]), nodes=dict(st["nodes"]), edges=list(st["edges"]))


def flip_bit(kmer, bit):
    """the k-mer whose packed form differs in this one bit of the 128"""
    lo, hi = dna.pack(kmer)
    if bit < 64:
        lo ^= 1 << bit
    else:
        hi ^= 1 << (bit - 64)
    return dna.unpack(lo, hi, len(kmer))


@pytest.mark.parametrize("k,bit", [(31, 61), (31, 60), (34, 64), (34, 67), (64, 64), (64, 127), (64, 100), (64, 63), (5, 9)])
def test_every_key_bit_enters(k, bit):
    """the top used bit of lo at k = 31, bits of hi at k = 34 and k = 64: in a table key, in a node that edges start and end in"""
    st = make_state(k)
    t = copy_of(st)
    key = next(iter(st["table"]))
    new = flip_bit(key, bit)
    assert len(new) == k and new != key and sum(a != b for a, b in zip(new, key)) == 1
    t["table"] = {(new if s == key else s): c for s, c in st["table"].items()}
    assert changed(st, t) == {"table"}
    t = copy_of(st)
    t["nodes"][2] = flip_bit(st["nodes"][2], bit)                          # edge 2 ends in node 2, edge 5 starts there
    assert changed(st, t) == {"nodes", "edges", "fp"}
    for node in (0, 6):                                                    # a start only, an end only
        t = copy_of(st)
        t["nodes"][node] = flip_bit(st["nodes"][node], bit)
        assert changed(st, t) == {"nodes", "edges", "fp"}


@pytest.mark.parametrize("k", [31, 34, 64])
def test_every_other_field_enters(k):
    st = make_state(k)
    assert len(st["edges"][0][3]) >= 40 and len(st["edges"][0][3]) % 4 == 1
    # a count by 1, each count in turn (1 -> 2 meets a count that is already there: the KEY is mixed in)
    for key in st["table"]:
        t = copy_of(st)
        t["table"][key] += 1
        assert changed(st, t) == {"table"}
    # one base of the 45-base edge: in the first byte (not the first base, which the fingerprint holds), a middle byte, the
    # last, partial byte
    for i in (1, 3, 22, 43, 44):
        t = copy_of(st)
        e, s, n, q = st["edges"][0]
        t["edges"][0] = (e, s, n, with_base(q, i))
        assert changed(st, t) == {"edges"}, i
    t = copy_of(st)
    t["edges"][0] = st["edges"][0][:3] + (with_base(st["edges"][0][3], 0),)
    assert changed(st, t) == {"edges", "fp"}                               # the first base is the fingerprint's too
    # the bits after the last base are no content: a 45-base edge and its first 45 of 46 differ (the length), yet bases 46..48
    # of the last byte enter only once they exist
    q = st["edges"][0][3]
    assert CS.pack_bases(q)[-1] >> 2 == 0 and CS.pack_bases(q + "A") == CS.pack_bases(q)
    t = copy_of(st)
    t["edges"][0] = st["edges"][0][:3] + (q + "A",)                        # the same bytes, one base more
    assert changed(st, t) == {"edges", "fp"}
    # the length alone, total kept: the last base of edge 2 goes to the end of edge 5 (first bases stay)
    t = copy_of(st)
    (e2, s2, n2, q2), (e5, s5, n5, q5) = st["edges"][1], st["edges"][2]
    t["edges"][1], t["edges"][2] = (e2, s2, n2, q2[:-1]), (e5, s5, n5, q5 + q2[-1])
    assert sum(len(x[3]) for x in t["edges"]) == sum(len(x[3]) for x in st["edges"])
    assert changed(st, t) == {"edges", "fp"}
    # two edges that swap their sequences: every byte is still there, under another start and end
    t = copy_of(st)
    t["edges"][1], t["edges"][2] = (e2, s2, n2, q5), (e5, s5, n5, q2)
    assert changed(st, t) == {"edges", "fp"}
    # start against end
    t = copy_of(st)
    e, s, n, q = st["edges"][0]
    t["edges"][0] = (e, n, s, q)
    assert changed(st, t) == {"edges", "fp"}
    # ids.  Node 4 carries node 1's k-mer: an edge that starts or ends in the copy instead is the same CONTENT
    t = copy_of(st)
    t["edges"][1] = (e2, 4, n2, q2)                                        # a start id
    assert changed(st, t) == {"fp"}
    t = copy_of(st)
    t["edges"][0] = (e, s, 4, q)                                           # an end id
    assert changed(st, t) == {"fp"}
    t = copy_of(st)
    t["edges"][2] = (4, s5, n5, q5)                                        # an edge id
    assert changed(st, t) == {"fp"}
    t = copy_of(st)
    t["nodes"][5] = t["nodes"].pop(4)                                      # a node id (no edge names node 4)
    assert changed(st, t) == {"fp"}
    t = copy_of(st)
    del t["nodes"][4]                                                      # the copy itself is content of the node sum
    assert changed(st, t) == {"nodes", "fp"}
    for bound in ("nb", "eb"):                                             # each of the two bounds
        t = copy_of(st)
        t[bound] += 1
        assert changed(st, t) == {"fp"}
    t = copy_of(st)
    t["nb"], t["eb"] = st["eb"], st["nb"]                                  # ... and which is which
    assert changed(st, t) == {"fp"}


@pytest.mark.parametrize("k", [31, 64])
def test_order_partitions_and_renumbering(k):
    st = make_state(k)
    rnd = random.Random(3)
    # shuffling the entries changes nothing
    t = copy_of(st)
    for name in ("table", "nodes"):
        items = list(st[name].items())
        rnd.shuffle(items)
        t[name] = dict(items)
        assert list(t[name]) != list(st[name])
    rnd.shuffle(t["edges"])
    assert changed(st, t) == set()
    # two partitions' table checksums add up to the union's
    items = list(st["table"].items())
    a, b = dict(items[:2]), dict(items[2:])
    assert (CS.table_checksum_of(a) + CS.table_checksum_of(b)) % M == values(st)["table"]
    assert CS.table_checksum_of({}) == 0 and CS.table_checksum(k, []) == 0
    # renumbering: every id through one injective map, references and bounds with it
    f = lambda i: 3 * i + 1
    t = copy_of(st)
    t["nodes"] = {f(i): s for i, s in st["nodes"].items()}
    t["edges"] = [(f(e), f(s), f(n), q) for e, s, n, q in st["edges"]]
    t["nb"], t["eb"] = f(st["nb"] - 1) + 1, f(st["eb"] - 1) + 1
    assert changed(st, t) == {"fp"}
    # ... and the bounds alone do not make up for it
    t["nb"], t["eb"] = st["nb"] + 99, st["eb"] + 99
    assert changed(st, t) == {"fp"}


def test_the_two_key_widths_are_two_formulas():
    """k <= 31 mixes lo with a constant of its own: a k = 31 table is not a k = 34 table whose high words are 0"""
    entries = [(12345, 0, 3)]
    assert CS.table_checksum(31, entries) != CS.table_checksum(34, entries)
    with pytest.raises(AssertionError):
        CS.table_checksum(32, entries)


# ---- the oracle's tables and graphs: the inputs are not degenerate ----------------------------------------------------------------
def table_of(ref):
    lo, hi, c = ref.export_sorted()
    return CS.table_checksum(ref.k, zip(map(int, lo), map(int, hi), map(int, c)))


def three(ref, og, content):
    """(table, nodes, edges) restated; the fingerprint is of ids, which the oracle numbers its own way"""
    return (table_of(ref),) + CS.graph_checksum(*content)


def golden_states(name):
    """the oracle's (keys, content, restated values) counted, after delete_lt(rounds), after removeBubbles + simplifyGraph"""
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    k = fx["k"]
    ref = O.PMap(k, 1)
    ref.count_reads(bytes.fromhex(fx["bin_hex"]), fx["nreads"])
    out = []

    def snap(og):
        content = _oracle_graph(og, k)
        out.append((ref.size(), content, three(ref, og, content)))
    og = O.Graph(ref); snap(og); og.close()
    ref.delete_lt(fx["rounds"])
    og = O.Graph(ref); snap(og)
    og.remove_bubbles(); og.simplify(); snap(og)
    og.close(); ref.close()
    return fx, out


def lengths(content):
    return [len(q) for _s, _t, q in content[1]]


@pytest.mark.parametrize("name", FIVE)
def test_golden_inputs_change_under_the_filter(name):
    fx, (counted, filtered, simplified) = golden_states(name)
    assert filtered[1] == (fx["nodes"], [tuple(e) for e in fx["edges"]])                  # it IS the golden graph
    assert simplified[1][1] == [tuple(e) for e in fx["edges_after_simplify"]]
    assert counted[0] > 2 * filtered[0] > 0 and len(counted[1][0]) > 2 * len(filtered[1][0]) > 0
    for i in range(3):                                                                     # table, nodes, edges: all three change
        assert counted[2][i] != filtered[2][i], i
    # removeBubbles + simplifyGraph finds nothing to do in the graph of a filtered golden table (the module's text): the state
    # "after simplify" of these five is the state before it.  The inputs below are the ones it changes.
    assert simplified[1] == filtered[1] and simplified[2] == filtered[2]
    assert max(lengths(simplified[1])) > 64


def _simplify_changes(ref, k):
    og = O.Graph(ref)
    before = _oracle_graph(og, k)
    og.remove_bubbles(); og.simplify()
    after = _oracle_graph(og, k)
    og.close()
    cb, ca = CS.graph_checksum(*before), CS.graph_checksum(*after)
    assert len(after[1]) < len(before[1]) and len(after[0]) < len(before[0])
    assert cb[0] != ca[0] and cb[1] != ca[1]
    return before, after


@pytest.mark.parametrize("name", ["snp_k11_p2", "snp_k35_p1"])
def test_golden_snp_inputs_change_under_simplify(name):
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    ref = O.PMap(fx["k"], 1)
    ref.count_reads(bytes.fromhex(fx["bin_hex"]), fx["nreads"])
    ref.delete_lt(fx["rounds"])
    _before, after = _simplify_changes(ref, fx["k"])
    assert max(lengths(after)) > 64
    ref.close()


@pytest.mark.parametrize("k", [11, 35, 64])
def test_small_grid_reads_change_under_simplify(k):
    reads = S.reads_case(k)
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    t0 = table_of(ref)
    ref.delete_lt(2)
    assert table_of(ref) != t0
    before, after = _simplify_changes(ref, k)
    assert len(before[0]) > 2 * 3 * S.BLOCK and len(before[1]) > 2 * 3 * S.BLOCK          # what the capped GPU cases rely on
    ln = lengths(after)
    assert {x % 4 for x in ln} == {0, 1, 2, 3} and sum(x > 64 for x in ln) >= 3
    ref.close()


def test_the_folded_k64_graph_changes_under_simplify():
    c = folded_case(64, SEEDS[64], "noisy")
    reads = c.graph_reads
    ref = O.PMap(64, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    ref.delete_lt(c.min_count)
    _before, after = _simplify_changes(ref, 64)
    assert {x % 4 for x in lengths(after)} == {0, 1, 2, 3} and max(lengths(after)) > 64
    ref.close()


def test_edge_lengths_the_gpu_tests_rely_on():
    """after removeBubbles + simplifyGraph: every residue of len mod 4 and an edge longer than 64 bases, in one golden graph"""
    _fx, (_c, _f, simplified) = golden_states("g_k35_p2")
    ln = lengths(simplified[1])
    assert {x % 4 for x in ln} == {0, 1, 2, 3}
    assert sum(x > 64 for x in ln) >= 1
    seen = set()
    for name in FIVE:
        seen |= {x % 4 for x in lengths(golden_states(name)[1][2][1])}
    assert seen == {0, 1, 2, 3}
