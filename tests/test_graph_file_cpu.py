"""The committed version-1 graph files (tests/golden/graph_v1_k*.gkg), read by a decoder of the documented layout
(include/genome_amd.h) without the library or a GPU: the header and the (start, end, sequence) edge set must be the golden
graph's, and the header's checksum pair and id fingerprint are the documented formulas (tests/checksum_ref.py) over that content.
This pins the file format, the three formulas included."""
import json
import os
import struct

import pytest

import checksum_ref as CS
from genome_amd import dna

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def decode(b):
    """version 1 -> (header dict, {id: k-mer}, {id: out-order}, [(edge id, start id, end id, sequence)])"""
    assert b[:8] == b"GKGRAPH\0"
    version, k = struct.unpack_from("<II", b, 8)
    nb, eb, nn, ne, pool = struct.unpack_from("<5Q", b, 16)
    cs_n, cs_e, fp = struct.unpack_from("<3Q", b, 56)
    assert b[80:128] == bytes(48)
    al8 = lambda v: (v + 7) & ~7
    arr = lambda fmt, off, n: list(struct.unpack_from("<%d%s" % (n, fmt), b, off))
    o = 128
    ids = arr("I", o, nn); o = al8(o + 4 * nn)
    lo = arr("Q", o, nn); o += 8 * nn
    hi = [0] * nn
    if k >= 34:
        hi = arr("Q", o, nn); o += 8 * nn
    order = arr("I", o, nn); o = al8(o + 4 * nn)
    eid = arr("I", o, ne); o = al8(o + 4 * ne)
    est = arr("I", o, ne); o = al8(o + 4 * ne)
    een = arr("I", o, ne); o = al8(o + 4 * ne)
    eln = arr("Q", o, ne); o += 8 * ne
    assert len(b) == o + pool
    nodes = {i: dna.unpack(a, c, k) for i, a, c in zip(ids, lo, hi)}
    edges = []
    for j in range(ne):
        nbytes = (eln[j] + 3) // 4
        seq = "".join("AGCT"[(b[o + i // 4] >> (2 * (i % 4))) & 3] for i in range(eln[j]))
        if eln[j] & 3:
            assert b[o + nbytes - 1] >> (2 * (eln[j] & 3)) == 0
        edges.append((eid[j], est[j], een[j], seq))
        o += nbytes
    head = {"version": version, "k": k, "node_bound": nb, "edge_bound": eb, "nodes": nn, "edges": ne, "pool": pool,
            "checksum": (cs_n, cs_e), "fingerprint": fp}
    return head, nodes, dict(zip(ids, order)), edges


@pytest.mark.parametrize("name,k", [("g_k11_p1", 11), ("g_k35_p2", 35)])
def test_committed_graph_file_decodes_to_the_golden_graph(name, k):
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    b = open(os.path.join(GOLDEN, "graph_v1_k%d.gkg" % k), "rb").read()
    assert len(b) < 64 << 10
    head, nodes, order, edges = decode(b)
    assert head["version"] == 1 and head["k"] == k == fx["k"]
    assert head["nodes"] == len(fx["nodes"]) and head["edges"] == len(fx["edges"])
    assert head["node_bound"] >= head["nodes"] and head["edge_bound"] >= head["edges"]
    assert head["pool"] == sum((len(e[2]) + 3) // 4 for e in fx["edges"])
    ids = sorted(nodes)
    assert ids == sorted(set(ids)) and sorted(e[0] for e in edges) == [e[0] for e in edges]
    assert sorted(nodes.values()) == sorted(fx["nodes"])
    assert sorted([nodes[s], nodes[t], seq] for _, s, t, seq in edges) == sorted(fx["edges"])
    # every edge: the last k bases of (start ++ sequence) are its end k-mer; out-orders list exactly the out-edges' first bases
    for _, s, t, seq in edges:
        assert (nodes[s] + seq)[-k:] == nodes[t]
    for n, o in order.items():
        listed = sorted("AGCT"[(o >> (4 + 2 * i)) & 3] for i in range(o & 7))
        assert listed == sorted(seq[0] for _, s, _, seq in edges if s == n)
    # the three values of header bytes 56..79 are the formulas of include/genome_amd.h (restated in tests/checksum_ref.py) over
    # the content just decoded
    assert head["checksum"] == CS.graph_checksum(list(nodes.values()), [(nodes[s], nodes[t], seq) for _, s, t, seq in edges])
    assert head["checksum"] == CS.graph_checksum(fx["nodes"], fx["edges"])
    assert head["fingerprint"] == CS.id_fingerprint_of(nodes, edges, head["node_bound"], head["edge_bound"])
    assert len({head["fingerprint"], *head["checksum"]}) == 3 and 0 not in head["checksum"] + (head["fingerprint"],)
