"""A plain restatement of the three 64-bit values the suite takes as proof of equality, and which version 1 of the graph file
stores (include/genome_amd.h): gk_map_verify's table checksum (k_verify, gk_table.hip), gk_graph_checksum's node and edge
checksums (k_graph_checksum, gk_graph_ops.hip) and gk_graph_id_fingerprint (k_graph_id_fingerprint, gk_pairs.hip, with the bounds
term its host side adds).  Python ints masked to 64 bits; nothing of the library is imported, so that the packing of a k-mer is
restated here as well.  Test infrastructure: tests/test_checksum_cpu.py holds it to hand-worked values and to the committed graph
files, tests/test_checksum_gpu.py holds the kernels to it.

Every sum is taken mod 2^64, so the order of the entries never matters.  Keys are (lo, hi) as genome_amd.dna.pack gives them
(base i at bits 2i of lo for i < 32, at bits 2(i - 32) of hi above; A0 G1 C2 T3); hi = 0 for k <= 31.

NOT restated here: the replica CONTENT fingerprints of the N-rank reduce (k_edge_content in gk_pairs.hip, and the path keys of
gk_links.h, which tests/pathkey_ref.py covers).  They are other formulas with other constants and are no part of the file format.
"""
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15                       # the golden-ratio constant of every formula below
TABLE_W1 = 0x243F6A8885A308D3                # k_verify, one key word
KEY_HI = 0x13198A2E03707344                  # k_verify with two key words, and the node sum
FP_NODE, FP_EDGE, FP_BOUNDS = 0x6E6F6465, 0x65646765, 0x626F756E6473        # "node", "edge", "bounds"
BASES = "AGCT"


def mix64(x: int) -> int:
    """gk_device.h: xor-shift by 33 around the two multiplications, and once more after the second"""
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def pack(seq: str):
    """a k-mer (k <= 64) as base string -> (lo, hi)"""
    lo = hi = 0
    for i, c in enumerate(seq):
        if i < 32:
            lo |= BASES.index(c) << (2 * i)
        else:
            hi |= BASES.index(c) << (2 * (i - 32))
    return lo, hi


def pack_bases(seq: str) -> bytes:
    """an edge's sequence as the pool holds it: four bases per byte, the first in the lowest bits, zero bits after the last"""
    out = bytearray((len(seq) + 3) // 4)
    for i, c in enumerate(seq):
        out[i // 4] |= BASES.index(c) << (2 * (i % 4))
    return bytes(out)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def table_checksum(k: int, entries) -> int:
    """entries: the live (lo, hi, count) of a table of k-mers of k bases (2..31 or 34..64).  A partitioned map's value is the sum
    of this over its partitions."""
    assert 2 <= k <= 31 or 34 <= k <= 64
    total = 0
    for lo, hi, count in entries:
        kh = mix64(lo ^ TABLE_W1) if k <= 31 else mix64(lo ^ mix64(hi ^ KEY_HI))
        total += mix64((kh + count * G) & M64)
    return total & M64


def table_checksum_of(counts: dict) -> int:
    """counts: stored k-mer (base string) -> count"""
    if not counts:
        return 0
    k = len(next(iter(counts)))
    return table_checksum(k, [pack(s) + (c,) for s, c in counts.items()])


# ---- the graph by content ------------------------------------------------------------------------------------------------------
def nodes_checksum(nodes) -> int:
    """nodes: (lo, hi) of every live node (a k-mer that several nodes carry enters once per node)"""
    return sum(mix64(lo ^ mix64(hi ^ KEY_HI)) for lo, hi in nodes) & M64


def edge_hash(start, end, seq: str) -> int:
    """start, end: (lo, hi) of the edge's end nodes; seq: its bases"""
    h = mix64(start[0] ^ mix64(start[1] ^ 1)) + 3 * mix64(end[0] ^ mix64(end[1] ^ 2)) + 5 * mix64(len(seq))
    h &= M64
    for i, b in enumerate(pack_bases(seq)):
        h = mix64(h ^ ((b + G * (i + 1)) & M64))
    return h


def graph_checksum(nodes, edges):
    """nodes: k-mers as base strings; edges: (start k-mer, end k-mer, sequence) as base strings, what HipGraph.canonical() and the
    oracle's export give.  Ids do not enter.  -> (nodes checksum, edges checksum)"""
    return (nodes_checksum(pack(s) for s in nodes),
            sum(edge_hash(pack(s), pack(t), q) for s, t, q in edges) & M64)


# ---- the graph by id -----------------------------------------------------------------------------------------------------------
def _m(a: int, v: int) -> int:
    return mix64(a ^ ((v + G) & M64))


def id_fingerprint(nodes, edges, node_bound: int, edge_bound: int) -> int:
    """nodes: (id, lo, hi) of every live node; edges: (id, start node id, end node id, first base code, length) of every live
    edge; the bounds: one above the largest id ever given, dead ones included"""
    total = mix64(mix64(node_bound ^ FP_BOUNDS) ^ ((edge_bound + G) & M64))
    for i, lo, hi in nodes:
        total += _m(_m(_m(FP_NODE, i), lo), hi)
    for i, s, t, first, length in edges:
        total += _m(_m(_m(_m(_m(FP_EDGE, i), s), t), first), length)
    return total & M64


def id_fingerprint_of(nodes: dict, edges, node_bound: int, edge_bound: int) -> int:
    """nodes: {id: k-mer string}; edges: [(edge id, start id, end id, sequence string)], as tests/test_graph_file_cpu.decode gives"""
    return id_fingerprint([(i,) + pack(s) for i, s in nodes.items()],
                          [(e, s, t, BASES.index(q[0]), len(q)) for e, s, t, q in edges], node_bound, edge_bound)
