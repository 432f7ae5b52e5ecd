"""What the scaffold-link GPU tests share: the oracle's graph of a fixture as the restatement takes it, with the content key (start
k-mer, first base code) of every edge, and the settings S of the key-width cases.  Content only: no ids, no device."""
from genome_amd import dna
from insert_ref import index_graph
from links_ref import joins, pair_links
from oracle import oracle as O
from pairs_ref import oracle_canonical


def settings(k):
    """S: min_len = 2k, max_span = 100 + k, support 3"""
    return dict(min_len=2 * k, max_span=100 + k, support=3)


def oracle_graph(k, reads, min_count=1):
    """-> (index, edge lengths, content key of every edge, edge paths) of the oracle's graph of `reads`"""
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    if min_count > 1:
        ref.delete_lt(min_count)
    nodes, edges = oracle_canonical(O.Graph(ref))
    index, lens = index_graph(k, [(s, q) for s, _, q in edges], nodes=nodes)
    return index, lens, [(s, dna.BASES.index(q[0])) for s, _, q in edges], [s + q for s, _, q in edges]


def by_content(links, keys):
    """{(e, f): [count, sum_u]} -> {(key e, key f): (count, sum_u)}"""
    out = {(keys[e], keys[f]): tuple(v) for (e, f), v in links.items()}
    assert len(out) == len(links)
    return out


def restate(k, graph_reads, reads, npairs, min_len, max_span, support, min_count=1):
    """-> (links by content, classes, joins by content as a sorted list, join stats)"""
    index, lens, keys, _ = oracle_graph(k, graph_reads, min_count)
    links, cls = pair_links(k, index, lens, reads, npairs, min_len, max_span)
    jn, st = joins(links, support)
    return by_content(links, keys), cls, sorted((keys[e], keys[f], c, s) for e, f, c, s in jn), st
