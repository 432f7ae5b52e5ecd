"""What the insert-range GPU tests share: fixtures from pairs_ref.make_pairs, and the restatement (tests/insert_ref.py) run on the
ORACLE's graph of the same reads — content only, no ids, no device."""
from genome_amd import dna
from insert_ref import index_graph, pair_distances
from oracle import oracle as O
from pairs_ref import make_pairs, oracle_canonical

GLEN = 2400
INS = (80, 100)
# Seeds for the planted-truth cases, chosen on the CPU: with these the restatement ALONE finds every counted fragment length
# inside the planted 80..100 (no fragment has both ends on one repeat edge at a false distance), k = 21 and 31.
PLANTED_SEEDS = {21: 1, 31: 1}
# end to end: an 8 kbp genome, 100-base mates, inserts 180..250; with this seed the restatement's trim-0 estimate is exactly 180..250
E2E = dict(k=31, glen=8000, nrep=4, L=100, npairs=1500)
E2E_SEED = 1
E2E_MAX_INSERT = 300


def small_pairs(seed, k, npairs=400, err=0.0, ins=INS):
    """glen 2400, L = k + 9 (ten k-mers a mate), three planted repeats"""
    return make_pairs(seed, k, glen=GLEN, L=k + 9, npairs=npairs, ins=ins, err=err)


def oracle_index(k, reads, min_count=1):
    """(index, edge lengths) of the oracle's graph of `reads` (every k-mer seen at least min_count times)"""
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    ref.count_reads(binb, len(reads))
    if min_count > 1:
        ref.delete_lt(min_count)
    nodes, edges = oracle_canonical(O.Graph(ref))
    return index_graph(k, [(s, q) for s, _, q in edges], nodes=nodes)


def restate(k, graph_reads, reads, npairs, bins, min_count=1):
    index, lens = oracle_index(k, graph_reads, min_count)
    return pair_distances(k, index, lens, reads, npairs, bins)
