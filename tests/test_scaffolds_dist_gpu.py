"""dist_pipeline.simplify_graph(links=...) over 2 and 3 loopback ranks, followed by HipGraph.scaffolds (-m gpu): every rank's
multiset of record sequences, and the link classes, equal those of the same call over one rank (world 1, the product transport)
on the same graph file and reads.  Record ORDER follows a rank's own ids and is not compared."""
import pytest

from genome_amd import dna
from genome_amd.dist import HipDist, unique_id
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import buildGraph
from test_pairs_dist_gpu import run_ranks
from test_pairs_gpu import make_pairs

pytestmark = pytest.mark.gpu
K, RNG = 21, (60, 95)
LINKS = dict(min_support=3, min_len=0, max_span=RNG[1] + K, mid=(RNG[0] + RNG[1]) // 2 + K)


def sequences(text):
    """a FASTA text -> the sorted list of its records' sequences"""
    return sorted("".join(rec.split("\n")[1:]) for rec in text.decode().split(">")[1:])


def stage(hd, path, data):
    g, stats = simplify_graph(hd, path, data, 3, *RNG, links=LINKS)
    lk = stats["links"]
    sc = g.scaffolds(lk["chains"], lk["gaps"])
    res = {"classes": lk["classes"], "seqs": sequences(sc.text()), "chains": sorted(len(c) for c in lk["chains"]), "counts": g.counts(),
           "joins": len(lk["joins"][0]), "size": lk["links"].size()}
    sc.close(); lk["links"].close(); g.close()
    return res


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    reads = make_pairs(1, K)
    data = PairedEndData(len(reads) // 2, dna.reads_to_bin(reads))
    path = str(tmp_path_factory.mktemp("scaf") / "graph.gkg")
    c = Context(0)
    m = HipDNAMap(c, K)
    m.count_reads(data.bin, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(K, m)
    g.save(path)
    g.close(); m.close()
    hd = HipDist(c, 0, 1, unique_id())
    want = stage(hd, path, data)
    hd.close(); c.close()
    assert want["classes"]["linked"] > 0 and want["joins"] > 0 and max(want["chains"]) >= 2       # there is a scaffold of two contigs
    return path, data, want


@pytest.mark.parametrize("world", [2, 3])
def test_scaffolds_over_ranks_equal_one_rank(one_rank, world):
    path, data, want = one_rank
    out = run_ranks(world, lambda rank, c, hd: stage(hd, path, data), timeout=120)
    for o in out:
        assert o == want
