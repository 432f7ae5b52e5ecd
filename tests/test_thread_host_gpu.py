"""graph_simplifier --thread-reads --no-pairs (the C++ host side over genome.hpp) against the Python path on the same graph file
and reads (-m gpu); modelled on tests/test_insert_host_gpu.py."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dist import HipDist, unique_id
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import Support, loadGraph
from thread_cases import build_graph, genome, tiling

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_simplifier")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


def test_graph_simplifier_thread_reads_no_pairs(exe, tmp_path):
    k, cutoff = 31, 2
    reads = tiling(genome(5, k, glen=1200, nrep=1), 100, 9)
    reads = reads[:len(reads) // 2 * 2]                               # the tool takes pairs: two records each
    binb, npairs = dna.reads_to_bin(reads), len(reads) // 2
    binf, gfile, ofile = tmp_path / "reads.bin", tmp_path / "g.graph", tmp_path / "out.graph"
    binf.write_bytes(binb)
    ctx = Context(0)
    g = build_graph(ctx, k, reads)
    g.save(gfile)
    g.close()
    # the Python path, call by call
    g = loadGraph(ctx, gfile)
    vm, sup = g.getGraphMap(), Support(ctx)
    st = g.threadReads(vm, sup, PairedEndData(npairs, binb))
    assert st["records"] == len(reads) and st["crossings"] > 0
    pairs = sup.sizes()[0]
    removed, new_nodes = g.splitBySupport(sup, cutoff)
    assert new_nodes > 0
    g.simplifyGraph()
    want_counts, want_sum = g.counts(), g.checksum()
    sup.close(); vm.close(); g.close()
    # the pipeline
    hd = HipDist(ctx, 0, 1, unique_id())
    gp, sp = simplify_graph(hd, gfile, PairedEndData(npairs, binb), cutoff, thread_reads=True, walk=False)
    assert sp["walk_pairs"]["thread_reads"] == st and gp.checksum() == want_sum
    assert (sp["walk_pairs"]["supported_edge_pairs"], sp["walk_pairs"]["orientations_walked"]) == (pairs, 0)
    gp.close(); hd.close()
    # the tool
    run = subprocess.run([exe, str(gfile), str(binf), str(npairs), "--cutoff", str(cutoff), "--thread-reads", "--no-pairs", "--save-graph", str(ofile)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    assert got["thread_reads"] == st
    assert got["walk_pairs"] == {"supported_edge_pairs": pairs, "bad_pairs": 0, "orientations_walked": 0, "removed_edges": removed, "new_nodes": new_nodes}
    assert (got["simplified_nodes"], got["simplified_edges"], got["simplified_edges_length"]) == want_counts
    g = loadGraph(ctx, ofile)
    assert g.checksum() == want_sum
    g.close()
    # --no-pairs without --thread-reads is a usage error; without either flag the JSON has no new key
    bad = subprocess.run([exe, str(gfile), str(binf), str(npairs), "--cutoff", str(cutoff), "--no-pairs"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
    plain = subprocess.run([exe, str(gfile), str(binf), str(npairs), "--cutoff", str(cutoff)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "thread_reads" not in json.loads(plain.stdout)
    ctx.close()
