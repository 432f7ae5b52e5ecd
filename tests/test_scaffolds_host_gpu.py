"""graph_simplifier --links --scaffold-fasta (the C++ host side over genome.hpp) against the Python path on the graph the tool itself
saved (-m gpu); modelled on tests/test_links_host_gpu.py.  The file must be the Python path's text byte for byte, the JSON's
"scaffolds" object its stats; without the new flag stdout's keys are what they were."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import HipLinks, buildGraph, loadGraph, scaffoldChains, scaffoldGaps
from insert_cases import E2E, E2E_MAX_INSERT, E2E_SEED
from pairs_ref import make_pairs
import scaffolds_ref as SR
from thread_cases import device_graph as graph_by_id
from test_links_gpu import edge_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_simplifier")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


def test_graph_simplifier_scaffold_fasta(exe, tmp_path):
    k = E2E["k"]
    reads = make_pairs(E2E_SEED, k, glen=E2E["glen"], nrep=E2E["nrep"], L=E2E["L"], npairs=E2E["npairs"], ins=(180, 250))
    binb = dna.reads_to_bin(reads)
    npairs, take, min_len, support = len(reads) // 2, 1400, 2 * k, 3
    binf, gfile = tmp_path / "reads.bin", tmp_path / "g.graph"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    base = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--take-first", str(take), "--range", "auto", "--max-insert", str(E2E_MAX_INSERT),
            "--links", str(tmp_path / "links.txt"), "--link-min-support", str(support), "--link-min-len", str(min_len)]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    keys_before = list(json.loads(plain.stdout))
    assert "links" in keys_before and "scaffolds" not in keys_before
    for width, both, min_gap in ((60, False, 10), (0, True, 3)):
        fa, final = tmp_path / ("s%d.fa" % width), tmp_path / ("final%d.graph" % width)
        cmd = base + ["--scaffold-fasta", str(fa), "--scaffold-width", str(width), "--scaffold-min-gap", str(min_gap), "--save-graph", str(final)]
        run = subprocess.run(cmd + (["--scaffold-both-strands"] if both else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        got = json.loads(run.stdout)
        assert [key for key in got if key != "scaffolds"] == keys_before and list(got).index("scaffolds") == list(got).index("links") + 1
        lk = got["links"]
        # the Python path on the graph the tool saved
        g = loadGraph(ctx, final)
        vm, links = g.getGraphMap(), HipLinks(ctx)
        g.pairLinks(vm, PairedEndData(npairs, binb), links, min_len=min_len, max_span=lk["max_span"], take_first=take)
        joins, _ = links.joins(support)
        chains = scaffoldChains(joins[0], joins[1])
        gaps = scaffoldGaps(chains, joins, lk["mid"])
        assert len(chains) == lk["chains"] > 0 and any(len(c) >= 2 for c in chains)
        s = g.scaffolds(chains, gaps, min_gap=min_gap, min_len=min_len, line_width=width, strands=2 if both else 1)
        st = s.stats()
        assert st["members"] > st["records"] - st["singletons"] > 0 and st["gapped"] + st["adjacent"] > 0      # (a chain of several members is written)
        assert fa.read_bytes() == s.text() and not os.path.exists(str(fa) + ".tmp")
        assert got["scaffolds"] == st
        # and the restatement on that graph, read back by id
        nodes, edges, _ = graph_by_id(g)
        live = sorted(edge_keys(g))
        named = {live[i]: (nodes[a], nodes[b], q) for i, (a, b, q) in enumerate(edges)}
        node_ids = {live[i]: (a, b) for i, (a, b, _q) in enumerate(edges)}
        want, want_st, _ = SR.scaffolds(named, chains, gaps, min_gap=min_gap, min_len=min_len, line_width=width, strands=2 if both else 1, node_ids=node_ids)
        assert fa.read_bytes() == want and st == want_st
        s.close(); links.close(); vm.close(); g.close()
    ctx.close()
    # the flag alone is refused, and says what it needs
    alone = subprocess.run(base[:base.index("--links")] + ["--scaffold-fasta", str(tmp_path / "x.fa")], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and "--scaffold-fasta PATH goes with --links PATH" in alone.stderr and not os.path.exists(tmp_path / "x.fa")
