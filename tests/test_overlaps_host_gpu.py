"""graph_simplifier --links --scaffolds --scaffold-fasta --overlap-gaps (the C++ host side over genome.hpp) against the Python path
on the graph the tool itself saved (-m gpu); modelled on tests/test_fillgaps_host_gpu.py.  The case is the end-to-end one of
tests/overlaps_cases.py: a 6 kb genome with three dips.  graph_builder --walk-pairs shares the stage: it takes the flags."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import OVERLAP_STATS, HipLinks, buildGraph, loadGraph, scaffoldChains, scaffoldGaps
from pairs_ref import make_pairs
from test_fillgaps_host_gpu import id_list
import overlaps_cases as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(os.path.join(HOST, "graph_simplifier")) or not os.path.exists(os.path.join(HOST, "graph_builder")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return os.path.join(HOST, "graph_simplifier")


def test_graph_simplifier_overlap_gaps(exe, tmp_path):
    E = OC.E2E
    k, support = E["k"], E["support"]
    pieces = OC.e2e_pieces()
    reads = make_pairs(E["seed"], k, glen=E["glen"], nrep=0, L=k + 9, npairs=E["npairs"], ins=E["ins"])
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    binf, gfile = tmp_path / "reads.bin", tmp_path / "g.graph"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(pieces), len(pieces))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    base = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--range", str(E["ins"][0]), str(E["ins"][1]), "--links", str(tmp_path / "links.txt"),
            "--link-min-support", str(support)]
    texts, objects = {}, {}
    for name, extra in (("plain", []), ("auto", ["--overlap-gaps"]), ("filled", ["--fill-gaps", "--overlap-gaps"]),
                        ("given", ["--overlap-gaps", "4", "--overlap-min", "15", "--overlap-max", "25"])):
        fa, ids, final = tmp_path / (name + ".fa"), tmp_path / (name + ".txt"), tmp_path / (name + ".graph")
        run = subprocess.run(base + ["--scaffolds", str(ids), "--scaffold-fasta", str(fa), "--save-graph", str(final)] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        got = json.loads(run.stdout)
        assert ("overlap" in got) == bool(extra) and ("fill" in got) == (name == "filled")
        if extra:
            assert list(got).index("overlap") == list(got).index("scaffolds") - 1 and "overlap-gaps: tol" in run.stderr
        lk = got["links"]
        # the Python path on the graph the tool saved
        g = loadGraph(ctx, final)
        vm, links = g.getGraphMap(), HipLinks(ctx)
        g.pairLinks(vm, PairedEndData(npairs, binb), links, min_len=0, max_span=lk["max_span"])
        joins, _ = links.joins(support)
        chains = scaffoldChains(joins[0], joins[1])
        gaps = scaffoldGaps(chains, joins, lk["mid"])
        assert len(chains) == lk["chains"] > 0
        ov = None
        if name == "filled":
            chains, gaps, frep = g.fillGaps(chains, gaps, (E["ins"][1] - E["ins"][0]) // 2)
            assert frep["filled"] == 0                                            # no graph path closes a dip
        if extra:
            tol, mn, mx = (4, 15, 25) if name == "given" else ((E["ins"][1] - E["ins"][0]) // 2, 10, k)
            ov, rep = g.overlapGaps(chains, gaps, tol, min_overlap=mn, max_overlap=mx)
            assert got["overlap"] == dict({"tol": tol, "min_overlap": mn, "max_overlap": mx}, **{n: rep[n] for n in OVERLAP_STATS})
            assert list(got["overlap"])[3:] == list(OVERLAP_STATS) and rep["junctions"] > 0 and rep["overlap"] > 0
            objects[name] = got["overlap"]
        s = g.scaffolds(chains, gaps, overlaps=ov)
        texts[name] = fa.read_bytes()
        assert texts[name] == s.text() and got["scaffolds"] == s.stats()
        shown = [[-o if o else x for x, o in zip(gp, oo)] for gp, oo in zip(gaps, ov)] if ov is not None else gaps
        assert id_list(ids) == (chains, shown)
        assert ("# --overlap-gaps:" in open(ids).read()) == bool(extra)
        s.close(); links.close(); vm.close(); g.close()
    ctx.close()
    assert texts["filled"] == texts["auto"] != texts["plain"] and objects["filled"] == objects["auto"]
    # the flag alone is refused, and says what it needs
    alone = subprocess.run(base + ["--overlap-gaps"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and "--overlap-gaps goes with --scaffolds PATH or --scaffold-fasta PATH" in alone.stderr
    usage = subprocess.run([os.path.join(HOST, "graph_builder")], capture_output=True, text=True, timeout=60)
    assert "--overlap-gaps [TOL] [--overlap-min N] [--overlap-max N]" in usage.stderr + usage.stdout
