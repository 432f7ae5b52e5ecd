"""graph_simplifier --links --scaffold-fasta --judge GENOME.fasta (the C++ host side over genome.hpp) against the Python path on the
graph the tool itself saved (-m gpu); modelled on tests/test_overlaps_host_gpu.py.  The case is the end-to-end one of
tests/overlaps_cases.py, a 6 kb genome with three dips, judged against a reference whose two records are the genome cut at the
second dip and swapped: the join across that dip is planted as `other_record`; the other two are right once --overlap-gaps
has found their overlaps, and `distance` when a clamped N run stands in their place.  graph_builder
--walk-pairs shares the stage: it takes the flags."""
import json
import os
import subprocess

import pytest

from genome_amd import check as GC
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import JUDGE_CLASSES, JUDGE_STATS, PLACE_STATS, HipLinks, buildGraph, loadGraph, scaffoldChains, scaffoldGaps
from pairs_ref import make_pairs
import judge_cases as JC
import overlaps_cases as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(os.path.join(HOST, "graph_simplifier")) or not os.path.exists(os.path.join(HOST, "graph_builder")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return os.path.join(HOST, "graph_simplifier")


def test_graph_simplifier_judge(exe, tmp_path):
    E = OC.E2E
    k, support = E["k"], E["support"]
    pieces = OC.e2e_pieces()
    reads = make_pairs(E["seed"], k, glen=E["glen"], nrep=0, L=k + 9, npairs=E["npairs"], ins=E["ins"])
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    G = OC.e2e_genome()
    p, w = E["dips"][1]
    records = [G[p + w:], G[:p + k - 1]]                      # the contigs on either side of the second dip, on two records, swapped
    binf, gfile, ref = tmp_path / "reads.bin", tmp_path / "g.graph", tmp_path / "genome.fasta"
    binf.write_bytes(binb)
    ref.write_bytes(JC.fasta(records, width=60).replace(b"\n", b"\r\n", 3))
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(pieces), len(pieces))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    base = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--range", str(E["ins"][0]), str(E["ins"][1]), "--links", str(tmp_path / "links.txt"),
            "--link-min-support", str(support)]
    half = (E["ins"][1] - E["ins"][0]) // 2
    seen = {}
    for name, extra, tol in (("auto", ["--overlap-gaps"], half), ("given", ["--overlap-gaps", "--judge-tol", "0"], 0), ("gapped", ["--judge-tol", "3"], 3)):
        fa, final = tmp_path / (name + ".fa"), tmp_path / (name + ".graph")
        run = subprocess.run(base + ["--scaffold-fasta", str(fa), "--save-graph", str(final), "--judge", str(ref)] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        got = json.loads(run.stdout)
        assert list(got).index("judge") == list(got).index("scaffolds") + 1 and run.stderr.count("judge: tol %d (" % tol) == 1
        lk, jd = got["links"], got["judge"]
        # the Python path on the graph the tool saved
        g = loadGraph(ctx, final)
        vm, links = g.getGraphMap(), HipLinks(ctx)
        g.pairLinks(vm, PairedEndData(npairs, binb), links, min_len=0, max_span=lk["max_span"])
        joins, _ = links.joins(support)
        chains = scaffoldChains(joins[0], joins[1])
        gaps = scaffoldGaps(chains, joins, lk["mid"])
        ov = g.overlapGaps(chains, gaps, half)[0] if "--overlap-gaps" in extra else None
        s = g.scaffolds(chains, gaps, overlaps=ov)
        assert fa.read_bytes() == s.text() and got["scaffolds"] == s.stats()
        with g.place(vm, records) as pl:
            want, pst = s.judge(pl, tol), pl.stats()
        ns = GC.scaffold_n50s(s.segments(), want["classes"])
        assert jd == dict(tol=tol, placements=pst, stats=want["stats"], classes=[JUDGE_CLASSES.index(c) for c in want["classes"]], err=want["err"],
                          n50=ns["n50"], n50_broken=ns["n50_broken"])
        assert list(jd["placements"]) == list(PLACE_STATS) and list(jd["stats"]) == list(JUDGE_STATS)
        assert GC.judge_scaffolds(g, ref, s, tol)["stats"] == want["stats"]
        print(name, {n: v for n, v in want["stats"].items() if v}, want["classes"], want["err"], {n: v for n, v in pst.items() if v}, s.segments())
        # one chain of four contigs: dips of 18, 10 and 3 missing k-mers = overlaps of 12, 20 and 27 bases; the reference is cut at the second.
        # Without --overlap-gaps a negative gap is clamped to min_gap = 10 bases N, which is 10 + o bases too many: `distance`.
        if "--overlap-gaps" in extra:
            assert (want["classes"], want["err"]) == (["correct", "other_record", "correct"], [0, 0, 0])
        else:
            assert (want["classes"], want["err"]) == (["distance", "other_record", "distance"], [10 + 12, 0, 10 + 27])
        assert jd["n50_broken"] < jd["n50"]
        seen[name] = want["stats"]
        s.close(); links.close(); vm.close(); g.close()
    ctx.close()
    assert seen["auto"]["overlapped_correct"] == 2 and seen["auto"] == seen["given"] and seen["gapped"]["gapped_distance"] == 2
    # the option is refused without --scaffold-fasta, and says what it needs
    alone = subprocess.run(base + ["--judge", str(ref)], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and alone.stdout == "" and "--judge GENOME.fasta goes with --scaffold-fasta PATH" in alone.stderr
    usage = subprocess.run([os.path.join(HOST, "graph_builder")], capture_output=True, text=True, timeout=60)
    assert "--judge GENOME.fasta [--judge-tol N]" in usage.stderr + usage.stdout
