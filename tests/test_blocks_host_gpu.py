"""check_graph --blocks and graph_simplifier --judge .. --blocks (the C++ host side over genome.hpp) against the restatement
(tests/blocks_ref.py) on the graph file the tool read or saved (-m gpu); modelled on tests/test_judge_host_gpu.py.  The "blocks" object
of the JSON holds the restatement's stats, genome fraction, NA50 and NGA50, and the rows file its rows."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import BLOCK_STATS, buildGraph, loadGraph
from pairs_ref import make_pairs
import blocks_cases as BC
import blocks_ref as BR
import judge_cases as JC
import overlaps_cases as OC
from test_judge_gpu import model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
TOOLS = ("check_graph", "graph_simplifier", "graph_builder")


@pytest.fixture(scope="module")
def exe():
    if not all(os.path.exists(os.path.join(HOST, t)) for t in TOOLS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return {t: os.path.join(HOST, t) for t in TOOLS}


def read_rows(path):
    lines = [ln for ln in open(path).read().splitlines() if not ln.startswith("#")]
    return [tuple(int(x) for x in ln.split("\t")) for ln in lines]


def held(blocks, rows_file, want, tol):
    st = want["stats"]
    assert blocks == dict(tol=tol, stats=st, genome_fraction=st["covered"] / st["windows"], na50=want["na50"], nga50=want["nga50"])
    assert list(blocks["stats"]) == list(BLOCK_STATS) and read_rows(rows_file) == want["rows"] and st["rows"] > 0


def test_check_graph_blocks(exe, tmp_path):
    """the main case and the planted chimeras, the default tol and a given one"""
    ctx = Context(0)
    for name, case, k in (("main", JC.main(31), 31), ("chimeras", BC.chimeras(34), 34)):
        gfile, ref, rows = tmp_path / (name + ".graph"), tmp_path / (name + ".fasta"), tmp_path / (name + ".rows")
        records = [r for r in case["records"] if r]
        ref.write_bytes(JC.fasta(records, width=60).replace(b"\n", b"\r\n", 3))
        m = HipDNAMap(ctx, k)
        m.count_reads(dna.reads_to_bin(case["reads"]), len(case["reads"]))
        g = buildGraph(k, m)
        g.save(gfile)
        g.close(); m.close()
        g = loadGraph(ctx, gfile)
        nodes, edges, _ends, ne = model(g)
        g.close()
        for extra, tol, how in ((["--block-tol", str(BC.TOL)], BC.TOL, "given"), ([], 1000, "the default, a choice")):
            run = subprocess.run([exe["check_graph"], str(gfile), str(ref), "--blocks", "--block-rows", str(rows)] + extra, capture_output=True, text=True, timeout=120)
            assert run.returncode == 0, run.stderr
            got = json.loads(run.stdout)
            assert list(got)[-1] == "blocks" and run.stderr.count("blocks: tol %d (%s), " % (tol, how)) == 1
            want = BR.align(k, nodes, edges, records, tol, id_bound=ne)
            held(got["blocks"], rows, want, tol)
        if name == "chimeras":
            assert want["stats"]["edges_misassembled"] == 4 and want["stats"]["brk_relocation"] == 0      # (at tol 1000 a shift of 50 is an indel)
        plain = subprocess.run([exe["check_graph"], str(gfile), str(ref)], capture_output=True, text=True, timeout=120)
        assert plain.returncode == 0 and "blocks" not in json.loads(plain.stdout) and "blocks:" not in plain.stderr
    ctx.close()


def test_graph_simplifier_judge_blocks(exe, tmp_path):
    """the end-to-end case of tests/test_judge_host_gpu.py: the blocks of the FINAL graph against the reference the judge reads"""
    E = OC.E2E
    k, support = E["k"], E["support"]
    pieces = OC.e2e_pieces()
    reads = make_pairs(E["seed"], k, glen=E["glen"], nrep=0, L=k + 9, npairs=E["npairs"], ins=E["ins"])
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    G = OC.e2e_genome()
    p, w = E["dips"][1]
    records = [G[p + w:], G[:p + k - 1]]
    binf, gfile, ref = tmp_path / "reads.bin", tmp_path / "g.graph", tmp_path / "genome.fasta"
    binf.write_bytes(binb)
    ref.write_bytes(JC.fasta(records, width=60))
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(dna.reads_to_bin(pieces), len(pieces))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    fa, final, rows = tmp_path / "s.fa", tmp_path / "final.graph", tmp_path / "rows.txt"
    run = subprocess.run([exe["graph_simplifier"], str(gfile), str(binf), str(npairs), "--cutoff", "3", "--range", str(E["ins"][0]), str(E["ins"][1]), "--links",
                          str(tmp_path / "links.txt"), "--link-min-support", str(support), "--scaffold-fasta", str(fa), "--save-graph", str(final), "--overlap-gaps",
                          "--judge", str(ref), "--blocks", "--block-tol", "7", "--block-rows", str(rows)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    assert list(got).index("blocks") == list(got).index("judge") + 1 and run.stderr.count("blocks: tol 7 (given), ") == 1
    g = loadGraph(ctx, final)
    nodes, edges, _ends, ne = model(g)
    g.close(); ctx.close()
    want = BR.align(k, nodes, edges, records, 7, id_bound=ne)
    held(got["blocks"], rows, want, 7)
    assert want["stats"]["edges_exact"] > 0 and want["stats"]["full_edges"] > 0
    usage = subprocess.run([exe["graph_builder"]], capture_output=True, text=True, timeout=60)
    assert "[--blocks [--block-tol N (default 1000: a choice, not a measurement)] [--block-rows PATH]]" in usage.stderr
