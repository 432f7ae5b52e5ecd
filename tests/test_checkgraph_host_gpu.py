"""The C++ check_graph tool (S/scripts/CheckGraph.scala as a stage): graph_builder --save-graph, then check_graph on the file.  Its
JSON must equal genome_amd.check.check_graph on the same inputs and the plain restatement tests/checkgraph_ref.py.  -m gpu."""
import json
import os
import subprocess

import pytest

import checkgraph_ref as ref
from genome_amd import dna
from genome_amd.check import check_graph
from genome_amd.dnamap import Context
from genome_amd.graph import loadGraph
from test_checkgraph_gpu import make_fasta, make_genome, tiled_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, CHECK = os.path.join(HOST, "graph_builder"), os.path.join(HOST, "check_graph")


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_check_graph_tool_matches_python_and_the_restatement(tmp_path):
    k = 31
    g = make_genome(7, 3000)
    reads = tiled_reads(g)
    (tmp_path / "r.bin").write_bytes(dna.reads_to_bin(reads))
    run([BUILDER, tmp_path / "r.bin", len(reads) // 2, k, "--rounds", 1, "--no-retain", "--save-graph", tmp_path / "g.gkg"])
    text, _ = make_fasta(g, k, 5)
    (tmp_path / "ref.fasta").write_bytes(text)
    c = Context(0)
    graph = loadGraph(c, tmp_path / "g.gkg")
    vm = graph.getGraphMap()
    lo, hi, _ = vm.items()
    present = {dna.unpack(int(a), int(b), k) for a, b in zip(lo, hi)}
    vm.close()
    lengths = [len(e[2]) for e in graph.canonical()[1]]
    for per_line in (False, True):
        got = run([CHECK, tmp_path / "g.gkg", tmp_path / "ref.fasta", "--longer-than", 100, "--missing", 7] + (["--per-line"] if per_line else []))
        want = check_graph(graph, tmp_path / "ref.fasta", longer_than=100, per_line=per_line, max_missing=7)
        assert got == json.loads(json.dumps(want))
        st, missing = ref.check(text, k, per_line, present)
        assert {key: got[key] for key in st} == st and st["missing"] > 7
        assert [(m["offset"], m["line"], m["column"], m["lo"], m["hi"]) for m in got["missing_list"]] == missing[:7]
        assert got["contigs"] == ref.contig_stats(lengths, 100) and got["contigs"]["count"] > 0
        assert got["coverage"] == st["covered_bases"] / st["valid_bases"] and got["k"] == k
    graph.close(); c.close()


def test_check_graph_tool_errors(tmp_path):
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([CHECK, "a.gkg", "b.fasta", "--what"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    r = subprocess.run([CHECK, str(tmp_path / "none.gkg"), str(tmp_path / "none.fasta")], capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, 2) and "none.gkg" in r.stderr
