"""graph_builder --keep-cycles and graph_simplifier --keep-cycles (the C++ tools): a circular genome comes out as a contig where
the plain run writes nothing; a circular genome with one tip survives --clip-tips; the simplifier keeps the self-loops of a saved
graph; the option is refused with --world.  -m gpu."""
import json
import os
import subprocess

import pytest

import cycles_cases as CC
import cycles_ref as CR
from genome_amd import dna

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, SIMPLIFIER = os.path.join(HOST, "graph_builder"), os.path.join(HOST, "graph_simplifier")
K = 15


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def circular_reads(circ, n=50):
    """the circular genome as tests/test_graph_gpu.py reads it: every window of n bases, twice"""
    cc = circ + circ[:n - 1]
    return [cc[i:i + n] for i in range(len(circ))] * 2


def records(path):
    return ["".join(r.split("\n")[1:]) for r in open(path).read().split(">") if r]


def is_rotation(seq, circ):
    """seq = the genome (or its reverse complement) read once around, plus the k bases it started with"""
    L = len(circ)
    return len(seq) == L + K and seq[:K] == seq[-K:] and (seq[:L] in circ + circ or seq[:L] in CR.rc(circ + circ))


def test_builder_writes_the_circular_contig(tmp_path):
    circ = CC.make("circular", K)[0][0]
    reads = circular_reads(circ)
    (tmp_path / "r.bin").write_bytes(dna.reads_to_bin(reads))
    base = [BUILDER, tmp_path / "r.bin", len(reads) // 2, K, "--no-retain"]
    js, err = run(base + ["--keep-cycles", "--contigs", tmp_path / "c.fa", "--save-graph", tmp_path / "g.gkg"])
    L = len(circ)
    assert js["cycles"]["build"] == {"cycle_kmers": 2 * L, "cycles": 2, "anchors": 2, "self_complementary": 0, "longest": L, "rounds": 8}
    assert js["cycles"]["simplify"] == dict.fromkeys(("kept_self_loops", "cycles_merged", "anchors_kept", "nodes_removed"), 0)
    assert (js["graph_nodes"], js["graph_edges"], js["total_edges_length"]) == (2, 2, 2 * L)
    assert "keep-cycles: build {\"cycle_kmers\":%d," % (2 * L) in err
    rec = records(tmp_path / "c.fa")
    assert len(rec) == 1 and is_rotation(rec[0], circ)
    # without the option the output is empty, as before
    js0, err0 = run(base + ["--contigs", tmp_path / "c0.fa"])
    assert "cycles" not in js0 and "keep-cycles" not in err0
    assert (js0["graph_nodes"], js0["graph_edges"]) == (0, 0) and records(tmp_path / "c0.fa") == []
    # the simplifier on the saved graph: its simplifyGraph deletes the self-loops unless told to keep them
    sim = [SIMPLIFIER, tmp_path / "g.gkg", tmp_path / "r.bin", len(reads) // 2, "--cutoff", 1, "--thread-reads", "--no-pairs"]
    js1, err1 = run(sim + ["--keep-cycles", "--contigs", tmp_path / "s.fa"])
    # (the split by support replaces a supported node by a copy and leaves the original isolated: those are what the simplify removes)
    copies = js1["walk_pairs"]["new_nodes"]
    assert js1["cycles"] == {"simplify": {"kept_self_loops": 2, "cycles_merged": 0, "anchors_kept": 0, "nodes_removed": copies}}
    assert (js1["simplified_nodes"], js1["simplified_edges"]) == (2, 2) and "keep-cycles: simplify {" in err1
    rec = records(tmp_path / "s.fa")
    assert len(rec) == 1 and is_rotation(rec[0], circ)
    js2, _ = run(sim)
    assert "cycles" not in js2 and (js2["simplified_nodes"], js2["simplified_edges"]) == (0, 0)


def test_builder_keeps_a_replicon_whose_tip_was_clipped(tmp_path):
    """the issue's case: after --clip-tips the junction has one way in and one way out, the same edge"""
    (circ,), (tip,) = CC.make("one_tip", K)
    reads = circular_reads(circ) + [tip, tip]
    (tmp_path / "r.bin").write_bytes(dna.reads_to_bin(reads))
    base = [BUILDER, tmp_path / "r.bin", len(reads) // 2, K, "--rounds", 1, "--no-retain", "--clip-tips"]
    js, _ = run(base + ["--keep-cycles", "--contigs", tmp_path / "c.fa"])
    assert js["cycles"]["build"]["cycle_kmers"] == 0, "the tip breaks the cycle: the build adds nothing"
    assert js["clip_tips"]["removed"][0] == 2
    assert js["cycles"]["simplify"]["kept_self_loops"] == 2 and (js["retained_nodes"], js["retained_edges"]) == (2, 2)
    rec = records(tmp_path / "c.fa")
    assert len(rec) == 1 and is_rotation(rec[0], circ)
    js0, _ = run(base + ["--contigs", tmp_path / "c0.fa"])
    assert (js0["retained_nodes"], js0["retained_edges"]) == (0, 0) and records(tmp_path / "c0.fa") == []


@pytest.mark.parametrize("tool, args", [(BUILDER, ["r.bin", "10", "31"]), (SIMPLIFIER, ["g.gkg", "r.bin", "10", "--cutoff", "2"])])
def test_keep_cycles_with_world_is_refused(tool, args):
    r = subprocess.run([tool] + args + ["--keep-cycles", "--world", "2", "--rank", "0", "--id-file", "id"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr == "--keep-cycles runs on one GPU only (not with --world): perfect cycles have no collective\n"
