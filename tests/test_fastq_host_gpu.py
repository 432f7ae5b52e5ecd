"""The FASTQ forms of the C++ tools (convert2bin, graph_builder --fastq, graph_simplifier --fastq).  -m gpu.

convert2bin must write what the plain restatement tests/fastq_ref.py writes and print its statistics; the --fastq forms of
graph_builder and graph_simplifier must print what the `.bin` forms print for the converted stream and its pair count, and
build the same graphs (gk_graph_checksum of the saved files)."""
import json
import os
import subprocess

import pytest

import fastq_ref as ref
from genome_amd import dna
from genome_amd.dnamap import Context
from genome_amd.graph import loadGraph
from test_fastq_gpu import fuzz_fastq
from test_pairs_gpu import make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
CONVERT, BUILDER, SIMPLIFIER = (os.path.join(HOST, x) for x in ("convert2bin", "graph_builder", "graph_simplifier"))


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("split", [36, 0])
def test_convert2bin_writes_the_restatement(tmp_path, split):
    data = fuzz_fastq(40 + split, 700, split)
    if split == 0 and (len(ref.lines(data)) // 4) % 2:
        data += ref.record(b"@x", b"ACGT", b"IIII")
    (tmp_path / "r.fastq").write_bytes(data)
    out = run([CONVERT, tmp_path / "r.fastq", tmp_path / "o"] + (["--interleaved"] if split == 0 else ["--split", split]) + ["--k", 21])
    want, st = ref.convert(data, split, 21)
    assert (tmp_path / "o.bin").read_bytes() == want
    assert out == dict(st, bin_bytes=len(want), text_bytes=len(data))
    assert not (tmp_path / "o.bin.tmp").exists()


def test_convert2bin_refuses_bad_input(tmp_path):
    (tmp_path / "bad.fastq").write_bytes(ref.record(b"@r", b"ACGT", b"IIII") + b"@r\nACGT\n")
    r = subprocess.run([CONVERT, str(tmp_path / "bad.fastq"), str(tmp_path / "o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FASTQ record 1" in r.stderr
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.bin.tmp").exists()
    r = subprocess.run([BUILDER, "--fastq", str(tmp_path / "bad.fastq"), "21", "--world", "2", "--rank", "0", "--id-file", str(tmp_path / "id")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2


def graph_checksum(path):
    c = Context(0)
    g = loadGraph(c, path)
    out = (g.counts(), g.checksum())
    g.close(); c.close()
    return out


def test_graph_tools_fastq_forms_match_bin_forms(tmp_path):
    k = 21
    reads = make_pairs(11, k)
    assert all(len(r) <= 255 for r in reads)
    fq = b"".join(ref.record(b"@p%d/%d" % (i // 2, 1 + i % 2), r.encode(), b"I" * len(r)) for i, r in enumerate(reads))
    (tmp_path / "r.fastq").write_bytes(fq)
    st = run([CONVERT, tmp_path / "r.fastq", tmp_path / "r", "--interleaved"])
    assert (tmp_path / "r.bin").read_bytes() == dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    assert st["pairs"] == npairs
    opts = ["--rounds", 2, "--simplify"]
    a = run([BUILDER, tmp_path / "r.bin", npairs, k] + opts + ["--save-graph", tmp_path / "a.gkg"])
    b = run([BUILDER, "--fastq", tmp_path / "r.fastq", k, "--interleaved"] + opts + ["--save-graph", tmp_path / "b.gkg"])
    assert a == b
    assert graph_checksum(tmp_path / "a.gkg") == graph_checksum(tmp_path / "b.gkg")
    w = ["--walk-pairs", 3, 60, 95]
    assert run([BUILDER, tmp_path / "r.bin", npairs, k] + opts + w) == run([BUILDER, "--fastq", tmp_path / "r.fastq", k, "--interleaved"] + opts + w)
    s_opts = ["--cutoff", 3, "--range", 60, 95]
    s1 = run([SIMPLIFIER, tmp_path / "a.gkg", tmp_path / "r.bin", npairs] + s_opts + ["--save-graph", tmp_path / "s1.gkg"])
    s2 = run([SIMPLIFIER, tmp_path / "a.gkg", "--fastq", tmp_path / "r.fastq", "--interleaved"] + s_opts + ["--save-graph", tmp_path / "s2.gkg"])
    assert s1 == s2 and s1["walk_pairs"]["orientations_walked"] > 0
    assert graph_checksum(tmp_path / "s1.gkg") == graph_checksum(tmp_path / "s2.gkg")
