"""graph_builder --contigs and graph_simplifier --contigs (the C++ tools): the FASTA file a tool writes must be, byte for byte, what
the Python API gives for the graph the same run saved (ids survive the graph file), and its "contigs_fasta" JSON the nine stats;
and end to end: a repeat-free genome, error-free reads, one contig that is the genome.  -m gpu."""
import json
import os
import subprocess

import numpy as np
import pytest

from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import loadGraph
from oracle import pyref as R
from test_checkgraph_gpu import make_genome, tiled_reads

import contigs_ref as CR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, SIMPLIFIER = os.path.join(HOST, "graph_builder"), os.path.join(HOST, "graph_simplifier")


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_tools_write_what_the_python_api_gives(tmp_path):
    k = 31
    reads = tiled_reads(make_genome(7, 3000))
    bin_ = dna.reads_to_bin(reads)
    (tmp_path / "r.bin").write_bytes(bin_)
    js = run([BUILDER, tmp_path / "r.bin", len(reads) // 2, k, "--rounds", 1, "--no-retain", "--save-graph", tmp_path / "g.gkg",
              "--contigs", tmp_path / "b.fa", "--contig-width", 50, "--contig-min-len", 40])
    c = Context(0)
    m = HipDNAMap(c, k)
    m.count_reads(bin_, len(reads))
    graph = loadGraph(c, tmp_path / "g.gkg")
    want = graph.contigs(m, min_len=40, line_width=50, strands=1)
    assert (tmp_path / "b.fa").read_bytes() == want.text() and js["contigs_fasta"] == want.stats()
    assert want.stats()["records"] >= 3 and want.stats()["missing_windows"] == 0 and b" cov=" in want.text()
    want.close()
    # both strands, the defaults otherwise
    js = run([BUILDER, tmp_path / "r.bin", len(reads) // 2, k, "--rounds", 1, "--no-retain", "--contigs", tmp_path / "b2.fa", "--contig-both-strands"])
    want = graph.contigs(m, strands=2)
    assert (tmp_path / "b2.fa").read_bytes() == want.text() and js["contigs_fasta"] == want.stats()
    assert js["contigs_fasta"]["records"] == js["contigs_fasta"]["live_edges"] == js["retained_edges"]
    want.close()
    # graph_simplifier: no count table, so no cov= field; the graph it saved is the graph it wrote
    # (the reads themselves are the support: the tiled reads are no pairs a walk could use)
    js = run([SIMPLIFIER, tmp_path / "g.gkg", tmp_path / "r.bin", len(reads) // 2, "--cutoff", 1, "--thread-reads", "--no-pairs",
              "--save-graph", tmp_path / "s.gkg", "--contigs", tmp_path / "s.fa", "--contig-width", 0])
    simplified = loadGraph(c, tmp_path / "s.gkg")
    want = simplified.contigs(line_width=0)
    text = (tmp_path / "s.fa").read_bytes()
    assert text == want.text() and js["contigs_fasta"] == want.stats() and b"cov=" not in text
    assert js["contigs_fasta"]["live_edges"] == js["simplified_edges"] > 0 and len(text.splitlines()) == 2 * want.stats()["records"]
    want.close(); simplified.close(); graph.close(); m.close(); c.close()
    # an unwritable path is the tool's error, and leaves nothing
    r = subprocess.run([BUILDER, str(tmp_path / "r.bin"), str(len(reads) // 2), str(k), "--rounds", "1", "--contigs", str(tmp_path / "none" / "x.fa")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "x.fa" in r.stderr and not (tmp_path / "none").exists()


def repeat_free_genome(k, size):
    """a genome from synth.genome_bases in which no k-mer occurs twice on either strand (checked here; the seed is redrawn if not)"""
    for seed in range(100, 120):
        g = synth.bases_to_str(synth.genome_bases(size, seed))
        if len({R.canon(g[i:i + k]) for i in range(size - k + 1)}) == size - k + 1:
            return g
    raise AssertionError("no repeat-free genome in 20 draws")


def test_end_to_end_one_contig_is_the_genome(tmp_path):
    k, size, length = 31, 20000, 100
    g = repeat_free_genome(k, size)
    codes = np.array([CR.CODE[c] for c in g], np.uint8)
    # error-free reads at about 30x: 6000 random ones (both strands), and two passes of a tiling that reaches both ends, so
    # that every k-mer of the genome is seen at least `rounds` = 2 times
    rec = [synth.reads_mode_g(6000, length, size, 0.0, config_id=5, genome=codes)]
    starts = np.array(list(range(0, size - length + 1, 50)) * 2)
    rec.append(synth.pack_reads(codes[starts[:, None] + np.arange(length)[None, :]]))
    bin_ = np.concatenate(rec).tobytes()
    nreads = 6000 + len(starts)
    (tmp_path / "r.bin").write_bytes(bin_)
    # --no-retain: the two strands of a repeat-free linear genome are two components, and the retain keeps one of them, whose one
    # edge is as often the reverse one (which one strand per contig leaves to its twin) as the forward one
    js = run([BUILDER, tmp_path / "r.bin", nreads // 2, k, "--rounds", 2, "--no-retain", "--contigs", tmp_path / "asm.fa"])
    recs = CR.parse((tmp_path / "asm.fa").read_bytes())
    st = js["contigs_fasta"]
    assert st["records"] == len(recs) and st["forward"] == st["reverse"] and st["missing_windows"] == 0
    rc = R.rev_comp(g)
    covered = set()
    for _id, n, cov, seq in recs:
        assert seq in g or seq in rc
        assert float(cov) >= 2.0
        covered.update(R.canon(seq[i:i + k]) for i in range(n - k + 1))
    assert {R.canon(g[i:i + k]) for i in range(size - k + 1)} <= covered
    assert len(recs) == 1 and recs[0][1] == size and recs[0][3] in (g, rc)
