"""graph_builder --pop-bubbles end to end on the GPU (-m gpu), on the k = 21 read case of tests/test_bubbles_gpu.py: the per-round
counts and the written graph against the Python mirror of the same flow; without the flag no trace of it; with --world exit 2."""
import json
import os
import subprocess

import pytest

from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_builder")
K, READS, CONFIG, ERR = 21, 3000, 3, 0.02


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    rec = synth.reads_mode_g(READS, 100, 2000, ERR, config_id=CONFIG)
    path = tmp_path_factory.mktemp("bubbles") / "reads.bin"
    path.write_bytes(rec.tobytes())
    return rec, str(path)


def run(exe, binf, *flags):
    res = subprocess.run([exe, binf, str(READS // 2), str(K), "--rounds", "2", *flags], capture_output=True)
    assert res.returncode == 0, res.stderr.decode()
    return res.stdout


def test_pop_bubbles_matches_the_python_mirror(exe, reads, tmp_path):
    rec, binf = reads
    out = str(tmp_path / "b")
    stats = json.loads(run(exe, binf, "--clip-tips", "--pop-bubbles", "--simplify", "--out", out))
    # the same flow through the Python binding: retain, (clip, pop, simplify) until a round removes nothing, bubbles, simplify
    ctx = Context(0)
    m = HipDNAMap(ctx, K, 1 << 16)
    m.count_reads(rec.tobytes(), READS)
    m.deleteAll_lt(2)
    g = buildGraph(K, m)
    g.retainLargest()
    tips, removed, pairs = [], [], []
    while len(tips) < 8:
        tips.append(g.clipTips(m))
        rm, cmp_ = g.popBubbles(m)
        removed.append(rm); pairs.append(cmp_)
        if not tips[-1] and not rm:
            break
        g.simplifyGraph()
    g.removeBubbles()
    g.simplifyGraph()
    assert stats["clip_tips"] == {"max_len": 2 * K, "removed": tips}
    assert stats["pop_bubbles"] == {"max_len": 2 * K, "max_diff": 3, "removed": removed, "pairs": pairs}
    assert len(removed) >= 2 and sum(removed) >= 2 and tips[-1] == 0 and removed[-1] == 0
    nodes, edges, length = g.counts()
    assert (stats["retained_nodes"], stats["retained_edges"], stats["retained_edges_length"]) == (nodes, edges, length)
    assert [line.split() for line in open(out + ".edges.txt").read().splitlines()] == [list(e) for e in g.canonical()[1]]
    assert open(out + ".nodes.txt").read().split() == g.canonical()[0]
    # the explicit forms of the two options give the same run
    again = json.loads(run(exe, binf, "--clip-tips", "auto", "--pop-bubbles", "3", "--bubble-max-len", str(2 * K), "--simplify"))
    assert again == stats
    g.close(); m.close(); ctx.close()


def test_without_the_flag_there_is_no_trace_of_it(exe, reads):
    _rec, binf = reads
    stats = json.loads(run(exe, binf, "--clip-tips", "--simplify"))
    assert "pop_bubbles" not in stats and "clip_tips" in stats
    assert b"pop_bubbles" not in run(exe, binf, "--simplify")


def test_pop_bubbles_does_not_run_over_ranks(exe, reads, tmp_path):
    _rec, binf = reads
    res = subprocess.run([exe, binf, str(READS // 2), str(K), "--pop-bubbles", "--world", "2", "--rank", "0", "--id-file", str(tmp_path / "id")], capture_output=True)
    assert res.returncode == 2 and b"--pop-bubbles" in res.stderr
    res = subprocess.run([exe, binf, str(READS // 2), str(K), "--pop-bubbles", "32"], capture_output=True)
    assert res.returncode == 2
