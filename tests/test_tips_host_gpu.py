"""graph_builder --clip-tips / --edge-coverage end to end on the GPU (-m gpu), on the k = 21 random case of tests/test_tips_gpu.py:
the per-round counts and the coverage file against the Python mirror of the same flow, and — without the new flags — the very
bytes the parent commit wrote (tests/golden/tips/parent_hashes.json: sha256 of stdout and of every output file, recorded
with the parent's build before the flags existed)."""
import hashlib
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
K, READS, CONFIG = 21, 3000, 2


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    rec = synth.reads_mode_g(READS, 100, 2000, 0.01, config_id=CONFIG)
    path = tmp_path_factory.mktemp("tips") / "reads.bin"
    path.write_bytes(rec.tobytes())
    return rec, str(path)


def run(exe, binf, *flags):
    res = subprocess.run([exe, binf, str(READS // 2), str(K), "--rounds", "2", *flags], capture_output=True)
    assert res.returncode == 0, res.stderr.decode()
    return res.stdout


def test_clip_tips_and_edge_coverage_match_the_python_mirror(exe, reads, tmp_path):
    rec, binf = reads
    out = str(tmp_path / "t")
    stats = json.loads(run(exe, binf, "--clip-tips", "auto", "--simplify", "--edge-coverage", "--out", out))
    # the same flow through the Python binding: retain, (clip, simplify) until a round removes nothing, bubbles, simplify
    ctx = Context(0)
    m = HipDNAMap(ctx, K, 1 << 16)
    m.count_reads(rec.tobytes(), READS)
    m.deleteAll_lt(2)
    g = buildGraph(K, m)
    g.retainLargest()
    rounds = []
    while len(rounds) < 8:
        rounds.append(g.clipTips(m))
        if not rounds[-1]:
            break
        g.simplifyGraph()
    g.removeBubbles()
    g.simplifyGraph()
    assert stats["clip_tips"] == {"max_len": 2 * K, "removed": rounds}
    assert len(rounds) >= 2 and rounds[0] >= 10 and rounds[-1] == 0
    nodes, edges, length = g.counts()
    assert (stats["retained_nodes"], stats["retained_edges"], stats["retained_edges_length"]) == (nodes, edges, length)
    assert [line.split() for line in open(out + ".edges.txt").read().splitlines()] == [list(e) for e in g.canonical()[1]]
    # <prefix>.coverage.txt: edge id, len, kmers, sum, min, max per live edge, ids ascending.  Two builds of one table need not
    # number their edges alike, so the rows are compared without the id.
    rows = [[int(x) for x in line.split()] for line in open(out + ".coverage.txt").read().splitlines()]
    assert len(rows) == edges and all(len(r) == 6 for r in rows)
    assert [r[0] for r in rows] == sorted({r[0] for r in rows})
    c = g.edgeCoverage(m)
    live = c["kmers"] > 0
    want = sorted(zip((c["kmers"][live] - 1).tolist(), c["kmers"][live].tolist(), c["sum"][live].tolist(), c["min"][live].tolist(), c["max"][live].tolist()))
    assert sorted(tuple(r[1:]) for r in rows) == want and c["missing"] == 0
    assert all(r[2] == r[1] + 1 and r[4] <= r[5] and r[4] * r[2] <= r[3] <= r[5] * r[2] for r in rows)
    # the new flags do not run over N ranks
    res = subprocess.run([exe, binf, str(READS // 2), str(K), "--clip-tips", "--world", "2", "--rank", "0", "--id-file", str(tmp_path / "id")], capture_output=True)
    assert res.returncode == 2 and b"--clip-tips" in res.stderr
    g.close(); m.close(); ctx.close()


@pytest.mark.parametrize("name,flags", [("plain", []), ("simplify", ["--simplify"])])
def test_without_the_new_flags_every_output_is_the_parents(exe, reads, tmp_path, name, flags):
    rec, binf = reads
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "tips", "parent_hashes.json")))
    assert hashlib.sha256(rec.tobytes()).hexdigest() == golden["reads_sha256"]
    out = str(tmp_path / name)
    stdout = run(exe, binf, *flags, "--out", out)
    got = {"stdout": hashlib.sha256(stdout).hexdigest()}
    for ext in (".nodes.txt", ".edges.txt", ".contigs", ".dot"):
        got[ext] = hashlib.sha256(open(out + ext, "rb").read()).hexdigest()
    assert got == golden[name]
    assert not os.path.exists(out + ".coverage.txt")
