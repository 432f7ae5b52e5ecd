"""graph_builder --gfa, graph_simplifier --gfa and check_graph --twins (the C++ tools): the GFA file a tool writes must be, byte for
byte, what HipGraph.gfa gives for the graph the same run saved (ids survive the graph file), its "gfa" JSON the nine stats, and
check_graph's "twins" the six stats of HipGraph.edgeTwins.  --gfa with --world is refused.  -m gpu."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import loadGraph
from test_checkgraph_gpu import make_genome, tiled_reads
from test_gfa_cpu import check_gfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, SIMPLIFIER, CHECK = (os.path.join(HOST, x) for x in ("graph_builder", "graph_simplifier", "check_graph"))


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def test_tools_write_what_the_python_api_gives(tmp_path):
    k = 31
    genome = make_genome(7, 3000)
    reads = tiled_reads(genome)
    bin_ = dna.reads_to_bin(reads)
    (tmp_path / "r.bin").write_bytes(bin_)
    (tmp_path / "ref.fa").write_text(">ref\n" + genome + "\n")
    js, _ = run([BUILDER, tmp_path / "r.bin", len(reads) // 2, k, "--rounds", 1, "--no-retain", "--save-graph", tmp_path / "g.gkg", "--gfa", tmp_path / "b.gfa"])
    c = Context(0)
    m = HipDNAMap(c, k)
    m.count_reads(bin_, len(reads))
    graph = loadGraph(c, tmp_path / "g.gkg")
    want = graph.gfa(m)
    text = (tmp_path / "b.gfa").read_bytes()
    assert text == want.text() and js["gfa"] == want.stats() and not os.path.exists(str(tmp_path / "b.gfa") + ".tmp")
    assert js["gfa"]["segments"] >= 3 and js["gfa"]["missing_windows"] == 0 and text.count(b"\tKC:i:") == js["gfa"]["segments"]
    assert js["gfa"]["live_edges"] == js["retained_edges"]
    check_gfa(text, k, want_kc=True)
    want.close()
    # check_graph --twins of the saved graph
    js, err = run([CHECK, tmp_path / "g.gkg", tmp_path / "ref.fa", "--twins"])
    st = graph.edgeTwins()[2]
    assert js["twins"] == st and st["missing"] == 0 and st["live_edges"] == st["paired"] + st["self"]
    assert "twins: live_edges %d paired %d self %d missing 0 ambiguous 0 key_collisions 0\n" % (st["live_edges"], st["paired"], st["self"]) in err
    assert "twins" not in run([CHECK, tmp_path / "g.gkg", tmp_path / "ref.fa"])[0]
    # graph_simplifier: no count table, so no KC tag; the graph it saved is the graph it wrote
    js, _ = run([SIMPLIFIER, tmp_path / "g.gkg", tmp_path / "r.bin", len(reads) // 2, "--cutoff", 1, "--thread-reads", "--no-pairs",
                 "--save-graph", tmp_path / "s.gkg", "--gfa", tmp_path / "s.gfa"])
    simplified = loadGraph(c, tmp_path / "s.gkg")
    want = simplified.gfa()
    text = (tmp_path / "s.gfa").read_bytes()
    assert text == want.text() and js["gfa"] == want.stats() and b"KC:i:" not in text
    assert js["gfa"]["live_edges"] == js["simplified_edges"] > 0
    check_gfa(text, k, want_kc=False)
    want.close(); simplified.close(); graph.close(); m.close(); c.close()
    # an unwritable path is the tool's error, and leaves nothing
    r = subprocess.run([BUILDER, str(tmp_path / "r.bin"), str(len(reads) // 2), str(k), "--rounds", "1", "--gfa", str(tmp_path / "none" / "x.gfa")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "x.gfa" in r.stderr and not (tmp_path / "none").exists()


@pytest.mark.parametrize("tool, args", [(BUILDER, ["r.bin", "10", "31"]), (SIMPLIFIER, ["g.gkg", "r.bin", "10", "--cutoff", "2"])])
def test_gfa_with_world_is_refused(tool, args):
    r = subprocess.run([tool] + args + ["--gfa", "x.gfa", "--world", "2", "--rank", "0", "--id-file", "id"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr == "--gfa runs on one GPU only (not with --world): write it from the saved graph\n"
