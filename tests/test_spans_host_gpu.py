"""--resolve-repeats on the C++ tools (genome.hpp's Spans, Graph::threadSpans and Graph::splitEdgesBySpans through tool_common.hpp's
paired-end stage) against the Python path on the same graph file and reads (-m gpu); modelled on tests/test_thread_host_gpu.py.
The input is the end-to-end case of tests/test_spans_gpu.py: the genome A R B R C with r = k + 60 and error-free 150-base reads at
step 1."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context
from genome_amd.graph import SPAN_STATS, SPLIT_EDGE_STATS, HipSpans, loadGraph
from oracle import pyref as R
from test_spans_gpu import live_paths, pieces, strands
from thread_cases import build_graph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, SIMPLIFIER = os.path.join(HOST, "graph_builder"), os.path.join(HOST, "graph_simplifier")
K, CUTOFF = 35, 3


@pytest.fixture(scope="module")
def tools():
    if not (os.path.exists(BUILDER) and os.path.exists(SIMPLIFIER)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])


@pytest.fixture(scope="module")
def case():
    """-> (the genome, its reads as an even number of records: the tools take pairs)"""
    A, Rp, B, C = pieces(K, K, [300, K + 60, 280, 310], lambda A, Rp, B, C: [A + Rp + B + Rp + C])
    gen = A + Rp + B + Rp + C
    reads = [gen[i:i + 150] for i in range(len(gen) - 150 + 1)]
    return gen, reads + reads[:len(reads) % 2]


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def check_counters(rounds, nreads):
    for x in rounds:
        ts, se = x["thread_spans"], x["split_edges"]
        assert tuple(ts) == SPAN_STATS and tuple(se) == SPLIT_EDGE_STATS
        assert ts["records"] == nreads and ts["crossings"] == ts["spans"] + ts["interrupted"] + ts["open"]
        assert se["candidates"] == se["resolved"] + se["unequal"] + se["ambiguous"] + se["unsupported"]
    assert all(x["split_edges"]["resolved"] > 0 for x in rounds[:-1])               # a round that resolves nothing is the last


def test_graph_simplifier_no_pairs_resolve_repeats_writes_the_python_path_s_contigs(tools, case, tmp_path):
    gen, reads = case
    binb, npairs = dna.reads_to_bin(reads), len(reads) // 2
    binf, gfile = tmp_path / "reads.bin", tmp_path / "g.gkg"
    binf.write_bytes(binb)
    ctx = Context(0)
    g = build_graph(ctx, K, reads)
    g.simplifyGraph()
    assert len(live_paths(g)) == 8                                                 # the tangle: four edges per strand
    g.save(gfile)
    g.close()
    # the Python path, call by call: the stage without walks or threaded reads gathers no support and runs no split by it (an
    # empty support would remove every edge at a branching node), then the rounds
    g = loadGraph(ctx, gfile)
    g.simplifyGraph()
    want_rounds = []
    for _ in range(3):
        vm, sp = g.getGraphMap(), HipSpans(ctx)
        ts = g.threadSpans(vm, sp, binb, len(reads))
        se = g.splitEdgesBySpans(sp, CUTOFF)
        sp.close(); vm.close()
        want_rounds.append({"thread_spans": ts, "split_edges": se})
        if not se["resolved"]:
            break
        g.simplifyGraph()
    assert [x["split_edges"]["resolved"] for x in want_rounds] == [2, 0]
    assert live_paths(g) == strands([gen])
    c = g.contigs()
    want_text, want_stats, want_counts = c.text(), c.stats(), g.counts()
    c.close(); g.close(); ctx.close()
    assert want_stats["records"] == 1
    # the tool: one round by default, CUTOFF = --cutoff's value
    js, err = run([SIMPLIFIER, gfile, binf, npairs, "--cutoff", CUTOFF, "--no-pairs", "--resolve-repeats", "--contigs", tmp_path / "one.fa"])
    assert js["resolve_repeats"] == {"cutoff": CUTOFF, "rounds": want_rounds[:1]}
    assert (tmp_path / "one.fa").read_bytes() == want_text and js["contigs_fasta"] == want_stats
    assert (js["simplified_nodes"], js["simplified_edges"], js["simplified_edges_length"]) == want_counts
    assert err.count("resolve-repeats round ") == 1 and "resolve-repeats round 1 (cutoff 3)" in err
    check_counters(js["resolve_repeats"]["rounds"], len(reads))
    # up to three rounds, the cutoff given: the second resolves nothing and is the last
    js, err = run([SIMPLIFIER, gfile, binf, npairs, "--cutoff", 1, "--no-pairs", "--resolve-repeats", CUTOFF, "--resolve-rounds", 3, "--contigs", tmp_path / "three.fa"])
    assert js["resolve_repeats"] == {"cutoff": CUTOFF, "rounds": want_rounds} and err.count("resolve-repeats round ") == 2
    check_counters(js["resolve_repeats"]["rounds"], len(reads))
    assert (tmp_path / "three.fa").read_bytes() == want_text
    # behind --thread-reads' split as well; without the option the JSON has no new key
    js, err = run([SIMPLIFIER, gfile, binf, npairs, "--cutoff", CUTOFF, "--no-pairs", "--thread-reads", "--resolve-repeats"])
    assert "thread_reads" in js and len(js["resolve_repeats"]["rounds"]) == 1
    check_counters(js["resolve_repeats"]["rounds"], len(reads))
    js, err = run([SIMPLIFIER, gfile, binf, npairs, "--cutoff", CUTOFF, "--no-pairs", "--thread-reads"])
    assert "resolve_repeats" not in js and "resolve-repeats" not in err


def test_graph_builder_walk_pairs_resolve_repeats_prints_the_counters(tools, case, tmp_path):
    gen, _ = case
    # real pairs: 150-base mates from the two ends of every 220-base fragment, the second as the reverse complement
    reads = [m for i in range(len(gen) - 220 + 1) for m in (gen[i:i + 150], R.rev_comp(gen[i + 70:i + 220]))]
    binf = tmp_path / "reads.bin"
    binf.write_bytes(dna.reads_to_bin(reads))
    js, err = run([BUILDER, binf, len(reads) // 2, K, "--rounds", 1, "--no-retain", "--walk-pairs", CUTOFF, 180, 250, "--resolve-repeats", "--resolve-rounds", 2])
    rr = js["resolve_repeats"]
    assert rr["cutoff"] == CUTOFF and 1 <= len(rr["rounds"]) <= 2 and err.count("resolve-repeats round ") == len(rr["rounds"])
    check_counters(rr["rounds"], len(reads))
    assert js["walk_pairs"]["orientations_walked"] > 0
    assert list(js).index("walk_pairs") + 1 == list(js).index("resolve_repeats")
