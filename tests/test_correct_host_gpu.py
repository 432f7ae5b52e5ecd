"""The host tools over gk_reads_correct (-m gpu): `correct_reads` against HipDNAMap.correct_reads on the same file, and
`graph_builder --correct auto` against the Python mirror of its flow (count, correct, count again, filter, build); modelled on
tests/test_spectrum_host_gpu.py."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import CORRECT_STATS, Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData, extractFilteredKmers
from genome_amd.graph import buildGraph, loadGraph
from spectrum_ref import genome_reads

import correct_ref as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
BUILDER, CORRECT = os.path.join(HOST, "graph_builder"), os.path.join(HOST, "correct_reads")
K = 21


@pytest.fixture(scope="module")
def tools():
    if not (os.path.exists(BUILDER) and os.path.exists(CORRECT)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return BUILDER, CORRECT


@pytest.fixture(scope="module")
def reads():
    return genome_reads(20262)


def test_correct_reads_tool_equals_the_python_call(tools, reads, tmp_path):
    binb = dna.reads_to_bin(reads)
    binf, outf, spec = tmp_path / "reads.bin", tmp_path / "fixed.bin", tmp_path / "spectrum.tsv"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, K, 0)
    occ = m.count_reads(binb, len(reads))
    want, st = m.correct_reads(binb, len(reads), "auto")
    want4, st4 = m.correct_reads(binb, len(reads), 4)
    m.close(); ctx.close()
    assert st["solid_auto"] is True and st["corrected"] > 0 and want != binb

    res = subprocess.run([tools[1], str(binf), str(len(reads)), str(K), "--out", str(outf), "--spectrum", str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = json.loads(res.stdout)
    assert outf.read_bytes() == want
    assert (got["k"], got["occurrences"], got["solid"], got["solid_auto"], got["valley"], got["peak"]) == (K, occ, st["solid"], True, st["valley"], st["peak"])
    assert {n: got[n] for n in CORRECT_STATS} == {n: st[n] for n in CORRECT_STATS}
    assert spec.read_text().startswith("1\t")
    res = subprocess.run([tools[1], str(binf), str(len(reads)), str(K), "--solid", "4", "--out", str(outf)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = json.loads(res.stdout)
    assert outf.read_bytes() == want4 and (got["solid"], got["solid_auto"]) == (4, False)
    assert {n: got[n] for n in CORRECT_STATS} == {n: st4[n] for n in CORRECT_STATS}
    # usage errors: no --out, solid = 0
    assert subprocess.run([tools[1], str(binf), str(len(reads)), str(K)], capture_output=True).returncode == 2
    assert subprocess.run([tools[1], str(binf), str(len(reads)), str(K), "--out", str(outf), "--solid", "0"], capture_output=True).returncode == 2


def test_graph_builder_correct_auto_equals_the_python_flow(tools, reads, tmp_path):
    binb = dna.reads_to_bin(reads)
    binf, gfile = tmp_path / "reads.bin", tmp_path / "graph.gk"
    binf.write_bytes(binb)
    # the restatement's own property first: a recount of the corrected reads holds strictly fewer weak k-mers
    ctx = Context(0)
    m = HipDNAMap(ctx, K, 0)
    m.count_reads(binb, len(reads))
    fixed, st = m.correct_reads(binb, len(reads), "auto")
    solid = st["solid"]
    hist_before = m.spectrum()["hist"]
    counts = X.count_reads(reads, K)
    fixed_ref, st_ref = X.correct(counts, reads, K, solid)
    assert dna.reads_to_bin(fixed_ref) == fixed
    weak_ref = (sum(1 for v in counts.values() if v < solid), sum(1 for v in X.count_reads(fixed_ref, K).values() if v < solid))
    assert weak_ref[1] < weak_ref[0]
    # the Python mirror of the flow: clear, count the corrected stream, rounds from its spectrum, build
    m.clear()
    m.count_reads(fixed, len(reads))
    hist_after = m.spectrum()["hist"]
    assert (int(hist_before[1:solid].sum()), int(hist_after[1:solid].sum())) == weak_ref
    m.close()
    m2 = extractFilteredKmers(PairedEndData(len(reads) // 2, fixed), K, "auto", ctx)
    good = m2.size()
    g = buildGraph(K, m2)
    want_counts, want_sum = g.counts(), g.checksum()
    g.close()

    args = [tools[0], str(binf), str(len(reads) // 2), str(K), "--no-retain", "--rounds", "auto"]
    res = subprocess.run(args + ["--correct", "auto", "--save-graph", str(gfile)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout)
    assert out["correct"] == dict({n: st[n] for n in CORRECT_STATS}, solid=solid, solid_auto=True)
    assert (out["rounds"], out["good_kmers"]) == (m2.auto["rounds"], good)
    assert (out["graph_nodes"], out["graph_edges"], out["total_edges_length"]) == tuple(want_counts)
    loaded = loadGraph(ctx, str(gfile))
    assert loaded.checksum() == want_sum
    loaded.close(); m2.close()
    # a number instead of auto; without the flag no "correct" object; with --world a usage error
    res = subprocess.run(args + ["--correct", str(solid)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    num = json.loads(res.stdout)
    assert num["correct"] == dict(out["correct"], solid_auto=False) and num["good_kmers"] == good
    res = subprocess.run(args, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "correct" not in json.loads(res.stdout)
    res = subprocess.run(args + ["--correct", "auto", "--world", "1", "--rank", "0", "--id-file", str(tmp_path / "id")], capture_output=True, text=True)
    assert res.returncode == 2
    ctx.close()
