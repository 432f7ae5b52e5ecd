"""graph_builder --rounds auto --spectrum FILE (the C++ host side over genome.hpp) against the Python flow and the oracle's
spectrum on the same input (-m gpu); modelled on tests/test_host_cpp_gpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from genome_amd import dna
from genome_amd.dnamap import Context
from genome_amd.freqfilter import PairedEndData, extractFilteredKmers
from genome_amd.graph import buildGraph
from oracle import oracle as O
from spectrum_ref import cutoff_of, genome_reads, spectrum_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_builder")
K = 21
# the JSON line of a run without the two new flags: its keys as they were before the flags existed
PLAIN_KEYS = ["k", "rounds", "good_kmers", "graph_nodes", "graph_edges", "total_edges_length", "components", "max_component_size",
              "retained_nodes", "retained_edges", "retained_edges_length", "components_histogram", "components_histogram_2"]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


def _parse_spectrum(path, bins):
    h = np.zeros(bins, np.uint64)
    for line in open(path).read().splitlines():
        c, n = line.split("\t")
        if c.startswith(">="):
            assert int(c[2:]) == bins - 1
            h[bins - 1] = int(n)
        else:
            assert 1 <= int(c) <= bins - 2 and int(n) > 0
            h[int(c)] = int(n)
    return h


def test_graph_builder_rounds_auto_and_spectrum_file(exe, tmp_path):
    reads = genome_reads(20261)
    binb = dna.reads_to_bin(reads)
    binf = tmp_path / "reads.bin"
    binf.write_bytes(binb)
    ref = O.PMap(K, 1)
    ref.count_reads(binb, len(reads))
    counts = ref.export_sorted()[2].astype(np.int64)
    ref.close()
    want_hist = spectrum_of(counts, 4096)
    valley, peak, gsize = cutoff_of(want_hist)
    # the Python flow
    ctx = Context(0)
    m = extractFilteredKmers(PairedEndData(len(reads) // 2, binb), K, "auto", ctx)
    good = m.size()
    g = buildGraph(K, m)
    nodes, edges, total = g.counts()
    assert (m.auto["valley"], m.auto["peak"], m.auto["genome_size_estimate"]) == (valley, peak, gsize)
    g.close(); m.close(); ctx.close()

    args = [exe, str(binf), str(len(reads) // 2), str(K), "--no-retain"]
    spec = tmp_path / "spectrum.tsv"
    res = subprocess.run(args + ["--rounds", "auto", "--spectrum", str(spec)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    st = json.loads(res.stdout)
    assert (st["rounds"], st["rounds_auto"], st["valley"], st["peak"], st["genome_size_estimate"]) == (valley, True, valley, peak, gsize)
    assert (st["good_kmers"], st["graph_nodes"], st["graph_edges"], st["total_edges_length"]) == (good, nodes, edges, total)
    assert np.array_equal(_parse_spectrum(spec, 4096), want_hist)
    assert not any(line.startswith(">=") for line in open(spec))                # nothing was seen 4095 times
    # --rounds auto alone: the same choice; behind the pre-filter (min_count = 2) too
    for extra in ([], ["--prefilter", str(len(counts))]):
        res = subprocess.run(args + ["--rounds", "auto"] + extra, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert json.loads(res.stdout) == st
    # --spectrum with a number: the number is used, the spectrum and what it suggests are reported
    res = subprocess.run(args + ["--rounds", "3", "--spectrum", str(tmp_path / "s3.tsv")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    st3 = json.loads(res.stdout)
    assert (st3["rounds"], st3["rounds_auto"], st3["valley"], st3["peak"]) == (3, False, valley, peak)
    assert st3["good_kmers"] == int((counts >= 3).sum())
    assert open(tmp_path / "s3.tsv").read() == open(spec).read()
    # without the two flags the JSON line has exactly the keys it had
    res = subprocess.run(args + ["--rounds", "3"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    plain = json.loads(res.stdout)
    assert list(plain) == PLAIN_KEYS
    assert plain == {key: st3[key] for key in PLAIN_KEYS}
    # a number is a number, as before the flags existed: --rounds 0 removes nothing
    res = subprocess.run(args + ["--rounds", "0"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    zero = json.loads(res.stdout)
    assert list(zero) == PLAIN_KEYS and (zero["rounds"], zero["good_kmers"]) == (0, len(counts))


def test_graph_builder_rounds_auto_without_a_valley(exe, tmp_path):
    """a spectrum that never rises (540 singletons, 180 keys seen twice, 180 seen three times): the reference's 3, and the
    output says the cutoff was not chosen from the spectrum"""
    import random
    rnd = random.Random(9)
    reads = ["".join(rnd.choice("AGCT") for _ in range(120)) for _ in range(10)]
    reads = reads + reads[:4] + reads[:2]
    binf = tmp_path / "reads.bin"
    binf.write_bytes(dna.reads_to_bin(reads))
    res = subprocess.run([exe, str(binf), "8", "31", "--no-retain", "--rounds", "auto"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    st = json.loads(res.stdout)
    assert (st["rounds"], st["rounds_auto"], st["valley"], st["peak"], st["genome_size_estimate"], st["good_kmers"]) == (3, False, 0, 0, 0, 180)
