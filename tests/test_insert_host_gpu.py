"""graph_simplifier --range auto (the C++ host side over genome.hpp) against the Python path on the same graph file and pairs
(-m gpu); modelled on tests/test_spectrum_host_gpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from genome_amd import dna
from genome_amd.dist import HipDist, unique_id
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import buildGraph, insertRange, loadGraph
from insert_cases import E2E, E2E_MAX_INSERT, E2E_SEED
from pairs_ref import make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_simplifier")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


def test_graph_simplifier_range_auto(exe, tmp_path):
    k = E2E["k"]
    reads = make_pairs(E2E_SEED, k, glen=E2E["glen"], nrep=E2E["nrep"], L=E2E["L"], npairs=E2E["npairs"], ins=(180, 250))
    binb = dna.reads_to_bin(reads)
    npairs, take = len(reads) // 2, 1400
    binf, gfile, hfile = tmp_path / "reads.bin", tmp_path / "g.graph", tmp_path / "insert.txt"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    # the Python path: the histogram itself, then the whole stage
    g = loadGraph(ctx, gfile)
    vm = g.getGraphMap()
    hist, classes = g.pairDistances(vm, PairedEndData(npairs, binb), bins=E2E_MAX_INSERT + 1, take_first=take)
    lo, hi, median = insertRange(hist)
    vm.close(); g.close()
    hd = HipDist(ctx, 0, 1, unique_id())
    gp, sp = simplify_graph(hd, gfile, PairedEndData(npairs, binb), 3, lo="auto", take_first=take, max_insert=E2E_MAX_INSERT)
    assert (sp["walk_pairs"]["insert_range"]["lo"], sp["walk_pairs"]["insert_range"]["hi"]) == (lo, hi)
    gp.close(); hd.close(); ctx.close()
    # the tool
    cmd = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--take-first", str(take)]
    run = subprocess.run(cmd + ["--range", "auto", "--max-insert", str(E2E_MAX_INSERT), "--insert-hist", str(hfile)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    est = got["insert_range"]
    assert (est["lo"], est["hi"], est["median"], est["estimated"]) == (lo, hi, median, True)
    assert est["classes"] == classes and est["observations"] == classes["counted"] and est["max_insert"] == E2E_MAX_INSERT
    assert "insert range %d to %d, median %d" % (lo, hi, median) in run.stderr
    assert got["walk_pairs"] == {key: v for key, v in sp["walk_pairs"].items() if key != "insert_range"}
    lines = [tuple(int(x) for x in ln.split()) for ln in hfile.read_text().splitlines()]
    assert lines == [(d, int(c)) for d, c in enumerate(hist) if c]
    # the same range given as numbers: the same stage, and the JSON keys of a run without the new flags
    plain = subprocess.run(cmd + ["--range", str(lo), str(hi)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    want = json.loads(plain.stdout)
    assert "insert_range" not in want and {key: v for key, v in got.items() if key != "insert_range"} == want
    # no estimate: --max-insert beyond every edge's length leaves no observation; the fallback is named
    none = subprocess.run(cmd + ["--range", "auto", "--max-insert", "65535"], capture_output=True, text=True, timeout=120)
    assert none.returncode == 0, none.stderr
    est = json.loads(none.stdout)["insert_range"]
    assert (est["lo"], est["hi"], est["median"], est["estimated"], est["observations"]) == (180, 250, None, False, 0)
    assert "falling back to the reference's 180 to 250" in none.stderr
