"""graph_simplifier --links --scaffolds --scaffold-fasta --fill-gaps (the C++ host side over genome.hpp) against the Python path on
the graph the tool itself saved (-m gpu); modelled on tests/test_scaffolds_host_gpu.py.  With the flag, the FASTA and the id list
are the Python path's over the filled chains and the JSON's "fill" object is its report; without it, both files and the JSON's
keys are what the Python path without fillGaps gives, as before this flag existed.  graph_builder --walk-pairs shares the stage:
it takes the flags and prints the same object."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import FILL_STATS, HipLinks, buildGraph, loadGraph, scaffoldChains, scaffoldGaps
from insert_cases import E2E, E2E_MAX_INSERT, E2E_SEED
from pairs_ref import make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(os.path.join(HOST, "graph_simplifier")) or not os.path.exists(os.path.join(HOST, "graph_builder")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return os.path.join(HOST, "graph_simplifier")


def id_list(path):
    """the --scaffolds file -> (chains, gaps); a cycle's closing gap is left out"""
    chains, gaps = [], []
    for line in open(path):
        if line.startswith("#"):
            continue
        f = line.split()
        if f[-1] == "cycle":
            f = f[:-2]
        assert f[0] == "s%d" % len(chains) and int(f[1]) == len(f[2::2])
        chains.append([int(x[1:]) for x in f[2::2]])
        gaps.append([int(x) for x in f[3::2]])
    return chains, gaps


def test_graph_simplifier_fill_gaps(exe, tmp_path):
    k = E2E["k"]
    reads = make_pairs(E2E_SEED, k, glen=E2E["glen"], nrep=E2E["nrep"], L=E2E["L"], npairs=E2E["npairs"], ins=(180, 250))
    binb = dna.reads_to_bin(reads)
    npairs, take, min_len, support = len(reads) // 2, 1400, 2 * k, 3
    binf, gfile = tmp_path / "reads.bin", tmp_path / "g.graph"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    base = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--take-first", str(take), "--range", "auto", "--max-insert", str(E2E_MAX_INSERT),
            "--links", str(tmp_path / "links.txt"), "--link-min-support", str(support), "--link-min-len", str(min_len)]
    texts = {}
    for name, extra in (("plain", []), ("auto", ["--fill-gaps"]), ("wide", ["--fill-gaps", "40", "--fill-max-edges", "8", "--fill-max-paths", "64"])):
        fa, ids, final = tmp_path / (name + ".fa"), tmp_path / (name + ".txt"), tmp_path / (name + ".graph")
        run = subprocess.run(base + ["--scaffolds", str(ids), "--scaffold-fasta", str(fa), "--save-graph", str(final)] + extra, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        got = json.loads(run.stdout)
        assert ("fill" in got) == bool(extra)
        if extra:
            assert list(got).index("fill") == list(got).index("links") + 1 == list(got).index("scaffolds") - 1
        else:
            keys_plain = list(got)
        assert [key for key in got if key != "fill"] == keys_plain
        lk = got["links"]
        # the Python path on the graph the tool saved
        g = loadGraph(ctx, final)
        vm, links = g.getGraphMap(), HipLinks(ctx)
        g.pairLinks(vm, PairedEndData(npairs, binb), links, min_len=min_len, max_span=lk["max_span"], take_first=take)
        joins, _ = links.joins(support)
        chains = scaffoldChains(joins[0], joins[1])
        gaps = scaffoldGaps(chains, joins, lk["mid"])
        assert len(chains) == lk["chains"] > 0
        if extra:
            rng = got["insert_range"]
            tol, me, mp = ((rng["hi"] - rng["lo"]) // 2, 16, 256) if name == "auto" else (40, 8, 64)
            chains, gaps, rep = g.fillGaps(chains, gaps, tol, max_edges=me, max_paths=mp)
            assert got["fill"] == dict({"tol": tol, "max_edges": me, "max_paths": mp}, **{n: rep[n] for n in FILL_STATS})
            assert list(got["fill"])[3:] == list(FILL_STATS) and rep["junctions"] > 0
        s = g.scaffolds(chains, gaps, min_len=min_len)
        texts[name] = fa.read_bytes()
        assert texts[name] == s.text() and got["scaffolds"] == s.stats()
        assert id_list(ids) == (chains, gaps)
        s.close(); links.close(); vm.close(); g.close()
    ctx.close()
    # the flag alone is refused, and says what it needs
    alone = subprocess.run(base + ["--fill-gaps"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 2 and "--fill-gaps goes with --scaffolds PATH or --scaffold-fasta PATH" in alone.stderr
    # graph_builder takes the same flags (its usage names them; the stage is the one tested above)
    usage = subprocess.run([os.path.join(HOST, "graph_builder")], capture_output=True, text=True, timeout=60)
    assert "--fill-gaps [TOL] [--fill-max-edges N] [--fill-max-paths N]" in usage.stderr + usage.stdout
