"""graph_simplifier --links --scaffolds (the C++ host side over genome.hpp) against the Python path and the restatement on the graph
the tool itself saved (-m gpu); modelled on tests/test_insert_host_gpu.py.  Ids are the final graph's: everything is compared by
content, an edge being its (start k-mer, first base)."""
import json
import os
import subprocess

import pytest

from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import HipLinks, buildGraph, loadGraph, scaffoldChains
from insert_cases import E2E, E2E_MAX_INSERT, E2E_SEED
from links_ref import chains, index_graph, joins, pair_links
from pairs_ref import make_pairs
from test_links_gpu import edge_keys
from thread_cases import device_graph as graph_by_id

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_simplifier")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


def gap(mid, count, sum_u):
    return mid - sum_u // count


def test_graph_simplifier_links_and_scaffolds(exe, tmp_path):
    k = E2E["k"]
    reads = make_pairs(E2E_SEED, k, glen=E2E["glen"], nrep=E2E["nrep"], L=E2E["L"], npairs=E2E["npairs"], ins=(180, 250))
    binb = dna.reads_to_bin(reads)
    npairs, take, min_len, support = len(reads) // 2, 1400, 2 * k, 3
    binf, gfile, final = tmp_path / "reads.bin", tmp_path / "g.graph", tmp_path / "final.graph"
    lfile, sfile = tmp_path / "links.txt", tmp_path / "scaffolds.txt"
    binf.write_bytes(binb)
    ctx = Context(0)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads))
    g = buildGraph(k, m)
    g.save(gfile)
    g.close(); m.close()
    cmd = [exe, str(gfile), str(binf), str(npairs), "--cutoff", "3", "--take-first", str(take), "--links", str(lfile), "--link-min-support", str(support),
           "--link-min-len", str(min_len), "--scaffolds", str(sfile), "--save-graph", str(final)]
    run = subprocess.run(cmd + ["--range", "auto", "--max-insert", str(E2E_MAX_INSERT)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout)
    est, lk = got["insert_range"], got["links"]
    assert est["estimated"] and (lk["mid"], lk["max_span"]) == (est["median"], est["hi"] + k)
    assert "links: max_span %d = %d + k, gap = %d - floor(sum_u / count): the median of the estimated insert range" % (est["hi"] + k, est["hi"], est["median"]) in run.stderr
    mid, max_span = lk["mid"], lk["max_span"]
    # the restatement and the Python path on the graph the tool saved
    g = loadGraph(ctx, final)
    keys = edge_keys(g)
    nodes, edges, okeys = graph_by_id(g)
    index, lens = index_graph(k, [(nodes[s], q) for s, _, q in edges], nodes=nodes)
    want_links, want_cls = pair_links(k, index, lens, reads, take, min_len, max_span)
    want_joins, want_st = joins(want_links, support)
    want_chains, want_cycles = chains([j[0] for j in want_joins], [j[1] for j in want_joins])
    assert want_cls["linked"] > 50 and want_st["joins"] > 0 and any(len(c) >= 2 for c in want_chains)
    vm, links = g.getGraphMap(), HipLinks(ctx)
    cls = g.pairLinks(vm, PairedEndData(npairs, binb), links, min_len=min_len, max_span=max_span, take_first=take)
    (e1, e2, cnt, su), st = links.joins(support)
    py_chains, py_cycles = scaffoldChains(e1, e2, with_cycles=True)
    assert cls == want_cls and st == want_st
    assert {name: lk[name] for name in cls} == cls and {name: lk[name] for name in st} == st
    assert (lk["chains"], lk["cycles"]) == (len(py_chains), py_cycles) == (len(want_chains), want_cycles)
    # --links: three header lines, then one line per link in ascending (e1, e2)
    text = lfile.read_text().splitlines()
    assert [ln[0] for ln in text[:3]] == ["#"] * 3 and text[2] == "# e1\te2\tcount\tsum_u\tgap" and not any(ln.startswith("#") for ln in text[3:])
    assert "min_len %d max_span %d mid %d;" % (min_len, max_span, mid) in text[1]
    rows = [tuple(int(x) for x in ln.split("\t")) for ln in text[3:]]
    assert [r[:2] for r in rows] == sorted(r[:2] for r in rows) and len(set(r[:2] for r in rows)) == len(rows)
    assert all(r[4] == gap(mid, r[2], r[3]) for r in rows)
    assert sorted(r[:4] for r in rows) == sorted(zip(*(a.tolist() for a in links.export())))
    assert {(keys[r[0]], keys[r[1]]): (r[2], r[3]) for r in rows} == {(okeys[e], okeys[f]): tuple(v) for (e, f), v in want_links.items()}
    # --scaffolds: three header lines, the second says both strands appear; chains by content with their gaps
    text = sfile.read_text().splitlines()
    assert [ln[0] for ln in text[:3]] == ["#"] * 3 and "both strands' chains appear" in text[1]
    gap_of = {(e, f): gap(mid, c, s) for e, f, c, s in zip(e1.tolist(), e2.tolist(), cnt.tolist(), su.tolist())}
    got_chains = []
    for i, ln in enumerate(text[3:]):
        f = ln.split("\t")
        cycle = f[-1] == "cycle"
        body = f[2:-1] if cycle else f[2:]
        members, gaps = [int(x[1:]) for x in body[0::2]], [int(x) for x in body[1::2]]
        assert f[0] == "s%d" % i and int(f[1]) == len(members) and all(x[0] == "e" for x in body[0::2])
        pairs = list(zip(members, members[1:] + members[:1])) if cycle else list(zip(members, members[1:]))
        assert gaps == [gap_of[p] for p in pairs]
        got_chains.append((members, cycle))
    assert [c for c, _ in got_chains] == py_chains and sum(cy for _, cy in got_chains) == py_cycles
    assert sorted([keys[e] for e in c] for c, _ in got_chains) == sorted([okeys[e] for e in c] for c in want_chains)
    links.close(); vm.close(); g.close(); ctx.close()
    # no estimate: the fallback range is named, mid = (180 + 250) div 2
    none = subprocess.run(cmd + ["--range", "auto", "--max-insert", "65535"], capture_output=True, text=True, timeout=120)
    assert none.returncode == 0, none.stderr
    lk = json.loads(none.stdout)["links"]
    assert (lk["mid"], lk["max_span"]) == (215, 250 + k)
    assert "links: max_span %d = 250 + k, gap = 215 - floor(sum_u / count): the middle of the fallback range (no estimate)" % (250 + k) in none.stderr
    # a given range
    given = subprocess.run(cmd + ["--range", "170", "261"], capture_output=True, text=True, timeout=120)
    assert given.returncode == 0, given.stderr
    lk = json.loads(given.stdout)["links"]
    assert (lk["mid"], lk["max_span"]) == (215, 261 + k) and "the middle of the given range" in given.stderr
