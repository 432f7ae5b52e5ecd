"""The graph file between GraphBuilder and GraphSimplifier (gk_graph_save / gk_graph_load, include/genome_amd.h version 1;
MapGraph.write / Graph(file), Graph.scala:232-261, 384-390; the load's checks after GraphSimplifier.scala:157-169).  -m gpu.

A loaded graph must be the saved one id for id: counts, id bounds, checksums, id fingerprint, every id's node and edge record
and every node's out-edge order; saving is deterministic; a corrupt file is refused with GK_E_FORMAT and leaves nothing
allocated.  The two-stage flow (graph_builder --save-graph, graph_simplifier; dist_pipeline.simplify_graph over N ranks) must
give what the one-process flow gives."""
import ctypes as C
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist import HipDist, unique_id
from genome_amd.dist_pipeline import simplify_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData
from genome_amd.graph import Support, buildGraph, loadGraph
from genome_amd.partitioned import PartitionedDNAMap
from graph_model import same_graph
from test_dist_bin_gpu import json_line, ragged_pairs, run_world
from test_pairs_gpu import gpu_canonical, gpu_support_by_content, make_pairs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILDER = os.path.join(ROOT, "genome_amd", "host", "graph_builder")
SIMPLIFIER = os.path.join(ROOT, "genome_amd", "host", "graph_simplifier")
GOLDEN_GRAPHS = ["g_k11_p1", "g_k21_p3", "g_k31_p1", "g_k35_p2", "g_k63_p1", "snp_k11_p2", "snp_k35_p1"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def golden_graph(ctx, name):
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    k, P = fx["k"], fx["P"]
    m = PartitionedDNAMap(ctx, k, P) if P > 1 else HipDNAMap(ctx, k)
    m.count_reads(bytes.fromhex(fx["bin_hex"]), fx["nreads"])
    m.deleteAll_lt(fx["rounds"])
    g = buildGraph(k, m)
    m.close()
    return fx, g


def layout(k, nn, ne, pool):
    """byte offsets of the version-1 arrays (include/genome_amd.h)"""
    al8 = lambda v: (v + 7) & ~7
    o = {"ids": 128}
    o["lo"] = al8(128 + 4 * nn)
    o["hi"] = o["lo"] + 8 * nn if k >= 34 else None
    o["order"] = o["lo"] + (16 if k >= 34 else 8) * nn
    o["eid"] = al8(o["order"] + 4 * nn)
    o["est"] = al8(o["eid"] + 4 * ne)
    o["een"] = al8(o["est"] + 4 * ne)
    o["elen"] = al8(o["een"] + 4 * ne)
    o["pool"] = o["elen"] + 8 * ne
    o["end"] = o["pool"] + pool
    return o


def header(b):
    k = struct.unpack_from("<I", b, 12)[0]
    nb, eb, nn, ne, pool = struct.unpack_from("<5Q", b, 16)
    return k, nb, eb, nn, ne, pool


def round_trip(g, tmp_path, name="g.gkg"):
    """save, load into a FRESH context, check, and check that saves are byte-stable -> (loaded graph, its context, bytes)"""
    p = tmp_path / name
    g.save(p)
    data = p.read_bytes()
    g.save(tmp_path / (name + ".2"))
    assert (tmp_path / (name + ".2")).read_bytes() == data
    assert not os.path.exists(str(p) + ".tmp")
    c2 = Context(0)
    h = loadGraph(c2, p)
    same_graph(g, h)
    h.save(tmp_path / (name + ".3"))
    assert (tmp_path / (name + ".3")).read_bytes() == data
    k, nb, eb, nn, ne, pool = header(data)
    assert (k, nb, eb) == (g.k, *g.idBounds()) and (nn, ne) == g.counts()[:2]
    assert len(data) == layout(k, nn, ne, pool)["end"]
    return h, c2, data


@pytest.mark.parametrize("name", GOLDEN_GRAPHS)
def test_round_trip_golden(ctx, tmp_path, name):
    fx, g = golden_graph(ctx, name)
    h, c2, _ = round_trip(g, tmp_path)
    for x in (g, h):
        x.removeBubbles()
        x.simplifyGraph()
    assert g.canonical() == h.canonical()
    assert [list(e) for e in h.canonical()[1]] == fx["edges_after_simplify"]
    h.close(); c2.close(); g.close()


def test_graph_states_round_trip(ctx, tmp_path):
    fx, g = golden_graph(ctx, "g_k21_p3")
    g.retainLargest()                                   # sparse ids
    h, c2, _ = round_trip(g, tmp_path, "retained.gkg"); h.close(); c2.close()
    g.removeBubbles(); g.simplifyGraph()                # pool holes, merged long edges
    h, c2, _ = round_trip(g, tmp_path, "simplified.gkg"); h.close(); c2.close()
    g.close()
    # after a node split: nodes that share a k-mer (node_lookup gives the smallest id)
    k = 21
    reads = make_pairs(1, k)
    binb = dna.reads_to_bin(reads)
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(k, m)
    vm, sup = g.getGraphMap(), Support(ctx)
    g.walkPairs(vm, sup, binb, len(reads) // 2, 60, 95)
    rm, nn = g.splitBySupport(sup, 3)
    assert nn > 0
    h, c2, _ = round_trip(g, tmp_path, "split.gkg")
    g.simplifyGraph(); h.simplifyGraph()
    assert g.checksum() == h.checksum() and g.idFingerprint() == h.idFingerprint()
    h.close(); c2.close(); sup.close(); vm.close(); g.close(); m.close()
    # an empty graph (a perfect cycle alone, Graph.scala:375), then one linear component beside it
    rnd = random.Random(5)
    k = 15
    circ = "".join(rnd.choice("AGCT") for _ in range(120))
    lin = "".join(rnd.choice("AGCT") for _ in range(200))
    cc = circ + circ[:60]
    reads = [cc[i:i + 50] for i in range(0, 121)] * 2
    m = HipDNAMap(ctx, k)
    b = dna.reads_to_bin(reads)
    m.count_reads(b, len(reads))
    g = buildGraph(k, m)
    assert g.counts() == (0, 0, 0)
    h, c2, data = round_trip(g, tmp_path, "empty.gkg")
    assert len(data) == 128 and h.counts() == (0, 0, 0)
    h.close(); c2.close(); g.close()
    reads2 = [lin[i:i + 50] for i in range(0, 151)] * 2
    b2 = dna.reads_to_bin(reads2)
    m.count_reads(b2, len(reads2))
    g = buildGraph(k, m)
    assert g.counts()[0] == 4
    h, c2, _ = round_trip(g, tmp_path, "cycle_and_linear.gkg")
    h.close(); c2.close(); g.close(); m.close()


@pytest.mark.parametrize("k,seed,rng", [(21, 1, (60, 95)), (35, 4, (50, 80)), (63, 7, (180, 250))])
def test_pairs_stage_on_a_loaded_graph(ctx, tmp_path, k, seed, rng):
    # (the row at the reference's range: 150-base mates with 0.5 % errors over an 8 kbp genome, walk distances inside 180..250)
    fx = dict(glen=8000, nrep=4, L=150, npairs=6000, err=0.005, ins=(k + 185, k + 245)) if rng == (180, 250) else {}
    reads = make_pairs(seed, k, **fx)
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(k, m)
    g.save(tmp_path / "g.gkg")
    c2 = Context(0)
    h = loadGraph(c2, tmp_path / "g.gkg")
    # What the file promises is the SAVED ids: the loaded graph's fingerprint before anything is edited, the support by id, and
    # the ids after the split (new nodes are numbered by a host pass in id order).  simplifyGraph numbers the merged edges with an
    # atomic cursor in the order its lanes arrive: the ids it leaves are reproducible only while one wave does all the chains
    # (the two small rows, whose fingerprint after it stays compared); the large row compares content there.
    ids_after_simplify = rng != (180, 250)
    out = []
    for x, c in ((g, ctx), (h, c2)):
        fp_loaded = x.idFingerprint()
        vm, sup = x.getGraphMap(), Support(c)
        x.walkPairs(vm, sup, binb, npairs, *rng)
        e1, e2, cnt = sup.items()
        order = np.lexsort((e2, e1))
        items = (e1[order].tolist(), e2[order].tolist(), cnt[order].tolist())
        by_content = gpu_support_by_content(x, k, sup)
        split = x.splitBySupport(sup, 3)
        fp_split = x.idFingerprint()
        x.simplifyGraph()
        out.append((items, sup.sizes(), by_content, split, x.checksum(), x.idFingerprint() if ids_after_simplify else x.counts(), gpu_canonical(x),
                    fp_loaded, fp_split))
        sup.close(); vm.close()
    assert out[0] == out[1]
    assert len(out[0][0][0]) > 0 and out[0][3][1] > 0
    h.close(); c2.close(); g.close(); m.close()


@pytest.mark.parametrize("name", ["g_k11_p1", "g_k35_p2"])
def test_committed_fixtures_load(ctx, name):
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    path = os.path.join(GOLDEN, "graph_v1_k%d.gkg" % fx["k"])
    g = loadGraph(ctx, path)
    assert g.k == fx["k"]
    nodes, edges = g.canonical()
    assert nodes == fx["nodes"]
    assert [list(e) for e in edges] == fx["edges"]
    # the fixture is what this library writes for that graph today
    _, built = golden_graph(ctx, name)
    assert built.checksum() == g.checksum()
    g.close(); built.close()


def _load_rc(ctx, path):
    h = L.vp()
    rc = L.lib().gk_graph_load(ctx.h, os.fsencode(str(path)), C.byref(h))
    return rc, h.value


def _corrupt_cases(data):
    k, nb, eb, nn, ne, pool = header(data)
    o = layout(k, nn, ne, pool)
    u32 = lambda off, j: struct.unpack_from("<I", data, off + 4 * j)[0]
    lens = [struct.unpack_from("<Q", data, o["elen"] + 8 * j)[0] for j in range(ne)]
    poff = np.concatenate([[0], np.cumsum([(x + 3) // 4 for x in lens])]).astype(int)
    ids = [u32(o["ids"], j) for j in range(nn)]
    cases = {}

    def patch(name, fn):
        b = bytearray(data)
        fn(b)
        cases[name] = bytes(b)

    patch("bad_magic", lambda b: b.__setitem__(0, ord("X")))
    patch("version_2", lambda b: struct.pack_into("<I", b, 8, 2))
    patch("k_32", lambda b: struct.pack_into("<I", b, 12, 32))
    for sec in ("ids", "lo", "hi", "order", "eid", "est", "een", "elen", "pool"):
        if o[sec] is not None:
            cases["truncated_at_" + sec] = data[:o[sec]]
    cases["truncated_in_header"] = data[:64]
    cases["truncated_mid_pool"] = data[:o["pool"] + pool // 2]
    cases["trailing_bytes"] = data + b"\0"
    patch("node_id_beyond_bound", lambda b: struct.pack_into("<I", b, o["ids"] + 4 * (nn - 1), nb))
    patch("node_ids_not_ascending", lambda b: (struct.pack_into("<I", b, o["ids"], ids[1]), struct.pack_into("<I", b, o["ids"] + 4, ids[0])))
    dead = sorted(set(range(nb)) - set(ids))
    patch("edge_to_absent_node", lambda b: struct.pack_into("<I", b, o["een"], dead[0] if dead else nb))
    firsts = [data[o["pool"] + poff[j]] & 3 for j in range(ne)]
    starts = [u32(o["est"], j) for j in range(ne)]
    j1, j2 = next((a, b_) for a in range(ne) for b_ in range(ne) if firsts[a] == firsts[b_] and starts[a] != starts[b_])
    patch("two_edges_same_start_and_base", lambda b: struct.pack_into("<I", b, o["est"] + 4 * j2, starts[j1]))
    jn = next(j for j in range(nn) if u32(o["order"], j) & 7)
    patch("out_order_disagrees", lambda b: struct.pack_into("<I", b, o["order"] + 4 * jn, 0))
    patch("zero_length_edge", lambda b: struct.pack_into("<Q", b, o["elen"], 0))
    jp = next(j for j in range(ne) if lens[j] & 3)
    patch("padding_bits", lambda b: b.__setitem__(o["pool"] + poff[jp + 1] - 1, b[o["pool"] + poff[jp + 1] - 1] | 0xC0))
    jl = int(np.argmax(lens))
    mid = lens[jl] // 2
    patch("flipped_base", lambda b: b.__setitem__(o["pool"] + poff[jl] + mid // 4, b[o["pool"] + poff[jl] + mid // 4] ^ (1 << (2 * (mid % 4)))))
    patch("wrong_checksum", lambda b: b.__setitem__(60, b[60] ^ 1))
    return cases


@pytest.mark.parametrize("name", ["g_k11_p1", "g_k35_p2"])
def test_corrupt_files_are_refused(ctx, tmp_path, name):
    _, g = golden_graph(ctx, name)
    g.retainLargest()
    good = tmp_path / "good.gkg"
    g.save(good)
    data = good.read_bytes()
    g.close()
    before = ctx.mem_stats()["live"]
    rc, h = _load_rc(ctx, good)
    assert rc == L.GK_OK and h
    L.lib().gk_graph_destroy(h)
    cases = _corrupt_cases(data)
    assert len(cases) >= 20
    for case, blob in cases.items():
        p = tmp_path / (case + ".gkg")
        p.write_bytes(blob)
        rc, h = _load_rc(ctx, p)
        assert rc == L.GK_E_FORMAT, (case, rc, L.lib().gk_last_error(ctx.h))
        assert h is None, case
        assert ctx.mem_stats()["live"] == before, case
    rc, h = _load_rc(ctx, tmp_path / "no_such_file.gkg")
    assert rc == L.GK_E_INVALID and h is None
    assert b"No such file" in L.lib().gk_last_error(ctx.h)
    with pytest.raises(L.GkError) as ei:
        loadGraph(ctx, tmp_path / "bad_magic.gkg")
    assert ei.value.code == L.GK_E_FORMAT


def test_save_into_a_missing_directory_leaves_nothing(ctx, tmp_path):
    _, g = golden_graph(ctx, "g_k11_p1")
    target = tmp_path / "missing" / "g.gkg"
    rc = L.lib().gk_graph_save(g.h, os.fsencode(str(target)))
    assert rc == L.GK_E_INVALID
    assert not target.exists() and not os.path.exists(str(target) + ".tmp") and not (tmp_path / "missing").exists()
    g.close()


def test_cli_two_stages_match_one_process(tmp_path):
    for exe in (BUILDER, SIMPLIFIER):
        if not os.path.exists(exe):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    k = 21
    reads = make_pairs(11, k)
    binf = tmp_path / "reads.bin"
    binf.write_bytes(dna.reads_to_bin(reads))
    npairs = str(len(reads) // 2)
    common = [BUILDER, str(binf), npairs, str(k), "--rounds", "2", "--simplify"]
    r1 = subprocess.run(common + ["--save-graph", str(tmp_path / "g.gkg")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    r2 = subprocess.run([SIMPLIFIER, str(tmp_path / "g.gkg"), str(binf), npairs, "--cutoff", "3", "--range", "60", "95", "--out", str(tmp_path / "a"),
                         "--save-graph", str(tmp_path / "s.gkg")], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    r3 = subprocess.run(common + ["--walk-pairs", "3", "60", "95", "--out", str(tmp_path / "b")], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stderr
    a, b = json_line(r2.stdout), json_line(r3.stdout)
    assert a["k"] == k and a["walk_pairs"] == b["walk_pairs"] and a["walk_pairs"]["orientations_walked"] > 0
    assert (a["simplified_nodes"], a["simplified_edges"], a["simplified_edges_length"]) == (b["retained_nodes"], b["retained_edges"], b["retained_edges_length"])
    for ext in (".nodes.txt", ".edges.txt"):
        assert sorted(open(str(tmp_path / "a") + ext).read().splitlines()) == sorted(open(str(tmp_path / "b") + ext).read().splitlines())
    c = Context(0)
    g = loadGraph(c, tmp_path / "s.gkg")
    assert g.counts() == (a["simplified_nodes"], a["simplified_edges"], a["simplified_edges_length"])
    g.close(); c.close()
    # world 1 over RCCL
    r4 = subprocess.run([SIMPLIFIER, str(tmp_path / "g.gkg"), str(binf), npairs, "--cutoff", "3", "--range", "60", "95", "--world", "1", "--rank", "0",
                         "--id-file", str(tmp_path / "id")], capture_output=True, text=True, timeout=300)
    assert r4.returncode == 0, r4.stderr
    d = json_line(r4.stdout)
    assert d["world"] == 1 and d["walk_pairs"] == a["walk_pairs"]


@pytest.mark.parametrize("world", [2, 3])
def test_simplify_graph_over_ranks_is_the_one_rank_result(tmp_path, world):
    k = 21
    reads = ragged_pairs(world + 40, k)
    binb = dna.reads_to_bin(reads)
    npairs, take = len(reads) // 2, len(reads) // 2 - 29
    data = PairedEndData(npairs, binb)
    c = Context(0)
    m = HipDNAMap(c, k)
    m.count_reads(binb, len(reads)); m.deleteAll_lt(2)
    g = buildGraph(k, m)
    g.retainLargest(); g.removeBubbles(); g.simplifyGraph()
    path = tmp_path / "g.gkg"
    g.save(path)
    g.close(); m.close()
    hd = HipDist(c, 0, 1, unique_id())
    try:
        g1, want = simplify_graph(hd, path, data, 3, 60, 95, take_first=take)
        want_sum, want_canon = g1.checksum(), gpu_canonical(g1)
        g1.close()
    finally:
        hd.close(); c.close()
    assert want["walk_pairs"]["orientations_walked"] > 0 and want["walk_pairs"]["supported_edge_pairs"] > 0

    def body(rank, c, hd):
        g, stats = simplify_graph(hd, path, data, 3, 60, 95, take_first=take)
        res = stats, g.checksum(), gpu_canonical(g)
        g.close()
        return res

    out = run_world(world, body)
    for stats, csum, canon in out:
        assert stats["world"] == world
        assert {x: v for x, v in stats.items() if x != "world"} == {x: v for x, v in want.items() if x != "world"}
        assert csum == want_sum and canon == want_canon
