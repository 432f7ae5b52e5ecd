"""Every temporary device buffer of a call goes back to the context's pool, on success and on the host-side failure that
happens while large temporaries exist (gk_graph_component_stats with too small a buffer).  -m gpu.

The pool counts blocks of 1 MiB and more (Context.mem_stats: "live", "peak"), so the graph has at least 2^18 node slots and
2^18 edges: a 4-byte-per-id array is then a counted block.  Reads of 40 random bases at k = 31 are, with overwhelming
probability, isolated unitigs with two terminal k-mers each; the test asserts the sizes it relies on.

A read-only call must leave "live" where it was, and "peak" must have risen by 1 MiB or more in between: the counter saw the
call's temporaries, so the first assertion is not vacuous.  gk_graph_checksum is the exception to the second: its only
scratch is two 64-bit words, which the pool does not count at any graph size — its peak must not move at all."""
import ctypes as C
import gc

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph

pytestmark = pytest.mark.gpu
MIB = 1 << 20
K, READ_LEN, READS = 31, 40, 300_000


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def test_every_call_returns_its_temporaries(ctx):
    gc.collect()
    live0 = ctx.mem_stats()["live"]
    rec = synth.reads_mode_u(READS, READ_LEN, config_id=8)
    m = HipDNAMap(ctx, K, READS * (READ_LEN - K + 1))
    assert m.count_reads(rec.tobytes(), READS) == READS * (READ_LEN - K + 1)
    g = buildGraph(K, m)
    node_bound, edge_bound = g.idBounds()
    nodes, edges, _ = g.counts()
    print("id bounds", node_bound, edge_bound, "live", nodes, edges)
    assert node_bound >= 1 << 18 and edge_bound >= 1 << 18 and nodes >= 1 << 18 and edges >= 1 << 18
    live1 = ctx.mem_stats()["live"]
    assert live1 > live0

    node_ids, edge_ids = np.arange(node_bound, dtype=np.uint32), np.arange(edge_bound, dtype=np.uint32)
    kept = {}
    calls = [("getNodes", g.getNodes, True), ("getEdges", g.getEdges, True), ("componentStats", g.componentStats, True),
             ("checksum", g.checksum, False),           # (16 bytes of scratch: nothing the pool counts)
             ("nodesById", lambda: g.nodesById(node_ids), True), ("edgesById", lambda: g.edgesById(edge_ids), True)]
    for name, call, big in calls:
        ctx.mem_stats(reset_peak=True)
        kept[name] = call()
        st = ctx.mem_stats()
        print(name, "peak - live1", st["peak"] - live1, "live - live1", st["live"] - live1)
        if big:
            assert st["peak"] - live1 >= MIB, name
        else:
            assert st["peak"] == live1, name
        assert st["live"] == live1, name

    # the one host-side failure behind large temporaries: the components are labelled, the caller's buffer is too small
    ncomp = C.c_uint64()
    one32, one64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    ctx.mem_stats(reset_peak=True)
    rc = L.lib().gk_graph_component_stats(g.h, L.ptr(one32, C.c_uint32), L.ptr(one64, C.c_uint64), 1, C.byref(ncomp))
    st = ctx.mem_stats()
    print("component_stats(cap = 1)", rc, ncomp.value, "peak - live1", st["peak"] - live1)
    assert rc == L.GK_E_CAPACITY and ncomp.value == len(kept["componentStats"][0]) > 1
    assert st["peak"] - live1 >= MIB
    assert st["live"] == live1

    # the mutating calls may change what the graph holds; each must succeed
    eb = kept["edgesById"]
    sel = np.flatnonzero(eb["alive"])[:1 << 17]
    assert len(sel) == 1 << 17
    start = g.nodesById(eb["start"][sel])
    lo, hi, first = np.ascontiguousarray(start["lo"]), np.ascontiguousarray(start["hi"]), np.ascontiguousarray(eb["first"][sel])
    removed = C.c_uint64()
    L.check(L.lib().gk_graph_remove_edges(g.h, L.ptr(lo, C.c_uint64), L.ptr(hi, C.c_uint64), L.ptr(first, C.c_uint8), len(sel), C.byref(removed)), ctx.h)
    assert 0 < removed.value <= len(sel)
    g.removeBubbles()
    g.simplifyGraph()
    vm = g.getGraphMap()
    g.retainLargest()

    vm.close()
    g.close()
    m.close()
    assert ctx.mem_stats()["live"] == live0
