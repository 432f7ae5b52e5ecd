"""Graph edits in ANY order on the device, beside the model of tests/graph_model.py (-m gpu): eight operations per committed
(k, seed), drawn by the model; after every step the operation's return values and then every read-only observer are compared
with the model.  What is looked at is the state only another operation changes: the lazily built k-mer index after splits and
added nodes, out_order after removals, dead and sparse ids, pool holes, node copies, a loaded graph without spare capacity,
the epoch that makes a contigs plan stale.

Once a node copy has been made, out_order is compared as a set.  A k-mer may then name several nodes: nodeId must give the
smallest live id among them (the device's own node arrays say which) and out_order(k-mer) must be that node's out-edges, which
must be those of one of the model's copies; which copy has the smallest id is a matter of ids, not of content.  And the ORDER
simplifyGraph leaves is the order in which it visits the merged-away nodes: the oracle visits by id, which is ascending k-mer
until copies are appended behind every original; the device replays ascending k-mer throughout (gk_graph_ops.hip); the
reference iterates a hash map (include/genome_amd.h: "unspecified").  Before the first copy the order is the oracle's, exactly.
The coverage and contigs observers run after the steps that edited the graph or swapped the handle.
"""
import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph, loadGraph
from oracle import pyref as R
from pairs_ref import gpu_support_by_content

import graph_model as GM

pytestmark = pytest.mark.gpu
THREAD_READS, DISTANCE_PAIRS = 1500, 1000          # the head of the reads the two seeded observers look at


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


class Device:
    """the device side of one sequence: the graph, the count table of its context, and the contexts a reload opened"""

    def __init__(self, ctx, model, grid=0):
        self.base, self.ctx, self.model, self.grid = ctx, ctx, model, grid
        self.cap_uses = 0
        if grid:
            ctx.set_option("test_max_grid", grid)
        self.before = ctx.grid_cap_uses() if grid else 0
        self.m = self.table(ctx)
        self.g = buildGraph(model.k, self.m)

    def table(self, ctx):
        m = HipDNAMap(ctx, self.model.k)
        m.count_reads(self.model.bin, len(self.model.reads))
        m.deleteAll_lt(2)
        return m

    def leave(self, ctx):
        """done with a context: its launches under the cap are counted, the cap lifted (the module's) or the context closed"""
        if self.grid:
            self.cap_uses += ctx.grid_cap_uses() - (self.before if ctx is self.base else 0)
            ctx.set_option("test_max_grid", 0)
        if ctx is not self.base:
            ctx.close()

    def reload(self, path):
        """save, load into a FRESH context, close the old handle (and its table, and its context unless it is the module's)"""
        old, old_m, old_ctx = self.g, self.m, self.ctx
        fp, chk = old.idFingerprint(), old.checksum()
        old.save(path)
        c2 = Context(0)
        if self.grid:
            c2.set_option("test_max_grid", self.grid)
        h = loadGraph(c2, path)
        self.ctx, self.g = c2, h
        assert (h.idFingerprint(), h.checksum()) == (fp, chk)
        GM.same_graph(old, h)
        old.close(); old_m.close()
        self.leave(old_ctx)
        self.m = self.table(c2)

    def close(self):
        self.g.close(); self.m.close()
        self.leave(self.ctx)


def live_graph(g):
    """the device's own arrays by id -> (node id -> k-mer of the live nodes, nodesById of all ids, {(start k-mer, first base): edge id})"""
    nb, eb = g.idBounds()
    nodes = g.nodesById(np.arange(nb, dtype=np.uint32))
    kmer = {int(i): dna.unpack(int(nodes["lo"][i]), int(nodes["hi"][i]), g.k) for i in np.flatnonzero(nodes["alive"])}
    e = g.edgesById(np.arange(eb, dtype=np.uint32))
    by_key = {}
    for i in np.flatnonzero(e["alive"]):
        key = (kmer[int(e["start"][i])], dna.BASES[int(e["first"][i])])
        assert key not in by_key, "two live edges share a start k-mer and a first base"
        by_key[key] = int(i)
    return kmer, nodes, by_key


def observe(dev, model, edited):
    g, k = dev.g, model.k
    want_nodes, want_edges = model.content()
    nodes, edges = g.canonical()
    assert sorted(nodes) == want_nodes, "canonical(): nodes"
    assert sorted(edges) == want_edges, "canonical(): edges"
    assert g.counts() == model.expect_counts(), "counts()"
    kmer, info, by_key = live_graph(g)
    assert len(by_key) == len(edges)
    # nodeId: every live node is found, the smallest live id of its k-mer; k-mers that are not nodes are not
    smallest = {}
    for i, s in kmer.items():
        smallest[s] = min(i, smallest.get(s, i))
    assert sorted(smallest) == sorted(set(want_nodes))
    for s, i in smallest.items():
        assert g.nodeId(s)[0] == i, f"nodeId({s}): not the smallest live id {i}"
    for s in model.absent_kmers():
        assert g.nodeId(s) == (None, None) and g.nodeId(R.rev_comp(s)) == (None, None), f"nodeId({s}) of no node"
    # out_order: the oracle's, while no node copy was ever made; from then on the out-edges of the node nodeId names (the module's text)
    out_bases = model.expect_out_bases()
    for s, i in smallest.items():
        got = g.out_order(s)
        if not model.copies:
            assert got == model.expect_out_order(s), f"out_order({s})"
        else:
            mine = "".join(sorted(b for (t, b), e in by_key.items() if t == s and g.nodeId(s, b)[1] == e))
            assert got is not None and "".join(sorted(dna.BASES[b] for b in got)) == mine and mine in out_bases[s], f"out_order({s}) with copies"
    # nodesById: degrees
    degrees = {}
    for i, s in kmer.items():
        degrees.setdefault(s, []).append((int(info["in_deg"][i]), int(info["out_deg"][i])))
    assert {s: sorted(v) for s, v in degrees.items()} == model.expect_degrees(), "nodesById(): degrees"
    cn, cl = g.componentStats()
    assert sorted(zip(cn.tolist(), cl.tolist())) == model.components()[0], "componentStats()"
    for c in (0, 2 * k):
        assert g.contigStats(c) == model.expect_contig_stats(c), f"contigStats({c})"
    if edited:
        ids = [by_key[(s, q[0])] for s, _e, q in edges]
        want, missing = model.expect_coverage(edges)
        got = g.edgeCoverage(dev.m, ids)
        assert list(zip(got["kmers"].tolist(), got["sum"].tolist(), got["min"].tolist(), got["max"].tolist())) == want, "edgeCoverage()"
        assert got["missing"] == missing
        plan = g.contigs(dev.m, strands=1)
        assert plan.text() == model.expect_contigs(edges, ids), "contigs().text()"
        plan.close()
    return by_key


def observe_reads(dev, model):
    """threadReads and pairDistances of the head of the reads, through a position map of the graph as it is now"""
    g, k = dev.g, model.k
    vm, sup = g.getGraphMap(), Support(dev.ctx)
    head = model.reads[:THREAD_READS]
    st = g.threadReads(vm, sup, (dna.reads_to_bin(head), len(head)))
    want_sup, want = model.expect_thread(head)
    assert st == want, "threadReads(): stats"
    assert gpu_support_by_content(g, k, sup) == want_sup, "threadReads(): support"
    hist, cls = g.pairDistances(vm, (model.bin, model.npairs), bins=GM.BINS, take_first=DISTANCE_PAIRS)
    want_hist, want_cls = model.expect_pair_distances(DISTANCE_PAIRS)
    assert (hist.tolist(), cls) == (want_hist, want_cls), "pairDistances()"
    sup.close(); vm.close()


def apply(dev, model, op, out, by_key, path):
    """the device's side of one step: the calls, and their return values against `out`, the model's"""
    g, k = dev.g, model.k
    if op == "simplify":
        g.simplifyGraph()
    elif op == "bubbles":
        g.removeBubbles()
    elif op == "clip":
        assert g.clipTips(dev.m, out["max_len"]) == out["removed"], "clipTips()"
    elif op == "pop":
        assert g.popBubbles(dev.m, out["max_len"], out["max_diff"]) == (out["removed"], out["compared"]), "popBubbles()"
    elif op == "remove_kmer":
        assert g.removeEdges(out["edges"]) == out["removed"], "removeEdges()"
    elif op == "remove_id":
        assert g.removeEdgesById([by_key[e] for e in out["edges"]]) == out["removed"], "removeEdgesById()"
    elif op == "retain":
        assert g.retainLargest() == (out["kept"], out["components"]), "retainLargest()"
    elif op == "reload":
        dev.reload(path)
    elif op == "split":
        vm, sup = g.getGraphMap(), Support(dev.ctx)
        g.walkPairs(vm, sup, model.bin, model.npairs, *model.rng)
        assert sup.sizes()[1:] == (out["bad"], out["walked"]), "walkPairs(): bad pairs, orientations walked"
        assert gpu_support_by_content(g, k, sup) == out["support"], "walkPairs(): support"
        assert g.splitBySupport(sup, GM.CUTOFF) == (out["removed"], out["new_nodes"]), "splitBySupport()"
        g.simplifyGraph()                                   # (the oracle's split ends with it, GraphSimplifier.scala:318)
        sup.close(); vm.close()
    elif op == "addnode":
        s, b = out["kmer"], out["out_base"]
        old, edge = g.nodeId(s, b)
        new = g.addNode(s)
        assert old is not None and edge is not None and new not in (None, old)
        g.replaceStart(edge, new)
        if out["in_edge"]:
            _, edge = g.nodeId(*out["in_edge"])
            g.replaceEnd(edge, new)
    else:
        raise AssertionError(op)


def run_sequence(ctx, tmp_path, k, seed, grid=0):
    model = GM.GraphModel(k, seed)
    dev = Device(ctx, model, grid)
    step, op = "build", None
    try:
        by_key = observe(dev, model, True)
        reads_at = GM.observer_steps(seed)
        for step in range(GM.STEPS):
            op = model.draw()
            plan = dev.g.contigs(dev.m, strands=1)
            out = model.step(op)
            if op == "reload":                              # (no edit: the old handle goes, and its plans before it)
                plan.close()
            if not out.get("skip"):
                apply(dev, model, op, out, by_key, tmp_path / f"step{step}.gkg")
            if out["effective"] and op != "reload":         # a plan made before an edit is refused
                with pytest.raises(L.GkError) as err:
                    plan.text()
                assert err.value.code == L.GK_E_STATE, "a contigs plan from before the step"
            plan.close()
            by_key = observe(dev, model, out["effective"])
            if step in reads_at:
                observe_reads(dev, model)
        return model, dev
    except Exception as e:
        done = " ".join(h[0] for h in model.history)
        raise AssertionError(f"k={k} seed={seed} step {step} ({op}) after [{done}]: {type(e).__name__}: {e}") from e
    finally:
        dev.close()


@pytest.mark.parametrize("k,seed", GM.SEQUENCES)
def test_sequence(ctx, tmp_path, k, seed):
    run_sequence(ctx, tmp_path, k, seed)


def test_sequence_under_a_grid_of_two_workgroups(ctx, tmp_path):
    """one committed sequence with every graph launch capped at two workgroups: the grid-stride paths on edited graphs"""
    k, seed = GM.SMALL_GRID
    _model, dev = run_sequence(ctx, tmp_path, k, seed, grid=2)
    assert dev.cap_uses > 0, "no launch consulted test_max_grid"
