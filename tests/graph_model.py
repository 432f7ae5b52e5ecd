"""A model that follows a device graph through graph edits in ANY order: the oracle's stateful graph (oracle.Graph) for the
reference's operations, the restatements under tests/ (tips_ref, bubbles_ref, components_ref, ...) for this project's own rules,
composed on graph CONTENT, the (start k-mer, end k-mer, seq) lists HipGraph.canonical() gives.  No device here: a method per
operation changes the model only and returns what the device must report; the `expect_*` methods give what the read-only
observers must see.  tests/test_graph_sequences_cpu.py runs the committed sequences through the model alone (the inputs are not
degenerate), tests/test_graph_sequences_gpu.py runs the device beside it, step by step.

Node copies.  Once a node split (pairs+split, add node) has made nodes that share a k-mer, the restatements that identify a node
by its k-mer do not apply: the model no longer DRAWS clip, pop and remove-by-k-mer (nothing is skipped for it), and it answers the
by-node questions (degrees, components, read threading) from the oracle's graph by id (by_id()).

Two things the model cannot do, and says so:
  * oracle.Graph.split_by_support ends with simplifyGraph (GraphSimplifier.scala:318), so the device's pairs+split step calls
    simplifyGraph too, and a simplify that follows pairs+split (with or without a reload between) never has work left.
  * at k = 64 the 40-base mates of pairs_ref.make_pairs hold no k-mer: shape() lengthens mates and inserts there.
"""
import random
from collections import Counter

import numpy as np

import bubbles_ref as B
import checkgraph_ref as CG
import components_ref as CR
import contigs_ref as FA
import insert_ref as IR
import thread_ref as TR
import tips_ref as T
from genome_amd import dna, synth
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import make_pairs, oracle_support_by_content

STEPS = 8
OPS = ("simplify", "bubbles", "clip", "pop", "remove_kmer", "remove_id", "retain", "reload", "split", "addnode")
BY_KMER_ONLY = ("clip", "pop", "remove_kmer")          # the restatement (or the call itself) names a node by its k-mer
CUTOFF = 3                                             # genome.cutoff of the split, as tests/test_pairs_gpu.py
BINS = 256                                             # pairDistances: above every insert shape() gives


def same_graph(a, b):
    """b is a, id for id"""
    assert a.k == b.k
    assert a.counts() == b.counts()
    assert a.idBounds() == b.idBounds()
    assert a.checksum() == b.checksum()
    assert a.idFingerprint() == b.idFingerprint()
    nb, eb = a.idBounds()
    na, nb_ = a.nodesById(np.arange(nb)), b.nodesById(np.arange(nb))
    assert np.array_equal(na["alive"], nb_["alive"])
    live = na["alive"]
    for key in ("lo", "hi", "in_deg", "out_deg"):
        assert np.array_equal(na[key][live], nb_[key][live]), key
    ea, eb_ = a.edgesById(np.arange(eb)), b.edgesById(np.arange(eb))
    assert np.array_equal(ea["alive"], eb_["alive"])
    live = ea["alive"]
    for key in ("start", "end", "len", "first"):
        assert np.array_equal(ea[key][live], eb_[key][live]), key
    for lo, hi in zip(na["lo"][na["alive"]], na["hi"][na["alive"]]):
        kmer = dna.unpack(int(lo), int(hi), a.k)
        assert a.out_order(kmer) == b.out_order(kmer)
        assert a.nodeId(kmer) == b.nodeId(kmer)


# ---- the input ---------------------------------------------------------------------------------------------------------------
def shape(k):
    """-> (mate length, (insert lo, hi), (walk range lo, hi)): make_pairs' defaults while a 40-base mate holds a few k-mers"""
    if k + 5 <= 40:
        L, ins = 40, (80, 100)
    else:
        L, ins = k + 20, (k + 60, k + 80)
    return L, ins, (ins[0] - k + 1, ins[1] - k + 16)


def genome_of(seed, k, glen=2400, nrep=3):
    """the genome make_pairs(seed, k) draws its fragments from: the same random numbers in the same order"""
    rnd = random.Random(seed)
    g = [rnd.choice("AGCT") for _ in range(glen)]
    for _ in range(nrep):
        a = rnd.randrange(100, glen // 2 - 100)
        b = rnd.randrange(glen // 2 + 100, glen - 100)
        g[b:b + k] = g[a:a + k]
    return "".join(g)


def make_input(seed, k, snp_pairs=150):
    """make_pairs(seed, k, err=0.004) and, behind it, error-free pairs of a second haplotype that differs in two planted SNPs
    (fragments that hold the SNP): a two-edge bubble each, for removeBubbles and popBubbles -> reads [mate 1, mate 2, ...]"""
    L, ins, _ = shape(k)
    reads = make_pairs(seed, k, err=0.004) if L == 40 else make_pairs(seed, k, err=0.004, L=L, ins=ins)
    g = genome_of(seed, k)
    assert sum(r in g or R.rev_comp(r) in g for r in reads[:200]) > 100          # it IS that genome (most mates are error-free)
    rnd = random.Random(seed * 7919 + k)
    for p in (rnd.randrange(300, 1000), rnd.randrange(1400, 2100)):
        hap = g[:p] + rnd.choice([c for c in "AGCT" if c != g[p]]) + g[p + 1:]
        for _ in range(snp_pairs):
            n = rnd.randint(*ins)
            s = rnd.choice((rnd.randrange(p - L + 1, p + 1), rnd.randrange(p - n + 1, p - n + L + 1)))     # the SNP in mate 1 or 2
            frag = hap[s:s + n]
            if rnd.random() < 0.5:
                frag = R.rev_comp(frag)
            reads += [frag[:L], R.rev_comp(frag)[:L]]
    return reads


def export_edges(og):
    """the oracle's live edges in ITS export order: (start k-mer, first base, edge id) ascending"""
    k, e = og.k, og.edges()
    out = []
    for i in range(len(e["len"])):
        seq = synth.bases_to_str(e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        out.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k), dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k), seq))
    return out


def twin(edge):
    s, _e, q = edge
    k, rpath = len(s), R.rev_comp(s + q)
    return rpath[:k], rpath[len(q):], rpath[k:]


def components_by_id(nodes, edges):
    """nodes: [node key]; edges: [(start key, end key, seq)] -> [(node count, summed length of the edges starting in it, members)]"""
    parent = {n: n for n in nodes}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, _q in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    members, length = {}, {}
    for n in nodes:
        members.setdefault(find(n), []).append(n)
    for a, _b, q in edges:
        length[find(a)] = length.get(find(a), 0) + len(q)
    return [(len(ms), length.get(r, 0), ms) for r, ms in members.items()]


class GraphModel:
    """One graph: the oracle handle, the count table as the dict tips_ref takes, the paired reads; see the module's text."""

    def __init__(self, k, seed):
        self.k, self.seed = k, seed
        self.reads = make_input(seed, k)
        self.bin = dna.reads_to_bin(self.reads)
        self.npairs = len(self.reads) // 2
        self.rng = shape(k)[2]
        ref = O.PMap(k, 1)
        ref.count_reads(self.bin, len(self.reads))
        ref.delete_lt(2)
        lo, hi, cnt = ref.export_sorted()
        self.counts = {dna.unpack(int(a), int(b), k): int(c) for a, b, c in zip(lo, hi, cnt)}
        self.og = O.Graph(ref)
        self.draws = random.Random(seed)            # the operations and their choices
        self.copies = False                         # some k-mer may be shared by several nodes
        self.one_strand = False                     # a retain broke a tie: the content is no longer strand-closed
        self.history = []                           # [(operation, effective, skipped)]
        self._content = self._ids = None
        self._cov = {}

    # ---- the state ------------------------------------------------------------------------------------------------------------
    def _edited(self):
        self._content = self._ids = None

    def content(self):
        """(sorted node k-mers, sorted edges): what gpu_canonical(g) must equal"""
        if self._content is None:
            nlo, nhi = self.og.nodes()
            self._content = (sorted(dna.unpack(int(a), int(b), self.k) for a, b in zip(nlo, nhi)), sorted(export_edges(self.og)))
        return self._content

    def by_id(self):
        """the oracle's live graph with ITS ids -> (nodes [(id, k-mer)] ascending, edges [(id, start id, end id, seq)])"""
        if self._ids is None:
            og, k = self.og, self.k
            lo, hi, is_edge, ident, _dist = og.graph_map_calls()
            nodes = [(int(ident[i]), dna.unpack(int(lo[i]), int(hi[i]), k)) for i in np.flatnonzero(is_edge == 0)]
            kmer = dict(nodes)
            live, e = [], 1
            while True:
                info = og.edge_info(e)
                if info["start"] == 0:              # node ids start at 1: nothing was written, e is beyond the last edge
                    break
                if info["alive"]:
                    live.append((CR.kmer_key(kmer[info["start"]]), info["first"], e, info))
                e += 1
            live.sort(key=lambda x: x[:3])           # gk_oracle.c's export order
            exported = export_edges(og)
            assert len(live) == len(exported)
            edges = []
            for (_key, first, e, info), (s, t, q) in zip(live, exported):
                assert (kmer[info["start"]], kmer[info["end"]], info["len"], dna.BASES[first]) == (s, t, len(q), q[0])
                edges.append((e, info["start"], info["end"], q))
            self._ids = nodes, edges
        return self._ids

    def has_copies(self):
        nodes = self.content()[0]
        return len(set(nodes)) < len(nodes)

    # ---- drawing the next operation --------------------------------------------------------------------------------------------
    def draw(self):
        """the next operation, by the model's own random numbers: with copies about, none that names a node by its k-mer; two
        times in three one of the orders the tools never use (the issue's list), otherwise any"""
        allowed = [op for op in OPS if not (self.copies and op in BY_KMER_ONLY)]
        prev = [h[0] for h in self.history[-2:]]
        follow = {"simplify": ["clip", "pop"], "retain": ["simplify", "reload"], "remove_id": ["retain"], "split": ["retain", "reload"],
                  "clip": ["split"], "addnode": ["split"], "reload": ["addnode"]}.get(prev[-1] if prev else None, [])
        if prev == ["retain", "reload"]:
            follow = ["clip"]
        if prev == ["split", "reload"]:
            follow = ["simplify"]
        follow = [op for op in follow if op in allowed]
        if follow and self.draws.random() < 2 / 3:
            return self.draws.choice(follow)
        return self.draws.choice(allowed)

    # ---- the operations: each changes the model and returns what the device must report ------------------------------------------
    def step(self, op):
        """-> dict: "skip" (the step is left out on both sides), the operation's arguments and expected return values"""
        before = self.content()
        out = getattr(self, "_op_" + op)()
        self._edited()
        skipped = bool(out.get("skip"))
        effective = not skipped and (op == "reload" or self.content() != before)
        out["effective"] = effective
        self.history.append((op, effective, skipped))
        return out

    def _remove(self, edges):
        for s, _e, q in edges:
            assert self.og.remove_edge(*dna.pack(s), dna.BASES.index(q[0]))

    def _op_simplify(self):
        self.og.simplify()
        return {}

    def _op_bubbles(self):
        self.og.remove_bubbles()
        return {}

    def _op_clip(self):
        assert not self.copies
        edges = self.content()[1]
        max_len = self.draws.choice((self.k, 2 * self.k))
        gone = [edges[i] for i in sorted(T.tips(self.counts, edges, max_len))]
        self._remove(gone)
        return {"max_len": max_len, "removed": len(gone)}

    def _op_pop(self):
        assert not self.copies
        edges = self.content()[1]
        max_diff = self.draws.choice((1, 3))
        idx, compared = B.pop(self.counts, edges, 2 * self.k, max_diff)
        self._remove([edges[i] for i in sorted(idx)])
        return {"max_len": 2 * self.k, "max_diff": max_diff, "removed": len(idx), "compared": compared}

    def _reachable(self, edge):
        """the oracle's remove_edge(start k-mer, base) names THIS edge (always, without copies)"""
        s, _e, q = edge
        node = self.og.find_node(*dna.pack(s))
        return bool(node and self.og.find_out_edge(node, dna.BASES.index(q[0])))

    def _choose_edges(self):
        """a seeded choice of live edges with their reverse-complement twins -> edges, each once"""
        edges = self.content()[1]
        keys = Counter((s, q[0]) for s, _e, q in edges)
        pool = [e for e in edges if keys[(e[0], e[2][0])] == 1 and (not self.copies or self._reachable(e))]
        chosen = []
        for e in self.draws.sample(pool, min(len(pool), self.draws.randint(1, 3))):
            for x in (e, twin(e)):
                if x in pool and x not in chosen:
                    chosen.append(x)
        return chosen

    def _op_remove_kmer(self):
        assert not self.copies
        chosen = self._choose_edges()
        self._remove(chosen)
        return {"edges": [(s, q[0]) for s, _e, q in chosen], "removed": len(chosen)}

    def _op_remove_id(self):
        chosen = self._choose_edges()
        self._remove(chosen)
        return {"edges": [(s, q[0]) for s, _e, q in chosen], "removed": len(chosen)}

    def components(self):
        """[(node count, length)] sorted, and the number of components tied for largest"""
        nodes, edges = self.content()
        if self.has_copies():
            ids, eids = self.by_id()
            comps = components_by_id([i for i, _s in ids], [(a, b, q) for _e, a, b, q in eids])
        else:
            comps = components_by_id(nodes, edges)
            assert sorted(c[:2] for c in comps) == CR.stats(nodes, edges)
        best = max((c[0] for c in comps), default=0)
        return sorted(c[:2] for c in comps), sum(1 for c in comps if c[0] == best)

    def _op_retain(self):
        stats, tied = self.components()
        by_kmer = not self.has_copies()              # components_ref applies: hold the oracle to it as well
        if tied != 1 and self.copies:                # the oracle breaks a tie by node id: the smallest k-mer only while ids are in
            return {"skip": "tie"}                   # k-mer order, which the ids of copies are not (the device goes by k-mer)
        if by_kmer:
            assert tied == len(CR.tied_for_largest(*self.content()))
            want = CR.retained(*self.content())
        comps = self.og.num_components()
        kept = self.og.retain_largest()
        assert (kept, comps) == (max(c[0] for c in stats), len(stats))
        if by_kmer:
            self._edited()
            assert (sorted(want[0]), sorted(want[1])) == self.content()
        self.one_strand = self.one_strand or tied != 1     # of a strand-closed graph's twin components one is kept
        return {"kept": kept, "components": comps}

    def _op_reload(self):
        return {}

    def _op_split(self):
        osup = O.Support()
        walked = self.og.walk_pairs(osup, self.bin, self.npairs, *self.rng)
        out = {"walked": walked, "bad": osup.bad_pairs(), "support": oracle_support_by_content(self.og, self.k, osup)}
        out["removed"], out["new_nodes"] = self.og.split_by_support(osup, CUTOFF)          # (ends with simplifyGraph, :318)
        self.copies = self.copies or out["new_nodes"] > 0
        osup.close()
        return out

    def _op_addnode(self):
        """a copy of a live node takes over its first out-edge (by base) and, if it has one, an in-edge from another node: the
        node split of GraphSimplifier.scala:296-309 by hand, as tests/test_vmap_gpu.py does on a fresh graph"""
        nodes, edges = self.content()
        once = {s for s, c in Counter(nodes).items() if c == 1}                   # named by k-mer on both sides: no copies of it
        outs, ins = {}, {}
        for e in edges:
            outs.setdefault(e[0], []).append(e)
            if e[0] != e[1] and e[0] in once:
                ins.setdefault(e[1], []).append(e)
        for want_out, want_in in ((2, True), (1, True), (1, False)):
            cand = sorted(s for s in once if len(outs.get(s, [])) >= want_out and (s in ins or not want_in))
            if cand:
                break
        else:
            return {"skip": "no node with an out-edge"}
        s = self.draws.choice(cand)
        og = self.og
        oid = og.find_node(*dna.pack(s))
        new = og.add_node(*dna.pack(s))
        first = min(outs[s], key=lambda e: dna.BASES.index(e[2][0]))
        og.replace_start(og.find_out_edge(oid, dna.BASES.index(first[2][0])), new)
        out = {"kmer": s, "out_base": first[2][0], "in_edge": None}
        if s in ins:
            a, _s, q = ins[s][0]
            ae = og.find_out_edge(og.find_node(*dna.pack(a)), dna.BASES.index(q[0]))
            assert ae and og.edge_info(ae)["end"] == oid
            og.replace_end(ae, new)
            out["in_edge"] = (a, q[0])
        self.copies = True
        return out

    # ---- what the observers must see ---------------------------------------------------------------------------------------------
    def expect_counts(self):
        nodes, edges = self.content()
        return len(nodes), len(edges), sum(len(q) for _s, _e, q in edges)

    def expect_out_order(self, kmer):
        return self.og.out_order(*dna.pack(kmer))

    def expect_degrees(self):
        """k-mer -> sorted [(in-degree, out-degree)] of the nodes that carry it"""
        nodes, edges = self.content()
        out = {}
        if self.has_copies():
            ids, eids = self.by_id()
            ind, outd = Counter(b for _e, _a, b, _q in eids), Counter(a for _e, a, _b, _q in eids)
            for i, s in ids:
                out.setdefault(s, []).append((ind[i], outd[i]))
        else:
            ind, outd = Counter(e for _s, e, _q in edges), Counter(s for s, _e, _q in edges)
            for s in nodes:
                out.setdefault(s, []).append((ind[s], outd[s]))
        return {s: sorted(v) for s, v in out.items()}

    def expect_out_bases(self):
        """k-mer -> the sorted first-base strings of the out-edges of each node that carries it (several with copies)"""
        out = {}
        if self.has_copies():
            ids, eids = self.by_id()
            per = {}
            for _e, a, _b, q in eids:
                per.setdefault(a, []).append(q[0])
            for i, s in ids:
                out.setdefault(s, []).append("".join(sorted(per.get(i, []))))
        else:
            for s in self.content()[0]:
                out[s] = [""]
            for s, _e, q in self.content()[1]:
                out[s] = ["".join(sorted(out[s][0] + q[0]))]
        return out

    def absent_kmers(self, n=20):
        """n k-mers, seeded, of which neither orientation is a node"""
        have, rnd, out = set(self.content()[0]), random.Random(self.seed + 1), []
        while len(out) < n:
            s = "".join(rnd.choice("AGCT") for _ in range(self.k))
            if s not in have and R.rev_comp(s) not in have:
                out.append(s)
        return out

    def expect_contig_stats(self, longer_than):
        return CG.contig_stats([len(q) for _s, _e, q in self.content()[1]], longer_than)

    def expect_coverage(self, edges):
        """tips_ref.coverage(counts, edges), edge by edge (an edge that outlives a step is computed once)"""
        rows, missing = [], 0
        for e in edges:
            if e not in self._cov:
                self._cov[e] = T.coverage(self.counts, [e])
            (row,), miss = self._cov[e]
            rows.append(row)
            missing += miss
        return rows, missing

    def expect_contigs(self, edges, ids):
        return FA.contigs(edges, ids, self.counts, strands=1)[0]

    def _indexed(self):
        """thread_ref's form: node k-mers (one entry per node) and edges (start index, end index, seq), and each edge's content key"""
        nodes, edges = self.content()
        if self.has_copies():
            ids, eids = self.by_id()
            at = {i: j for j, (i, _s) in enumerate(ids)}
            kmers = [s for _i, s in ids]
            return kmers, [(at[a], at[b], q) for _e, a, b, q in eids], [(kmers[at[a]], dna.BASES.index(q[0])) for _e, a, _b, q in eids]
        at = {s: j for j, s in enumerate(nodes)}
        return nodes, [(at[s], at[t], q) for s, t, q in edges], [(s, dna.BASES.index(q[0])) for s, _t, q in edges]

    def expect_thread(self, reads):
        """-> (support by content as pairs_ref.gpu_support_by_content keys it, the seven stats)"""
        nodes, edges, keys = self._indexed()
        sup, st = TR.thread_reads(self.k, nodes, edges, reads)
        out = Counter()
        for (e, f), c in sup.items():
            out[(keys[e], keys[f])] += c
        return out, st

    def expect_pair_distances(self, npairs):
        nodes, edges = self.content()
        index, lens = IR.index_graph(self.k, [(s, q) for s, _e, q in edges], nodes=nodes)
        return IR.pair_distances(self.k, index, lens, self.reads, npairs, BINS)


# ---- the committed sequences ---------------------------------------------------------------------------------------------------
# (k, seed), chosen on the CPU so that the conditions tests/test_graph_sequences_cpu.py asserts hold; 21 and 31: one key word,
# 35 and 64: two words and the tagged table
SEQUENCES = [(21, 3), (21, 27), (31, 3), (31, 27), (35, 2), (35, 8), (35, 20), (64, 6), (64, 42), (64, 52)]
SMALL_GRID = (21, 3)                                    # the one that also runs with every graph launch capped at two workgroups


def observer_steps(seed):
    """the two steps (of STEPS) after which threadReads and pairDistances are compared as well"""
    return sorted(random.Random(seed + 77).sample(range(STEPS), 2))
