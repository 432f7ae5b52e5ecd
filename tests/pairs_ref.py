"""What the paired-end test modules share: the fixture generator and the content-keyed comparison of a library result with the
oracle's.  Edge ids are arbitrary on both sides: support counts are compared after translation to content, (start k-mer, first
base) of both edges; the graphs as canonical node / edge lists (copies of a node share a sequence: lists, not sets)."""
import random
from collections import Counter

from genome_amd import dna, synth
from oracle import pyref as R


def make_pairs(seed, k, glen=2400, nrep=3, L=40, npairs=5000, ins=(80, 100), err=0.0, replen=None):
    """A random genome in which `nrep` k-mers occur twice in different contexts (a node with two in- and two out-edges each,
    which only read pairs can resolve), and read pairs of insert size `ins` from both strands.  L: the mates' length (a
    fragment shorter than L gives shorter mates); replen: the length of the planted repeats (k unless given).  The defaults
    draw the same random numbers in the same order as before the two knobs existed."""
    rnd = random.Random(seed)
    replen = k if replen is None else replen
    g = [rnd.choice("AGCT") for _ in range(glen)]
    for _ in range(nrep):
        a = rnd.randrange(100, glen // 2 - 100)
        b = rnd.randrange(glen // 2 + 100, glen - 100)
        g[b:b + replen] = g[a:a + replen]
    g = "".join(g)
    reads = []
    for _ in range(npairs):
        ins_len = rnd.randint(*ins)
        s = rnd.randrange(0, glen - ins_len)
        frag = g[s:s + ins_len]
        if rnd.random() < 0.5:
            frag = R.rev_comp(frag)
        m1, m2 = frag[:L], R.rev_comp(frag)[:L]
        if err:
            m1 = "".join(c if rnd.random() >= err else rnd.choice([x for x in "AGCT" if x != c]) for c in m1)
            m2 = "".join(c if rnd.random() >= err else rnd.choice([x for x in "AGCT" if x != c]) for c in m2)
        reads += [m1, m2]
    return reads


def oracle_canonical(og):
    k = og.k
    nlo, nhi = og.nodes()
    nodes = sorted(dna.unpack(int(a), int(b), k) for a, b in zip(nlo, nhi))
    e = og.edges()
    edges = []
    for i in range(len(e["len"])):
        seq = synth.bases_to_str(e["bases"][e["off"][i]:e["off"][i] + e["len"][i]])
        edges.append((dna.unpack(int(e["slo"][i]), int(e["shi"][i]), k), dna.unpack(int(e["elo"][i]), int(e["ehi"][i]), k), seq))
    return nodes, sorted(edges)


def gpu_canonical(g):
    nodes, edges = g.canonical()
    return sorted(nodes), sorted(edges)


def gpu_support_by_content(g, k, sup):
    e1, e2, cnt = sup.items()
    ids = sorted(set(e1.tolist()) | set(e2.tolist()))
    if not ids:
        return Counter()
    info = g.edgesById(ids)
    nid = sorted({int(x) for x in info["start"]})
    ninfo = g.nodesById(nid)
    nkmer = {n: dna.unpack(int(ninfo["lo"][j]), int(ninfo["hi"][j]), k) for j, n in enumerate(nid)}
    key = {e: (nkmer[int(info["start"][j])], int(info["first"][j])) for j, e in enumerate(ids)}
    out = Counter()                                            # (content keys that collide would add up, on both sides alike)
    for a, b, c in zip(e1, e2, cnt):
        out[(key[int(a)], key[int(b)])] += int(c)
    return out


def oracle_support_by_content(og, k, osup):
    e1, e2, cnt = osup.items()
    def key(e):
        info = og.edge_info(int(e))
        return (dna.unpack(*og.node_seq(info["start"]), k), info["first"])
    out = Counter()
    for a, b, c in zip(e1, e2, cnt):
        out[(key(a), key(b))] += int(c)
    return out
