"""What the scaffold GPU tests share: the oracle's graph of a fixture by content, chains constructed over it from a seeded
generator, and a check of a scaffold text that does not use the restatement's assembly.  Content only: no ids, no device; an
edge is its (start k-mer, first base code), and a test maps that to the device's id."""
import random

from genome_amd import dna
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import oracle_canonical

GAPS = (-50, 0, 1, 9, 10, 11, 63, 64, 65, 1000)


def oracle_edges(k, reads, min_count=1):
    """{content key: (start k-mer, end k-mer, seq)} of the oracle's graph of `reads`"""
    ref = O.PMap(k, 1)
    ref.count_reads(dna.reads_to_bin(reads), len(reads))
    if min_count > 1:
        ref.delete_lt(min_count)
    _nodes, edges = oracle_canonical(O.Graph(ref))
    out = {(s, dna.BASES.index(q[0])): (s, e, q) for s, e, q in edges}
    assert len(out) == len(edges)
    return out


def twins(edges):
    """key -> the key of the edge whose path is the reverse complement (a strand-closed graph)"""
    by_path = {s + q: key for key, (s, _e, q) in edges.items()}
    return {key: by_path[R.rev_comp(s + q)] for key, (s, _e, q) in edges.items()}


def constructed(edges, seed, nchains=14):
    """Disjoint chains over the edges (keys) and their gaps: a chain of three with its exact twin chain, an edge followed by its own twin, a
    chain of one member, then random ones.  A successor is drawn from the out-edges of the end node (an adjacent junction by construction) or elsewhere; the
    gaps elsewhere run through GAPS in turn.  -> (chains as lists of keys, gaps as lists one shorter)"""
    rnd = random.Random(seed)
    keys = sorted(edges)
    free = set(keys)
    out = {}
    for key in keys:
        out.setdefault(edges[key][0], []).append(key)
    twin = twins(edges)
    turn = [0]

    def grow(c, length, avoid=()):
        g = []
        while len(c) < length:
            near = [f for f in out.get(edges[c[-1]][1], []) if f in free and f not in avoid and twin[f] not in c and twin[f] != f]
            if near and rnd.random() < 0.5:
                f = rnd.choice(near)
                g.append(rnd.choice(GAPS))                   # (not looked at)
            else:
                far = [f for f in sorted(free) if f not in avoid and edges[f][0] != edges[c[-1]][1] and twin[f] not in c and twin[f] != f]
                f = rnd.choice(far)
                g.append(GAPS[turn[0] % len(GAPS)])
                turn[0] += 1
            free.discard(f)
            c.append(f)
        return g

    chains, gaps = [], []
    # a chain of three whose twins are three other edges, and the chain of its twins
    first = next(key for key in keys if twin[key] != key and any(f != key and twin[f] not in (key, f) for f in out.get(edges[key][1], [])))
    free.discard(first)
    c = [first]
    g = grow(c, 3, avoid={twin[first]})
    tc = [twin[e] for e in reversed(c)]
    assert len(set(c) | set(tc)) == 6
    free.difference_update(tc)
    chains += [c, tc]
    gaps += [g, g[::-1]]
    # an edge, a gap and its twin: the same on both strands
    x = next(key for key in sorted(free) if twin[key] != key and twin[key] in free)
    free.difference_update((x, twin[x]))
    chains.append([x, twin[x]])
    gaps.append([64])
    # one member
    lone = rnd.choice(sorted(free))
    free.discard(lone)
    chains.append([lone])
    gaps.append([])
    while len(chains) < nchains and len(free) > 8:
        c = [rnd.choice(sorted(free))]
        free.discard(c[0])
        gaps.append(grow(c, rnd.choice((2, 3, 4, 6))))
        chains.append(c)
    return chains, gaps


def covered(paths, seq):
    """The members' paths lie in the record's sequence in order (each found at or after the base behind the start of the one
    before: two that share a node overlap by its k bases), and together they cover exactly the bases that are not N."""
    at, mark = 0, [False] * len(seq)
    for p in paths:
        pos = seq.find(p, at)
        if pos < 0:
            return False
        mark[pos:pos + len(p)] = [True] * len(p)
        at = pos + 1
    return all(m == (c != "N") for m, c in zip(mark, seq))
