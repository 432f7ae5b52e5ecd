"""What the overlap tests share: reads whose graphs hold junctions of every class of the overlap rule (include/genome_amd.h,
"overlap detection"), by content only: no ids, no device.  A test builds the graph of the reads (the oracle's, or the device's),
finds the two edges by their paths and, for a planted case, replaces the start of f by an added node of the k-mer given here.

dip      reads G[0 : p + k - 1] and G[p + w :] of a random genome G: w k-mers are missing, the two contigs overlap by exactly
         o = k - 1 - w bases and no k-mer of one is next to a k-mer of the other.
planted  P(f) is made to begin with k chosen bases X, so that the last k + d bases of P(e) are the first k + d of P(f):
         d = -1 (o = k - 1): X = the last k - 1 bases of P(e) and one more;  d = 0 (o = k): X = e's end k-mer;
         1 <= d <= k - 2: read 1 ends in d bases D and read 2 is K' + D + V, so seq(f) begins with D, X = the k bases before D;
         d = k - 1 (o = 2k - 1, 127 at k = 64): as before, but x + D, the last k-mer of read 1, and D + V0 of read 2 are neighbours in
         the graph.  A third read gives x + D a second predecessor, so that e still ends there, and f is the edge K' -> D + V0 of
         exactly k bases: |P(f)| = 2k, and o = 2k - 1 is the largest candidate it admits.
periodic read 1 ends in (AC)^8 and X = (AC)^7 GG ..: the even o up to 14 are hits.
"""
import random

from fillgaps_cases import KS  # noqa: F401  (the key widths of the dip graphs)

MIN_OVERLAP = 10
TOLS = (0, 3, 35)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}
COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def rand(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def tile(seqs, k, L=200):
    """reads of at most L bases (a .bin record holds 255) with every k-mer of every sequence: their graph is the sequences'"""
    return [q[s:s + L] for q in seqs for s in range(0, max(len(q) - k, 1), L - k)]


def dip_overlaps(k):
    """the overlaps the dip graphs are built for: 1, min_overlap - 1, min_overlap, k - 2"""
    return (1, MIN_OVERLAP - 1, MIN_OVERLAP, k - 2)


def dip(seed, k, o, glen=400):
    """-> (reads, left path, right path, G)"""
    rnd = random.Random(seed)
    G = rand(rnd, glen)
    w, p = k - 1 - o, glen // 2
    assert 1 <= w <= k - 2
    left, right = G[:p + k - 1], G[p + w:]
    assert left[len(left) - o:] == right[:o]
    return tile([left, right], k), left, right, G


def sweep(o, tol):
    """the gaps around -o at which the candidates' range gains and loses o"""
    return (-o - tol - 1, -o - tol, -o, -o + tol, -o + tol + 1)


def planted(seed, k, d):
    """-> (reads, the path of e, the first k bases of f's path as built, X)"""
    rnd = random.Random(seed)
    U, V, K1 = rand(rnd, 3 * k + 17), rand(rnd, 2 * k + 9), rand(rnd, k)
    D = rand(rnd, max(d, 0))
    if d == k - 1:
        if K1[-1] == U[-1]:
            K1 = K1[:-1] + OTHER[K1[-1]]
        third = rand(rnd, k + 5) + OTHER[U[-2]] + U[-1] + D[:-1]
        reads = [U + D, K1 + D + V, third]
    else:
        reads = [U + D, K1 + D + V]
    pe = U + D
    X = pe[len(pe) - (k + d):len(pe) - d] if d > 0 else pe[len(pe) - k:] if d == 0 else pe[len(pe) - (k - 1):] + OTHER[pe[len(pe) - k]]
    return tile(reads, k), pe, K1, X


def periodic(seed, k):
    """-> (reads, the path of e, the first k bases of f's path as built, X): hits at the even o from 2 to 14"""
    rnd = random.Random(seed)
    U, V, K1 = rand(rnd, 3 * k) + "GG", rand(rnd, 2 * k), rand(rnd, k)
    pe = U + "AC" * 8
    X = "AC" * 7 + "GG" + rand(rnd, k - 16)
    return tile([pe, K1 + V], k), pe, K1, X


def many(seed, k, n=300, glen=160):
    """n short genomes with a dip each, in one graph -> (reads, [(left path, right path, o)])"""
    rnd = random.Random(seed)
    reads, pairs = [], []
    for i in range(n):
        o = 1 + (i * 7) % (k - 2)
        r, left, right, _ = dip(rnd.randrange(1 << 30), k, o, glen)
        reads += r
        pairs.append((left, right, o))
    return reads, pairs


def find(edges, want, head=False):
    """the id of the one edge whose path is `want` (head: begins with it)"""
    got = [e for e, (s, _t, q) in edges.items() if ((s + q).startswith(want) if head else s + q == want)]
    assert len(got) == 1, (want, len(got))
    return got[0]


# the end-to-end case: a 6 kb genome, three dips, pairs from pairs_ref.make_pairs (nrep = 0: its genome is the first glen draws)
E2E = dict(seed=4242, k=31, glen=6000, dips=((1500, 3), (3000, 10), (4500, 18)), npairs=2500, ins=(80, 100), mid=90, tol=10, support=3)


def e2e_genome():
    rnd = random.Random(E2E["seed"])
    return "".join(rnd.choice("AGCT") for _ in range(E2E["glen"]))


def e2e_pieces():
    """the reads the graph is built from: the genome without the dips' k-mers"""
    G, k, out, at = e2e_genome(), E2E["k"], [], 0
    for p, w in E2E["dips"]:
        out.append(G[at:p + k - 1])
        at = p + w
    return tile(out + [G[at:]], k)


def plant(edges, node_ids, f, X, node):
    """the model after replaceStart(f, addNode(X)): -> (edges, node_ids); node_ids None: the nodes are the k-mers"""
    ids = dict(node_ids) if node_ids is not None else {e: (s, t) for e, (s, t, _q) in edges.items()}
    edges = dict(edges)
    edges[f] = (X, edges[f][1], edges[f][2])
    ids[f] = (node, ids[f][1])
    return edges, ids
