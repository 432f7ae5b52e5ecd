"""What the judge tests share: genomes, reads and chains in which every class of the placement rule and of the judge is planted on
purpose (include/genome_amd.h, "placements" and "the judge"), by content only: no ids, no device.

main(k)    two reference records G0 (2400 bp) and G1 (1200 bp).  The reads are error-free tiles of pieces of them, so the contigs
           are known by their paths (both strands: t(x) is the twin, the reverse complement of x):
             c0a = G0[0 : 300 + k]   c0b = G0[300 : 600]    a spur X + G0[300 : 300 + k + 5] gives the k-mer at 300 a second way in:
                                                            c0a ends and c0b starts at that node (an ADJACENT junction)
             c1  = G0[650 : 1100 + k - 1]                   50 bases after c0b (a GAPPED junction)
             c2  = G0[1100 + w : 1700], w = k - 1 - 12      a coverage dip of w k-mers: c1 and c2 OVERLAP by 12 bases
             c3  = G0[1760 : 2400]
             d0  = G1[0 : 500]       d1 = G1[545 : 1200]
           chains (class of each junction):
             A [c0a, c0b, c1, c2]        adjacent correct, gapped (the estimate off by `delta`), overlapped correct
             B [d1, d0]                  order
             C [t(c2), c3]               strand (an inversion: a contig joined to a twin)
             D [t(d1), t(c3)]            other_record
             E [t(c1), t(c0b), t(c0a)]   the reference's reverse strand: gapped correct, adjacent correct
             F [t(d0)]                   no junction
             G [spur, t(spur)]           unjudged (the spur is not in the reference: both edges are unplaced)
variants   the reference with an N and a lowercase run inside c0a and one substituted base inside c3 (still one diagonal, fewer
           windows), and with one base deleted inside d1 (scattered)
repeats(k) a genome with an exact repeat and an inverted repeat longer than k: a scattered and a both_strands edge
long_record(k)  one record of 3 T + 700 bases, T = 4096 window starts being one workgroup's tile of the placement pass, with
           contigs on and around every tile boundary (long_coords), long_marks: invalid characters on, just before and k - 1
           after a boundary, long_truncations: records that end at the first boundary
"""
import random

from overlaps_cases import rand, rc, tile  # noqa: F401

KS = (21, 31, 34, 55, 64)                                  # one word, a full word, the first two-word k, two words, the tagged table
OVERLAP = 12
GAP_C0B_C1, GAP_C2_C3, GAP_D0_D1 = 50, 60, 45
LOWER = {"A": "a", "C": "c", "G": "g", "T": "t"}
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def main(k, seed=None):
    """-> dict(reads, records=[G0, G1], paths={name: path})"""
    rnd = random.Random(9000 + k if seed is None else seed)
    G0, G1, X = rand(rnd, 2400), rand(rnd, 1200), rand(rnd, 40)
    w = k - 1 - OVERLAP
    assert w >= 1
    if X[-1] == G0[299]:                                   # the spur must enter the k-mer at 300 by another base than the genome does
        X = X[:-1] + OTHER[X[-1]]
    pieces = [G0[0:600], X + G0[300:300 + k + 5], G0[650:1100 + k - 1], G0[1100 + w:1700], G0[1760:2400], G1[0:500], G1[545:1200]]
    paths = dict(c0a=G0[0:300 + k], c0b=G0[300:600], spur=X + G0[300:300 + k], c1=pieces[2], c2=pieces[3], c3=pieces[4], d0=pieces[5], d1=pieces[6])
    assert paths["c1"][-OVERLAP:] == paths["c2"][:OVERLAP]
    return dict(reads=tile(pieces, k), records=[G0, G1], paths=paths, w=w)


# where base 0 of each path lies on its record, forward; the twin lies at that coordinate + len(path) - 1, reverse
def coords(k):
    return dict(c0a=(0, 0), c0b=(0, 300), c1=(0, 650), c2=(0, 1100 + k - 1 - OVERLAP), c3=(0, 1760), d0=(1, 0), d1=(1, 545))


def chains(find, paths, k, delta=0):
    """find(path) -> edge id.  -> (chains, gaps, expected classes per chain, expected err per chain)"""
    t = lambda n: find(rc(paths[n]))
    f = lambda n: find(paths[n])
    ch = [[f("c0a"), f("c0b"), f("c1"), f("c2")], [f("d1"), f("d0")], [t("c2"), f("c3")], [t("d1"), t("c3")], [t("c1"), t("c0b"), t("c0a")], [t("d0")],
          [f("spur"), t("spur")]]
    gaps = [[-k, GAP_C0B_C1 + delta, -OVERLAP], [GAP_D0_D1], [GAP_C2_C3], [30], [GAP_C0B_C1, -k], [], [25]]
    return ch, gaps


def overlaps():
    """what overlapGaps finds for chains(): the dip between c1 and c2"""
    return [[0, 0, OVERLAP], [0], [0], [0], [0, 0], [], [0]]


def expected(tol, delta):
    """the class of every junction of chains(), in row order, and its err where one is written (None: whatever the rule gives)"""
    gapped = "correct" if abs(delta) <= tol else "distance"
    classes = ["correct", gapped, "correct", "order", "strand", "other_record", "correct", "correct", "unjudged"]
    errs = [0, delta, 0, None, 0, 0, 0, 0, 0]
    return classes, errs


def variant_marks(records, k):
    """an N at G0[100], a lowercase run G0[120:125] (inside c0a) and a substituted base at G0[2000] (inside c3)"""
    g = list(records[0])
    g[100] = "N"
    for i in range(120, 125):
        g[i] = LOWER[g[i]]
    g[2000] = OTHER[g[2000]]
    return ["".join(g), records[1]]


def variant_deletion(records):
    """G1[900] deleted (inside d1)"""
    return [records[0], records[1][:900] + records[1][901:]]


def repeats(k, seed=None):
    """G = A R B R C Q D rc(Q) E with |R| = |Q| = k + 10 -> dict(reads, records=[G], R, Q)"""
    rnd = random.Random(7000 + k if seed is None else seed)
    A, B, Cc, D, E = (rand(rnd, 300) for _ in range(5))
    R, Q = rand(rnd, k + 10), rand(rnd, k + 10)
    G = A + R + B + R + Cc + Q + D + rc(Q) + E
    return dict(reads=tile([G], k), records=[G], R=R, Q=Q)


# ---- a record of several tiles ---------------------------------------------------------------------------------------------------
T = 4096                                                   # window starts per workgroup of the placement pass
LONG_LEN = 3 * T + 700
LONG_KS = (31, 34, 64)


def long_record(k, seed=None):
    """-> dict(reads, record, paths={name: path}).  The contigs, by the record's coordinates (long_coords):
      a     G[T - 300 : T + 300]          crosses the first boundary: its run of hits is cut by it
      b     G[2T - 5 : 2T + 400]          crosses the second: its first windows start in the last k - 1 characters of a tile
      e     G[3T - 400 : 3T + k]          ends at the k-mer at 3T, which a spur X + G[3T : 3T + k] enters a second way, so it is a node:
      f     G[3T : 3T + k + 4]            e's last interior window starts at 3T - 1 and f's path starts at 3T.  The break between two
                                          edges falls exactly on the third boundary (the first two lie inside a and b)
      tail  G[3T + 10 : ]                 only the last, partly filled tile"""
    rnd = random.Random(9500 + k if seed is None else seed)
    G, X = rand(rnd, LONG_LEN), rand(rnd, 40)
    if X[-1] == G[3 * T - 1]:                              # the spur must enter the k-mer at 3T by another base than the record does
        X = X[:-1] + OTHER[X[-1]]
    pieces = [G[T - 300:T + 300], G[2 * T - 5:2 * T + 400], G[3 * T - 400:3 * T + k + 4], X + G[3 * T:3 * T + k + 4], G[3 * T + 10:]]
    paths = dict(a=pieces[0], b=pieces[1], e=G[3 * T - 400:3 * T + k], f=G[3 * T:3 * T + k + 4], tail=pieces[4], spur=X + G[3 * T:3 * T + k])
    return dict(reads=tile(pieces, k), record=G, paths=paths)


# where base 0 of each path of long_record lies on the record, forward; the twin lies at that coordinate + len(path) - 1, reverse
def long_coords(k):
    return dict(a=T - 300, b=2 * T - 5, e=3 * T - 400, f=3 * T, tail=3 * T + 10)


def long_marked_at(k):
    """the coordinates long_marks changes: an N, a lowercase base, a substituted base"""
    return (T - 1, 2 * T, 2 * T + k - 2)


def long_marks(record, k):
    """an N at T - 1 (inside a), a lowercase base at 2T and a substituted base at 2T + k - 2 (inside b): on, just before and k - 1
    after a tile boundary"""
    g = list(record)
    n_at, lower_at, subst_at = long_marked_at(k)
    g[n_at] = "N"
    g[lower_at] = LOWER[g[lower_at]]
    g[subst_at] = OTHER[g[subst_at]]
    return "".join(g)


def long_truncations(record, k):
    """the record cut to T - 1, T and T + 1 windows; at T windows the second workgroup holds k - 1 characters and no window"""
    return [record[:T - 1 + k - 1], record[:T + k - 1], record[:T + k]]


def fasta(records, width=70, names=None):
    """the records as FASTA text"""
    out = []
    for i, r in enumerate(records):
        out.append(">" + (names[i] if names else f"r{i}") + "\n")
        out += [r[j:j + width] + "\n" for j in range(0, len(r), width)]
    return "".join(out).encode()
