"""Graphs with planted edge lengths for the contig statistics (gk_graph_contig_stats: k_contig_reduce, then one k_contig_hist pass
per byte of the maximum).  A helper, not a test: tests/test_contig_stats_cpu.py proves what every case is named for,
tests/test_contig_stats_gpu.py runs them on the device.

A case is a list of target edge lengths.  Every target becomes one linear random chromosome of target + overhead(k) bases, covered
by error-free 150-base reads tiled every 100 bases on both strands with an extra last read at the end (k <= 47: consecutive reads
share 50 >= k - 1 bases, so every k-window of the chromosome lies in a read).  count -> buildGraph -> simplifyGraph then leaves one
edge per strand per chromosome: the first and the last k-mer of a chromosome are its only nodes (a k-mer with no way in, one with
no way out), and the unitig between them has one base per further k-mer.  overhead(k) is not written down here: it is read off
the CPU model (oracle.pyref) on a 200-base chromosome.  That the graph is the planted one and nothing else holds when all
(k-1)-mers of all chromosomes of a case, reverse complements included, are distinct — no k-mer then has a neighbour the
chromosome did not give it — which the CPU test asserts for every case (odd k: no k-mer is its own reverse complement).

The lengths of the edges are every target twice.  What each case is for, in terms of the select's loop (`shift` = 8 * level):

  one_level            the maximum is exactly 255: one pass, shift 0, both prefixes 0; duplicates, and sorted[count / 2] is the
                       upper middle of an even count
  boundary_256_split   255, 256, 257 and a maximum of 260: the select starts at shift 8; the median is 255 and the N50 256, so the
                       two prefixes differ (0 and 1) after the first pass
  boundary_256_above   the same neighbourhood with both the median and the N50 at 256, the 255 just below them (prefixes 1 and 1)
  boundary_256_below   both at 255 with 256, 257, 258 above them (prefixes 0 and 0 under a maximum whose top byte is 1)
                       (the N50 is never below the median — the upper half of the sorted lengths weighs at least as much as the lower
                       half — so "median 256, N50 255" does not exist; these three are the arrangements around the boundary that do)
  two_level_split      40 edges around 300 and three around 40 000: the median's top byte is 1, the N50's 156, and the N50 is not in
                       the top occupied bin (41 234 lies above it), so the running sum carried into the second pass is not 0
  three_level          65 535, 65 536, 65 537 and 70 000 beside 150 short edges: the loop starts at shift 16, the N50 is 65 536
                       (prefix 1, then 0x0100) and the median a short edge (prefix 0, then 0x0000)
  three_level_tie      65 536 three times and 65 537 twice, nothing else: the median and the N50 are both 65 536 at cutoff 0 and both
                       65 537 at cutoff 65 536 — the last byte decides, under the two-byte prefix 0x0100
  three_level_tie_split  one edge of 1 base beside 65 536 twice and 65 537 twice: the same two-byte prefix for both selects, and then
                       the median is 65 536 and the N50 65 537 in ONE call (with the three_level_tie lengths alone that cannot
                       happen: both conditions come to "as many 65 537 as 65 536")
  all_equal            40 edges of 300: one occupied bin in every histogram of every pass
  single               one chromosome: its two strand edges are the whole input
"""
import random
from functools import lru_cache

from oracle import pyref as R

KS = (31, 47)                    # one-word and two-word keys; odd, so that no k-mer is a palindrome
READ_LEN, READ_STEP = 150, 100
ZERO = dict(count=0, sum=0, median=0, n50=0, max=0)

CASES = {
    "one_level": [1, 2, 3, 7, 31, 64, 64, 100, 127, 128, 128, 129, 200, 254, 255, 255],
    "boundary_256_split": [10, 20, 30, 255, 255, 256, 257, 260],
    "boundary_256_above": [255, 256, 256, 257, 260],
    "boundary_256_below": [255] * 6 + [256, 257, 258],
    "two_level_split": [290 + (7 * i) % 40 for i in range(40)] + [39999, 40000, 41234],
    "three_level": [40 + (37 * i) % 261 for i in range(150)] + [65535, 65536, 65537, 70000],
    "three_level_tie": [65536] * 3 + [65537] * 2,
    "three_level_tie_split": [1, 65536, 65536, 65537, 65537],
    "all_equal": [300] * 20,
    "single": [1000],
}
BOUNDARY_256 = ("boundary_256_split", "boundary_256_above", "boundary_256_below")


def lengths_of(name):
    """the edge lengths the case plants: every target once per strand"""
    return sorted(2 * CASES[name])


def tiled_reads(chrom):
    """150-base reads every 100 bases on both strands, and the last 150 bases once more (a chromosome shorter than a read: itself)"""
    last = max(len(chrom) - READ_LEN, 0)
    reads = []
    for s in list(range(0, last + 1, READ_STEP)) + [last]:
        frag = chrom[s:s + READ_LEN]
        reads += [frag, R.rev_comp(frag)]
    return reads


def model_lengths(k, chroms):
    """the CPU model's count -> buildGraph -> simplifyGraph over the reads of `chroms` -> the sorted edge lengths"""
    reads = [r for c in chroms for r in tiled_reads(c)]
    g = R.build_graph(k, R.extract_filtered_kmers(reads, k, 1, do_filter=False))
    g.simplify()
    return sorted(len(q) for _s, _e, q in g.edges.values())


@lru_cache(maxsize=None)
def overhead(k):
    """chromosome length minus the length of its edge, from the model on one 200-base chromosome"""
    chrom = "".join(random.Random(k).choices(R.BASES, k=200))
    a, b = model_lengths(k, [chrom])                  # one edge per strand
    assert a == b
    return 200 - a


def chromosomes(name, k):
    """one random chromosome per target of the case, target + overhead(k) bases each; the same for every caller"""
    rnd = random.Random(f"{name} {k}")
    return ["".join(rnd.choices(R.BASES, k=t + overhead(k))) for t in CASES[name]]


def all_reads(name, k):
    return [r for c in chromosomes(name, k) for r in tiled_reads(c)]


def levels(x):
    """the passes the select makes for a maximum of x: its bytes up to the top non-zero one (1 for 0)"""
    return max(1, (int(x).bit_length() + 7) // 8)


def cutoffs(lengths):
    """the cutoffs the device is held to for these lengths: 0 and the smallest length (strict >: it drops out), the byte-boundary
    lengths the case has (a cutoff that removes exactly them, and the start level changes where one was the maximum), and the two at
    the maximum (only its copies remain; nothing remains)"""
    have = set(lengths)
    return sorted({0, min(lengths), max(lengths) - 1, max(lengths)} | {c for c in (254, 255, 256, 65535, 65536) if c in have})
