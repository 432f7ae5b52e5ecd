"""What the alignment-block tests share: a reference and contigs in which every breakpoint class and every edge class of
include/genome_amd.h ("alignment blocks", "breakpoints") is planted on purpose, by content only: no ids, no device.  Built on
judge_cases.py, whose main(k), variant_marks, variant_deletion, repeats(k) and long_record(k) the tests run as they are.

chimeras(k)   two reference records H0 (2600 bp) and H1 (800 bp + a second copy of H1[300:500]) and, behind them, a record
              shorter than k, an empty one and one of exactly k bases.  The graph is built from CONTIGS ONLY (error-free tiles), each
              from a stretch of the reference no other contig uses, so every contig is one edge and its twin:
                transloc   H0[0:150] + H1[0:150]                      translocation      misassembled
                invert     H0[200:350] + rc(H0[400:550])              inversion          misassembled
                reloc      H0[600:750] + H0[800:950]                  shift 50 > TOL     misassembled
                near       H0[1000:1150] + H0[1190:1340]              shift 40 = TOL     indel (by distance)
                ins3       H0[1400:1550] + 3 bases + H0[1550:1700]    shift -3           indel
                del1       H0[1750:1900] + H0[1901:2050]              shift +1           indel
                subst      H0[2350:2500], one base substituted         shift 0            colinear
                whole      H0[2100:2300]                              one row            exact, full
                part       H1[600:700] + 80 bases of nothing          one row            exact, not full
                twice      H1[300:500]                                 two rows, overlap  repeat
                kmer       100 bases of nothing; the last record is its bases 10 .. 10 + k: one row of one k-mer
                nowhere    120 bases of nothing                        no row             unaligned
"""
import random

from judge_cases import OTHER
from overlaps_cases import rand, rc, tile

TOL = 40


def chimeras(k, seed=None):
    """-> dict(reads, records, paths={name: path}, classes={name: (edge class, full)})"""
    rnd = random.Random(9900 + k if seed is None else seed)
    H0, H1 = rand(rnd, 2600), rand(rnd, 800)
    nothing, kx, junk = rand(rnd, 120), rand(rnd, 100), rand(rnd, 80)
    ins = OTHER[H0[1550]] + rand(rnd, 2)                     # (its first base is not the base the reference goes on with)
    sub = H0[2350:2500]
    sub = sub[:75] + OTHER[sub[75]] + sub[76:]
    paths = dict(transloc=H0[0:150] + H1[0:150], invert=H0[200:350] + rc(H0[400:550]), reloc=H0[600:750] + H0[800:950],
                 near=H0[1000:1150] + H0[1190:1340], ins3=H0[1400:1550] + ins + H0[1550:1700], del1=H0[1750:1900] + H0[1901:2050],
                 subst=sub, whole=H0[2100:2300], part=H1[600:700] + junk, twice=H1[300:500], kmer=kx, nowhere=nothing)
    classes = dict(transloc=("misassembled", 1), invert=("misassembled", 1), reloc=("misassembled", 1), near=("indel", 1), ins3=("indel", 1),
                   del1=("indel", 1), subst=("colinear", 1), whole=("exact", 1), part=("exact", 0), twice=("repeat", 1), kmer=("exact", 0),
                   nowhere=("unaligned", 0))
    records = [H0, H1 + H1[300:500], H1[:k - 1], "", kx[10:10 + k]]
    return dict(reads=tile(list(paths.values()), k), records=records, paths=paths, classes=classes)


def marked(records, k):
    """chimeras' records with an N inside `whole` (at H0[2200]) and a lowercase run inside `part` (H1[640:643])"""
    g0, g1 = list(records[0]), list(records[1])
    g0[2200] = "N"
    for i in range(640, 643):
        g1[i] = g1[i].lower()
    return ["".join(g0), "".join(g1)] + list(records[2:])


def slice_values(k):
    """test_place_slice values for judge_cases.variant_marks(main(k)["records"]), whose record 0 holds an N at 100 inside the contig
    c0a = G0[0 : 300 + k]: its runs are the window starts 1 .. 100 - k and 101 .. 299.  A slice of S characters starts at every
    multiple of S and its first window start of its own lies k - 1 before that:
      inside a run                                      257, 50
      on the second run's first start 101               101 (the slice), 101 + k - 1 (its first own window)
      on the first run's last start 100 - k             100 - k, 99 (= 100 - k + k - 1)
      k - 1 and k characters after the N                100 + k - 1, 100 + k
    """
    return (257, 50, 101, 101 + k - 1, 100 - k, 99, 100 + k - 1, 100 + k)


def short_slices(k):
    """slices shorter than k + 1"""
    return (1, k - 1, k)
