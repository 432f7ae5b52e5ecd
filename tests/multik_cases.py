"""What the multi-k tests share (no device code): the end-to-end construction of the issue — a genome with a coverage dip that k = 55
alone cannot cross and k = 21 can — and planted linear genomes for single-edge graphs.  The seeds are pinned on the CPU
(tests/test_multik_cpu.py asserts what they promise)."""
import random

from oracle import pyref as R

GENOME_LEN, DIP, READ_LEN, COPIES = 3000, 1500, 100, 3
MISSING_55 = 14                    # the 55-mers that start in (DIP - 35, DIP - 20): in no read
GENOME_SEED = 1                    # the smallest seed whose genome repeats no 20-mer on either strand (test_multik_cpu.py)


def rand_seq(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def dip_genome(seed=GENOME_SEED):
    return rand_seq(random.Random(seed), GENOME_LEN)


def repeats_kmer(s, k):
    """True if a k-mer of s occurs twice in s or in its reverse complement"""
    both = s + "N" + R.rev_comp(s)
    seen = set()
    for i in range(len(both) - k + 1):
        w = both[i:i + k]
        if "N" in w:
            continue
        if w in seen:
            return True
        seen.add(w)
    return False


def dip_reads(genome, p=DIP):
    """every READ_LEN-base window of genome[0 : p + 20] and of genome[p - 20 :], each COPIES times: every 21-mer is then seen
    >= COPIES times, and the 55-mers that start in (p - 35, p - 20) are in no read"""
    left, right = genome[:p + 20], genome[p - 20:]
    reads = [part[i:i + READ_LEN] for part in (left, right) for i in range(len(part) - READ_LEN + 1)]
    return reads * COPIES


def linear_genome(k1, n, seed):
    """n random bases in which no k1-mer repeats on either strand and which is not its own reverse complement: one edge of
    n - k1 bases and its twin"""
    for t in range(64):
        s = rand_seq(random.Random(seed * 64 + t), n)
        if n < k1 or (not repeats_kmer(s, k1) and s != R.rev_comp(s)):
            return s
    raise AssertionError("no linear genome found")
