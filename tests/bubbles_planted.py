"""Genomes with planted bubbles and dead-end arms for the device tests of the edge distance and the bubble rule
(tests/test_edge_distance_gpu.py, tests/test_bubbles_gpu.py): a random genome at count C_G and, at lower counts, second copies of
stretches of it that carry a variant — the construction of tests/bubbles_cases.py, laid out along the genome by a plan.  What
the graph of the k-mers is, is for the device and the oracle to say; nothing here is an expected value.
"""
import random

from oracle import pyref as R

C_G = 10


def other(base, i=0):
    return [b for b in "AGCT" if b != base][i % 3]


def add_piece(counts, seq, c, k):
    for i in range(len(seq) - k + 1):
        key = R.canon(seq[i:i + k])
        counts[key] = counts.get(key, 0) + c


def substituted(s, places):
    s = list(s)
    for p in places:
        s[p] = other(s[p], p)
    return "".join(s)


def spread(w, n):
    """n places of 0 .. w-1, the first and the last among them, evenly spread"""
    return [0] if w == 1 else sorted({round(i * (w - 1) / (n - 1)) for i in range(n)})


def variant(kind, s, rnd):
    """the variant of the stretch s: it differs from s in its first and in its last base (what a bubble's branches do)"""
    w = len(s)
    if kind[0] == "subs":                                    # ("subs", n): n substitutions, first and last base among them
        return substituted(s, spread(w, kind[1]))
    ends = substituted(s, [0, w - 1])
    if kind[0] == "ins":                                     # ("ins", at, n): n bases more, inserted after base `at`
        return ends[:kind[1] + 1] + "".join(rnd.choice("AGCT") for _ in range(kind[2])) + ends[kind[1] + 1:]
    if kind[0] == "del":                                     # ("del", at, n): n bases fewer, from base `at` on (at >= 1, at + n < w - 1)
        return ends[:kind[1]] + ends[kind[1] + kind[2]:]
    raise ValueError(kind)


def planted(k, plan, seed, head=7):
    """plan: a list of (what, spacer) laid out left to right; `spacer` = the length of the genome's edge from this element's last
    node to the next element's branch node.  `what` is
      ("bubble", w, kind, count[, boost])  the w bases at the element's place, and a copy with variant(kind) at `count` (+ boost)
      ("arms", [tail edits], count)        dead-end arms of fewer than k bases leaving the branch node: arm i starts with the i-th
                                           base that is not the genome's; its tail is a common random one with the i-th edit:
                                           None, ("sub_last",), ("del_last",), ("ins_after_first",)
    -> (genome, counts)"""
    rnd = random.Random(seed)
    total = head + k + sum((w[1] if w[0] == "bubble" else 0) + k + s for w, s in plan) + k
    g = "".join(rnd.choice("AGCT") for _ in range(total))
    counts = {}
    add_piece(counts, g, C_G, k)
    j = head + k
    for what, spacer in plan:
        if what[0] == "bubble":
            w, kind, c = what[1], what[2], what[3]
            v = variant(kind, g[j:j + w], rnd)
            add_piece(counts, g[j - k + 1:j] + v + g[j + w:j + w + k - 1], c, k)
            j += w + k + spacer
        else:
            tail = "".join(rnd.choice("AGCT") for _ in range(k - 3))
            for i, edit in enumerate(what[1]):
                t = tail
                if edit == ("sub_last",):
                    t = tail[:-1] + other(tail[-1])
                elif edit == ("del_last",):
                    t = tail[:-1]
                elif edit == ("ins_after_first",):
                    t = other(tail[0], 1) + tail
                add_piece(counts, g[j - k + 1:j] + other(g[j], i) + t, what[2], k)
            j += spacer
    assert j <= len(g)
    return g, counts


def distance_plan(k):
    """for tests/test_edge_distance_gpu.py: SNP bubbles with the genome's edges between them of 1..5, 31..33, 63..65 and 200
    bases; branches of those lengths where k allows; dead-end arms whose tails differ by a substitution at the last base, a
    deletion at the end, an insertion right after the first base; branches of about 50 bases 1 to 4 bases apart in length and
    a few edits apart; branches of about 200 bases 31 and 32 substitutions, and 31 and 32 bases of length, apart"""
    snp = ("bubble", 1, ("subs", 1), 3)
    plan = [(snp, s) for s in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 200)]

    def branch(length, kind):
        return ("bubble", length - k, kind, 3)

    if k <= 20:
        plan += [(branch(n, ("subs", 2 + n % 3)), 6) for n in (31, 32, 33, 63, 64, 65)]
    plan += [(("arms", [None, ("sub_last",), ("del_last",)], 2), 9), (("arms", [None, ("ins_after_first",)], 2), 9),
             (branch(48, ("ins", 0, 1)), 6), (branch(48, ("del", 3, 1)), 6), (branch(50, ("subs", 4)), 6), (branch(50, ("ins", 5, 3)), 6),
             (branch(52, ("del", 4, 4)), 6),
             (branch(200, ("subs", 31)), 6), (branch(200, ("subs", 32)), 6), (branch(201, ("ins", 100, 31)), 6), (branch(202, ("del", 50, 32)), 6)]
    return plan


def haplotype_case(k, seed, length=3000, c_hap=4):
    """for tests/test_bubbles_gpu.py: a random genome at C_G and a whole second haplotype at c_hap that differs from it every k + 8
    to k + 30 bases, in turn by a SNP, a SNP whose copy is raised to the genome's own count (a tie), an inserted base, two deleted
    bases, four SNPs within seven bases (too far apart for max_diff = 3), two inserted bases, a deleted base -> (genome, counts)"""
    rnd = random.Random(seed)
    g = "".join(rnd.choice("AGCT") for _ in range(length))
    kinds = ("snp", "tie", "ins1", "del2", "four", "ins2", "del1")
    hap, ties, pos, at, i = [], [], k + 5, 0, 0
    while pos + 7 + k + 5 < length:
        kind = kinds[i % len(kinds)]
        w, v = {"snp": (1, None), "tie": (1, None), "ins1": (0, rnd.choice("AGCT")), "ins2": (0, rnd.choice("AGCT") + rnd.choice("AGCT")),
                "del1": (1, ""), "del2": (2, ""), "four": (7, None)}[kind]
        if v is None:
            v = substituted(g[pos:pos + w], [0, 2, 4, 6][:(w + 1) // 2])
        hap.append(g[at:pos])
        if kind == "tie":
            ties.append(sum(len(x) for x in hap))            # where the variant sits in the haplotype
        hap.append(v)
        at = pos + w
        pos = at + k + rnd.randrange(8, 31)
        i += 1
    hap = "".join(hap) + g[at:]
    counts = {}
    add_piece(counts, g, C_G, k)
    add_piece(counts, hap, c_hap, k)
    for p in ties:
        add_piece(counts, hap[p - k + 1:p + k], C_G - c_hap, k)
    return g, counts
