"""A planted read set for graph_builder --remove-weak (tests/test_weak_host_gpu.py; tests/test_weak_cpu.py checks it with the oracle
and the restatement alone): two random 600-base segments, each read error-free at about 60x — a 100-base read from every fifth
start, four times over: 64 reads over every 21-mer away from the ends — and 3 chimeric reads that follow the first segment up to
its middle and go on with the second from its middle.  At k = 21 and rounds = 2 the chimera's 20 windows of its own (count 3)
make one edge of 21 bases between the middles of the two segments, 22 windows with sum 67 + 67 + 20 * 3 = 194 (mean 8.8); its
weakest competitor, a half segment whose coverage tapers towards the segment's end, has sum 15610 over 280 windows (mean 55.8):
5 * 194 * 280 = 271600 < 15610 * 22 = 343420, so the rule removes it (and its twin), and simplifyGraph makes each segment one
contig per strand again.  It is no tip and has no parallel edge: the tip and bubble rules leave it alone.
"""
import random

K, ROUNDS, SEG, READ, STEP, COPIES, CHIMERAS, MID = 21, 2, 600, 100, 5, 4, 3, 300
SEED = 20


def segments():
    rnd = random.Random(SEED)
    return ["".join(rnd.choice("AGCT") for _ in range(SEG)) for _ in range(2)]


def reads():
    """an even number of reads (a `.bin` stream of pairs): 2 * 101 * 4 tiling reads, 3 chimeras and one more tiling read"""
    s1, s2 = segments()
    out = [s[p:p + READ] for s in (s1, s2) for p in range(0, SEG - READ + 1, STEP)] * COPIES
    out += [s1[MID - READ // 2:MID] + s2[MID:MID + READ // 2]] * CHIMERAS + [s1[:READ]]
    assert len(out) % 2 == 0
    return out


def bridge():
    """the chimeric edge as (start k-mer, end k-mer, seq)"""
    s1, s2 = segments()
    return (s1[MID - K:MID], s2[MID:MID + K], s2[MID:MID + K])
