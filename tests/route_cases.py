"""route_cases.py — the shared inputs of tests/test_route_cpu.py and tests/test_route_gpu.py (test infrastructure).

Read sets of 200 reads — four tiles of the routing kernels: 64 + 64 + 64 + 8 — whose lengths sit on the edges of the record
cutting rule (tests/route_ref.py): no window (0, k - 1 bases), one and two windows (k, k + 1), one block of 64 windows less
one, exactly one block, one block and one window (k + 62, k + 63, k + 64), and the declared length.  Whatever follows a read's
last base inside its record — the rest of its last byte and, with a fixed stride, the bytes up to the stride — is RANDOM, not
zero: a kernel that looks past the length byte shows.  The first four reads of a set are low-complexity (a homopolymer, (AC)n,
(ACGT)n — its own reverse complement —, the other homopolymer): one owner from end to end, so runs longer than `rmax` exist at
every P.  Everything is a pure function of (k, L): the expectations are computed once per session and shared."""
import functools
import random

import numpy as np

import route_ref as RR

NREADS = 200
K_ALL = (7, 11, 21, 31, 34, 63, 64)
P_ALL = (1, 3, 16, 64)
L_ALL = (60, 150, 255)

# (k, declared L, P): every k with every P, every L with every k that has a window in it; (31, 1) and (34, 1) have one owner
CASES = [
    (7, 60, 1), (7, 150, 3), (7, 255, 16), (7, 60, 64), (7, 255, 3), (7, 150, 16), (7, 255, 64),
    (11, 150, 1), (11, 255, 3), (11, 60, 16), (11, 150, 64), (11, 60, 3), (11, 255, 16),
    (21, 255, 1), (21, 60, 3), (21, 150, 16), (21, 255, 64), (21, 150, 3), (21, 60, 64),
    (31, 150, 1), (31, 60, 1), (31, 255, 1), (31, 150, 3), (31, 255, 16), (31, 60, 64), (31, 255, 3), (31, 150, 64),
    (34, 150, 1), (34, 60, 1), (34, 255, 1), (34, 255, 3), (34, 60, 16), (34, 150, 64), (34, 150, 16),
    (63, 150, 1), (63, 255, 3), (63, 150, 16), (63, 255, 64), (63, 150, 3),
    (64, 255, 1), (64, 150, 3), (64, 255, 16), (64, 150, 64), (64, 255, 3),
]
assert {c[0] for c in CASES} == set(K_ALL) and {c[2] for c in CASES} == set(P_ALL) and 40 <= len(CASES) <= 60
assert {(k, P) for k, _, P in CASES} == {(k, P) for k in K_ALL for P in P_ALL}

# the ragged sets (offset framing): P in {1, 3, 16}
RAGGED_CASES = [(7, 255, 16), (11, 60, 3), (21, 150, 1), (31, 150, 3), (31, 255, 16), (34, 150, 1), (34, 255, 16), (63, 255, 3), (64, 150, 16), (64, 255, 1)]
# the mixed regroup set
MIXED_K, MIXED_P, MIXED_L = 7, 16, 255


def edge_lengths(k, L):
    return sorted({n for n in (0, k - 1, k, k + 1, k + 62, k + 63, k + 64, L) if n <= L})


def _random_value(rnd, n):
    return rnd.getrandbits(2 * n) if n else 0


def _pattern(unit, n):
    codes = ["AGCT".index(c) for c in unit]
    return sum(codes[i % len(codes)] << (2 * i) for i in range(n))


def make_reads(k, L, short_tile=False):
    """[(value, length)] x NREADS.  short_tile: the second tile (reads 64..127) holds only reads shorter than k."""
    rnd = random.Random(100000 * k + 10 * L + (1 if short_tile else 0))
    lens = edge_lengths(k, L)
    picks = [lens[i % len(lens)] for i in range(NREADS)]            # every edge length 25 times ...
    rnd.shuffle(picks)                                               # ... in any order
    reads = [(_random_value(rnd, n), n) for n in picks]
    for i, unit in enumerate(("A", "AC", "ACGT", "T")):
        reads[i] = (_pattern(unit, L), L)
    if short_tile:
        short = [n for n in lens if n < k]
        for i in range(64, 128):
            n = short[i % len(short)]
            reads[i] = (_random_value(rnd, n), n)
    return reads


def pack_fixed(reads, L, seed):
    """-> uint8 array (nreads, stride): [len][bases][random], every record 1 + ceil(L / 4) bytes"""
    rnd = random.Random(seed)
    stride = 1 + (L + 3) // 4
    out = np.zeros((len(reads), stride), np.uint8)
    for r, (v, n) in enumerate(reads):
        assert n <= L and v >> (2 * n) == 0
        body = v | (rnd.getrandbits(8 * (stride - 1) - 2 * n) << (2 * n)) if 8 * (stride - 1) > 2 * n else v
        out[r] = np.frombuffer(bytes([n]) + body.to_bytes(stride - 1, "little"), np.uint8)
    return out


def pack_ragged(reads, seed):
    """-> (uint8 array, uint32 offsets of nreads + 1): the records back to back, each 1 + ceil(len / 4) bytes; the bits of a
    record's last byte past its last base are random"""
    rnd = random.Random(seed)
    out = bytearray()
    off = [0]
    for v, n in reads:
        nb = (n + 3) // 4
        body = v | (rnd.getrandbits(8 * nb - 2 * n) << (2 * n)) if 8 * nb > 2 * n else v
        out += bytes([n]) + body.to_bytes(nb, "little")
        off.append(len(out))
    return np.frombuffer(bytes(out), np.uint8).copy(), np.array(off, np.uint32)


@functools.lru_cache(maxsize=None)
def fixed_set(k, L):
    """-> (records array (NREADS, stride), FixedStride view of it)"""
    rec = pack_fixed(make_reads(k, L), L, seed=k * 7 + L)
    rec.setflags(write=False)
    return rec, RR.FixedStride(rec.tobytes(), NREADS, L)


@functools.lru_cache(maxsize=None)
def ragged_set(k, L):
    """-> (byte array, offsets array, OffsetTable view, windows): the lengths of fixed_set(k, L) with one tile of short reads"""
    reads = make_reads(k, L, short_tile=True)
    buf, off = pack_ragged(reads, seed=k * 11 + L)
    buf.setflags(write=False); off.setflags(write=False)
    return buf, off, RR.OffsetTable(buf.tobytes(), [int(x) for x in off]), sum(max(0, n - k + 1) for _, n in reads)


@functools.lru_cache(maxsize=None)
def uniform_set(k, L):
    """every read exactly L long: the one stream both framings describe"""
    rnd = random.Random(k * 13 + L)
    reads = [(_random_value(rnd, L), L) for _ in range(NREADS)]
    rec = pack_fixed(reads, L, seed=1)
    stride = rec.shape[1]
    off = np.arange(NREADS + 1, dtype=np.uint32) * np.uint32(stride)
    rec.setflags(write=False)
    return rec, off, RR.FixedStride(rec.tobytes(), NREADS, L)


@functools.lru_cache(maxsize=None)
def mixed_set():
    """k = 7, P = 16, declared 255: the first tile's reads are 255 long (more runs than the kernel's descriptor list holds: the
    tile is redone in groups of 16), every later read k + 3 (those tiles fit)"""
    k, L = MIXED_K, MIXED_L
    rnd = random.Random(4242)
    reads = [(_random_value(rnd, L), L) for _ in range(64)] + [(_random_value(rnd, k + 3), k + 3) for _ in range(NREADS - 64)]
    rec = pack_fixed(reads, L, seed=2)
    rec.setflags(write=False)
    return rec, RR.FixedStride(rec.tobytes(), NREADS, L)


@functools.lru_cache(maxsize=None)
def expected_records(kind, k, L, P):
    """superkmer_records of a set: kind = "fixed" | "ragged" | "uniform" | "mixed" """
    return RR.superkmer_records(view(kind, k, L), k, P)


@functools.lru_cache(maxsize=None)
def expected_keys(kind, k, L, P):
    return RR.shard_keys(view(kind, k, L), k, P)


def view(kind, k, L):
    if kind == "fixed":
        return fixed_set(k, L)[1]
    if kind == "ragged":
        return ragged_set(k, L)[2]
    if kind == "uniform":
        return uniform_set(k, L)[2]
    assert kind == "mixed" and (k, L) == (MIXED_K, MIXED_L)
    return mixed_set()[1]
