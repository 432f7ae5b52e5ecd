"""The inputs of the exact pre-filter tests, shared by tests/test_prefilter_cpu.py (which holds the restatement's populations on
them) and tests/test_prefilter_gpu.py (which holds the device to the restatement).  Seeded, pure Python; the restatement of every
(case, k) is computed once per process (`restated`)."""
from __future__ import annotations

import random

import prefilter_ref as P
from oracle import pyref as R

KS_ALL = (2, 5, 21, 31, 34, 47, 63, 64)
KS_CHUNK = (21, 55)
KS_COLLIDE = (31, 47)


def _genome(rnd, n):
    return "".join(rnd.choice("AGCT") for _ in range(n))


def _mutate(rnd, r, e):
    return "".join(c if rnd.random() >= e else rnd.choice([x for x in "AGCT" if x != c]) for c in r)


def _sample(rnd, g, ln, e):
    st = rnd.randrange(0, len(g) - ln + 1)
    r = g[st:st + ln]
    if rnd.random() < 0.5:
        r = R.rev_comp(r)
    return _mutate(rnd, r, e)


def record_bytes(ln: int) -> int:
    return 1 + (ln + 3) // 4


# ---- (a) every key form --------------------------------------------------------------------------------------------------------
def ragged(k: int):
    """300 reads of k - 3 .. 255 bases from both strands of a 3000-base genome, 3 % substitutions, plus "", a 2-base read and five
    255-base reads (k = 2: 254 windows each; k = 34: 222 windows of two words)"""
    rnd = random.Random(700 + k)
    g = _genome(rnd, 3000)
    reads = [_sample(rnd, g, rnd.randint(max(1, k - 3), 255), 0.03) for _ in range(300)]
    reads += ["", "AG"] + [_sample(rnd, g, 255, 0.03) for _ in range(5)]
    rnd.shuffle(reads)
    return reads


def fixed_255(k: int):
    """70 records of 255 bases: more than one pass-2 tile at every k (32 reads per tile at k = 2, 18 at k = 34)"""
    rnd = random.Random(800 + k)
    g = _genome(rnd, 2000)
    return [_sample(rnd, g, 255, 0.03) for _ in range(70)]


def fixed_k(k: int):
    """3000 records of exactly k bases: one window per read, 47 tiles"""
    rnd = random.Random(900 + k)
    g = _genome(rnd, 1500)
    return [_sample(rnd, g, k, 0.02) for _ in range(3000)]


# ---- (b) collisions at the smallest filter (expected_distinct = 1: 262 144 buckets) -------------------------------------------
COLLIDE_GENOME, COLLIDE_READS, COLLIDE_LEN, COLLIDE_ERR = 40000, 1900, 100, 0.008
COLLIDE_SEED = {31: 3101, 47: 4701}


def collide(k: int):
    rnd = random.Random(COLLIDE_SEED[k])
    g = _genome(rnd, COLLIDE_GENOME)
    return [_sample(rnd, g, COLLIDE_LEN, COLLIDE_ERR) for _ in range(COLLIDE_READS)]


# ---- (c) host streams for the chunker -----------------------------------------------------------------------------------------
GROW_STAGE = 1000          # "test_max_stage" of grow()


def grow(k: int):
    """A ragged stream for a 1000-byte stage.  120 records of 97..100 bases (26 bytes each: chunks of 38 records, 988 bytes), then
    60 of 193..196 bases (50 bytes: chunks of 20 records, 1000 bytes and more windows than any chunk before: the staging area and
    the key buffer regrow), then 400 of k .. k + 3 bases (more records per chunk than any chunk before: the offset table regrows).
    Neighbouring records differ in length, so no chunk is a fixed-stride run."""
    rnd = random.Random(1000 + k)
    g = _genome(rnd, 4000)
    lens = [97 + (i % 4) for i in range(120)] + [193 + (i % 4) for i in range(60)] + [k + (i % 4) for i in range(400)]
    return [_sample(rnd, g, ln, 0.02) for ln in lens]


def by_windows(k: int):
    """A ragged stream that a window cap cuts long before a byte cap would: 150 reads of k .. 255 bases"""
    rnd = random.Random(1100 + k)
    g = _genome(rnd, 3000)
    return [_sample(rnd, g, rnd.randint(k, 255), 0.02) for _ in range(150)]


MIXED_CAP_RECORDS = 5000   # records of the main run that fit the stage of mixed()


def mixed_stage(k: int) -> int:
    return MIXED_CAP_RECORDS * record_bytes(k + 3)


def mixed(k: int):
    """For a stage of mixed_stage(k) bytes, in stream order:
      11 700 records of k + 3 bases  two fixed-stride chunks of 5000, then 1700 that are too few for a third;
      60 ragged records              one offset-table chunk: the 1700, these, and the head of the next run, up to the stage's bytes;
      records of 10 bases            (no window at any k here) enough that 4500 are left after that chunk: one fixed-stride chunk
                                     without a window, for which pass 2 launches nothing;
      4200 records of k + 7 bases    the closing run, taken as the whole remainder."""
    rnd = random.Random(1200 + k)
    g = _genome(rnd, 2500)
    reads = [_sample(rnd, g, k + 3, 0.01) for _ in range(2 * MIXED_CAP_RECORDS + 1700)]
    tail = [_sample(rnd, g, rnd.randint(k - 3, 255), 0.02) for _ in range(60)]
    for i in range(1, len(tail)):                        # (no two neighbours of one length, and none like the runs around)
        while len(tail[i]) in (len(tail[i - 1]), 10, k + 3):
            tail[i] = _sample(rnd, g, rnd.randint(k - 3, 255), 0.02)
    used = 1700 * record_bytes(k + 3) + sum(record_bytes(len(r)) for r in tail)
    short = (mixed_stage(k) - used) // record_bytes(10) + 4500
    reads += tail + [_sample(rnd, g, 10, 0.0) for _ in range(short)]
    reads += [_sample(rnd, g, k + 7, 0.01) for _ in range(4200)]
    return reads


# ---- (d) the `_dev` pass-2 loop: synth mode G records, as tests/test_prefilter_gpu.py's round-3 test makes them ----------------
DEV_N, DEV_L, DEV_G, DEV_E, DEV_CID = 4000, 100, 30000, 0.02, 11
DEV_CHUNK_READS = 999      # 999 x 26 bytes is no multiple of 16; 4000 records make 5 chunks


def dev_records():
    from genome_amd import synth
    return synth.reads_mode_g(DEV_N, DEV_L, DEV_G, DEV_E, DEV_CID)


def dev_loop(k: int):
    return R.reads_from_bin(dev_records().tobytes(), DEV_N)


# ---- (f) records shorter than the declared read length ------------------------------------------------------------------------
def short_records(k: int):
    """declared read_len = 100: 300 records, every seventh shorter (0, 1, k - 1, k, 60 .. 99 bases)"""
    rnd = random.Random(1300 + k)
    g = _genome(rnd, 2000)
    shorter = [0, 1, k - 1, k] + list(range(60, 100))
    return [_sample(rnd, g, shorter[(i // 7) % len(shorter)] if i % 7 == 3 else 100, 0.02) for i in range(300)]


CASES = {"ragged": ragged, "fixed_255": fixed_255, "fixed_k": fixed_k, "collide": collide, "grow": grow, "by_windows": by_windows,
         "mixed": mixed, "dev_loop": dev_loop, "short_records": short_records}

_reads: dict = {}
_restated: dict = {}


def reads(case: str, k: int):
    if (case, k) not in _reads:
        _reads[case, k] = CASES[case](k)
    return _reads[case, k]


def expected_distinct(case: str, k: int) -> int:
    if case == "collide":
        return 1                 # the smallest filter the library makes
    if case == "ragged":
        return 100003            # 400 012 buckets: no power of two, and the last counter word is partly used
    return max(1, len(P.window_counts(reads(case, k), k)))


def restated(case: str, k: int) -> P.Result:
    """the restatement of pass 1 + pass 2 over the case's reads (computed once; callers must not change it)"""
    if (case, k) not in _restated:
        _restated[case, k] = P.run(reads(case, k), k, expected_distinct(case, k))
    return _restated[case, k]


def fixed_stride_records(rds, read_len: int) -> bytes:
    """`.bin` records of one stride, 1 + (read_len + 3) / 4 bytes, zero padded (a `_dev` call's buffer)"""
    stride = record_bytes(read_len)
    out = bytearray()
    for r in rds:
        rec = R.reads_to_bin([r])
        assert len(rec) <= stride
        out += rec + bytes(stride - len(rec))
    return bytes(out)
