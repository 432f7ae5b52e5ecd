"""A plain restatement of the exact two-pass singleton pre-filter (genome_amd/csrc/gk_prefilter.hip read as the specification).
Python / numpy only; test infrastructure.  It reads nothing from the library under test: the mixer and the slot hash are
tests/slot_ref.py's (held to the device by the adversarial-key tests), the orientation rule is oracle/pyref.py's.

The filter is `nbuckets` two-bit saturating counters (0, 1, "2 or more").
  pass 1   every k-mer window of every read bumps the counter of bucket(canonical k-mer);
  pass 2   a window enters the table iff its bucket's counter says "2 or more".
So after pass 2 the table holds exactly the k-mers whose bucket received at least two WINDOWS in pass 1 — two occurrences of
one k-mer, or one occurrence each of two k-mers that collide — and each of them with its true count.  Three populations:
  multi             k-mers of true count >= 2 (always in the table);
  single_admitted   k-mers of true count 1 whose bucket another window also hit (in the table with count 1);
  single_rejected   k-mers of true count 1 alone in their bucket (absent).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import slot_ref as S
from oracle import pyref as R

M32 = np.uint64(0xFFFFFFFF)
MIN_DISTINCT = 1 << 16
BUCKETS_PER_KMER = 4


def nbuckets(expected_distinct: int) -> int:
    return max(int(expected_distinct), MIN_DISTINCT) * BUCKETS_PER_KMER


# ---- bucket of a CANONICAL k-mer (lo, hi = oracle/pyref.py pack of pyref.canon's choice) -------------------------------------
def bucket(k: int, lo: int, hi: int, nb: int) -> int:
    W = S.words_for_k(k)
    h = S.mix64(S.slot_hash(W, lo, hi) ^ S.GOLDEN)
    return (h * nb) >> 64


def mulhi64_np(a: np.ndarray, b: int) -> np.ndarray:
    """floor(a * b / 2^64) for uint64 a and a 64-bit b, from 32-bit halves (no partial sum exceeds 64 bits)"""
    a = a.astype(np.uint64, copy=False)
    a1, a0 = a >> np.uint64(32), a & M32
    b1, b0 = np.uint64(b >> 32), np.uint64(b & 0xFFFFFFFF)
    p00, p10, p01, p11 = a0 * b0, a1 * b0, a0 * b1, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p10 & M32) + (p01 & M32)
    return p11 + (p10 >> np.uint64(32)) + (p01 >> np.uint64(32)) + (mid >> np.uint64(32))


def bucket_np(k: int, lo: np.ndarray, hi: np.ndarray, nb: int) -> np.ndarray:
    W = S.words_for_k(k)
    lo = np.asarray(lo, np.uint64)
    hi = np.asarray(hi, np.uint64)
    h = S.mix64_np(S.slot_hash_np(W, lo, hi) ^ np.uint64(S.GOLDEN))
    return mulhi64_np(h, nb)


# ---- windows of reads -> canonical keys -------------------------------------------------------------------------------------
_canon_cache: dict = {}


def canon_key(window: str):
    """(lo, hi) of the hash-rule orientation of one k-mer window (memoised: a read set repeats its windows many times)"""
    key = _canon_cache.get(window)
    if key is None:
        if len(_canon_cache) > 2_000_000:
            _canon_cache.clear()
        key = _canon_cache[window] = R.pack(R.canon(window))
    return key


def window_counts(reads, k: int) -> dict:
    """{canonical (lo, hi): number of windows}: plain counting (FreqFilter.scala:28-36)"""
    out: dict = {}
    for seq in reads:
        for p in range(len(seq) - k + 1):
            key = canon_key(seq[p:p + k])
            out[key] = out.get(key, 0) + 1
    return out


@dataclass
class Result:
    k: int
    buckets: int
    state: np.ndarray            # uint8 [buckets]: 0, 1, 2 (= "2 or more") after pass 1
    seen_once: int
    seen_twice_or_more: int
    windows: int                 # windows of pass 1 (= windows pass 2 looks at, over the same reads)
    counts: dict                 # plain counting of the pass-2 reads: {(lo, hi): count}, every k-mer
    table: dict                  # what pass 2 must leave: {(lo, hi): true count} of the k-mers whose bucket is saturated
    admitted: int                # windows pass 2 inserts = sum of table's counts
    multi: int                   # the three populations (k-mers)
    single_admitted: int
    single_rejected: int

    def sorted_table(self):
        """(lo, hi, count) arrays in the table's canonical order, (hi, lo) unsigned ascending"""
        return sorted_arrays(self.table)

    def filtered(self, rounds: int) -> dict:
        """deleteAll(v < rounds) of the pre-filtered table"""
        return {key: c for key, c in self.table.items() if c >= rounds}

    def plain_filtered(self, rounds: int) -> dict:
        """deleteAll(v < rounds) of plain counting"""
        return {key: c for key, c in self.counts.items() if c >= rounds}


def sorted_arrays(table: dict):
    keys = sorted(table, key=lambda kk: (kk[1], kk[0]))
    return (np.array([a for a, _ in keys], np.uint64), np.array([b for _, b in keys], np.uint64),
            np.array([table[kk] for kk in keys], np.int64))


class Filter:
    """The filter as a caller drives it: add() any number of times (pass 1), then count() (pass 2)."""

    def __init__(self, k: int, expected_distinct: int):
        self.k, self.buckets = k, nbuckets(expected_distinct)
        self.hits = np.zeros(self.buckets, np.int64)        # windows per bucket
        self.windows = 0

    def _buckets_of(self, keys):
        lo = np.array([a for a, _ in keys], np.uint64)
        hi = np.array([b for _, b in keys], np.uint64)
        return bucket_np(self.k, lo, hi, self.buckets).astype(np.int64)

    def add(self, reads):
        wc = window_counts(reads, self.k)
        if wc:
            keys = list(wc)
            np.add.at(self.hits, self._buckets_of(keys), np.array([wc[kk] for kk in keys], np.int64))
            self.windows += sum(wc.values())

    def count(self, reads) -> Result:
        state = np.minimum(self.hits, 2).astype(np.uint8)
        counts = window_counts(reads, self.k)
        keys = list(counts)
        sat = state[self._buckets_of(keys)] == 2 if keys else np.zeros(0, bool)
        table = {kk: counts[kk] for kk, s in zip(keys, sat) if s}
        multi = sum(1 for c in counts.values() if c >= 2)
        single_admitted = sum(1 for c in table.values() if c == 1)
        return Result(self.k, self.buckets, state, int((state == 1).sum()), int((state == 2).sum()), self.windows, counts, table,
                      sum(table.values()), multi, single_admitted, len(counts) - multi - single_admitted)


def run(reads, k: int, expected_distinct: int) -> Result:
    """pass 1 and pass 2 over the same reads"""
    return run_chunked([reads], k, expected_distinct)


def run_chunked(calls, k: int, expected_distinct: int) -> Result:
    """pass 1 as several calls (a list of read lists), pass 2 over the same reads: only the union matters"""
    f = Filter(k, expected_distinct)
    for reads in calls:
        f.add(reads)
    return f.count([r for reads in calls for r in reads])
