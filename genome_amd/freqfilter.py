"""FreqFilter.extractFilteredKmers (S/data/FreqFilter.scala:25-58) on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .dnamap import Context, HipDNAMap
from .partitioned import PartitionedDNAMap

DEFAULT_ROUNDS = 3          # GraphBuilder.scala:30: what `rounds="auto"` falls back to when the spectrum has no valley


def spectrum_cutoff(hist, min_count: int = 1) -> tuple[int, int, int]:
    """gk_spectrum_cutoff (pure host code: no GPU needed) -> (valley, peak, genome_size); (0, 0, 0) = no valley.  The last
    entry of `hist` is the overflow bin and is never looked at.  min_count = 2 for a table counted through the singleton
    pre-filter, whose bin 1 is incomplete by construction."""
    h = np.ascontiguousarray(hist, np.uint64)
    v, p, g = C.c_uint32(), C.c_uint32(), C.c_uint64()
    L.check(L.lib().gk_spectrum_cutoff(L.ptr(h, C.c_uint64), len(h), min_count, C.byref(v), C.byref(p), C.byref(g)))
    return v.value, p.value, g.value


def auto_rounds(kmers, min_count: int = 1, bins: int = 4096) -> dict:
    """The spectrum of `kmers` (anything with .spectrum(bins)) and the cutoff it suggests -> {"rounds", "rounds_auto", "valley",
    "peak", "genome_size_estimate", "spectrum"}: rounds = the valley, or DEFAULT_ROUNDS when there is none (rounds_auto False)."""
    spec = kmers.spectrum(bins)
    valley, peak, gsize = spectrum_cutoff(spec["hist"], min_count)
    return {"rounds": valley if valley else DEFAULT_ROUNDS, "rounds_auto": bool(valley), "valley": valley, "peak": peak,
            "genome_size_estimate": gsize, "spectrum": spec}


class PairedEndData:
    """S/data/PairedEndData.scala:11-36: `count` pairs in a `.bin` record stream (2 records/pair).
    The Java-serialised descriptor (:14-18, :39-42) is replaced by explicit fields."""

    def __init__(self, count: int, bin_bytes: bytes, insert: int = 0):
        self.count, self.bin, self.insert = count, bin_bytes, insert


def extractFilteredKmers(data: PairedEndData, k: int, rounds, ctx: Context | None = None,
                         take_first: int | None = None, partitions: int = 1, capacity_hint: int = 0,
                         prefilter_distinct: int = 0):
    """Count every canonical k-mer of the first `take_first` pairs (genome.takeFirst,
    FreqFilter.scala:40,44), then deleteAll(v < rounds) (:55).  Returns the DNAMap[Int].

    prefilter_distinct > 0 (single partition, rounds >= 2): run the exact two-pass singleton
    pre-filter sized for that many distinct k-mers first (genome_amd/prefilter.py) — same result,
    but k-mers seen once never take a table slot, so `capacity_hint` can be the number of k-mers
    seen at least twice.

    rounds = "auto": the cutoff is the valley of the table's count spectrum (auto_rounds; min_count = 2 behind the pre-filter),
    DEFAULT_ROUNDS when the spectrum has none; the returned map carries what was chosen as `.auto` (auto_rounds' dict)."""
    auto = rounds == "auto"
    ctx = ctx or Context(0)
    pairs = data.count if take_first is None else min(take_first, data.count)
    if prefilter_distinct:
        if partitions != 1 or (not auto and rounds < 2):
            raise ValueError("the singleton pre-filter needs partitions == 1 and rounds >= 2 (it drops k-mers seen once)")
        from .prefilter import HipPrefilter
        kmers = HipDNAMap(ctx, k, capacity_hint)
        pf = HipPrefilter(ctx, k, prefilter_distinct)
        pf.add_reads(data.bin, 2 * pairs)
        pf.count_reads(kmers, data.bin, 2 * pairs)
        pf.close()
        if auto:
            kmers.auto = auto_rounds(kmers, min_count=2)
            rounds = max(2, kmers.auto["rounds"])
        kmers.deleteAll_lt(rounds)
        return kmers
    if partitions == 1:
        kmers = HipDNAMap(ctx, k, capacity_hint)
    else:
        kmers = PartitionedDNAMap(ctx, k, partitions, capacity_hint)
    kmers.count_reads(data.bin, 2 * pairs)
    if auto:
        kmers.auto = auto_rounds(kmers)
        rounds = kmers.auto["rounds"]
    kmers.deleteAll_lt(rounds)
    return kmers
