"""PartitionedDNAMap[Int] over the GPUs of one node (S/ds/PartitionedDNAMap.scala:15-64), one rank per GPU, behind the
C-ABI's gk_dist_* entry points (RCCL over xGMI inside the library — no torch on the data path).

The Python side only carries the 128-byte RCCL id from rank 0 to the others (any channel will do: bench.py uses
torch.distributed's broadcast, a C++ host a file or MPI, the Scala driver its Akka channel)."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L
from .dnamap import Context, HipDNAMap


def unique_id() -> bytes:
    """rank 0: a fresh RCCL id (128 bytes) to hand to every rank"""
    buf = C.create_string_buffer(128)
    L.check(L.lib().gk_dist_unique_id(buf))
    return buf.raw


def share_id(rank: int, world: int, make_id=unique_id, backend: str = "gloo") -> bytes:
    """Bootstrap over torch.distributed (what bench.py does; a JVM host uses its own channel): rank 0 makes the 128-byte id,
    everybody gets it.  RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT come from the launcher; the process group is created
    here if there is none.  Only the id travels this way — the data path is RCCL inside the library."""
    import torch
    import torch.distributed as td
    if not td.is_initialized():
        td.init_process_group(backend, rank=rank, world_size=world)
    idt = torch.zeros(128, dtype=torch.uint8)
    if rank == 0:
        raw = make_id()
        assert len(raw) == 128
        idt = torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone()
    td.broadcast(idt, 0)
    return bytes(idt.numpy().tobytes())


class HipDist:
    """One rank of the communicator (gk_dist_create is collective: every rank calls it with the same id)."""

    def __init__(self, ctx: Context, rank: int, world: int, id128: bytes, loopback: bool = False):
        """loopback: the test transport (gk_dist_create_loopback) — the ranks are threads of this process on one device."""
        assert len(id128) == 128
        self.ctx, self.rank, self.world = ctx, rank, world
        self.h = L.vp()
        create = L.test_hook("gk_dist_create_loopback") if loopback else L.lib().gk_dist_create
        L.check(create(ctx.h, rank, world, C.create_string_buffer(id128, 128), C.byref(self.h)), ctx.h)

    def close(self):
        if self.h:
            if self.ctx.h:               # (a handle that outlived its context is dropped, not followed: gk_dist_destroy uses the context)
                L.lib().gk_dist_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def barrier(self):
        L.check(L.lib().gk_dist_barrier(self.h), self.ctx.h)

    def allreduce(self, values, op: str = "sum") -> np.ndarray:
        v = np.ascontiguousarray(values, np.float64).copy()
        L.check(L.lib().gk_dist_allreduce_f64(self.h, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), 1 if op == "max" else 0), self.ctx.h)
        return v

    def reduce_support(self, graph, support):
        """COLLECTIVE (gk_dist_reduce_support): every rank's `support` (its share of the pairs walked on its replica `graph`)
        becomes the sum over all ranks, in this rank's own edge ids.  The replicas may number differently but must hold the same
        edges (refused on every rank with GK_E_STATE otherwise, or after a node split); on any
        failure every rank raises and every support is unchanged.  `graph` / `support` may be None on a rank that cannot take
        part: it still joins the agreement, and every rank raises."""
        L.check(L.lib().gk_dist_reduce_support(self.h, graph.h if graph is not None else None,
                                               support.h if support is not None else None), self.ctx.h)

    def reduce_links(self, graph, links):
        """COLLECTIVE (gk_dist_reduce_links): every rank's `links` (HipGraph.pairLinks of its share of the pairs on its replica
        `graph`) becomes the element-wise sum over all ranks, in this rank's own edge ids.  The graph may be edited (split,
        simplified): the records travel in a numbering by path content (include/genome_amd.h, "the path key"), so the replicas
        must hold the same edge paths (GK_E_STATE on every rank otherwise) and no record may name a dead edge or one of two
        edges with equal paths.  On any failure every rank raises and every table is unchanged.  `graph` / `links` may be None
        on a rank that cannot take part: it still joins the agreement, and every rank raises."""
        L.check(L.lib().gk_dist_reduce_links(self.h, graph.h if graph is not None else None, links.h if links is not None else None), self.ctx.h)

    def reduce_spans(self, graph, spans):
        """COLLECTIVE (gk_dist_reduce_spans): reduce_links for a span table, (e, m, f) -> count: every rank's `spans`
        (HipGraph.threadSpans of its share of the reads) becomes the sum over all ranks, in this rank's own edge ids."""
        L.check(L.lib().gk_dist_reduce_spans(self.h, graph.h if graph is not None else None, spans.h if spans is not None else None), self.ctx.h)

    def pair_distances(self, graph, positions, bin_bytes, npairs: int, bins: int = 4096):
        """COLLECTIVE (gk_dist_pair_distances): HipGraph.pairDistances of this rank's share of the pairs on its replica, summed
        over the ranks -> (hist, classes) of ALL pairs on every rank.  `graph` / `positions` may be None on a rank that cannot
        take part: it still joins the agreement, and every rank raises."""
        from .graph import PAIR_CLASSES
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        hist, cls = np.zeros(max(int(bins), 1), np.uint64), np.zeros(len(PAIR_CLASSES), np.uint64)
        L.check(L.lib().gk_dist_pair_distances(self.h, graph.h if graph is not None else None, positions.h if positions is not None else None,
                                               L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, npairs, int(bins),
                                               L.ptr(hist, C.c_uint64), L.ptr(cls, C.c_uint64)), self.ctx.h)
        return hist, dict(zip(PAIR_CLASSES, (int(x) for x in cls)))

    def last_ms(self):
        ms = (C.c_float * 4)()
        L.check(L.lib().gk_dist_last_ms(self.h, ms), self.ctx.h)
        return dict(zip(("route_wait", "exchange", "owner_count", "total"), (float(x) for x in ms)))


class DistDNAMap:
    """`PartitionedDNAMap[Int]` with one partition per rank: this object is ONE rank's view (its partition + the communicator)."""

    def __init__(self, dist: HipDist, k: int, capacity_hint: int = 0):
        self.dist, self.ctx, self.k = dist, dist.ctx, k
        self.local = HipDNAMap(dist.ctx, k, capacity_hint)

    def close(self):
        self.local.close()

    def count_reads_dev(self, d_records: int, nreads: int, read_len: int):
        """FreqFilter.add over this rank's reads -> (windows sent, windows this rank counted as owner)."""
        sent, owned = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_dist_count_reads_dev(self.dist.h, self.local.h, d_records, nreads, read_len, C.byref(sent), C.byref(owned)), self.ctx.h)
        return sent.value, owned.value

    def count_reads(self, bin_bytes, nreads: int):
        """FreqFilter.add over this rank's share of the reads as a host `.bin` stream (ragged mates allowed; any length, 0 included)
        -> (windows sent, windows this rank counted as owner).  COLLECTIVE: a malformed stream on any rank raises GK_E_FORMAT on
        every rank with every local map unchanged; a failure after streaming began raises on every rank and leaves the local map
        with an unspecified part of the counts (clear it)."""
        buf = np.frombuffer(bin_bytes, np.uint8) if not isinstance(bin_bytes, np.ndarray) else np.ascontiguousarray(bin_bytes, np.uint8).reshape(-1)
        sent, owned = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_dist_count_reads(self.dist.h, self.local.h, L.ptr(buf, C.c_uint8) if buf.size else None, buf.size, nreads,
                                            C.byref(sent), C.byref(owned)), self.ctx.h)
        return sent.value, owned.value

    def route_begin(self, d_records: int, nreads: int, read_len: int):
        """First half of count_reads_dev, asynchronous: route the batch on the second stream.  Call it for batch i+1 before
        count_routed() of batch i and the routing kernel hides behind the owner pipeline; with batch i+2 begun as well (three
        is the limit), count_routed(i) also posts the exchange of batch i+1 beside the count of batch i."""
        L.check(L.lib().gk_dist_route_begin(self.dist.h, self.k, d_records, nreads, read_len), self.ctx.h)

    def count_routed(self):
        """Second half: exchange and count the batch route_begin started -> (windows sent, windows counted as owner)."""
        sent, owned = C.c_uint64(), C.c_uint64()
        L.check(L.lib().gk_dist_count_routed(self.dist.h, self.local.h, C.byref(sent), C.byref(owned)), self.ctx.h)
        return sent.value, owned.value

    def size(self) -> int:                                    # PartitionedDNAMap.scala:31
        n = C.c_uint64()
        L.check(L.lib().gk_dist_size(self.dist.h, self.local.h, C.byref(n)), self.ctx.h)
        return n.value

    def spectrum(self, bins: int = 4096) -> dict:
        """The count spectrum of the WHOLE map on every rank (gk_dist_spectrum; HipDNAMap.spectrum's keys).  COLLECTIVE: a rank
        whose local pass fails still takes part, and every rank raises."""
        hist = np.zeros(bins, np.uint64)
        n, occ, mx = C.c_uint64(), C.c_uint64(), C.c_uint32()
        L.check(L.lib().gk_dist_spectrum(self.dist.h, self.local.h if self.local is not None else None, L.ptr(hist, C.c_uint64), bins,
                                         C.byref(n), C.byref(occ), C.byref(mx)), self.ctx.h)
        return {"hist": hist, "distinct": n.value, "occurrences": occ.value, "max_count": mx.value}

    def deleteAll_lt(self, rounds: int):                      # :49-51 — local on every rank
        self.local.deleteAll_lt(rounds)

    def gathered(self, classified: bool = False) -> HipDNAMap:
        """every partition's survivors in one table on this rank (what Graph.buildGraph needs).  classified: the keys' owners
        classify them first (Graph.scala:320-329 on every partition, PartitionedDNAMap.scala:55-58: local lookups + one query
        all-to-all) and the degree masks travel with the keys — buildGraph on the result then skips its neighbour lookups."""
        h = L.vp()
        f = L.lib().gk_dist_gather_classified_map if classified else L.lib().gk_dist_gather_map
        L.check(f(self.dist.h, self.local.h, C.byref(h)), self.ctx.h)
        return HipDNAMap.adopt(self.ctx, self.k, h)

    def classify_queries(self) -> int:
        """neighbour lookups this rank has asked of other ranks in classified gathers"""
        n = C.c_uint64()
        L.check(L.lib().gk_dist_classify_queries(self.dist.h, C.byref(n)), self.ctx.h)
        return n.value
