"""FASTQ text to the `.bin` read stream, parsed on the GPU: the twin of Convert2bin (S/scripts/Convert2bin.scala).

The conversion rules and this converter's deviations from the reference are stated in include/genome_amd.h ("FASTQ").
"""
from __future__ import annotations

import ctypes as C
import gzip
import os
import sys

import numpy as np

from . import _lib as L


def _text(text):
    """bytes / bytearray / memoryview / uint8 array -> a contiguous uint8 array (no copy where possible)"""
    if isinstance(text, np.ndarray):
        return np.ascontiguousarray(text, np.uint8).reshape(-1)
    return np.frombuffer(text, np.uint8)


class FastqReader:
    """A FASTQ conversion in progress (gk_fastq): feed the text in pieces of any size, the last one with last=True.

    split_at >= 1: Convert2bin's n (each line split into two mates); 0: interleaved (records 2i, 2i+1 are pair i).
    k_stats: the k of the `kmers` / `short_pairs` statistics.  max_pairs: emit only the first so many pairs (0: all)."""

    def __init__(self, ctx, split_at: int = 36, k_stats: int = 23, max_pairs: int = 0):
        self.ctx = ctx
        self.h = L.vp()
        L.check(L.lib().gk_fastq_create(ctx.h, int(split_at), int(k_stats), int(max_pairs), C.byref(self.h)), ctx.h)

    def close(self):
        if self.h:
            if self.ctx.h:               # (a handle that outlived its context — a failed test's traceback — is dropped, not followed)
                L.lib().gk_fastq_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def carried(self) -> int:
        return self.stats()["carried_bytes"]

    def convert(self, text, last: bool = False) -> bytes:
        """the `.bin` records of every pair this piece completes"""
        buf = _text(text)
        cap = self.carried() + buf.size
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_size_t()
        L.check(L.lib().gk_fastq_convert(self.h, buf.ctypes.data if buf.size else None, buf.size, 1 if last else 0, out.ctypes.data, cap,
                                         C.byref(n)), self.ctx.h)
        return out[:n.value].tobytes()

    def count(self, dnamap, text, last: bool = False) -> int:
        """count the k-mers of every mate this piece completes into dnamap (FreqFilter.add); -> windows counted"""
        buf = _text(text)
        occ = C.c_uint64()
        L.check(L.lib().gk_fastq_count(self.h, dnamap.h, buf.ctypes.data if buf.size else None, buf.size, 1 if last else 0, C.byref(occ)),
                self.ctx.h)
        return occ.value

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in range(5)]
        L.check(L.lib().gk_fastq_stats(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("pairs", "short_pairs", "kmers", "text_bytes", "carried_bytes"), (x.value for x in v)))

    def last_ms(self) -> dict:
        out = (C.c_float * 4)()
        L.check(L.lib().gk_fastq_last_ms(self.h, out), self.ctx.h)
        return dict(zip(("upload", "kernels", "sink", "total"), list(out)))


def _open(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def iter_pieces(path, piece_bytes: int):
    """the file's bytes in pieces (a `.gz` file decompressed with the standard library); the last piece is flagged"""
    with _open(path) as f:
        cur = f.read(piece_bytes)
        while True:
            nxt = f.read(piece_bytes) if cur else b""
            yield cur, not nxt
            if not nxt:
                return
            cur = nxt


def convert2bin(ctx, fastq_path, out_prefix, split_at: int = 36, k: int = 23, piece_bytes: int = 256 << 20) -> dict:
    """Convert2bin.main: write <out_prefix>.bin (through <out_prefix>.bin.tmp and a rename) and return the statistics
    (pairs, kmers, short_pairs, bin_bytes, text_bytes)."""
    out_path = str(out_prefix) + ".bin"
    tmp = out_path + ".tmp"
    bin_bytes = 0
    with FastqReader(ctx, split_at, k) as rd:
        try:
            with open(tmp, "wb") as f:
                for piece, last in iter_pieces(fastq_path, piece_bytes):
                    b = rd.convert(piece, last=last)
                    f.write(b)
                    bin_bytes += len(b)
            os.replace(tmp, out_path)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise
        st = rd.stats()
    return {"pairs": st["pairs"], "kmers": st["kmers"], "short_pairs": st["short_pairs"], "bin_bytes": bin_bytes,
            "text_bytes": st["text_bytes"]}


def count_fastq(dnamap, path_or_bytes, split_at: int = 36, piece_bytes: int = 256 << 20):
    """FreqFilter.add over a FASTQ file (path, `.gz` read on the host) or its bytes -> (pairs, occurrences)"""
    occ = 0
    with FastqReader(dnamap.ctx, split_at) as rd:
        if isinstance(path_or_bytes, (str, os.PathLike)):
            for piece, last in iter_pieces(path_or_bytes, piece_bytes):
                occ += rd.count(dnamap, piece, last=last)
        else:
            occ += rd.count(dnamap, path_or_bytes, last=True)
        return rd.stats()["pairs"], occ
