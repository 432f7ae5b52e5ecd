"""Host-side mirror of the reference's sequence primitives (S/dna/Base.scala, S/dna/DNASeq.scala):
just enough to move k-mers across the C-ABI — packing, unpacking and reverse complement of base
strings.  (Bit layout: base i at bits 2i, A0 G1 C2 T3, first base at the LSB; DNASeq.scala:84,256.)
"""
from __future__ import annotations

import numpy as np

BASES = "AGCT"                                   # Base.scala:13-18
_CODE = {c: i for i, c in enumerate(BASES)}
_COMP = {"A": "T", "T": "A", "G": "C", "C": "G"}  # Base.scala:19


def pack(seq: str) -> tuple[int, int]:
    """DNASeq.newBuilder (DNASeq.scala:237-281) -> (lo, hi)."""
    lo = hi = 0
    for i, c in enumerate(seq):
        if i < 32:
            lo |= _CODE[c] << (2 * i)
        else:
            hi |= _CODE[c] << (2 * (i - 32))
    return lo, hi


def unpack(lo: int, hi: int, k: int) -> str:
    return "".join(BASES[((lo if i < 32 else hi) >> (2 * (i % 32))) & 3] for i in range(k))


def rev_complement(seq: str) -> str:
    """DNASeq.revComplement (DNASeq.scala:27-28)."""
    return "".join(_COMP[c] for c in reversed(seq))


def pack_many(seqs) -> tuple[np.ndarray, np.ndarray]:
    lo = np.zeros(len(seqs), np.uint64)
    hi = np.zeros(len(seqs), np.uint64)
    for i, s in enumerate(seqs):
        a, b = pack(s)
        lo[i], hi[i] = a, b
    return lo, hi


def reads_to_bin(reads) -> bytes:
    """Convert2bin.write (S/scripts/Convert2bin.scala:35-38): [len:u8][toByteArray] per read."""
    out = bytearray()
    for r in reads:
        if len(r) > 255:
            raise ValueError("a .bin record holds at most 255 bases")
        out.append(len(r))
        data = bytearray((len(r) + 3) // 4)
        for i, c in enumerate(r):
            data[i // 4] |= _CODE[c] << (2 * (i % 4))
        out += data
    return bytes(out)


def unpack_2bit(buf: np.ndarray, nbases: int) -> str:
    """Edge sequences come back as 2-bit codes, 4 per byte, LSB first."""
    return "".join(BASES[(int(buf[i // 4]) >> (2 * (i % 4))) & 3] for i in range(nbases))


def bin_pair_offsets(bin_bytes, npairs: int) -> np.ndarray:
    """Byte offsets of pairs 0..npairs in a `.bin` stream of mate records ([len:u8][ceil(len/4) bytes] each, two per pair):
    entry i is where pair i starts, entry npairs where the last one ends.  ValueError if the stream ends inside a record."""
    buf = bytes(bin_bytes) if not isinstance(bin_bytes, (bytes, bytearray)) else bin_bytes
    if npairs and len(buf):
        # a stream of equal-length records (what a sequencer's run and the generators give): the offsets are arithmetic, and
        # one vectorised look at the length bytes confirms it
        stride = 1 + (buf[0] + 3) // 4
        if len(buf) >= 2 * npairs * stride:
            lens = np.frombuffer(buf, np.uint8, count=2 * npairs * stride)[::stride]
            if (lens == buf[0]).all():
                return np.arange(npairs + 1, dtype=np.int64) * (2 * stride)
    out = np.zeros(npairs + 1, np.int64)
    pos = 0
    for i in range(npairs):
        out[i] = pos
        for _ in range(2):
            if pos >= len(buf):
                raise ValueError(f"the stream ends inside pair {i}")
            pos += 1 + (buf[pos] + 3) // 4
            if pos > len(buf):
                raise ValueError(f"the stream ends inside pair {i}")
    out[npairs] = pos
    return out


def bin_pairs(bin_bytes, a: int, b: int) -> bytes:
    """Pairs [a, b) of a `.bin` stream of mate records, as a stream of their own (a rank's share for walkPairs)."""
    if not 0 <= a <= b:
        raise ValueError("need 0 <= a <= b")
    off = bin_pair_offsets(bin_bytes, b)
    return bytes(bin_bytes[int(off[a]):int(off[b])])
