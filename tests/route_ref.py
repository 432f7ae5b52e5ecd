"""route_ref.py — plain-Python restatement of the owner routing (test infrastructure, NOT product code).

What csrc/gk_skm.hip (k_skm_route) and csrc/gk_shard.hip (k_shard_count / k_shard_scatter) compute, stated from the READS with
Python integers and lists: no ballots, no tiles, no LDS, and no import of the library.  A read is one Python integer (base i at
bits 2i, codes A0 G1 C2 T3: the `.bin` payload read as a little-endian number) and its length.

  owner      m = min(11, k); the score of an m-mer is hash32 of the smaller of its value and its reverse complement's value; the
             minimizer of a window is the smallest score of its k - m + 1 m-mers; owner = (hash32(minimizer ^ 0x5bd1e995) * P) >> 32.
  keys       every window's canonical k-mer (FreqFilter.scala:31-32: the smaller signed hashCode of x and rc(x), a tie -> rc(x))
             goes to its owner (shard_keys).
  records    a read of `len` bases has len - k + 1 windows (none if that is <= 0).  They are taken in blocks of 64, counted from
             the read's first window.  Inside a block every maximal run of equal owners is cut, from its start, into pieces of at
             most rmax = (slot - 1) * 4 - k + 1 windows.  A piece of wl windows starting at window p is one record of `slot` bytes
             (16 for k <= 31, 32 for k >= 34): byte 0 = wl + k - 1, then bases p .. p + wl + k - 2, 2 bits each, LSB first, the
             rest zero (superkmer_records).

Both framings of a record stream: FixedStride (record r at r * (1 + ceil(read_len / 4)); its length byte may be BELOW read_len,
and whatever follows its last base is ignored) and OffsetTable (record r at offsets[r], offsets[nreads] = the end)."""
from collections import namedtuple

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
REMIX = 0x5BD1E995


def hash32(x):
    """gk_device.h: hash32"""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def mask(nbases):
    return (1 << (2 * nbases)) - 1


def rev_comp(v, n):
    """reverse complement of the n bases of v (complement = 3 - code; Base.scala:19)"""
    r = 0
    for i in range(n):
        r |= (3 - ((v >> (2 * i)) & 3)) << (2 * (n - 1 - i))
    return r


def slot_bytes(k):
    return 16 if k <= 31 else 32


def max_run(k):
    return (slot_bytes(k) - 1) * 4 - k + 1


# ---- framings: -> [(value, length)] -------------------------------------------------------------------------------------------
class FixedStride(namedtuple("FixedStride", "buf nreads read_len")):
    def reads(self):
        stride = 1 + (self.read_len + 3) // 4
        assert len(self.buf) >= self.nreads * stride
        out = []
        for r in range(self.nreads):
            rec = bytes(self.buf[r * stride:(r + 1) * stride])
            ln = rec[0]
            if ln > self.read_len:
                raise ValueError("length byte above the declared read length")
            out.append((int.from_bytes(rec[1:], "little") & mask(ln), ln))
        return out


class OffsetTable(namedtuple("OffsetTable", "buf offsets")):
    def reads(self):
        out = []
        for a, b in zip(self.offsets[:-1], self.offsets[1:]):
            rec = bytes(self.buf[a:b])
            ln = rec[0]
            if b - a != 1 + (ln + 3) // 4:
                raise ValueError("offset table and length byte disagree")
            out.append((int.from_bytes(rec[1:], "little") & mask(ln), ln))
        return out


# ---- owner --------------------------------------------------------------------------------------------------------------------
def mmer_scores(v, n, k):
    """score of the m-mer at every position of a read (n - m + 1 of them)"""
    m = min(11, k)
    rc = rev_comp(v, n)
    out = []
    for q in range(n - m + 1):
        a = (v >> (2 * q)) & mask(m)
        b = (rc >> (2 * (n - m - q))) & mask(m)            # the reverse complement of the same m bases
        out.append(hash32(min(a, b)))
    return out


def window_minimizers(v, n, k):
    """the minimizer (smallest m-mer score) of every window of a read"""
    w = k - min(11, k) + 1
    s = mmer_scores(v, n, k)
    return [min(s[p:p + w]) for p in range(n - k + 1)]


def owner_of_minimizer(best, P):
    return (hash32(best ^ REMIX) * P) >> 32


def window_owners(v, n, k, P):
    return [owner_of_minimizer(b, P) for b in window_minimizers(v, n, k)]


def owner_of_kmer(x, k, P):
    """the owner of ONE k-mer given as a number (lo | hi << 64): gk_owner_of"""
    return window_owners(x, k, k, P)[0]


# ---- canonical keys -------------------------------------------------------------------------------------------------------------
def _s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def ref_hash(x, k):
    """the reference's hashCode of a k-mer (gk_device.h: ref_hash; DNASeq.scala:103, :204-208 with seed 42)"""
    lo, hi = x & M64, x >> 64
    if k <= 32:
        return _s32(lo ^ (lo >> 32))
    a, b = _s64(lo), _s64(hi)
    t = _s64((a ^ (a >> 32)) * 42)
    t1 = _s64((b ^ (b >> 32) ^ t) * 42)
    return _s32(t1 ^ (t1 >> 32))


def canonical(x, k):
    rc = rev_comp(x, k)
    return x if ref_hash(x, k) < ref_hash(rc, k) else rc


def shard_keys(records, k, P):
    """-> (keys, counts): keys[p] = the sorted list of canonical keys (lo, hi) of owner p's windows, counts[p] = len(keys[p])"""
    keys = [[] for _ in range(P)]
    for v, n in records.reads():
        for p, o in enumerate(window_owners(v, n, k, P)):
            y = canonical((v >> (2 * p)) & mask(k), k)
            keys[o].append((y & M64, y >> 64))
    for ks in keys:
        ks.sort()
    return keys, [len(ks) for ks in keys]


# ---- super-k-mer records ----------------------------------------------------------------------------------------------------------
def pieces_of_read(owners, k):
    """[(owner, first window, windows)] of one read, by the cutting rule"""
    rmax = max_run(k)
    out = []
    for b0 in range(0, len(owners), 64):
        blk = owners[b0:b0 + 64]
        i = 0
        while i < len(blk):
            j = i
            while j < len(blk) and blk[j] == blk[i]:
                j += 1
            for s in range(i, j, rmax):
                out.append((blk[i], b0 + s, min(rmax, j - s)))
            i = j
    return out


def record_bytes(v, p, wl, k):
    nb = wl + k - 1
    slot = slot_bytes(k)
    assert k <= nb <= (slot - 1) * 4
    return bytes([nb]) + ((v >> (2 * p)) & mask(nb)).to_bytes(slot - 1, "little")


Region = namedtuple("Region", "rows recs kmers")


def superkmer_records(records, k, P):
    """-> [Region] per owner: rows = the sorted list of its records (byte strings of slot size), recs = their number, kmers = its windows"""
    rows = [[] for _ in range(P)]
    kmers = [0] * P
    for v, n in records.reads():
        for o, p, wl in pieces_of_read(window_owners(v, n, k, P), k):
            rows[o].append(record_bytes(v, p, wl, k))
            kmers[o] += wl
    return [Region(sorted(r), len(r), c) for r, c in zip(rows, kmers)]


def runs_of_read(owners):
    """the runs the kernel's descriptor list holds for one read: maximal runs of equal owners inside blocks of 64 windows"""
    n = 0
    for b0 in range(0, len(owners), 64):
        blk = owners[b0:b0 + 64]
        n += sum(1 for i in range(len(blk)) if i == 0 or blk[i] != blk[i - 1])
    return n
