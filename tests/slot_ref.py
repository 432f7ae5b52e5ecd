"""A plain restatement of where a key goes in a table segment (genome_amd/csrc/gk_device.h read as the specification), and a
finder of ADVERSARIAL keys: keys that share their first stored word and their start position.  numpy only; test infrastructure.

Every slot layout but the 16-byte Slot<1> stores a key as two separately claimed words, and the claim protocol (seg_add,
seg_claim_unique, seg_find and their LDS forms) only matters when two keys of one probe chain share the FIRST of them.  Keys
from random genomes never do (2^-31 x 2^-11 per pair for the 12-byte count slot, essentially never for 63-bit halves), but the
slot hash is a fixed bijection of the key, so such keys are cheap to search for: fix the first stored word, vary the bits that
land in the second, hash, bucket by start position.

  layout                 gk_map_stats "last_slot"   k        bits free in the second word
  12-byte count slots    count12                    27, 31   23, 31
  24-byte slots          slot24                     47, 63   31, 63
  24-byte tagged slots   slot24 (k = 64)            64       63 (the last base is the TAG: fixed per group, kept in the slot index)
  16-byte slots          slot16 (after deleteAll)   27, 31   the control: one 64-bit word, no shared-word hazard, same chains

k = 21 and k = 35 are NOT usable: a 21-mer has 42 bits, 11 above the 31 of the first word; a 35-mer has 70, 7 above the 63 — 2^11
or 2^7 keys in all over 2048 / 1024 start positions, nowhere near a group.

The scalar functions take and return Python ints (the tests check the finder's output with them, one key at a time); the
`_np` forms are the same arithmetic on uint64 arrays and exist only for the search.
The hash rule (which orientation of a k-mer is the stored one) is NOT restated here: it is oracle/pyref.py's.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import pyref as R

M64 = (1 << 64) - 1
M63 = (1 << 63) - 1
M31 = (1 << 31) - 1
KEY_EMPTY, KEY_TOMB = M64, M64 - 1                      # 64-bit key words (Slot<1>, Slot<2>)
KEY_EMPTY32, KEY_TOMB32 = 0xFFFFFFFF, 0xFFFFFFFE        # 32-bit key words (CSlot)
SEG_BITS = {1: 11, 2: 10}                               # SegBits<W>: 2048 slots of 8-byte keys, 1024 of 16-byte keys
GOLDEN = 0x9E3779B97F4A7C15
KS = {"count12": (27, 31), "slot24": (47, 63), "tagged": (64,), "slot16": (27, 31)}


def words_for_k(k: int) -> int:
    return 1 if k <= 32 else 2


def seg_slots(k: int) -> int:
    return 1 << SEG_BITS[words_for_k(k)]


# ---- scalar restatement (Python ints) -----------------------------------------------------------------------------------
def mix64(x: int) -> int:
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def slot_hash(W: int, lo: int, hi: int = 0) -> int:
    if W == 1:
        return mix64(lo)
    return mix64(lo ^ ((mix64(hi) + GOLDEN) & M64))


def c_w0(lo: int) -> int:
    return lo & M31


def c_w1(lo: int) -> int:
    return lo >> 31


def to_stored(lo: int, hi: int):
    """Kmer<2> -> (w0, w1): bits 0..62 and 63..125 of the 128-bit k-mer; bits 126..127 (k = 64's last base) are the tag"""
    return lo & M63, (lo >> 63) | ((hi << 1) & M63)


def from_stored(w0: int, w1: int, tag: int = 0):
    return (w0 | (w1 << 63)) & M64, (w1 >> 1) | (tag << 62)


def key_tag(W: int, hi: int = 0) -> int:
    return 0 if W == 1 else hi >> 62


def seg_pos(W: int, h: int) -> int:
    return h & ((1 << SEG_BITS[W]) - 1)


def start_pos(k: int, lo: int, hi: int = 0) -> int:
    """where a key's probe starts in its segment; a tagged table (k = 64) starts at the slot of the key's tag in the 4-slot group"""
    W = words_for_k(k)
    p = seg_pos(W, slot_hash(W, lo, hi))
    return (p & ~3) | key_tag(W, hi) if k == 64 else p


def first_word(k: int, lo: int, hi: int = 0) -> int:
    """the stored word that is claimed first, in the two-word layouts (count12 for k <= 31, slot24 above)"""
    return c_w0(lo) if words_for_k(k) == 1 else to_stored(lo, hi)[0]


def is_canonical(k: int, lo: int, hi: int = 0) -> bool:
    """the key is the hash-rule orientation of its k-mer (oracle/pyref.py canon): a read of exactly k bases holding it counts IT"""
    s = R.unpack(lo, hi, k)
    return R.canon(s) == s


# ---- the same on uint64 arrays --------------------------------------------------------------------------------------------
def mix64_np(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def slot_hash_np(W: int, lo: np.ndarray, hi: np.ndarray | None = None) -> np.ndarray:
    if W == 1:
        return mix64_np(lo)
    with np.errstate(over="ignore"):
        return mix64_np(lo ^ (mix64_np(hi) + np.uint64(GOLDEN)))


# ---- the finder -----------------------------------------------------------------------------------------------------------
@dataclass
class Group:
    start: int                      # restated start position of every key and sibling
    tag: int                        # k = 64: the keys' last base; 0 otherwise
    keys: list                      # [(lo, hi)] Python ints: to be inserted
    siblings: list                  # [(lo, hi)]: same first word, same start (and tag), NEVER inserted


@dataclass
class Groups:
    k: int
    W: int
    S: int                          # slots per segment
    tagged: bool
    w0: int                         # the first stored word every key and sibling shares
    groups: list = field(default_factory=list)

    def keys(self):
        return [kk for g in self.groups for kk in g.keys]

    def siblings(self):
        return [kk for g in self.groups for kk in g.siblings]


def arrays(keys):
    """[(lo, hi)] -> (lo, hi) uint64 arrays, as the maps' batch calls take them"""
    return np.array([a for a, _ in keys], np.uint64), np.array([b for _, b in keys], np.uint64)


N_SIBLINGS = 16


def find_groups(k: int, n_groups: int, group_size: int, canonical_only: bool = False, seed: int = 0, per_start: int = 1024) -> Groups:
    """n_groups groups of group_size keys, all with ONE first stored word; inside a group one start position (and, k = 64, one
    tag), plus N_SIBLINGS more keys of the same kind per group that the caller never inserts.  Group 0 starts at the LAST
    position of a segment (k = 64: in the last 4-slot group), the others in the lower half of the segment (their chains do not
    wrap), groups 1 and 2 (k = 64: 1 and 5, which share a tag) three slots (one 4-slot group) apart, so their chains run into
    each other.  k = 64: group g has tag g % 4.  per_start: candidates enumerated per start position, on average."""
    W = words_for_k(k)
    if (W == 1 and not 27 <= k <= 31) or (W == 2 and k < 47):
        raise ValueError(f"k={k}: too few bits in the second stored word to fill a group")
    S = 1 << SEG_BITS[W]
    tagged = k == 64
    rng = np.random.default_rng([seed, k])
    free = 2 * k - 31 if W == 1 else 2 * (k - 32) + 1 - (2 if tagged else 0)
    while True:
        w0 = int(rng.integers(0, 1 << 31)) if W == 1 else int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 2)) << 62)
        if not canonical_only:
            break
        # For 8-byte keys the hash rule compares 32-bit folds of x and rc(x) whose top bits both come from the first word: some
        # first words have NO canonical key at all.  Keep one under which a sample of keys is canonical about as often as not.
        sample = [int(x) for x in rng.integers(0, 1 << min(free, 62), 48)]
        keys = [(w0 | (x << 31), 0) if W == 1 else from_stored(w0, x, 0) for x in sample]
        if sum(is_canonical(k, lo, hi) for lo, hi in keys) >= 12:
            break
    need = (group_size + N_SIBLINGS) * (3 if canonical_only else 1)
    per_start = max(per_start, 2 * need)
    n = min((S // 4 if tagged else S) * per_start, 1 << free)
    # n distinct values of the free bits: i -> i * odd is a bijection of Z / 2^free
    odd = np.uint64(int(rng.integers(0, 1 << 62)) * 2 + 1)
    with np.errstate(over="ignore"):
        v = (np.arange(n, dtype=np.uint64) * odd) & np.uint64((1 << free) - 1)

    def candidates(tag):
        if W == 1:
            lo = np.uint64(w0) | (v << np.uint64(31))
            return lo, np.zeros_like(lo), mix64_np(lo) & np.uint64(S - 1)
        lo = np.uint64(w0) | ((v & np.uint64(1)) << np.uint64(63))          # v is the second stored word (without the tag)
        hi = (v >> np.uint64(1)) | np.uint64(tag << 62)
        pos = slot_hash_np(2, lo, hi) & np.uint64(S - 1)
        if tagged:
            pos = (pos & np.uint64(S - 4)) | np.uint64(tag)
        return lo, hi, pos

    # start positions, valid by construction: group 0 last; the others are distinct EVEN units of the lower half, and the group
    # that runs into group a's chain starts one unit above a's (an odd unit: nobody else's, and still in the lower half)
    unit = 4 if tagged else 1
    step = 4 if tagged else 3                    # slots between the two chains that run into each other
    even = rng.permutation(S // 2 // unit // 4)[:n_groups] * (4 * unit)
    starts = [S - unit] + [int(x) for x in even[:n_groups - 1]]
    a, b = (1, 5) if tagged else (1, 2)
    if n_groups > b:
        starts[b] = starts[a] + step
    assert len(set(starts)) == n_groups and all(x < S // 2 for x in starts[1:])
    out = Groups(k, W, S, tagged, w0)
    cache = {}
    for g in range(n_groups):
        tag = g % 4 if tagged else 0
        if tag not in cache:
            cache[tag] = candidates(tag)
        lo, hi, pos = cache[tag]
        start = starts[g] | tag
        idx = np.flatnonzero(pos == np.uint64(start))
        found = []
        for i in idx:
            key = (int(lo[i]), int(hi[i]))
            if canonical_only and not is_canonical(k, *key):
                continue
            found.append(key)
            if len(found) == group_size + N_SIBLINGS:
                break
        if len(found) < group_size + N_SIBLINGS:
            raise ValueError(f"k={k}: only {len(found)} of {group_size + N_SIBLINGS} keys at start {start}: raise per_start")
        out.groups.append(Group(start, tag, found[:group_size], found[group_size:]))
    return out
