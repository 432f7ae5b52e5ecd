"""The path key of include/genome_amd.h ("the path key"), restated on strings and Python integers: the canonical numbering by
path content that gk_dist_reduce_links / gk_dist_reduce_spans move their records in.  Nothing here looks at the library."""

M = (1 << 64) - 1
CODE = {"A": 0, "G": 1, "C": 2, "T": 3}
GOLD, WORD, SECOND, H1, H2, FP, LIVE = 0x9e3779b97f4a7c15, 0x70617468776f7264, 0x7365636f6e64, 0x7061746831, 0x7061746832, 0x66696e676572, 0x6c697665
CHUNK_BASES = 64 * 32                     # what one wave step of the device pass takes (no part of the rule: the tests aim at it)


def mix64(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M
    return x ^ x >> 33


def fold(a, v):
    return mix64(a ^ (v + GOLD & M))


def pack(s):
    """bases as one integer, base i at bits 2i"""
    return sum(CODE[c] << 2 * i for i, c in enumerate(s))


def words(seq):
    return [pack(seq[j:j + 32]) for j in range(0, len(seq), 32)]


def path_key(k, path):
    """(h1, h2) of the path start k-mer ++ seq"""
    kmer, seq = path[:k], path[k:]
    lo, hi = pack(kmer[:32]), pack(kmer[32:])
    s1 = s2 = 0
    for j, w in enumerate(words(seq)):
        t = w ^ mix64(j + WORD & M)
        s1 = s1 + mix64(t) & M
        s2 = s2 + mix64(t ^ SECOND) & M
    h1 = fold(fold(fold(fold(H1, s1), lo), hi), len(seq))
    h2 = fold(fold(fold(fold(H2, s2), lo), hi), len(seq))
    return (M - 1 if h1 == M else h1), h2


def numbering(k, paths):
    """paths: {edge id: path of a live edge} -> (keys {id: (h1, h2)}, canon {id: place} for the ids whose key is theirs alone,
    the set of canonical places the duplicates share between them {key: sorted places}, dup ids, fingerprint)"""
    keys = {e: path_key(k, p) for e, p in paths.items()}
    order = sorted(keys, key=lambda e: keys[e])
    count = {}
    for e in order:
        count[keys[e]] = count.get(keys[e], 0) + 1
    dup = {e for e in order if count[keys[e]] > 1}
    canon = {e: i for i, e in enumerate(order) if e not in dup}
    shared = {}
    for i, e in enumerate(order):
        if e in dup:
            shared.setdefault(keys[e], []).append(i)
    fp = mix64(len(keys) ^ LIVE)
    for h1, h2 in keys.values():
        fp = fp + mix64(h1 ^ mix64(h2 + FP & M)) & M
    return keys, canon, shared, dup, fp
