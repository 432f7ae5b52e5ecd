"""The rules of gk_graph_edge_distance and gk_graph_pop_bubbles (include/genome_amd.h) restated in plain Python, from the header's
text: the device is held to this value for value (tests/test_edge_distance_gpu.py, tests/test_bubbles_gpu.py), and this file to
hand-written answers (tests/test_bubbles_cpu.py).

Input as tests/tips_ref.py: `counts`, stored k-mer -> count, and `edges`, a list of (start k-mer, end k-mer, seq).  A node is
identified by its k-mer: graphs with node copies (after a node split) are outside this restatement.
"""
import numpy as np

import tips_ref as T


def levenshtein(a, b):
    """the full matrix, row by row: substitution, insertion and deletion cost 1 each"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(prev[j - 1] + (x != y), prev[j] + 1, row[j - 1] + 1))
        prev = row
    return prev[-1]


def levenshtein_many(a, bs):
    """levenshtein(a, b) for every b of `bs` -> list: the same full matrix, row by row, for all of them at once (numpy; the
    tests that compare thousands of pairs use it, tests/test_bubbles_cpu.py holds it to the function above)"""
    if not bs:
        return []
    width = max(len(b) for b in bs)
    cols = np.arange(width + 1)
    mat = np.zeros((len(bs), width), np.uint8)
    for n, b in enumerate(bs):
        mat[n, :len(b)] = np.frombuffer(b.encode(), np.uint8)
    prev = np.tile(cols, (len(bs), 1))
    for i, x in enumerate(a, 1):
        row = np.empty_like(prev)
        row[:, 0] = i
        row[:, 1:] = np.minimum(prev[:, :-1] + (mat != ord(x)), prev[:, 1:] + 1)
        prev = np.minimum.accumulate(row - cols, axis=1) + cols          # row[j] = min(row[j], row[j-1] + 1), left to right
    return [int(prev[n, len(b)]) for n, b in enumerate(bs)]


def distance(a, b, max_diff):
    """min(Levenshtein(a, b), max_diff + 1); the header's "lengths that differ by more than max_diff give max_diff + 1 without any
    comparison" is taken at its word (Levenshtein(a, b) >= |len(a) - len(b)|: tests/test_bubbles_cpu.py holds the matrix to it)"""
    if abs(len(a) - len(b)) > max_diff:
        return max_diff + 1
    return min(levenshtein(a, b), max_diff + 1)


def parallel_pairs(edges, max_len):
    """the unordered pairs (i < j) of edges with the same start and the same end node, both of at most max_len bases"""
    by = {}
    for i, (s, e, q) in enumerate(edges):
        if len(q) <= max_len:
            by.setdefault((s, e), []).append(i)
    return [(g[a], g[b]) for g in by.values() for a in range(len(g)) for b in range(a + 1, len(g))]


def pop(counts, edges, max_len, max_diff):
    """-> (the set of indices into `edges` that one round removes, the number of pairs whose distance was computed).  Coverage is
    looked at for the candidate edges only: those in some parallel pair within max_len."""
    pairs = parallel_pairs(edges, max_len)
    cand = sorted({i for p in pairs for i in p})
    cov = dict(zip(cand, T.coverage(counts, [edges[i] for i in cand])[0]))
    removed, compared = set(), 0
    for i, j in pairs:
        a, b = edges[i][2], edges[j][2]
        if abs(len(a) - len(b)) > max_diff:                  # max_diff + 1 without any comparison: not counted
            continue
        compared += 1
        if levenshtein(a, b) <= max_diff:
            if T._weaker(cov[i], cov[j]):
                removed.add(i)
            if T._weaker(cov[j], cov[i]):
                removed.add(j)
    return removed, compared


strand_closed = T.strand_closed
