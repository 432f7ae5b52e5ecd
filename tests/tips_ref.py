"""The rules of gk_graph_edge_coverage and gk_graph_clip_tips (include/genome_amd.h) restated in plain Python, from the header's
text: the device is held to this bit for bit (tests/test_edge_coverage_gpu.py, tests/test_tips_gpu.py), and this file to
hand-computed answers (tests/test_tips_cpu.py).

Input: `counts`, a dict stored k-mer (string) -> count as a table filled by the hash rule holds it (key = oracle.pyref.canon of
every window counted), and `edges`, a list of (start k-mer, end k-mer, seq) as HipGraph.canonical() gives them.  A node is
identified by its k-mer: graphs with node copies (after a node split) are outside the tip restatement (coverage does not look
at nodes at all beyond the start k-mer).
"""
from oracle import pyref as R


def kmer_count(counts, w):
    """Count of one window: the stored count of its hash-rule orientation, 0 if absent.  Where the rule cannot tell the two
    strands apart (equal hashes, the k-mer not its own reverse complement) the table may hold both: their counts add up."""
    rc = R.rev_comp(w)
    c = counts.get(R.canon(w), 0)
    if w != rc and R.hash_code(w) == R.hash_code(rc):
        c += counts.get(R.canon(rc), 0)
    return c


def canonical_counts(items):
    """(k-mer string, count) pairs in ANY orientation (a table filled with verbatim keys) -> the dict the functions below take"""
    out = {}
    for s, c in items:
        key = R.canon(s)
        out[key] = out.get(key, 0) + int(c)
    return out


def coverage(counts, edges):
    """-> per edge (kmers, sum, min, max) over the len + 1 windows of start ++ seq, and the number of windows with count 0
    because the table does not hold them"""
    out, missing = [], 0
    for start, _end, seq in edges:
        k = len(start)
        path = start + seq
        cs = [kmer_count(counts, path[d:d + k]) for d in range(len(seq) + 1)]
        missing += sum(1 for c in cs if c == 0)
        out.append((len(cs), sum(cs), min(cs), max(cs)))
    return out, missing


def _weaker(a, b):
    """mean coverage of a strictly below that of b, exactly: sum_a / kmers_a < sum_b / kmers_b"""
    return a[1] * b[0] < b[1] * a[0]


def tips(counts, edges, max_len):
    """-> the set of indices into `edges` that one round of the tip rule removes, decided from the graph as given"""
    cov, _ = coverage(counts, edges)
    out_of, in_of = {}, {}
    for i, (s, e, _q) in enumerate(edges):
        out_of.setdefault(s, []).append(i)
        in_of.setdefault(e, []).append(i)
    removed = set()
    for i, (u, v, q) in enumerate(edges):
        if len(q) > max_len:
            continue
        out_u, in_u = len(out_of.get(u, [])), len(in_of.get(u, []))
        out_v, in_v = len(out_of.get(v, [])), len(in_of.get(v, []))
        rivals = []
        if out_v == 0 and in_v == 1 and out_u >= 2:          # out-tip: the other out-edges of u
            rivals += [j for j in out_of[u] if j != i]
        if in_u == 0 and out_u == 1 and in_v >= 2:           # in-tip: the other in-edges of v
            rivals += [j for j in in_of[v] if j != i]
        if any(_weaker(cov[i], cov[j]) for j in rivals):
            removed.add(i)
    return removed


def strand_closed(edges):
    """every edge's reverse-complement twin (rc(end) -> rc(start), spelling rc of the path) is in the list"""
    have = set(edges)
    for s, e, q in edges:
        k = len(s)
        rpath = R.rev_comp(s + q)
        if (rpath[:k], rpath[len(q):], rpath[k:]) not in have:
            return False
    return True
