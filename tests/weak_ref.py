"""The rule of gk_graph_remove_weak_edges (include/genome_amd.h) restated in plain Python, from the header's text: the device is
held to this bit for bit (tests/test_weak_gpu.py), and this file to hand-computed answers (tests/test_weak_cpu.py).

Input: `counts` and `edges` as tests/tips_ref.py takes them (a dict stored k-mer -> count, a list of (start k-mer, end k-mer,
seq)); coverage is tips_ref.coverage's.  A node is identified by its k-mer — or, for a graph with node copies, by what `ends`
gives: a list of (start node, end node) per edge, any hashable (the device's node ids).
"""
import tips_ref as T

STATS = ("candidates", "removed_ratio", "removed_floor_only", "removed")
MAX_RATIO = 65535


def below(ratio, a, b):
    """`ratio` times a is below b, exactly: sum_a * (ratio * kmers_b) < sum_b * kmers_a, with a, b = (kmers, sum, ...)"""
    return a[1] * (ratio * b[0]) < b[1] * a[0]


def weak(counts, edges, max_len, ratio, floor, ends=None):
    """-> (the set of indices into `edges` that one round removes, the four stats as a dict), decided from the graph as given"""
    assert 0 <= ratio <= MAX_RATIO
    cov, _ = T.coverage(counts, edges)
    ends = [(s, e) for s, e, _q in edges] if ends is None else list(ends)
    out_of, in_of = {}, {}
    for i, (u, v) in enumerate(ends):
        out_of.setdefault(u, []).append(i)
        in_of.setdefault(v, []).append(i)
    by_ratio, by_floor, candidates = set(), set(), 0
    for i, (u, v) in enumerate(ends):
        if len(edges[i][2]) > max_len:
            continue
        if len(out_of[u]) >= 2 and len(in_of[v]) >= 2:
            candidates += 1
            if ratio >= 1 and any(below(ratio, cov[i], cov[j]) for j in out_of[u] if j != i) \
                    and any(below(ratio, cov[i], cov[j]) for j in in_of[v] if j != i):
                by_ratio.add(i)
        if floor >= 1 and cov[i][1] < floor * cov[i][0]:
            by_floor.add(i)
    only = by_floor - by_ratio
    return by_ratio | only, dict(zip(STATS, (candidates, len(by_ratio), len(only), len(by_ratio) + len(only))))


def strongest_survive(counts, edges, removed, ends=None):
    """under (A): at every node no out-edge of maximal mean coverage and no in-edge of maximal mean coverage is in `removed` (an
    edge that goes has a strictly stronger competitor at each end; ties at the top all stay)"""
    cov, _ = T.coverage(counts, edges)
    ends = [(s, e) for s, e, _q in edges] if ends is None else list(ends)
    for side in (0, 1):
        groups = {}
        for i, uv in enumerate(ends):
            groups.setdefault(uv[side], []).append(i)
        for members in groups.values():
            top = [i for i in members if not any(T._weaker(cov[i], cov[j]) for j in members)]
            if not top or any(i in removed for i in top):
                return False
    return True
