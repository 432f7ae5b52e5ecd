"""A string-based restatement of the scaffold-link rules of include/genome_amd.h ("scaffold links"), for the tests: the classes of
a pair orientation and u, one `if` per row; the joins; the chains.  Graphs and positions are insert_ref.index_graph's: edges as
(start k-mer, sequence) strings, positions ("N", node index) or ("E", edge index, distance).  It never touches the device."""
from insert_ref import index_graph      # noqa: F401  (the tests take it from here)
from oracle import pyref as R

CLASSES = ("orientations", "unplaced", "repetitive", "at_node", "same_edge", "short_edge", "too_far", "linked")
JOIN_STATS = ("links", "supported", "joins", "forks", "merges")


def classify(P1, P2, k, lens, min_len, max_span):
    """one orientation -> (class name, (e, f, u) or None)"""
    if not P1 or not P2:
        return "unplaced", None
    if len(P1) >= 2 or len(P2) >= 2:
        return "repetitive", None
    a, b = P1[0], P2[0]
    if a[0] == "N" or b[0] == "N":
        return "at_node", None
    e, f = a[1], b[1]
    if e == f:
        return "same_edge", None
    if k + lens[e] < min_len or k + lens[f] < min_len:
        return "short_edge", None
    u = (lens[e] + k - a[2]) + (b[2] + k)
    if u > max_span:
        return "too_far", None
    return "linked", (e, f, u)


def pair_links(k, index, lens, reads, npairs, min_len, max_span):
    """the first `npairs` pairs of reads = [mate 1, mate 2, mate 1, ...] -> ({(e, f): [count, sum_u]}, {class: count})"""
    links, cls = {}, dict.fromkeys(CLASSES, 0)
    for p in range(min(npairs, len(reads) // 2)):
        m1, m2 = reads[2 * p], reads[2 * p + 1]
        if len(m1) < k or len(m2) < k:
            continue
        for x, y in ((m1, m2), (m2, m1)):
            c, hit = classify(index.get(x[:k], []), index.get(R.rev_comp(y[:k]), []), k, lens, min_len, max_span)
            cls["orientations"] += 1
            cls[c] += 1
            if hit:
                slot = links.setdefault(hit[:2], [0, 0])
                slot[0] += 1
                slot[1] += hit[2]
    return links, cls


def joins(links, min_support):
    """-> ([(e, f, count, sum_u)] in ascending e, {stat: count} over JOIN_STATS)"""
    sup = {key: v for key, v in links.items() if v[0] >= min_support}
    succ, pred = {}, {}
    for e, f in sup:
        succ.setdefault(e, []).append(f)
        pred.setdefault(f, []).append(e)
    out = [(e, fs[0], *sup[(e, fs[0])]) for e, fs in sorted(succ.items()) if len(fs) == 1 and len(pred[fs[0]]) == 1]
    st = dict(links=len(links), supported=len(sup), joins=len(out), forks=sum(len(v) >= 2 for v in succ.values()),
              merges=sum(len(v) >= 2 for v in pred.values()))
    return out, st


def chains(e1, e2):
    """a join list -> (chains as lists of edge ids in ascending order of first member, cycles among them); None if an id
    occurs twice as e1 or twice as e2"""
    if len(set(e1)) != len(e1) or len(set(e2)) != len(e2):
        return None
    succ, has_pred = dict(zip(e1, e2)), set(e2)
    out, seen, ncycles = [], set(), 0
    for head in sorted(e for e in succ if e not in has_pred):
        c = [head]
        while c[-1] in succ:
            c.append(succ[c[-1]])
        seen.update(c)
        out.append(c)
    for head in sorted(succ):                                  # what is left lies on cycles: each starts at its smallest id
        if head in seen:
            continue
        c = [head]
        while succ[c[-1]] != head:
            c.append(succ[c[-1]])
        seen.update(c)
        out.append(c)
        ncycles += 1
    return sorted(out), ncycles
