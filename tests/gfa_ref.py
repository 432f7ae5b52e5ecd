"""A restatement of the two rules of include/genome_amd.h, "edge twins" and "the graph as GFA", in plain Python: the classes,
twins and six stats of gk_graph_edge_twins and the GFA 1.0 text and nine stats of gk_graph_gfa_plan, from a graph's edges as
(start k-mer, end k-mer, seq) strings, their ids and the ids of their start and end nodes (gk_graph_edges_by_id).

No hashing and no sorting by key: the classes come from collections.Counter over path strings, the pairs from a double loop.
key_collisions is the device's own business and is not restated (always 0 here).
"""
from collections import Counter

import tips_ref as T
from contigs_ref import CODE, classify
from oracle import pyref as R

TWIN_STATS = ("live_edges", "paired", "self", "missing", "ambiguous", "key_collisions")
TWIN_CLASSES = ("dead", "paired", "self", "missing", "ambiguous")
GFA_STATS = ("live_edges", "segments", "folded", "pairs", "links", "mirrored", "bases", "text_bytes", "missing_windows")
NONE = 0xFFFFFFFF
HEADER = "H\tVN:Z:1.0\n"


def twins(edges, ids):
    """-> (twin: id -> id or NONE, cls: id -> class name, stats)"""
    paths = [s + q for s, _e, q in edges]
    n_with = Counter(paths)
    some_id = {}
    for p, i in zip(paths, ids):
        some_id.setdefault(p, i)
    twin, cls = {}, {}
    st = dict.fromkeys(TWIN_STATS, 0)
    for p, i in zip(paths, ids):
        r = R.rev_comp(p)
        if n_with[r] == 0:
            c, t = "missing", NONE
        elif n_with[p] > 1 or n_with[r] > 1:
            c, t = "ambiguous", NONE
        elif some_id[r] == i:
            c, t = "self", i
        else:
            c, t = "paired", some_id[r]
        twin[i], cls[i] = t, c
        st[c] += 1
        st["live_edges"] += 1
    return twin, cls, st


def segment(i, path, twin, cls):
    """seg(e) -> (segment id, orientation)"""
    if cls[i] == "paired" and classify(path) == "reverse":
        return twin[i], "-"
    return i, "+"


def gfa(edges, ids, starts, ends, k, counts=None):
    """starts[j] / ends[j]: the node ids of edges[j]'s start and end -> (text bytes, stats dict)"""
    assert len(edges) == len(ids) == len(starts) == len(ends) == len(set(ids))
    twin, cls, _ = twins(edges, ids)
    at = {i: j for j, i in enumerate(ids)}
    path = {i: edges[at[i]][0] + edges[at[i]][2] for i in ids}
    seg = {i: segment(i, path[i], twin, cls) for i in ids}
    st = dict.fromkeys(GFA_STATS, 0)
    st["live_edges"] = len(ids)
    out = [HEADER]
    for i in sorted(ids):
        if seg[i] != (i, "+"):
            continue
        line = "S\te%d\t%s\tLN:i:%d" % (i, path[i], len(path[i]))
        if counts is not None:
            ((_kmers, total, _mn, _mx),), missing = T.coverage(counts, [edges[at[i]]])
            st["missing_windows"] += missing
            line += "\tKC:i:%d" % total
        out.append(line + "\n")
        st["segments"] += 1
        st["bases"] += len(path[i])
    closed = lambda i: cls[i] in ("paired", "self")
    by_start = list(zip(starts, ids))
    for e in sorted(ids):
        end = ends[at[e]]
        nexts = [f for s, f in by_start if s == end]
        for f in sorted(nexts, key=lambda f: CODE[edges[at[f]][2][0]]):
            st["pairs"] += 1
            if closed(e) and closed(f):
                mirror = (twin[f], twin[e])
                if ends[at[mirror[0]]] == starts[at[mirror[1]]] and mirror != (e, f) and mirror < (e, f):
                    st["mirrored"] += 1
                    continue
            (a, oa), (b, ob) = seg[e], seg[f]
            out.append("L\te%d\t%s\te%d\t%s\t%dM\n" % (a, oa, b, ob, k))
            st["links"] += 1
    st["folded"] = st["live_edges"] - st["segments"]
    text = "".join(out).encode()
    st["text_bytes"] = len(text)
    return text, st
