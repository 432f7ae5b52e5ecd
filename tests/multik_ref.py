"""A restatement of the multi-k rule (include/genome_amd.h, "multi-k") in plain Python: what gk_map_add_graph_paths adds to a table
of k2 and its six stats, from a graph's live edges as (start k-mer, end k-mer, seq) strings (g.canonical()[1]).

Classes and paths as strings (the contigs' classes with min_len = k2: contigs_ref.classify), then every k2-window of every forward
or self_twin path oriented with oracle/pyref.py's hash rule (canon: the smaller signed hashCode, a tie to the reverse complement).
"""
from contigs_ref import classify
from oracle import pyref as R

STATS = ("live_edges", "short", "forward", "self_twin", "reverse", "windows")


def add_graph_paths(edges, k2, weight):
    """-> (stored k2-mer string -> added count, stats dict)"""
    added = {}
    st = dict.fromkeys(STATS, 0)
    for start, _end, seq in edges:
        path = start + seq
        c = classify(path, k2)
        st["live_edges"] += 1
        st[c] += 1
        if c in ("short", "reverse"):
            continue
        for i in range(len(path) - k2 + 1):
            key = R.canon(path[i:i + k2])
            added[key] = added.get(key, 0) + weight
            st["windows"] += 1
    return added, st


def records(edges, k2):
    """the sequences of gk_graph_contigs_plan(g, NULL, 0, 0, strands = 1)'s records (any order), for the identity with counting"""
    return [s + q for s, _e, q in edges if classify(s + q, 0) in ("forward", "self_twin")]


def merged(before_rows, added):
    """the table's content after the call: before + added, as sorted (hi, lo, count) rows of packed keys; before_rows likewise"""
    total = {(hi, lo): c for hi, lo, c in before_rows}
    for key, c in added.items():
        lo, hi = R.pack(key)
        total[(hi, lo)] = total.get((hi, lo), 0) + c
    return sorted((hi, lo, c) for (hi, lo), c in total.items())
