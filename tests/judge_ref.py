"""A plain restatement of the placement rule and of the judge (include/genome_amd.h, "placements" and "the judge"), over dicts and
ints, for the tests to compare the device against.  A helper, not a test; it does not use the library.

A graph is {node id: k-mer} for the live nodes and {edge id: (start k-mer, seq)} for the live edges: P(e) = start k-mer + seq.
"""
COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}
PLACE_STATS = ("records", "bases", "valid_bases", "windows", "fwd_absent", "fwd_repetitive", "fwd_at_node", "fwd_edge", "rev_absent", "rev_repetitive",
               "rev_at_node", "rev_edge", "unplaced", "both_strands", "scattered", "forward", "reverse", "forward_bases", "reverse_bases", "saturated")
PLACE_CLASSES = ("unplaced", "both_strands", "scattered", "forward", "reverse")
JUDGE_CLASSES = ("unjudged", "other_record", "strand", "order", "distance", "correct")
JUDGE_KINDS = ("adjacent", "gapped", "overlapped")
JUDGE_STATS = (("junctions",) + JUDGE_CLASSES + tuple(f"{kd}_{c}" for kd in JUDGE_KINDS for c in JUDGE_CLASSES)
               + ("gapped_correct_abs_err_sum", "gapped_correct_abs_err_max", "records_judged", "records_clean"))
MISJOINS = ("other_record", "strand", "order", "distance")
COUNT_MAX = (1 << 32) - 1


def rev_comp(s):
    return "".join(COMP[c] for c in reversed(s))


def position_map(k, nodes, edges):
    """Graph.getGraphMap: every node's k-mer -> a node position, the k-mers at distance 1 .. len - 1 of every edge -> (e, d); a
    multimap, as putNew makes it"""
    pm = {}
    for n, kmer in nodes.items():
        pm.setdefault(kmer, []).append(("node", n))
    for e, (start, seq) in edges.items():
        path = start + seq
        for d in range(1, len(seq)):
            pm.setdefault(path[d:d + k], []).append(("edge", e, d))
    return pm


def lookup(pm, w):
    """-> (class name, the position if the class is `edge`)"""
    got = pm.get(w, [])
    if not got:
        return "absent", None
    if len(got) >= 2:
        return "repetitive", None
    if got[0][0] == "node":
        return "at_node", None
    return "edge", got[0]


def place(k, nodes, edges, records, id_bound=None):
    """records: the joined sequence of every reference record, str.  -> (the stats by name, {edge id: (class name, record, pos,
    windows_fwd, windows_rev)} for every id below the bound; dead ids are unplaced with zeros)"""
    pm = position_map(k, nodes, edges)
    st = dict.fromkeys(PLACE_STATS, 0)
    hits = {}                                          # (e, strand) -> [count, min, max] of (record, coordinate)
    for r, rec in enumerate(records):
        st["records"] += 1
        st["bases"] += len(rec)
        st["valid_bases"] += sum(c in "AGCT" for c in rec)
        for x in range(len(rec) - k + 1):
            w = rec[x:x + k]
            if any(c not in "AGCT" for c in w):
                continue
            st["windows"] += 1
            for strand, key in ((0, w), (1, rev_comp(w))):
                cls, pos = lookup(pm, key)
                st[("fwd_", "rev_")[strand] + cls] += 1
                if cls == "edge":
                    _, e, d = pos
                    cand = (r, x - d) if strand == 0 else (r, x + d + k - 1)
                    h = hits.setdefault((e, strand), [0, cand, cand])
                    h[0], h[1], h[2] = min(h[0] + 1, COUNT_MAX), min(h[1], cand), max(h[2], cand)
    bound = (max(edges) + 1 if edges else 0) if id_bound is None else id_bound
    out = {}
    for e in range(bound):
        f, rv = hits.get((e, 0)), hits.get((e, 1))
        if e not in edges or (not f and not rv):
            cls, rec, pos = "unplaced", 0, 0
        elif f and rv:
            cls, rec, pos = "both_strands", 0, 0
        else:
            h = f or rv
            if h[1] != h[2]:
                cls, rec, pos = "scattered", 0, 0
            else:
                cls, (rec, pos) = ("forward" if f else "reverse"), h[1]
                st[cls + "_bases"] += k + len(edges[e][1])
        if e in edges:
            st[cls] += 1
            st["saturated"] += any(h and h[0] == COUNT_MAX for h in (f, rv))
            out[e] = (cls, rec, pos, f[0] if f else 0, rv[0] if rv else 0)
        else:
            out[e] = ("unplaced", 0, 0, 0, 0)
    return st, out


def judge(rows, ends, placed, tol, chain_records):
    """rows: gk_scaffolds_segments' (record, edge, first, bases, skipped) in text order; ends: {edge id: (start node id, end node
    id)}; placed: place()'s per-edge dict; chain_records: how many records of the text are chains (they come first).
    -> (class names, err, the stats by name), one entry per junction in row order"""
    st = dict.fromkeys(JUDGE_STATS, 0)
    classes, errs = [], []
    judged, misjoined = set(), set()
    for (r1, e, first_e, bases_e, skip_e), (r2, f, first_f, _b, skip_f) in zip(rows, rows[1:]):
        if r1 != r2:
            continue
        kind = "gapped" if first_f > first_e + bases_e else "adjacent" if ends[e][1] == ends[f][0] else "overlapped"
        (ce, re_, pe, _, _), (cf, rf, pf, _, _) = placed[e], placed[f]
        err = 0
        if ce not in ("forward", "reverse") or cf not in ("forward", "reverse"):
            cls = "unjudged"
        elif re_ != rf:
            cls = "other_record"
        elif ce != cf:
            cls = "strand"
        else:
            dscaf = first_f - first_e
            dref = (pf + skip_f) - (pe + skip_e) if ce == "forward" else (pe - skip_e) - (pf - skip_f)
            err = dscaf - dref
            if dref <= 0:
                cls = "order"
            elif (abs(err) > tol) if kind == "gapped" else err != 0:
                cls = "distance"
            else:
                cls = "correct"
                if kind == "gapped":
                    st["gapped_correct_abs_err_sum"] += abs(err)
                    st["gapped_correct_abs_err_max"] = max(st["gapped_correct_abs_err_max"], abs(err))
        classes.append(cls)
        errs.append(err)
        st["junctions"] += 1
        st[cls] += 1
        st[kind + "_" + cls] += 1
        if cls != "unjudged":
            judged.add(r1)
        if cls in MISJOINS:
            misjoined.add(r1)
    st["records_judged"] = len(judged)
    st["records_clean"] = chain_records - len(misjoined)
    return classes, errs, st


def identities(pst=None, jst=None, live_edges=None):
    """the counter identities the header states"""
    if pst is not None:
        for s in ("fwd_", "rev_"):
            assert sum(pst[s + c] for c in ("absent", "repetitive", "at_node", "edge")) == pst["windows"]
        assert pst["valid_bases"] <= pst["bases"]
        if live_edges is not None:
            assert sum(pst[c] for c in PLACE_CLASSES) == live_edges
    if jst is not None:
        assert sum(jst[c] for c in JUDGE_CLASSES) == jst["junctions"]
        for c in JUDGE_CLASSES:
            assert sum(jst[f"{kd}_{c}"] for kd in JUDGE_KINDS) == jst[c]
