"""A restatement of the overlap rule (include/genome_amd.h, "overlap detection") and of the scaffold plan that takes the
overlaps (gk_graph_scaffolds_plan_overlaps) in plain Python strings: slices and ==, no packing, no words, no strands.

Edges are scaffolds_ref's: {edge id: (start, end, seq)}, the path start + seq; `node_ids`, where node copies share a k-mer or an
edge's start was replaced, maps an edge id to its (start node id, end node id) for the adjacency test alone.  Chains are lists of
edge ids; gaps[c][i] / overlaps[c][i] belong to the junction after member i of chain c.
"""
import contigs_ref as CR
import scaffolds_ref as SR

STATS = ("junctions", "adjacent", "out_of_range", "none", "ambiguous", "overlap", "overlap_bases")
CLASSES = ("last", "adjacent", "out_of_range", "none", "ambiguous", "overlap")
OVERLAP_MAX = 127
I31 = 2 ** 31 - 1


def path(edges, e):
    return edges[e][0] + edges[e][2]


def junction(edges, node_ids, e, f, G, tol, min_overlap, max_overlap):
    """-> (class, o)"""
    if SR.junction(edges, node_ids, e, f) == "adjacent":
        return "adjacent", 0
    pe, pf = path(edges, e), path(edges, f)
    lo = max(min_overlap, -G - tol)
    hi = min(max_overlap, -G + tol, len(pe) - 1, len(pf) - 1)
    if lo > hi:
        return "out_of_range", 0
    hits = [o for o in range(lo, hi + 1) if pe[len(pe) - o:] == pf[:o]]
    if not hits:
        return "none", 0
    if len(hits) > 1:
        return "ambiguous", 0
    return "overlap", hits[0]


def check(edges, chains, gaps, tol, min_overlap, max_overlap, node_ids=None):
    """None, or the name of the error the input has"""
    if not 0 <= tol <= I31 or not 1 <= min_overlap <= OVERLAP_MAX or not min_overlap <= max_overlap <= OVERLAP_MAX:
        return "GK_E_INVALID"
    seen = set()
    for c in chains:
        if not c:
            return "GK_E_INVALID"
        for e in c:
            if e not in edges or e in seen:
                return "GK_E_INVALID"
            seen.add(e)
    for c, g in zip(chains, gaps):
        for e, f, G in zip(c, c[1:], g):
            if SR.junction(edges, node_ids, e, f) != "adjacent" and abs(G) > I31:
                return "GK_E_INVALID"
    return None


def overlaps(edges, chains, gaps, tol, min_overlap=10, max_overlap=None, node_ids=None):
    """-> (overlaps per chain, report) in the shape of HipGraph.overlapGaps; max_overlap None: k"""
    if max_overlap is None:
        max_overlap = len(next(iter(edges.values()))[0])
    assert check(edges, chains, gaps, tol, min_overlap, max_overlap, node_ids) is None
    st = dict.fromkeys(STATS, 0)
    out, classes = [], []
    for c, g in zip(chains, gaps):
        found = [junction(edges, node_ids, e, f, G, tol, min_overlap, max_overlap) for e, f, G in zip(c, c[1:], g)]
        for cls, o in found:
            st[cls] += 1
            st["junctions"] += 1
            st["overlap_bases"] += o
        out.append([o for _cls, o in found])
        classes.append([cls for cls, _o in found])
    return out, dict(st, classes=classes)


def plan_check(edges, chains, overlaps, node_ids=None):
    """what the plan refuses in an overlap array: None, or GK_E_INVALID"""
    for c, ov in zip(chains, overlaps):
        for e, f, o in zip(c, c[1:], ov):
            if o == 0:
                continue
            pe, pf = path(edges, e), path(edges, f)
            if SR.junction(edges, node_ids, e, f) == "adjacent" or o > OVERLAP_MAX or o >= len(pe) or o >= len(pf) or pe[len(pe) - o:] != pf[:o]:
                return "GK_E_INVALID"
    return None


def assemble(edges, chain, gaps, min_gap, node_ids=None, overlaps=None):
    """scaffolds_ref.assemble with the third junction class -> (sequence, pieces [(edge id, first base, bases written, bases
    skipped)], {adjacent, gapped, clamped, n_bases, overlapped, dropped})"""
    k = len(edges[chain[0]][0])
    seq, pieces = "", []
    cnt = dict(adjacent=0, gapped=0, clamped=0, n_bases=0, overlapped=0, dropped=0)
    for i, e in enumerate(chain):
        p = path(edges, e)
        skip = 0
        if i:
            o = overlaps[i - 1] if overlaps is not None else 0
            if SR.junction(edges, node_ids, chain[i - 1], e) == "adjacent":
                cnt["adjacent"] += 1
                skip = k
            elif o > 0:
                cnt["overlapped"] += 1
                cnt["dropped"] += o
                skip = o
            else:
                cnt["gapped"] += 1
                cnt["clamped"] += gaps[i - 1] < min_gap
                run = max(gaps[i - 1], min_gap)
                cnt["n_bases"] += run
                seq += "N" * run
        pieces.append((e, len(seq), len(p) - skip, skip))
        seq += p[skip:]
    return seq, pieces, cnt


def scaffolds(edges, chains, gaps, overlaps=None, min_gap=10, min_len=0, line_width=60, strands=1, singletons=True, node_ids=None):
    """-> (text bytes, the thirteen stats, segment rows, {overlapped, dropped}); scaffolds_ref.scaffolds where overlaps is None or
    all zeros"""
    assert SR.check(edges, chains, gaps, min_gap, strands) is None
    if overlaps is not None:
        assert plan_check(edges, chains, overlaps, node_ids) is None
    st = dict.fromkeys(SR.STATS, 0)
    ost = dict(overlapped=0, dropped=0)
    out, rows = [], []
    st["chains"] = len(chains)
    for c, (chain, g) in enumerate(zip(chains, gaps)):
        seq, pieces, cnt = assemble(edges, chain, g, min_gap, node_ids, overlaps[c] if overlaps is not None else None)
        cls = SR.classify(seq)
        st["chain_" + cls] += 1
        if cls == "reverse" and strands == 1:
            continue
        rows += [(len(out), *p) for p in pieces]
        out.append(">s%d len=%d contigs=%d gaps=%d\n" % (c, len(seq), len(chain), cnt["n_bases"]) + CR.wrap(seq, line_width))
        st["members"] += len(chain)
        st["bases"] += len(seq)
        for name, v in cnt.items():
            if name in ost:
                ost[name] += v
            else:
                st[name] += v
    if singletons:
        claimed = {e for c in chains for e in c}
        for e in sorted(set(edges) - claimed):
            p = path(edges, e)
            cls = CR.classify(p, min_len)
            if cls == "short" or (cls == "reverse" and strands == 1):
                continue
            rows.append((len(out), e, 0, len(p), 0))
            out.append(CR.record(e, p, line_width))
            st["singletons"] += 1
            st["bases"] += len(p)
    text = "".join(out).encode()
    st["records"] = len(out)
    st["text_bytes"] = len(text)
    return text, st, rows, ost
