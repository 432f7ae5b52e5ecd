"""A plain restatement of the alignment-block rule and of the breakpoint rule (include/genome_amd.h, "alignment blocks" and
"breakpoints"), over dicts and ints, for the tests to compare the device against.  A helper, not a test; it does not use the
library.  Built on judge_ref's position map and lookup; the windows are enumerated one by one, nothing is tiled.

A graph is {node id: k-mer} for the live nodes and {edge id: (start k-mer, seq)} for the live edges: P(e) = start k-mer + seq.
"""
from judge_ref import lookup, position_map, rev_comp

BREAKS = ("first", "overlap", "translocation", "inversion", "relocation", "indel", "colinear")
EDGE_CLASSES = ("unaligned", "repeat", "misassembled", "indel", "colinear", "exact")
STATS = (("records", "bases", "valid_bases", "windows", "covered", "rows") + tuple("brk_" + b for b in BREAKS[1:])
         + tuple("edges_" + c for c in EDGE_CLASSES)
         + ("full_edges", "aligned_kmers", "pieces", "piece_bases", "indel_shift_sum", "indel_shift_max"))
ROW_FIELDS = ("edge", "strand", "record", "pos", "dlo", "dhi", "brk", "shift")


def hits(k, pm, rec):
    """-> per window start x of the record, (h_0(x), h_1(x)): (e, c) for an `edge` lookup, None otherwise (no valid window at x too)"""
    out = []
    for x in range(len(rec) - k + 1):
        w = rec[x:x + k]
        if any(c not in "AGCT" for c in w):
            out.append(None)
            continue
        h = []
        for strand, key in ((0, w), (1, rev_comp(w))):
            cls, pos = lookup(pm, key)
            h.append(None if cls != "edge" else (pos[1], x - pos[2] if strand == 0 else x + pos[2] + k - 1))
        out.append(tuple(h))
    return out


def runs(k, pm, records):
    """the maximal runs -> [(edge, strand, record, pos, dlo, dhi, x0)], unordered; and the five counters of the windows"""
    st = dict(records=len(records), bases=0, valid_bases=0, windows=0, covered=0)
    out = []
    for r, rec in enumerate(records):
        st["bases"] += len(rec)
        st["valid_bases"] += sum(c in "AGCT" for c in rec)
        hs = hits(k, pm, rec)
        st["windows"] += sum(h is not None for h in hs)
        st["covered"] += sum(h is not None and (h[0] is not None or h[1] is not None) for h in hs)
        for s in (0, 1):
            x = 0
            while x < len(hs):
                h = hs[x][s] if hs[x] is not None else None
                if h is None:
                    x += 1
                    continue
                x1 = x
                while x1 + 1 < len(hs) and hs[x1 + 1] is not None and hs[x1 + 1][s] == h:
                    x1 += 1
                e, c = h
                dlo, dhi = (x - c, x1 - c) if s == 0 else (c - (x1 + k - 1), c - (x + k - 1))
                out.append((e, s, r, c, dlo, dhi, x))
                x = x1 + 1
    return out, st


def nx50(lengths, total) -> int:
    """lengths descending, the first at which twice the running sum reaches `total`; 0 for none"""
    run = 0
    for x in sorted(lengths, reverse=True):
        run += x
        if 2 * run >= total:
            return x
    return 0


def align(k, nodes, edges, records, tol, id_bound=None):
    """-> dict(rows=[(edge, strand, record, pos, dlo, dhi, brk, shift)] in the rule's order, edges={id: (class name, full,
    first_row, nrows)} for every id below the bound (a dead id: unaligned, 0, 0, 0), pieces=[(bases, edge)] in row order,
    stats by name, na50, nga50)"""
    pm = position_map(k, nodes, edges)
    raw, win = runs(k, pm, records)
    raw.sort(key=lambda t: (t[0], t[4], t[5], t[1], t[2], t[6]))
    st = dict.fromkeys(STATS, 0)
    st.update(win)
    rows = []
    for i, (e, s, r, c, dlo, dhi, _x0) in enumerate(raw):
        brk, shift = 0, 0
        if i and raw[i - 1][0] == e:
            _pe, ps, pr, pc, _plo, phi, _px = raw[i - 1]
            if dlo <= phi:
                brk = 1
            elif pr != r:
                brk = 2
            elif ps != s:
                brk = 3
            else:
                shift = c - pc if s == 0 else pc - c
                brk = 4 if abs(shift) > tol else 5 if shift else 6
        rows.append((e, s, r, c, dlo, dhi, brk, shift))
        st["rows"] += 1
        st["aligned_kmers"] += dhi - dlo + 1
        if brk:
            st["brk_" + BREAKS[brk]] += 1
        if brk == 5:
            st["indel_shift_sum"] += abs(shift)
            st["indel_shift_max"] = max(st["indel_shift_max"], abs(shift))
    bound = (max(edges) + 1 if edges else 0) if id_bound is None else id_bound
    by_edge = {}
    for i, row in enumerate(rows):
        by_edge.setdefault(row[0], []).append(i)
    out_edges, pieces = {}, []
    for e in range(bound):
        if e not in edges:
            out_edges[e] = ("unaligned", 0, 0, 0)
            continue
        ix = by_edge.get(e, [])
        brks = [rows[i][6] for i in ix[1:]]
        if not ix:
            cls = "unaligned"
        elif 1 in brks:
            cls = "repeat"
        elif any(2 <= b <= 4 for b in brks):
            cls = "misassembled"
        elif 5 in brks:
            cls = "indel"
        elif brks:
            cls = "colinear"
        else:
            cls = "exact"
        full = int(bool(ix) and rows[ix[0]][4] == 1 and rows[ix[-1]][5] == len(edges[e][1]) - 1)
        out_edges[e] = (cls, full, ix[0] if ix else 0, len(ix))
        st["edges_" + cls] += 1
        st["full_edges"] += full
        if ix and cls != "repeat":
            first = ix[0]
            for j, i in enumerate(ix):
                if j and 2 <= rows[i][6] <= 4:
                    pieces.append((rows[i - 1][5] - rows[first][4] + k, e))
                    first = i
            pieces.append((rows[ix[-1]][5] - rows[first][4] + k, e))
    st["pieces"] = len(pieces)
    st["piece_bases"] = sum(p[0] for p in pieces)
    lens = [p[0] for p in pieces]
    return dict(rows=rows, edges=out_edges, pieces=pieces, stats=st, na50=nx50(lens, st["piece_bases"]), nga50=nx50(lens, st["valid_bases"]))


def identities(st, live_edges=None):
    """the counter identities the header states"""
    assert st["valid_bases"] <= st["bases"] and st["covered"] <= st["windows"] and st["aligned_kmers"] <= 2 * st["windows"]
    assert st["covered"] <= st["aligned_kmers"]
    aligned = sum(st["edges_" + c] for c in EDGE_CLASSES[1:])
    assert sum(st["brk_" + b] for b in BREAKS[1:]) == st["rows"] - aligned
    assert st["edges_exact"] <= st["rows"] and st["full_edges"] <= aligned
    assert st["pieces"] >= aligned - st["edges_repeat"] and st["piece_bases"] >= st["pieces"]
    assert st["indel_shift_max"] <= st["indel_shift_sum"] and (st["indel_shift_sum"] == 0) == (st["brk_indel"] == 0)
    if live_edges is not None:
        assert sum(st["edges_" + c] for c in EDGE_CLASSES) == live_edges
