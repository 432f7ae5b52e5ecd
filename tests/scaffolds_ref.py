"""A restatement of the scaffold rule (include/genome_amd.h, "scaffolds: this project's own rule") in plain Python strings: the
FASTA text, the thirteen stats and the segment rows of gk_graph_scaffolds_plan.

scaffolds(edges, ...) takes the live edges as {edge id: (start, end, seq)}: start and end name the edge's nodes and start is also
the node's k-mer, so the path is start + seq and two edges meet in a node iff one's end equals the other's start (an unedited
graph holds a k-mer once).  `node_ids`, where node copies share a k-mer, maps an edge id to its (start node id, end node id) for
that comparison alone.  Chains are lists of edge ids, gaps[c][i] the gap after member i of chain c.
"""
import contigs_ref as CR

STATS = ("chains", "chain_forward", "chain_self_twin", "chain_reverse", "singletons", "records", "members", "adjacent", "gapped", "clamped",
         "n_bases", "bases", "text_bytes")
CODE = {"A": 0, "G": 1, "C": 2, "T": 3, "N": 4}


def rev_comp(seq):
    """R(S): reversed, code c -> 3 - c below 4, N stays N"""
    return "".join("N" if c == "N" else "AGCT"[3 - CODE[c]] for c in reversed(seq))


def classify(seq):
    s, r = [CODE[c] for c in seq], [CODE[c] for c in rev_comp(seq)]
    return "forward" if s < r else "self_twin" if s == r else "reverse"


def junction(edges, node_ids, e, f):
    ends = node_ids if node_ids is not None else {i: (s, t) for i, (s, t, _q) in edges.items()}
    return "adjacent" if ends[e][1] == ends[f][0] else "gapped"


def assemble(edges, chain, gaps, min_gap, node_ids=None):
    """-> (sequence, pieces [(edge id, first base, bases written, bases skipped)], {adjacent, gapped, clamped, n_bases})"""
    k = len(edges[chain[0]][0])
    seq, pieces = "", []
    cnt = dict(adjacent=0, gapped=0, clamped=0, n_bases=0)
    for i, e in enumerate(chain):
        path = edges[e][0] + edges[e][2]
        skip = 0
        if i:
            if junction(edges, node_ids, chain[i - 1], e) == "adjacent":
                cnt["adjacent"] += 1
                skip = k
            else:
                cnt["gapped"] += 1
                cnt["clamped"] += gaps[i - 1] < min_gap
                run = max(gaps[i - 1], min_gap)
                cnt["n_bases"] += run
                seq += "N" * run
        pieces.append((e, len(seq), len(path) - skip, skip))
        seq += path[skip:]
    return seq, pieces, cnt


def check(edges, chains, gaps, min_gap, strands):
    """None, or the name of the first error of the rule's list that the input has"""
    seen = set()
    if not 1 <= min_gap <= 2 ** 31 - 1 or strands not in (1, 2):
        return "GK_E_INVALID"
    for c, g in zip(chains, gaps):
        if not c:
            return "GK_E_INVALID"
        for e in c:
            if e not in edges or e in seen:
                return "GK_E_INVALID"
            seen.add(e)
    return None


def scaffolds(edges, chains, gaps, min_gap=10, min_len=0, line_width=60, strands=1, singletons=True, node_ids=None):
    """-> (text bytes, stats dict, segment rows [(record, edge id, first base, bases written, bases skipped)])"""
    assert check(edges, chains, gaps, min_gap, strands) is None
    st = dict.fromkeys(STATS, 0)
    out, rows = [], []
    st["chains"] = len(chains)
    for c, (chain, g) in enumerate(zip(chains, gaps)):
        seq, pieces, cnt = assemble(edges, chain, g, min_gap, node_ids)
        cls = classify(seq)
        st["chain_" + cls] += 1
        if cls == "reverse" and strands == 1:
            continue
        rows += [(len(out), *p) for p in pieces]
        out.append(">s%d len=%d contigs=%d gaps=%d\n" % (c, len(seq), len(chain), cnt["n_bases"]) + CR.wrap(seq, line_width))
        st["members"] += len(chain)
        st["bases"] += len(seq)
        for name, v in cnt.items():
            st[name] += v
    if singletons:
        claimed = {e for c in chains for e in c}
        for e in sorted(set(edges) - claimed):
            path = edges[e][0] + edges[e][2]
            cls = CR.classify(path, min_len)
            if cls == "short" or (cls == "reverse" and strands == 1):
                continue
            rows.append((len(out), e, 0, len(path), 0))
            out.append(CR.record(e, path, line_width))
            st["singletons"] += 1
            st["bases"] += len(path)
    text = "".join(out).encode()
    st["records"] = len(out)
    st["text_bytes"] = len(text)
    return text, st, rows


def parse(text):
    """[(name, n, sequence)] of a text this rule wrote: name = 's<c>' or 'e<id>'"""
    recs = []
    for block in text.decode().split(">")[1:]:
        head, *lines = block.split("\n")
        f = head.split()
        seq = "".join(lines)
        assert f[1].startswith("len=") and len(seq) == int(f[1][4:]) and "" not in lines[:-1]
        if f[0][0] == "s":
            assert f[2].startswith("contigs=") and f[3].startswith("gaps=") and seq.count("N") == int(f[3][5:])
        recs.append((f[0], len(seq), seq))
    return recs
