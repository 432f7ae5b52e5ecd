"""A restatement of the contig rule (include/genome_amd.h, "contigs: this project's own rule") in plain Python: the FASTA text
and the nine stats of gk_graph_contigs_plan, from a graph's edges as (start k-mer, end k-mer, seq) strings and their ids.

contigs(edges, ids, ...) takes the edges in any order (g.canonical()[1] with the ids tests/test_edge_coverage_gpu.py's
edges_with_ids finds for them) and, for the cov= field, the count table as the dict tests/tips_ref.py takes.
"""
import tips_ref as T

CODE = {"A": 0, "G": 1, "C": 2, "T": 3}
STATS = ("live_edges", "short", "forward", "self_twin", "reverse", "records", "bases", "text_bytes", "missing_windows")


def rev_comp_codes(codes):
    return [3 - c for c in reversed(codes)]


def classify(path, min_len=0):
    """'short' | 'forward' | 'self_twin' | 'reverse' of one path (start k-mer ++ seq)"""
    if len(path) < min_len:
        return "short"
    p = [CODE[c] for c in path]
    r = rev_comp_codes(p)
    return "forward" if p < r else "self_twin" if p == r else "reverse"


def wrap(seq, line_width):
    """the bases and their line ends: a newline after every line_width bases (0: none) and after the last, never an empty line"""
    if line_width == 0:
        return seq + "\n"
    return "".join(seq[i:i + line_width] + "\n" for i in range(0, len(seq), line_width))


def cov_field(total, kmers):
    q = (100 * total) // kmers                               # Python integers do not overflow
    return " cov=%d.%02d" % (q // 100, q % 100)


def record(eid, path, line_width, cov=None):
    """cov: None, or (sum, kmers) of the edge"""
    return ">e%d len=%d%s\n" % (eid, len(path), cov_field(*cov) if cov is not None else "") + wrap(path, line_width)


def contigs(edges, ids, counts=None, min_len=0, line_width=60, strands=1):
    """-> (text bytes, stats dict)"""
    assert strands in (1, 2) and len(edges) == len(ids)
    st = dict.fromkeys(STATS, 0)
    out = []
    for i in sorted(range(len(edges)), key=lambda j: ids[j]):
        start, _end, seq = edges[i]
        path = start + seq
        c = classify(path, min_len)
        st[c] += 1
        st["live_edges"] += 1
        if c == "short" or (c == "reverse" and strands == 1):
            continue
        cov = None
        if counts is not None:
            ((kmers, total, _mn, _mx),), missing = T.coverage(counts, [edges[i]])
            st["missing_windows"] += missing
            cov = (total, kmers)
        out.append(record(ids[i], path, line_width, cov))
        st["records"] += 1
        st["bases"] += len(path)
    text = "".join(out).encode()
    st["text_bytes"] = len(text)
    return text, st


def parse(text):
    """[(id, n, cov string or None, sequence)] of a text this rule wrote"""
    recs = []
    for block in text.decode().split(">")[1:]:
        head, *lines = block.split("\n")
        f = head.split()
        assert f[0][0] == "e" and f[1].startswith("len=")
        seq = "".join(lines)
        assert len(seq) == int(f[1][4:])
        recs.append((int(f[0][1:]), len(seq), f[2][4:] if len(f) > 2 else None, seq))
    return recs
