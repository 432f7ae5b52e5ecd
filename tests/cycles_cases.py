"""The inputs of the perfect-cycle tests: each case is (circular sequences, linear sequences) for a given k; the table is the
k-mers of all of them (tests/cycles_ref.py: circular_kmers, linear_kmers).  Sequences are drawn without a repeated (k-1)-mer on
either strand, so a circular one is a perfect cycle of exactly its length unless the case says otherwise."""
import random

from cycles_ref import circular_kmers, linear_kmers, rc

KS = (11, 12, 31, 34, 64)


def _windows(s, w, circular):
    if not circular:
        return [s[i:i + w] for i in range(len(s) - w + 1)]
    ext = (s * (w // len(s) + 2))[:len(s) + w - 1]
    return [ext[i:i + w] for i in range(len(s))]


def _fresh(wins, used):
    """the windows and their reverse complements as a set — or None if one repeats, is a palindrome or is in `used`"""
    seen = set()
    for t in wins:
        r = rc(t)
        if t == r or t in seen or t in used:
            return None
        seen.add(t); seen.add(r)
    return seen


def _draw(rnd, n, k, used, circular):
    """n bases whose (k-1)-mers (when circular, those across the junction too) occur once over both strands and are new to `used`"""
    w = k - 1
    for _ in range(500):
        if n < 4 * k:
            s = "".join(rnd.choice("AGCT") for _ in range(n))
        else:                                   # long: grow base by base past the windows already taken
            s = "".join(rnd.choice("AGCT") for _ in range(w))
            mine = {s, rc(s)}
            while len(s) < n:
                for b in rnd.sample("AGCT", 4):
                    t = s[len(s) - w + 1:] + b
                    if t not in mine and t not in used and rc(t) != t:
                        mine.add(t); mine.add(rc(t))
                        s += b
                        break
                else:
                    break
            if len(s) < n:
                continue
        got = _fresh(_windows(s, w, circular), used)
        if got is not None:
            used |= got
            return s
    raise AssertionError("no sequence without a repeated (k-1)-mer")


def make(name, k):
    """-> (circular sequences, linear sequences)"""
    rnd = random.Random(f"{name}/{k}")
    used = set()
    if name == "circular":                      # a circular genome alone, as tests/test_graph_gpu.py builds it: 120 bases at k = 15 there
        return [_draw(rnd, 120, k, used, True)], []
    if name == "beside_linear":
        return [_draw(rnd, 120, k, used, True)], [_draw(rnd, 200, k, used, False)]
    if name == "homopolymer":                   # a cycle of one k-mer (and its reverse complement's)
        return ["A"], []
    if name == "len2":
        return ["AG"], []
    if name == "len3":
        return ["AGC"], []
    if name == "atat":                          # even k: two palindromes, one anchor; odd k: self-complementary, two anchors
        return ["AT"], []
    if name in ("len63", "len64", "len65", "len5000"):
        return [_draw(rnd, int(name[3:]), k, used, True)], []
    if name == "many":                          # 1000 small cycles: anchors span workgroups and scan chunks
        return [_draw(rnd, k + 2 + i % 7, k, used, True) for i in range(1000)], []
    if name == "no_cycles":
        return [], [_draw(rnd, 300, k, used, False), _draw(rnd, 150, k, used, False)]
    if name == "one_tip":                       # a circular genome with one tip hanging off a junction
        c = _draw(rnd, 150, k, used, True)
        tip = "".join(rnd.choice("AGCT") for _ in range(6))
        j = 40
        return [c], [c[j:j + k - 1] + _other(c[j + k - 1]) + tip]
    if name == "bubbles":                       # a circular genome and a second haplotype with SNPs: bubbles to pop
        c = _draw(rnd, 400, k, used, True)
        h = list(c)
        for p in range(30, 400 - k, 3 * k + 7):
            h[p] = _other(h[p])
        return [c, "".join(h)], []
    raise KeyError(name)


def _other(b):
    return {"A": "G", "G": "C", "C": "T", "T": "A"}[b]


BUILD_CASES = ("circular", "beside_linear", "homopolymer", "len2", "len3", "atat", "len63", "len64", "len65", "len5000", "many",
               "no_cycles", "one_tip", "bubbles")


def table_of(name, k):
    """-> (the k-mers to store, as they appear: forward strand of every sequence, duplicates removed, order kept;
           the strong ones among them: the first circular sequence's, to be counted three times where coverage decides)"""
    circ, lin = make(name, k)
    out = []
    for c in circ:
        out += circular_kmers(c, k)
    for s in lin:
        out += linear_kmers(s, k)
    strong = list(dict.fromkeys(circular_kmers(circ[0], k))) if circ else []
    return list(dict.fromkeys(out)), strong
