"""An independent restatement of the k-mer count spectrum and of the cutoff rule (include/genome_amd.h: gk_map_spectrum,
gk_spectrum_cutoff), in plain Python / numpy: what the spectrum tests compare the library with."""
import numpy as np


def spectrum_of(counts, bins: int) -> np.ndarray:
    """hist[c] = how many of `counts` equal c for c <= bins-2; hist[bins-1] = how many are >= bins-1 (the overflow fold)."""
    counts = np.asarray(counts, np.int64)
    assert bins >= 2 and (counts >= 1).all()
    h = np.bincount(np.minimum(counts, bins - 1), minlength=bins)
    assert len(h) == bins and h[0] == 0
    return h.astype(np.uint64)


def cutoff_of(hist, min_count: int = 1):
    """The four-step rule -> (valley, peak, genome_size); (0, 0, 0) = no valley.  Only c in [min_count, bins-2] is looked at."""
    h = [int(x) for x in hist]
    last = len(h) - 2                                                   # the last counted bin; h[-1] is the overflow bin
    rises = [c for c in range(min_count, last) if h[c] < h[c + 1]]      # c + 1 <= last
    if not rises:
        return 0, 0, 0
    r = rises[0]
    highest = max(h[r + 1:last + 1])
    peak = min(c for c in range(r + 1, last + 1) if h[c] == highest)
    lowest = min(h[min_count:peak + 1])
    valley = min(c for c in range(min_count, peak + 1) if h[c] == lowest)
    return valley, peak, sum(c * h[c] for c in range(valley, last + 1)) // peak


def genome_reads(seed: int, genome_len: int = 3000, coverage: int = 30, err: float = 0.01, read_len: int = 100):
    """The spectrum tests' sequencing run: a seeded random genome, reads of read_len from either strand at `coverage`, each base
    wrong with probability err -> an even number of read strings (pairs)."""
    import random
    rnd = random.Random(seed)
    comp = {"A": "T", "T": "A", "G": "C", "C": "G"}
    g = "".join(rnd.choice("AGCT") for _ in range(genome_len))
    n = 2 * (genome_len * coverage // read_len // 2)
    reads = []
    for _ in range(n):
        st = rnd.randrange(0, genome_len - read_len + 1)
        r = g[st:st + read_len]
        if rnd.random() < 0.5:
            r = "".join(comp[c] for c in reversed(r))
        reads.append("".join(c if rnd.random() >= err else rnd.choice([x for x in "AGCT" if x != c]) for c in r))
    return reads
