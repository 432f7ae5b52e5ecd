"""gk_map_spectrum / gk_dist_spectrum / rounds="auto" on the GPU (-m gpu).  Every spectrum is compared, exactly, with the
oracle's table (O.PMap(k, 1)) on the same `.bin` through spectrum_ref.spectrum_of; the chosen cutoff with the restatement of
the rule (spectrum_ref.cutoff_of) applied to the oracle's spectrum."""
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dist import DistDNAMap, HipDist, unique_id
from genome_amd.dist_pipeline import build_graph
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.freqfilter import PairedEndData, extractFilteredKmers
from genome_amd.graph import buildGraph
from genome_amd.partitioned import PartitionedDNAMap
from oracle import oracle as O
from oracle import pyref as R
from spectrum_ref import cutoff_of, genome_reads, spectrum_of

pytestmark = pytest.mark.gpu
LDS_BINS = 8192            # gk_spectrum.hip: counts from here on go straight to the global histogram


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ragged_reads(k, seed=None):
    """a few hundred ragged reads over a 1 200-base genome, as test_table_gpu.py makes them"""
    rnd = random.Random(k if seed is None else seed)
    g = "".join(rnd.choice("AGCT") for _ in range(1200))
    reads = []
    for _ in range(300):
        ln = rnd.randint(max(1, k - 5), min(255, k + 120))
        st = rnd.randrange(0, 1200 - ln + 1)
        r = g[st:st + ln]
        if rnd.random() < 0.5:
            r = R.rev_comp(r)
        reads.append("".join(c if rnd.random() >= 0.02 else rnd.choice([x for x in "AGCT" if x != c]) for c in r))
    return reads + ["", "A", "".join(rnd.choice("AGCT") for _ in range(255))]


_ORACLE = {}


def _oracle_counts(k, rounds=0):
    """counts of the oracle's table over _ragged_reads(k), after delete_lt(rounds) — computed once and shared"""
    if (k, rounds) not in _ORACLE:
        reads = _ragged_reads(k)
        ref = O.PMap(k, 1)
        occ = ref.count_reads(dna.reads_to_bin(reads), len(reads))
        if rounds:
            ref.delete_lt(rounds)
        cnt = ref.export_sorted()[2].astype(np.int64)
        cnt.setflags(write=False)
        _ORACLE[(k, rounds)] = (cnt, occ)
        ref.close()
    return _ORACLE[(k, rounds)]


def _check(m, counts, bins=4096):
    """m.spectrum(bins) against the oracle's counts, gk_map_size and gk_map_verify; the table is not changed"""
    before = m.verify_checksum()
    s = m.spectrum(bins)
    assert np.array_equal(s["hist"], spectrum_of(counts, bins)), bins
    assert s["distinct"] == len(counts) == m.size() == before[0]
    assert s["occurrences"] == int(counts.sum()) == before[2]
    assert s["max_count"] == (int(counts.max()) if len(counts) else 0)
    assert m.verify_checksum() == before and before[1] == 0
    return s


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k", [21, 31, 34, 47, 63, 64])
def test_every_slot_layout(ctx, k, path):
    """12-byte count slots (a fresh count at k <= 31), 16-byte graph slots (the same map after deleteAll), 24-byte slots
    (k >= 34) and k = 64's tagged slots, filled by either insert path."""
    reads = _ragged_reads(k)
    binb = dna.reads_to_bin(reads)
    counts, occ = _oracle_counts(k)
    m = HipDNAMap(ctx, k, 1 << 13)
    m.set_insert_path(path)
    assert m.count_reads(binb, len(reads)) == occ
    st = m.stats()
    assert st["slot_bytes"] == (12 if k <= 31 else 24)
    if path == "partitioned" and st["retries_direct"] == 0:
        assert st["partitioned_launches"] >= 1 and st["last_slot"] == ("count12" if k <= 31 else "slot24")
    _check(m, counts)
    kept = _oracle_counts(k, 2)[0]
    assert 0 < len(kept) < len(counts)
    m.deleteAll_lt(2)
    assert m.stats()["slot_bytes"] == (16 if k <= 31 else 24)
    _check(m, kept)
    m.close()


def test_bins_edges(ctx):
    """the overflow fold around the largest count, the smallest and the largest histogram"""
    k = 21
    reads = _ragged_reads(k)
    counts, _ = _oracle_counts(k)
    top = int(counts.max())
    assert top >= 4
    m = HipDNAMap(ctx, k, 1 << 13)
    m.count_reads(dna.reads_to_bin(reads), len(reads))
    for bins in (2, 3, top, top + 1, top + 2, LDS_BINS, 1 << 20):
        s = _check(m, counts, bins)
        assert int(s["hist"].sum()) == len(counts) and s["hist"][0] == 0
    assert _check(m, counts, top)["hist"][top - 1] == int((counts >= top - 1).sum())             # the top two counts fold
    assert _check(m, counts, top + 1)["hist"][top] == int((counts == top).sum()) >= 1            # the overflow bin holds exactly the top
    assert _check(m, counts, top + 2)["hist"][top + 1] == 0                                      # and is empty one further
    for bad in (0, 1, (1 << 20) + 1):
        with pytest.raises(L.GkError) as e:
            m.spectrum(bad)
        assert e.value.code == L.GK_E_INVALID
    # null out-pointers are skipped
    h = np.zeros(64, np.uint64)
    L.check(L.lib().gk_map_spectrum(m.h, L.ptr(h, L.C.c_uint64), 64, None, None, None), ctx.h)
    assert np.array_equal(h, spectrum_of(counts, 64))
    m.close()


@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_counts_beyond_the_lds_range(ctx, path):
    """300 reads of 255 x A at k = 31 give one key a count of 67 500, far past the 8192 bins a workgroup keeps in LDS: it goes
    straight to the global histogram — into its own bin, or into an overflow bin on either side of the LDS range."""
    k = 31
    reads = _ragged_reads(k, seed=77) + ["A" * 255] * 300
    random.Random(5).shuffle(reads)
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, len(reads))
    counts = ref.export_sorted()[2].astype(np.int64)
    ref.close()
    assert counts.max() == 300 * 225 > LDS_BINS
    m = HipDNAMap(ctx, k, 1 << 13)
    m.set_insert_path(path)
    assert m.count_reads(binb, len(reads)) == occ
    for bins in (1 << 17, 67500, 67501, 67502, LDS_BINS + 1, LDS_BINS, LDS_BINS - 1, 4096):
        s = _check(m, counts, bins)
        assert s["max_count"] == 67500
        assert s["hist"][min(67500, bins - 1)] == 1
    m.close()


@pytest.mark.parametrize("k,n", [(31, 40), (47, 64)])
def test_all_singletons(ctx, k, n):
    """random reads with no repeats: every live lane of every wave is in bin 1 (the ballot path), and nothing else is"""
    rnd = random.Random(1000 + k)
    reads = ["".join(rnd.choice("AGCT") for _ in range(150)) for _ in range(n)]
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(k, 1)
    ref.count_reads(binb, n)
    counts = ref.export_sorted()[2].astype(np.int64)
    ref.close()
    assert len(counts) == n * (150 - k + 1) >= 4000 and counts.max() == 1
    m = HipDNAMap(ctx, k, len(counts))
    m.count_reads(binb, n)
    s = _check(m, counts)
    assert s["hist"][1] == len(counts)
    assert _check(m, counts, 2)["hist"][1] == len(counts)
    m.close()


def test_void_tables(ctx):
    """A new map and a cleared one hold void bytes (the clear is deferred): all zeros, without the slots being read.  After a
    clear and a small count only the new keys are seen."""
    k = 21
    reads = _ragged_reads(k)
    counts, _ = _oracle_counts(k)
    zero = np.zeros(0, np.int64)
    for path in ("direct", "partitioned"):
        m = HipDNAMap(ctx, k, 1 << 13)
        m.set_insert_path(path)
        s = m.spectrum(64)
        assert not s["hist"].any() and (s["distinct"], s["occurrences"], s["max_count"]) == (0, 0, 0)
        assert m.size() == 0
        m.count_reads(dna.reads_to_bin(reads), len(reads))
        _check(m, counts)
        m.clear()
        s = m.spectrum(64)
        assert not s["hist"].any() and (s["distinct"], s["occurrences"], s["max_count"]) == (0, 0, 0)
        few = ["AGCTTGCATGCCGATAGCATCGATTAGC", "AGCTTGCATGCCGATAGCATCGATTAGC", "TTTTTTTTTTTTTTTTTTTTTTTTT"]
        ref = O.PMap(k, 1)
        ref.count_reads(dna.reads_to_bin(few), len(few))
        small = ref.export_sorted()[2].astype(np.int64)
        ref.close()
        m.count_reads(dna.reads_to_bin(few), len(few))
        _check(m, small, 64)
        m.clear()
        _check(m, zero, 64)              # (gk_map_verify materialises the clear: an empty table whose slots ARE read)
        _check(m, zero, 64)
        m.close()


@pytest.mark.parametrize("P", [2, 5])
@pytest.mark.parametrize("k", [21, 47])
def test_logical_partitions_add_up(ctx, k, P):
    reads = _ragged_reads(k)
    counts, occ = _oracle_counts(k)
    pm = PartitionedDNAMap(ctx, k, P)
    assert pm.count_reads(dna.reads_to_bin(reads), len(reads)) == occ
    s = pm.spectrum(256)
    assert np.array_equal(s["hist"], spectrum_of(counts, 256)) and s["hist"].dtype == np.uint64
    assert (s["distinct"], s["occurrences"], s["max_count"]) == (len(counts), int(counts.sum()), int(counts.max()))
    assert sum(1 for p in pm.parts if p.size()) >= 2
    pm.close()


def _run_ranks(world, body, timeout=120):
    """`body(rank, ctx, hd)` on one thread per rank over the loopback transport (as tests/test_dist_gpu.py does)"""
    import threading
    id128 = bytes(random.Random(world * 104729 + 7).getrandbits(8) for _ in range(128))
    out, errors = [None] * world, []

    def run(rank):
        try:
            c = Context(0)
            hd = HipDist(c, rank, world, id128, loopback=True)
            out[rank] = body(rank, c, hd)
            hd.barrier()
            hd.close(); c.close()
        except BaseException as e:          # noqa: BLE001 — reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    assert not errors, errors
    return out


@pytest.mark.parametrize("world,k", [(2, 31), (3, 47)])
def test_ranks_over_the_loopback_transport(world, k):
    """Every rank's gk_dist_spectrum is the one-rank spectrum of the union of the ranks' reads.  Then one rank cannot take its
    spectrum (it passes no map: no failure-injection hook of the test build reaches this call, so the failure is a real local
    one): it still enters the collective, EVERY rank gets an error, nobody hangs, and the handle works afterwards."""
    reads = _ragged_reads(k)
    counts, occ = _oracle_counts(k)
    bad = world - 1

    def body(rank, c, hd):
        pm = DistDNAMap(hd, k, 1 << 10)
        mine = reads[len(reads) * rank // world:len(reads) * (rank + 1) // world]
        pm.count_reads(dna.reads_to_bin(mine), len(mine))
        first = pm.spectrum(512)
        local = pm.local.spectrum(512)
        keep, err = pm.local, None
        if rank == bad:
            pm.local = None
        try:
            pm.spectrum(512)
        except L.GkError as e:
            err = (e.code, str(e))
        pm.local = keep
        again = pm.spectrum(300)
        size = pm.size()
        pm.close()
        return first, local, err, again, size

    res = _run_ranks(world, body)
    assert sum(r[1]["distinct"] for r in res) == len(counts) and sum(1 for r in res if r[1]["distinct"]) >= 2
    for rank, (first, local, err, again, size) in enumerate(res):
        for s, bins in ((first, 512), (again, 300)):
            assert np.array_equal(s["hist"], spectrum_of(counts, bins))
            assert (s["distinct"], s["occurrences"], s["max_count"]) == (len(counts), occ, int(counts.max()))
        assert size == len(counts)
        assert err is not None and err[0] == (L.GK_E_INVALID if rank == bad else L.GK_E_COMM), (rank, err)


def test_one_rank_communicator(ctx):
    """world 1 over RCCL: the two all-reduces run through the real transport"""
    k = 31
    reads = _ragged_reads(k)
    counts, occ = _oracle_counts(k)
    hd = HipDist(ctx, 0, 1, unique_id())
    pm = DistDNAMap(hd, k)
    pm.count_reads(dna.reads_to_bin(reads), len(reads))
    s = pm.spectrum(1024)
    assert np.array_equal(s["hist"], spectrum_of(counts, 1024))
    assert (s["distinct"], s["occurrences"], s["max_count"]) == (len(counts), occ, int(counts.max()))
    pm.close(); hd.close()


SEED, K = 20261, 21


@pytest.fixture(scope="module")
def genome_run():
    """the 3 000-base genome at 30x with 1 % errors (the recorded spectrum of tests/golden/spectrum/ is the oracle's over it)"""
    reads = genome_reads(SEED)
    binb = dna.reads_to_bin(reads)
    ref = O.PMap(K, 1)
    ref.count_reads(binb, len(reads))
    counts = ref.export_sorted()[2].astype(np.int64)
    ref.close()
    return PairedEndData(len(reads) // 2, binb), counts, cutoff_of(spectrum_of(counts, 4096))


def test_auto_cutoff_end_to_end(ctx, genome_run):
    data, counts, (valley, peak, gsize) = genome_run
    assert (valley, peak, gsize) == (5, 18, 3205)
    m = extractFilteredKmers(data, K, "auto", ctx)
    assert np.array_equal(m.auto["spectrum"]["hist"], spectrum_of(counts, 4096))
    assert (m.auto["rounds"], m.auto["rounds_auto"], m.auto["valley"], m.auto["peak"], m.auto["genome_size_estimate"]) == (valley, True, valley, peak, gsize)
    assert m.size() == int((counts >= valley).sum())
    g = buildGraph(K, m)
    m2 = extractFilteredKmers(data, K, valley, ctx)
    g2 = buildGraph(K, m2)
    assert g.checksum() == g2.checksum() and g.counts() == g2.counts()
    # the same through the singleton pre-filter (min_count = 2: bin 1 is incomplete) and over logical partitions
    m3 = extractFilteredKmers(data, K, "auto", ctx, prefilter_distinct=len(counts))
    assert m3.auto["valley"] == cutoff_of(spectrum_of(counts, 4096), 2)[0] == valley
    assert m3.verify_checksum() == m.verify_checksum()
    m4 = extractFilteredKmers(data, K, "auto", ctx, partitions=3)
    assert m4.auto["valley"] == valley and m4.verify() == m.verify_checksum()
    # the N-rank flow at world 1
    hd = HipDist(ctx, 0, 1, unique_id())
    g5, st = build_graph(hd, data, K, rounds="auto", retain=False)
    g6, st6 = build_graph(hd, data, K, rounds=valley, retain=False)
    assert (st["rounds"], st["rounds_auto"], st["valley"], st["peak"], st["genome_size_estimate"]) == (valley, True, valley, peak, gsize)
    assert g5.checksum() == g.checksum() == g6.checksum()
    assert set(st) - set(st6) == {"rounds_auto", "valley", "peak", "genome_size_estimate"} and {x: st[x] for x in st6} == st6
    for x in (g, g2, g5, g6, m, m2, m3, m4):
        x.close()
    hd.close()


def test_auto_without_a_valley_falls_back_to_three(ctx):
    """a spectrum that never rises (540 singletons, 180 keys seen twice, 180 seen three times): the cutoff is the reference's 3
    and the result says it was not chosen"""
    rnd = random.Random(9)
    reads = ["".join(rnd.choice("AGCT") for _ in range(120)) for _ in range(10)]
    reads = reads + reads[:4] + reads[:2]
    m = extractFilteredKmers(PairedEndData(8, dna.reads_to_bin(reads)), 31, "auto", ctx)
    assert m.auto["spectrum"]["hist"][:5].tolist() == [0, 540, 180, 180, 0]
    assert (m.auto["rounds"], m.auto["rounds_auto"], m.auto["valley"], m.auto["peak"]) == (3, False, 0, 0)
    assert m.size() == 180
    m.close()
