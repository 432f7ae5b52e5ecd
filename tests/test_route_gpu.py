"""The owner-routing kernels held EXACTLY to the plain restatement tests/route_ref.py (-m gpu): k_skm_route (both framings:
gk_shard_superkmers_dev and, through the test build's gk_test_skm_route_offsets, the offset-table instantiation that only
gk_dist_* reaches in the product) and k_shard_count / k_shard_scatter (gk_shard_reads_dev), on the shared inputs of
tests/route_cases.py: 200 reads — four tiles — whose lengths sit on the edges of the record cutting rule, with random bytes behind
every read's last base.

Every output buffer lies between two guards inside one allocation that starts as one byte pattern: the counts, the sorted
records (keys) of every owner's region, every byte of a region past its records and both guards are compared, so a record too
many, a stale slot, a region that starts in the wrong place or a write beside the buffer all show.  Every case also runs under
"test_max_grid" = 1 and 3 (include/genome_amd_test.h): one workgroup then takes all four tiles — a regrouped tile and ordinary
ones in the mixed set —, carries its k-mer counts across tiles and clears its per-tile counters.  tests/test_route_cpu.py holds
the restatement itself to gk_owner_of, to hand-written records and to the naive oracle."""
import ctypes as C

import numpy as np
import pytest

import route_cases as RC
import route_ref as RR
from genome_amd import _lib as L
from genome_amd.dnamap import Context, HipDNAMap, skm_slot_bytes
from genome_amd.partitioned import PartitionedDNAMap
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PATTERN = 0xC7
GUARD = 4096             # bytes before the buffer (a multiple of 16: the records are written with 16-byte stores)
GRIDS = (0, 1, 3)
N = RC.NREADS


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


class capped:
    """the context under "test_max_grid" = grid; the echo must have risen by `launches` per call made inside (grid > 0), by 0 (grid 0)"""

    def __init__(self, ctx, grid, launches):
        self.ctx, self.grid, self.launches = ctx, grid, launches

    def __enter__(self):
        self.ctx.set_option("test_max_grid", self.grid)
        self.before = self.ctx.grid_cap_uses()
        return self

    def __exit__(self, et, ev, tb):
        rose = self.ctx.grid_cap_uses() - self.before
        self.ctx.set_option("test_max_grid", 0)
        if et is None:
            assert rose == (self.launches if self.grid else 0), (rose, self.grid)
        return False


def upload(ctx, arr, shift=0):
    """-> (allocation, pointer to the data `shift` bytes into it)"""
    arr = np.ascontiguousarray(arr)
    d = ctx.alloc(arr.nbytes + 64)
    ctx.upload(d + shift, arr.view(np.uint8).reshape(-1))
    return d, d + shift


def route(ctx, k, P, cap, d_rec, read_len=None, d_off=None, windows=0, nreads=N):
    """one routing call into a guarded, pattern-filled buffer of `cap` slots, straight through the C-ABI (the Python wrapper raises
    before it returns the counts of a GK_E_CAPACITY).  -> (status, records per owner, windows per owner, the whole block)"""
    slot = skm_slot_bytes(k)
    total = GUARD + cap * slot + GUARD
    d_blk = ctx.alloc(total)
    ctx.upload(d_blk, np.full(total, PATTERN, np.uint8))
    recs, kmers = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
    if d_off is None:
        rc = L.lib().gk_shard_superkmers_dev(ctx.h, k, d_rec, nreads, read_len, P, d_blk + GUARD, cap, L.ptr(recs, C.c_uint64), L.ptr(kmers, C.c_uint64))
    else:
        rc = L.test_hook("gk_test_skm_route_offsets")(ctx.h, k, d_rec, d_off, nreads, windows, P, d_blk + GUARD, cap, L.ptr(recs, C.c_uint64),
                                                      L.ptr(kmers, C.c_uint64))
    blk = ctx.download(d_blk, total)
    ctx.free(d_blk)
    return rc, [int(x) for x in recs], [int(x) for x in kmers], blk


def assert_guards(blk, nbytes):
    assert (blk[:GUARD] == PATTERN).all(), "written before the buffer"
    assert (blk[GUARD + nbytes:] == PATTERN).all(), "written behind the buffer"


def assert_regions(blk, k, P, cap, recs, kmers, want):
    slot = RR.slot_bytes(k)
    assert slot == skm_slot_bytes(k)
    assert recs == [w.recs for w in want], "records per owner"
    assert kmers == [w.kmers for w in want], "windows per owner"
    assert_guards(blk, cap * slot)
    out = blk[GUARD:GUARD + cap * slot]
    region = cap // P
    for p in range(P):
        reg = out[p * region * slot:(p + 1) * region * slot]
        rows = sorted(bytes(r) for r in reg[:recs[p] * slot].reshape(-1, slot))
        assert rows == want[p].rows, f"owner {p}: the records of its region"
        assert (reg[recs[p] * slot:] == PATTERN).all(), f"owner {p}: slots past its records were written"
    assert (out[P * region * slot:] == PATTERN).all(), "slots behind the last region were written"


def roomy(want, P):
    """slots for the fullest region and three more, and a total that is no multiple of P (the regions are floor(cap / P) slots)"""
    return P * (max(w.recs for w in want) + 3) + (1 if P > 1 else 0)


# ---- gk_shard_superkmers_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k,L_,P", RC.CASES)
def test_superkmer_records_exact(ctx, k, L_, P, grid):
    want = RC.expected_records("fixed", k, L_, P)
    assert sum(w.recs for w in want) > N // 2
    d, d_rec = upload(ctx, RC.fixed_set(k, L_)[0])
    try:
        cap = roomy(want, P)
        with capped(ctx, grid, 1):
            rc, recs, kmers, blk = route(ctx, k, P, cap, d_rec, read_len=L_)
        assert rc == L.GK_OK
        assert_regions(blk, k, P, cap, recs, kmers, want)
    finally:
        ctx.free(d)


@pytest.mark.parametrize("grid", GRIDS)
def test_regrouped_tile_then_ordinary_tiles(ctx, grid):
    """the mixed set (tests/test_route_cpu.py asserts its run counts): tile 0 overflows the descriptor list and is redone in
    groups of 16 reads, tiles 1 to 3 are not; under one workgroup the same workgroup does both, one after the other"""
    k, P, L_ = RC.MIXED_K, RC.MIXED_P, RC.MIXED_L
    want = RC.expected_records("mixed", k, L_, P)
    d, d_rec = upload(ctx, RC.mixed_set()[0])
    try:
        cap = roomy(want, P)
        with capped(ctx, grid, 1):
            rc, recs, kmers, blk = route(ctx, k, P, cap, d_rec, read_len=L_)
        assert rc == L.GK_OK
        assert_regions(blk, k, P, cap, recs, kmers, want)
    finally:
        ctx.free(d)


FIT_CASES = [("fixed", 31, 150, 3), ("fixed", 7, 255, 16), ("fixed", 34, 255, 16), ("fixed", 64, 150, 64), ("fixed", 21, 255, 1), ("fixed", 11, 60, 3),
             ("mixed", RC.MIXED_K, RC.MIXED_L, RC.MIXED_P)]


@pytest.mark.parametrize("grid", (0, 1))
@pytest.mark.parametrize("kind,k,L_,P", FIT_CASES)
def test_exact_fit_and_overflow(ctx, kind, k, L_, P, grid):
    """out_cap_records = P * max(recs) holds everything (the fullest region ends exactly at its last slot); one slot per region less
    is GK_E_CAPACITY, with the counts reported all the same and nothing written outside the buffer"""
    want = RC.expected_records(kind, k, L_, P)
    rec = RC.fixed_set(k, L_)[0] if kind == "fixed" else RC.mixed_set()[0]
    need = max(w.recs for w in want)
    assert need > 1
    d, d_rec = upload(ctx, rec)
    try:
        with capped(ctx, grid, 2):
            rc, recs, kmers, blk = route(ctx, k, P, P * need, d_rec, read_len=L_)
            rc2, recs2, kmers2, blk2 = route(ctx, k, P, P * (need - 1), d_rec, read_len=L_)
        assert rc == L.GK_OK
        assert_regions(blk, k, P, P * need, recs, kmers, want)
        assert rc2 == L.GK_E_CAPACITY
        assert recs2 == [w.recs for w in want] and kmers2 == [w.kmers for w in want]
        assert_guards(blk2, P * (need - 1) * RR.slot_bytes(k))
    finally:
        ctx.free(d)


UNALIGNED_CASES = [(31, 150, 3), (7, 255, 16), (34, 255, 16), (64, 150, 64), (11, 60, 3)]


@pytest.mark.parametrize("grid", (0, 1))
@pytest.mark.parametrize("k,L_,P", UNALIGNED_CASES)
def test_unaligned_record_pointer(ctx, k, L_, P, grid):
    """the same records 5 bytes into an allocation: the staging widens the tile's byte range to 16-byte blocks below the pointer"""
    want = RC.expected_records("fixed", k, L_, P)
    d, d_rec = upload(ctx, RC.fixed_set(k, L_)[0], shift=5)
    assert d_rec % 16 == 5
    try:
        cap = roomy(want, P)
        with capped(ctx, grid, 1):
            rc, recs, kmers, blk = route(ctx, k, P, cap, d_rec, read_len=L_)
        assert rc == L.GK_OK
        assert_regions(blk, k, P, cap, recs, kmers, want)
    finally:
        ctx.free(d)


# ---- the offset-table instantiation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k,L_,P", RC.RAGGED_CASES)
def test_offset_framing_exact(ctx, k, L_, P, grid):
    buf, off, _, windows = RC.ragged_set(k, L_)
    want = RC.expected_records("ragged", k, L_, P)
    d, d_rec = upload(ctx, buf)
    d2, d_off = upload(ctx, off)
    try:
        cap = roomy(want, P)
        with capped(ctx, grid, 1):
            rc, recs, kmers, blk = route(ctx, k, P, cap, d_rec, d_off=d_off, windows=windows)
        assert rc == L.GK_OK
        assert sum(kmers) == windows
        assert_regions(blk, k, P, cap, recs, kmers, want)
    finally:
        ctx.free(d); ctx.free(d2)


@pytest.mark.parametrize("k,L_,P", [(31, 150, 3), (34, 255, 16), (7, 60, 16)])
def test_uniform_stream_both_framings(ctx, k, L_, P):
    """a stream of equal-length records is both: the offset table r * stride gives the fixed-stride call's records"""
    rec, off, _ = RC.uniform_set(k, L_)
    want = RC.expected_records("uniform", k, L_, P)
    d, d_rec = upload(ctx, rec)
    d2, d_off = upload(ctx, off)
    try:
        cap = roomy(want, P)
        for grid in (0, 1):
            with capped(ctx, grid, 2):
                a = route(ctx, k, P, cap, d_rec, read_len=L_)
                b = route(ctx, k, P, cap, d_rec, d_off=d_off, windows=N * (L_ - k + 1))
            for rc, recs, kmers, blk in (a, b):
                assert rc == L.GK_OK
                assert_regions(blk, k, P, cap, recs, kmers, want)
    finally:
        ctx.free(d); ctx.free(d2)


# ---- gk_shard_reads_dev -------------------------------------------------------------------------------------------------------------------
SHARD_CASES = [(31, 60, P) for P in RC.P_ALL] + [(34, 60, P) for P in RC.P_ALL] + [(7, 150, 16), (64, 150, 3), (21, 150, 64), (63, 150, 1)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k,L_,P", SHARD_CASES)
def test_shard_reads_exact(ctx, k, L_, P, grid):
    """counts, the prefix-summed region layout and every owner's keys ([lo] or [lo, hi] interleaved), exactly.  The key buffer has
    the declared nreads * (L - k + 1) keys; the guard behind it is four buffers long, so that a cursor or a rank that is not
    reset between the four tiles of one workgroup (each adds at most one buffer) lands in the guard, not in someone's memory."""
    W = 1 if k <= 32 else 2
    want_keys, want_counts = RC.expected_keys("fixed", k, L_, P)
    keys_cap = N * (L_ - k + 1)
    nbytes = keys_cap * 8 * W
    total = GUARD + nbytes + 4 * nbytes
    assert 0 < sum(want_counts) < keys_cap
    d, d_rec = upload(ctx, RC.fixed_set(k, L_)[0])
    d_blk = ctx.alloc(total)
    try:
        ctx.upload(d_blk, np.full(total, PATTERN, np.uint8))
        counts = np.zeros(P, np.uint64)
        with capped(ctx, grid, 2):
            rc = L.lib().gk_shard_reads_dev(ctx.h, k, d_rec, N, L_, P, d_blk + GUARD, keys_cap, L.ptr(counts, C.c_uint64))
        assert rc == L.GK_OK
        blk = ctx.download(d_blk, total)
        assert [int(c) for c in counts] == want_counts
        assert_guards(blk, nbytes)
        words = blk[GUARD:GUARD + nbytes].view(np.uint64).reshape(-1, W)
        off = 0
        for p in range(P):
            part = words[off:off + want_counts[p]]
            got = sorted((int(r[0]), int(r[1]) if W == 2 else 0) for r in part)
            assert got == want_keys[p], f"owner {p}: the keys of its region"
            off += want_counts[p]
        assert (blk[GUARD + off * 8 * W:GUARD + nbytes] == PATTERN).all(), "keys behind the last region"
    finally:
        ctx.free(d_blk); ctx.free(d)


@pytest.mark.parametrize("k,P", [(31, 3), (31, 8), (34, 3), (34, 8)])
def test_partitioned_map_from_routed_keys(ctx, k, P):
    """PartitionedDNAMap.count_reads_dev_keys (gk_shard_reads_dev with P > 1, then owner-side inserts of every region): the
    oracle's table, and no key in a partition that is not its owner's"""
    L_ = 150
    rec = RC.uniform_set(k, L_)[0]
    ref = O.PMap(k, 1)
    occ = ref.count_reads(rec.tobytes(), N)
    d, d_rec = upload(ctx, rec)
    pm = PartitionedDNAMap(ctx, k, P)
    try:
        assert pm.count_reads_dev_keys(d_rec, N, L_) == occ == N * (L_ - k + 1)
        for name, a, b in zip(("lo", "hi", "count"), pm.sorted_items(), ref.export_sorted()):
            assert np.array_equal(a, b), name
        assert pm.foreign_keys() == 0
        assert min(p.size() for p in pm.parts) > 0
    finally:
        pm.close(); ctx.free(d)


# ---- the receiver ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,L_,P", [(31, 150, 3), (64, 255, 16)])
def test_receiver_counts_the_exact_records(ctx, k, L_, P):
    """the restatement's records — not the kernel's — through gk_map_count_superkmers_dev, both insert paths: the oracle's table of
    the reads the records were cut from"""
    regions = RC.expected_records("fixed", k, L_, P)
    rows = [r for reg in regions for r in reg.rows]
    kmers = sum(reg.kmers for reg in regions)
    stream = b"".join(bytes([n]) + v.to_bytes((n + 3) // 4, "little") for v, n in RC.fixed_set(k, L_)[1].reads())
    ref = O.PMap(k, 1)
    assert ref.count_reads(stream, N) == kmers
    d, d_rows = upload(ctx, np.frombuffer(b"".join(rows), np.uint8))
    try:
        for path in ("direct", "partitioned"):
            m = HipDNAMap(ctx, k)
            m.set_insert_path(path)
            assert m.count_superkmers_dev(d_rows, len(rows), kmers) == kmers
            for name, a, b in zip(("lo", "hi", "count"), m.sorted_items(), ref.export_sorted()):
                assert np.array_equal(a, b), (path, name)
            m.close()
    finally:
        ctx.free(d)


# ---- the switch's echo ---------------------------------------------------------------------------------------------------------------------
def test_grid_cap_reaches_all_three_entry_points(ctx):
    k, L_, P = 31, 150, 3
    rec = RC.fixed_set(k, L_)[0]
    buf, off, _, windows = RC.ragged_set(k, L_)
    d, d_rec = upload(ctx, rec)
    d1, d_rag = upload(ctx, buf)
    d2, d_off = upload(ctx, off)
    d_keys = ctx.alloc(N * (L_ - k + 1) * 8)
    try:
        calls = (lambda: route(ctx, k, P, 4096 * P, d_rec, read_len=L_)[0],
                 lambda: route(ctx, k, P, 4096 * P, d_rag, d_off=d_off, windows=windows)[0],
                 lambda: L.lib().gk_shard_reads_dev(ctx.h, k, d_rec, N, L_, P, d_keys, N * (L_ - k + 1), L.ptr(np.zeros(P, np.uint64), C.c_uint64)))
        for call in calls:
            before = ctx.grid_cap_uses()
            assert call() == 0
            assert ctx.grid_cap_uses() == before              # switch off: nothing is counted
            ctx.set_option("test_max_grid", 1)
            try:
                assert call() == 0
                assert ctx.grid_cap_uses() > before
            finally:
                ctx.set_option("test_max_grid", 0)
    finally:
        for p in (d, d1, d2, d_keys):
            ctx.free(p)
