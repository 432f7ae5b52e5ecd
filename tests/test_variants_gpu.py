"""Every switchable kernel variant against the CPU oracle, at a size the oracle can follow (-m gpu).

The partitioned insert pipeline, the filter, the graph table and the components' link pass are each a FAMILY of kernels, and
the host picks a member from the table's geometry (fine buckets per L1 bucket, LDS fit), which no oracle-sized input controls.
The test build's A/B switches (gk_ctx_set_option, include/genome_amd_test.h) force each member on a small table; gk_map_stats'
"last_*" keys say which member the last partitioned batch really launched, and every case asserts them — a forced switch that
silently fell back to the default kernel would prove nothing.

Every forced option lives inside `with forced(ctx, ...)`, which restores the defaults of gk_internal.h in `finally`.

Pairs that cannot run anywhere (by the code, not by choice):
  * p4_wide = 1 with 16-byte keys never sorts 8192 keys: the 16-byte family has ONE 1024-thread member, 6144 keys
    (gk_partition.hip P4_FORMS; p4_choose_op and p4_choose_exact take "sort12288" for `W == 1` only); p4_wide = 1 and 2 are
    both asserted as "sort6144" there.
  * p2_wide = 1 under min_lnb1 = 9 / 10: the 1024-bucket L1 scatter has no 1024-thread member (part_choose: p2_threads is
    1024 only for `nb1 <= 256`); asserted as "plain" / "sorted".
  * p45_stripes, p4_grid, p24_pieces on the exact fine level: stripes are `fine_exact ? 1 : ch.op_stripes`, pieces need `!fine_exact`,
    and only PartBatch::launch_p4_op reads p4_grid (p4_per_cu); they are run with fine_exact = 0 and asserted on batches that stayed over-provisioned.
  * target_load_pct at k = 64: target_load() returns 0.45 for the tagged table before it looks at the switch; asserted as
    "no change of slots()".  graph_load_pct at k = 64 is capped at the tagged table's densest step, 45 (graph_table_load).
  * filter_classic = 0 at k = 64: filter_compact_streaming refuses tagged slots; asserted as "classic".
  * graph_mbt = 1 at k = 64: graph_build_entry never buckets tagged slots (`m->k != 64`); asserted as "no bucketed table".
Taken on trust: cc_find has no echo — the four forms differ only in which parent pointers they write, never in the result, so
the result against the oracle is the whole check.  With this module every option name of gk_testhooks.hip is set by some test
("test_max_grid", the cap of the graph phase's launch grids, by tests/test_small_grid_gpu.py through forced() below).
"""
import os
import random
from contextlib import contextmanager

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from genome_amd import _lib as L
from genome_amd import dna, synth
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import buildGraph
from oracle import oracle as O
from oracle import pyref as R
from test_fuzz_gpu import _oracle_graph, _reads

pytestmark = pytest.mark.gpu

# gk_internal.h: -1 for the tri-states, cc_find 3, graph_mbt_keys 256, 0 otherwise
DEFAULTS = {"p4_wide": -1, "p4_direct": -1, "p2_wide": -1, "p2_sorted": -1, "p45_stripes": -1, "p4_grid": -1, "p24_pieces": -1,
            "fine_exact": -1, "filter_classic": -1, "graph_load_pct": -1, "graph_mbt": -1, "graph_mbt_keys": 256, "cc_find": 3,
            "part_exact": 0, "host_ragged": 0, "min_lnb1": 0, "target_load_pct": 0, "test_no_reserve": 0, "test_max_grid": 0}

KS = (21, 31, 35, 55, 64)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@contextmanager
def forced(ctx, **opts):
    """Set test-build switches for the duration of the block; the defaults come back whatever happens inside."""
    try:
        for name, v in opts.items():
            assert name in DEFAULTS, name
            ctx.set_option(name, v)
        yield
    finally:
        for name in opts:
            ctx.set_option(name, DEFAULTS[name])


def assert_same_table(got, want):
    for name, a, b in zip(("lo", "hi", "count"), got, want):
        assert a.shape == b.shape, f"{name}: {a.shape} vs {b.shape}"
        assert np.array_equal(a, b), name


def _W(k):
    return 1 if k <= 32 else 2


# ---------------------------------------------------------------------------------------------------------------------------
# (a) insert variants x key width x input shape x table state
# ---------------------------------------------------------------------------------------------------------------------------
# reads of the device-resident inputs.  Repeat-heavy: enough for several pieces of a forced "p24_pieces" batch at every k (its table
# stays small whatever the read count); near-distinct: every window is a key the comparison has to sort
N_DEV = {"G": 8000, "U": 3000, "keys": 4000}
_CACHE = {}


def _dev_reads(k, kind):
    L_ = k + 99
    if kind != "U":    # a small genome: every k-mer many times over (spills of the over-provisioned level, m->repeats)
        return synth.reads_mode_g(N_DEV[kind], L_, 3000, 0.0005, config_id=100 + k), L_
    return synth.reads_mode_u(N_DEV[kind], L_, 200 + k), L_


def _ragged_stream(k):
    """lengths 0, k-1, k, k+1, 255 mixed with uniform runs long enough (>= 4096) to become fixed-stride chunks"""
    rnd = random.Random(3000 + k)
    g = "".join(rnd.choice("AGCT") for _ in range(4000))

    def reads(n, ln):
        return [g[s:s + ln] for s in (rnd.randrange(0, len(g) - ln + 1) for _ in range(n))]
    odd = reads(40, k - 1) + reads(40, k) + reads(40, k + 1) + reads(20, 255) + [""] * 5
    rnd.shuffle(odd)
    stream = reads(4200, 100) + odd[:70] + reads(4100, 120) + odd[70:] + reads(300, k + 3) + reads(4096, 90) + reads(5, k - 1)
    return dna.reads_to_bin(stream), len(stream)


def _oracle_states(k, kind):
    """the oracle's table after each step of the sequence every variant runs, computed once per (k, input)"""
    key = (k, kind)
    if key in _CACHE:
        return _CACHE[key]
    if kind == "ragged":
        binb, n = _ragged_stream(k)
        half_b, half_n = binb, n
        rec, L_ = None, 0
    else:
        rec, L_ = _dev_reads(k, kind)
        binb, n = rec.tobytes(), N_DEV[kind]
        half_n = n // 2
        half_b = rec[:half_n].tobytes()
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, n)
    t1 = ref.export_sorted()
    occ_half = ref.count_reads(half_b, half_n)
    t2 = ref.export_sorted()
    ref.delete_lt(2)
    t3 = ref.export_sorted()
    assert ref.count_reads(binb, n) == occ
    t4 = ref.export_sorted()
    ref.close()
    _CACHE[key] = dict(rec=rec, L=L_, binb=binb, n=n, half_b=half_b, half_n=half_n, occ=occ, occ_half=occ_half, t1=t1, t2=t2, t3=t3, t4=t4)
    return _CACHE[key]


def _expected_p4(opts, W, exact):
    wide = opts.get("p4_wide", -1)
    if exact and opts.get("p4_direct", -1) > 0:
        return "direct"
    if wide <= 0:                       # (auto takes the wide forms from 256 / 512 fine buckets per L1 bucket: no small table)
        return "sort4096"
    if W == 2:
        return "sort6144"
    return "sort12288" if wide == 2 else "sort8192"


def _check_names(opts, W, kind, st0, st1, from_empty, fits):
    """the last_* keys name the variant that was asked for; `fits`: no mid-batch sizing, so the fine level is not data-dependent"""
    host = kind.startswith("ragged")
    op1 = not opts.get("part_exact", 0) and kind != "ragged_walked"
    nb1 = st1["last_nb1"]
    lnb = opts.get("min_lnb1", 0)
    if lnb and fits:
        assert nb1 == 1 << lnb, (nb1, lnb)
    # P2
    if kind == "keys":
        assert st1["last_p2"] == ("keys" if op1 else "keys_exact")
    elif not host:
        if not op1:
            assert st1["last_p2"] == "exact"
        else:
            srt = opts.get("p2_sorted", -1)
            srt = W == 2 if srt < 0 else srt > 0
            wide = opts.get("p2_wide", -1) > 0 and nb1 <= 256
            assert st1["last_p2"] == (("wide_sorted" if srt else "wide") if wide else ("sorted" if srt else "plain"))
    else:      # a host stream ends in whatever its last chunk was
        assert st1["last_p2"] in ("exact", "plain", "sorted", "wide", "wide_sorted")
        if not op1:
            assert st1["last_p2"] == "exact"
    # fine level
    fe = opts.get("fine_exact", -1)
    must_exact = fe == 1 or not op1 or (fits and (not from_empty or (fe < 0 and st0["repeat_heavy"])))
    if host and op1:
        must_exact = fe == 1
        fits = False
    if must_exact:
        assert st1["last_fine"] == "exact"
    elif fits:
        assert st1["last_fine"] == "overprovisioned"
    else:
        assert st1["last_fine"] in ("exact", "overprovisioned")
    exact = st1["last_fine"] == "exact"
    assert st1["last_p4"] == _expected_p4(opts, W, exact)
    # stripes and pieces exist on the over-provisioned level only
    want_stripes = 1
    if not exact:
        want_stripes = max(1, min(max(opts.get("p45_stripes", -1), 1), nb1, 16))
        while nb1 % want_stripes:
            want_stripes -= 1
    assert st1["last_p4_stripes"] == want_stripes
    if kind == "G" and not exact and fits and from_empty and opts.get("p24_pieces", -1) > 1 and opts.get("p45_stripes", -1) <= 1:
        assert 2 <= st1["last_p4_pieces"] <= 8          # (N_DEV["G"] reads are several pieces of 64 tiles each at every k)
    elif exact or opts.get("p24_pieces", -1) <= 1:
        assert st1["last_p4_pieces"] == 1
    assert st1["last_slot"] == {12: "count12", 16: "slot16", 24: "slot24"}[st1["slot_bytes"]]
    assert st1["last_slot"] != "count12" or W == 1


class _Feeder:
    """one input shape: how a batch reaches the map"""

    def __init__(self, ctx, k, kind):
        self.ctx, self.k, self.kind = ctx, k, kind
        self.S = _oracle_states(k, "ragged" if kind.startswith("ragged") else "G" if kind == "hostG" else kind)
        self.d = self.dk = None
        S = self.S
        if kind in ("G", "U", "keys"):
            self.d = ctx.alloc(S["rec"].size + 64)
            ctx.upload(self.d, S["rec"])
        if kind == "keys":      # routed key arrays: one partition = the plain canonical key stream (the owner side of the exchange)
            self.dk = ctx.alloc(S["occ"] * 8 * _W(k))
            assert int(ctx.shard_reads(k, self.d, S["n"], S["L"], 1, self.dk, S["occ"])[0]) == S["occ"]
            self.dk_half = ctx.alloc(S["occ_half"] * 8 * _W(k))
            assert int(ctx.shard_reads(k, self.d, S["half_n"], S["L"], 1, self.dk_half, S["occ_half"])[0]) == S["occ_half"]

    def full(self, m):
        S = self.S
        if self.kind == "keys":
            m.update_inc_dev(self.dk, S["occ"])
            return S["occ"]
        if self.kind in ("G", "U"):
            return m.count_reads_dev(self.d, S["n"], S["L"])
        return m.count_reads(S["binb"], S["n"])

    def half(self, m):
        S = self.S
        if self.kind == "keys":
            m.update_inc_dev(self.dk_half, S["occ_half"])
            return S["occ_half"]
        if self.kind in ("G", "U"):
            return m.count_reads_dev(self.d, S["half_n"], S["L"])
        return m.count_reads(S["half_b"], S["half_n"])

    def close(self):
        for p in (self.d, self.dk, getattr(self, "dk_half", None)):
            if p:
                self.ctx.free(p)


def _step(m, feed, opts, batch, want_table, from_empty, fits, total_occ=None):
    k, kind = feed.k, feed.kind
    st0 = m.stats()
    if batch == "half":
        assert feed.half(m) == feed.S["occ_half"]
    else:
        assert feed.full(m) == feed.S["occ"]
    assert_same_table(m.sorted_items(), want_table)
    live, bad, total = m.verify()
    assert bad == 0 and live == len(want_table[0]) == m.size()
    assert total == int(want_table[2].astype(np.int64).sum())
    if total_occ is not None:
        assert total == total_occ
    st1 = m.stats()
    if st1["retries_direct"] > st0["retries_direct"]:
        # the one legitimate other route: over-provisioned regions AND the spill list overflowed on repeat-heavy input, the batch
        # was taken again by the direct path (PartBatch::give_back).  Only forced over-provisioning on the small genome gets there.
        assert opts.get("fine_exact", -1) != 1 and kind in ("G", "hostG", "keys"), (opts, kind, st1)
        assert st1["direct_launches"] > st0["direct_launches"] and st1["last_fine"] == "overprovisioned"
    else:
        assert st1["partitioned_launches"] > st0["partitioned_launches"], st1
    _check_names(opts, _W(k), kind, st0, st1, from_empty, fits)
    return st1


def _run_states(ctx, feed, opts):
    """from empty with hint 0 / with a generous hint; a second batch on top; deleteAll_lt(2) and another batch; clear() and again"""
    S, k = feed.S, feed.k
    big = 3_000_000                              # enough segments for 1024 L1 buckets: "min_lnb1" takes effect
    with forced(ctx, **opts):
        m0 = HipDNAMap(ctx, k, 0)
        m0.set_insert_path("partitioned")
        _step(m0, feed, opts, "full", S["t1"], True, False, S["occ"])
        m0.close()
        m = HipDNAMap(ctx, k, big)
        m.set_insert_path("partitioned")
        _step(m, feed, opts, "full", S["t1"], True, True, S["occ"])
        _step(m, feed, opts, "half", S["t2"], False, True, S["occ"] + S["occ_half"])
        m.deleteAll_lt(2)
        assert_same_table(m.sorted_items(), S["t3"])
        # (8-byte keys: the filter leaves 16-byte graph slots — P5's other instantiation — unless it had nothing to remove and
        #  took the tombstone form, which then does not rebuild: the ragged stream, whose second pass doubled every count)
        widened = m.stats()["slot_bytes"] == 16
        assert widened or _W(k) == 2 or len(S["t3"][0]) == len(S["t2"][0])
        st = _step(m, feed, opts, "full", S["t4"], False, False)
        if _W(k) == 1 and st["retries_direct"] == 0:
            assert st["last_slot"] == ("slot16" if widened else "count12")
        m.clear()
        assert m.size() == 0
        st = _step(m, feed, opts, "full", S["t1"], True, False, S["occ"])
        assert st["last_slot"] == ("count12" if _W(k) == 1 else "slot24")
        m.close()
    if feed.kind in ("G", "keys") and not opts.get("min_lnb1", 0):
        # A table sized for the DISTINCT keys of repeat-heavy input and not grown for the batch's windows ("test_no_reserve"): a
        # handful of L1 buckets of tens of thousands of keys each, so every bucket is several full chunks of whichever P4 form
        # runs plus a partial last one; then the same on top of the content.
        with forced(ctx, test_no_reserve=1, **opts):
            m = HipDNAMap(ctx, k, len(S["t2"][0]))
            m.set_insert_path("partitioned")
            st = _step(m, feed, opts, "full", S["t1"], True, True, S["occ"])
            assert st["last_nb1"] <= 64 and S["occ"] // st["last_nb1"] > 12288, st
            _step(m, feed, opts, "half", S["t2"], False, True, S["occ"] + S["occ_half"])
            m.close()


VARIANTS = [{}]
VARIANTS += [{"p4_wide": w, "fine_exact": f} for w in (0, 1, 2) for f in (0, 1)]
VARIANTS += [{"p4_direct": 1, "fine_exact": 1}, {"p4_direct": 1}]
VARIANTS += [{"p2_sorted": 0}, {"p2_sorted": 1}, {"p2_wide": 1, "p2_sorted": 0}, {"p2_wide": 1, "p2_sorted": 1}, {"p2_wide": 1}]
VARIANTS += [{"p45_stripes": s, "fine_exact": 0} for s in (2, 4, 16)]
VARIANTS += [{"p4_grid": g, "fine_exact": 0} for g in (1, 8)]
VARIANTS += [{"p24_pieces": 8, "p4_wide": w, "fine_exact": 0} for w in (1, 2)]
VARIANTS += [{"min_lnb1": l, "p4_wide": w, "fine_exact": f} for l in (9, 10) for w in (0, 2) for f in (0, 1)]
VARIANTS += [{"min_lnb1": 10, "p2_wide": 1, "fine_exact": 0}]


def _vid(o):
    return ",".join(f"{a}={b}" for a, b in o.items()) or "defaults"


@pytest.mark.parametrize("kind", ["G", "U", "keys", "hostG"])
@pytest.mark.parametrize("k", KS)
def test_insert_variants_device_inputs(ctx, k, kind):
    """Device-resident fixed-stride reads (repeat-heavy and near-distinct), routed key arrays, and the repeat-heavy reads as one
    uniform stream from HOST memory (its length bytes checked on the device, its upload in pieces beside P2) through every forced
    member of the P2 / P4 / P5 families: occurrences, the sorted table bit for bit, gk_map_verify, and the variant's name."""
    feed = _Feeder(ctx, k, kind)
    try:
        for opts in VARIANTS:
            try:
                _run_states(ctx, feed, opts)
            except Exception as e:
                raise AssertionError(f"variant [{_vid(opts)}] k={k} input={kind}: {e!r}") from e
    finally:
        feed.close()


# the exact level is all a walked / ragged stream can take: its members, under both ways of forcing the walk
EXACT_VARIANTS = [{}, {"p4_wide": 0}, {"p4_wide": 1}, {"p4_wide": 2}, {"p4_direct": 1}, {"min_lnb1": 9, "p4_wide": 2}, {"min_lnb1": 10, "p4_wide": 0},
                  {"min_lnb1": 10, "p4_wide": 2}]


@pytest.mark.parametrize("k", KS)
def test_insert_variants_ragged_host_stream(ctx, k):
    """A host stream of lengths 0, k-1, k, k+1, 255 between long uniform runs through count_reads: as the product cuts it, with
    host_ragged = 1 (every chunk walked) and with part_exact = 1 (P1's histogram, the exact level).  map_cut_chunk makes a
    fixed-stride chunk of the LEADING uniform run only and walks everything behind the first odd record as one ragged chunk, so
    the call's last batch — what the last_* keys describe — is always on the exact level here: the fixed-stride members are held
    to their names on the uniform host stream of test_insert_variants_device_inputs[*-hostG], and here by their results."""
    plain = _Feeder(ctx, k, "ragged")
    walked = _Feeder(ctx, k, "ragged_walked")
    for feed, base, variants in ((plain, {}, VARIANTS), (walked, {"host_ragged": 1}, EXACT_VARIANTS), (plain, {"part_exact": 1}, EXACT_VARIANTS)):
        for v in variants:
            opts = dict(base, **v)
            try:
                _run_states(ctx, feed, opts)
            except Exception as e:
                raise AssertionError(f"variant [{_vid(opts)}] k={k} ragged host stream: {e!r}") from e


# ---------------------------------------------------------------------------------------------------------------------------
# (b) filter variants
# ---------------------------------------------------------------------------------------------------------------------------
def _small_reads(k, seed, n=260):
    rnd = random.Random(seed)
    reads = _reads(rnd, n, k, 700, 0.01, 2)
    return reads, R.reads_to_bin(reads)


def _graph_steps(g, og, k):
    assert g.canonical() == _oracle_graph(og, k)
    g.removeBubbles(); og.remove_bubbles()
    assert g.canonical() == _oracle_graph(og, k)
    g.simplifyGraph(); og.simplify()
    assert g.canonical() == _oracle_graph(og, k)


@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("k", [21, 31, 55, 64])
def test_filter_variants(ctx, k, classic):
    """deleteAll_lt as the streaming rebuild and as tombstones + k_rehash, for every threshold: the table, a further batch on the
    filtered table, and the graph built from it, with the form that ran asserted by name.
    The streaming form needs the old and the new table to have the same L1 fan-out (filter_compact_streaming).  The new table is
    planned for at least 1024 / 0.25 + 1 = 4097 slots and clamped to the old geometry when that is more than the old table has, so
    on a table of at most 4096 slots — checked before every filter — the fan-out provably stays and the route is fixed: streaming,
    unless the switch or k = 64's tagged slots say classic."""
    rnd = random.Random(7 * k)
    reads = _reads(rnd, 40, k, 300, 0.003, 1)
    more = _reads(rnd, 15, k, 300, 0.0, 0) + reads[:5]
    binb, binb2 = R.reads_to_bin(reads), R.reads_to_bin(more)
    want_name = "classic" if classic or k == 64 else "streaming"
    for rounds in (1, 2, 3, 1 << 20):
        ref = O.PMap(k, 1)
        occ = ref.count_reads(binb, len(reads))
        with forced(ctx, filter_classic=classic):
            m = HipDNAMap(ctx, k, 0)
            assert m.count_reads(binb, len(reads)) == occ
            assert m.slots() <= 4096, "the test's own construction: the table must be too small for the filter to shrink it"
            m.deleteAll_lt(rounds); ref.delete_lt(rounds)
            assert m.stats()["last_filter"] == want_name
            assert_same_table(m.sorted_items(), ref.export_sorted())
            assert m.size() == ref.size() and m.verify()[1] == 0
            assert (ref.size() == 0) == (rounds == 1 << 20)
            assert m.count_reads(binb2, len(more)) == ref.count_reads(binb2, len(more))
            assert_same_table(m.sorted_items(), ref.export_sorted())
            g, og = buildGraph(k, m), O.Graph(ref)
            _graph_steps(g, og, k)
            g.close(); m.close()
        og.close(); ref.close()


@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("k", [21, 31, 55, 64])
def test_filter_variants_on_tables_that_shrink(ctx, k, classic):
    """The same on tables of tens of segments, which the filter shrinks: a table whose L1 fan-out changes takes the classic form
    whatever the switch says, so only a forced classic form and k = 64 have a fixed name here; the results are compared alike."""
    reads, binb = _small_reads(k, 7 * k)
    more, binb2 = _small_reads(k, 7 * k + 1, 120)
    for rounds in (1, 2, 3, 1 << 20):
        ref = O.PMap(k, 1)
        occ = ref.count_reads(binb, len(reads))
        with forced(ctx, filter_classic=classic):
            m = HipDNAMap(ctx, k, 0)
            assert m.count_reads(binb, len(reads)) == occ
            m.deleteAll_lt(rounds); ref.delete_lt(rounds)
            got_name = m.stats()["last_filter"]
            assert got_name == "classic" if classic or k == 64 else got_name in ("classic", "streaming")
            assert_same_table(m.sorted_items(), ref.export_sorted())
            assert m.size() == ref.size() and m.verify()[1] == 0
            assert m.count_reads(binb2, len(more)) == ref.count_reads(binb2, len(more))
            assert_same_table(m.sorted_items(), ref.export_sorted())
            g, og = buildGraph(k, m), O.Graph(ref)
            assert g.canonical() == _oracle_graph(og, k)
            g.close(); m.close()
        og.close(); ref.close()


@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("k", [21, 31])
def test_count_slots_widen_to_graph_slots_and_count_again(ctx, k, classic):
    """8-byte keys: count into 12-byte slots, filter (16-byte graph slots), build the graph, count again ON the widened table."""
    reads, binb = _small_reads(k, 11 * k)
    ref = O.PMap(k, 1)
    with forced(ctx, filter_classic=classic):
        m = HipDNAMap(ctx, k, 0)
        m.set_insert_path("partitioned")
        assert m.count_reads(binb, len(reads)) == ref.count_reads(binb, len(reads))
        assert m.stats()["slot_bytes"] == 12
        m.deleteAll_lt(2); ref.delete_lt(2)
        assert m.stats()["slot_bytes"] == 16
        g, og = buildGraph(k, m), O.Graph(ref)
        assert g.canonical() == _oracle_graph(og, k)
        g.close(); og.close()
        assert m.count_reads(binb, len(reads)) == ref.count_reads(binb, len(reads))
        assert m.stats()["slot_bytes"] == 16
        assert_same_table(m.sorted_items(), ref.export_sorted())
        g, og = buildGraph(k, m), O.Graph(ref)
        _graph_steps(g, og, k)
        g.close(); m.close()


@pytest.mark.parametrize("mbt_keys", [16, 100, 256])
@pytest.mark.parametrize("k", [21, 31, 55, 64])
def test_graph_on_the_minimizer_bucketed_table(ctx, k, mbt_keys):
    """graph_mbt = 1: classify and walk on the bucketed copy, whose slot count is no multiple of 64 in general (the terminal
    bitmap then has a last partial word: (slots + 63) / 64 words, gk_graph.hip graph_build_impl)."""
    n, L_ = 2000, 100
    binb = synth.reads_mode_g(n, L_, 20000, 0.01, config_id=400 + k).tobytes()
    partial = []
    for rounds in (2, 3, 4):
        ref = O.PMap(k, 1)
        m = HipDNAMap(ctx, k, 0)
        assert m.count_reads(binb, n) == ref.count_reads(binb, n)
        m.deleteAll_lt(rounds); ref.delete_lt(rounds)
        assert ref.size() >= 4096 or k == 64            # (graph_build_entry: smaller tables are read in place)
        with forced(ctx, graph_mbt=1, graph_mbt_keys=mbt_keys):
            g = buildGraph(k, m)
        og = O.Graph(ref)
        # k = 64's tagged slots are never bucketed (graph_build_entry: `m->k != 64`): asserted as "not built"
        slots = g.buildStats()["bucketed_table"]["slots"]
        assert (slots > 0) == (k != 64), "the bucketed table: built for every k but 64"
        partial.append(slots % 64 != 0)
        _graph_steps(g, og, k)
        g.close(); m.close()
    # regions are powers of two from 8 slots up: with 16 keys per bucket the total is a multiple of 64 only by chance, and one of
    # these tables must end in a partial bitmap word — the case the (slots + 63) / 64 words are for
    if mbt_keys == 16 and k != 64:
        assert any(partial), "no table with slots % 64 != 0: the partial last word of the terminal bitmap did not run"


# ---------------------------------------------------------------------------------------------------------------------------
# (c) load factors
# ---------------------------------------------------------------------------------------------------------------------------
def test_load_options_refuse_what_cannot_work(ctx):
    """A load at or above the growth limit (0.8; 0.6 tagged) is a grow loop or a full segment by construction: refused."""
    for name in ("target_load_pct", "graph_load_pct"):
        for bad in (-2, 1, 9, 76, 80, 95, 100, 1000):
            with pytest.raises(L.GkError) as e:
                ctx.set_option(name, bad)
            assert e.value.code == L.GK_E_INVALID
        for ok in (0, -1, 10, 75):
            with forced(ctx, **{name: ok}):
                pass


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k", [31, 55, 64])
def test_load_factor_variants(ctx, k, path):
    """Tables sized for 30 % / 75 % instead of 65 %, graph tables for 25 / 40 / 60 / 75 %: slots() shows the load changed; the
    table, the graph after build / removeBubbles / simplifyGraph and retainLargest are the oracle's."""
    n, L_ = 3000, 100
    rec = synth.reads_mode_g(n, L_, 30000, 0.01, config_id=300 + k)
    binb = rec.tobytes()
    ref = O.PMap(k, 1)
    occ = ref.count_reads(binb, n)
    want = ref.export_sorted()
    hint = len(want[0])
    ref_top = O.PMap(k, 1)
    ref_top.count_reads(binb, n)
    occ_half = ref_top.count_reads(rec[:n // 2].tobytes(), n // 2)
    want_top = ref_top.export_sorted()
    ref_top.close()
    ref_f = O.PMap(k, 1)
    ref_f.count_reads(binb, n)
    ref_f.delete_lt(2)
    slots = {}
    for pct in (0, 30, 75):
        with forced(ctx, target_load_pct=pct):
            m = HipDNAMap(ctx, k, hint)
            m.set_insert_path(path)
            assert m.count_reads(binb, n) == occ
            assert_same_table(m.sorted_items(), want)
            assert m.count_reads(rec[:n // 2].tobytes(), n // 2) == occ_half       # on top: grows at the forced load
            assert_same_table(m.sorted_items(), want_top)
            m.clear()
            assert m.count_reads(binb, n) == occ
            assert_same_table(m.sorted_items(), want)
            assert m.verify()[1] == 0
            m.deleteAll_lt(2)
            g, og = buildGraph(k, m), O.Graph(ref_f)
            _graph_steps(g, og, k)
            kept, comps = g.retainLargest()
            assert comps == og.num_components() and kept == og.retain_largest()
            assert g.canonical() == _oracle_graph(og, k)
            g.close(); og.close(); m.close()
    ref_f.close()
    # the load itself, on tables of enough segments that the geometry's rounding (whole fine buckets per L1 bucket) does not hide it
    big = 3_000_000
    for pct in (0, 30, 75):
        with forced(ctx, target_load_pct=pct):
            m = HipDNAMap(ctx, k, big)
            slots[pct] = m.slots()
            m.close()
    if k == 64:
        assert slots[30] == slots[0] == slots[75]          # the tagged table's 0.45 comes first (target_load)
    else:
        assert slots[30] > slots[0] > slots[75], slots
        assert big / slots[30] <= 0.30 < big / slots[0] <= 0.65 < big / slots[75] <= 0.75, slots
    ref.delete_lt(2)
    want2 = ref.export_sorted()
    size = len(want2[0])
    gslots = {}
    for pct in (25, 40, 60, 75):
        with forced(ctx, graph_load_pct=pct):
            m = HipDNAMap(ctx, k, occ)
            m.set_insert_path(path)
            assert m.count_reads(binb, n) == occ
            m.deleteAll_lt(2)
            gslots[pct] = m.slots()
            assert_same_table(m.sorted_items(), want2)
            g, og = buildGraph(k, m), O.Graph(ref)
            _graph_steps(g, og, k)
            kept, comps = g.retainLargest()
            assert comps == og.num_components() and kept == og.retain_largest()
            assert g.canonical() == _oracle_graph(og, k)
            g.close(); og.close(); m.close()
    # never denser than asked for (k = 64: capped at the tagged table's densest step), sparser tables for smaller loads; the
    # geometry rounds to whole fine buckets per L1 bucket, so neighbouring loads may share a size: the extremes may not
    eff = {p: (min(p, 45) if k == 64 else p) for p in gslots}
    for p, s_ in gslots.items():
        assert size / s_ <= eff[p] / 100 + 1e-9, (p, size, s_)
    assert gslots[25] >= gslots[40] >= gslots[60] >= gslots[75] and gslots[25] > gslots[75], gslots
    if k == 64:
        assert gslots[60] == gslots[75]


# ---------------------------------------------------------------------------------------------------------------------------
# (d) components
# ---------------------------------------------------------------------------------------------------------------------------
def _component_sizes(og, k):
    """node counts of the weakly connected components of the oracle's graph, by a plain union-find over its edge list"""
    nodes, edges = _oracle_graph(og, k)
    idx = {s: i for i, s in enumerate(nodes)}
    parent = list(range(len(nodes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, _ in edges:
        ra, rb = find(idx[a]), find(idx[b])
        if ra != rb:
            parent[ra] = rb
    sizes = {}
    for i in range(len(nodes)):
        r = find(i)
        sizes[r] = sizes.get(r, 0) + 1
    return sorted(sizes.values())


def _cc_reads(k, shape):
    rnd = random.Random(k * 31 + len(shape))
    seq = lambda n: "".join(rnd.choice("AGCT") for _ in range(n))

    def tiled(s, ln, step):
        return [s[i:i + ln] for i in range(0, len(s) - ln + 1, step)]
    if shape == "equal":            # many components of exactly the same shape and size: the tie rule picks the one to keep
        out = []
        for _ in range(24):
            s = seq(3 * k)
            fork = s[:2 * k] + seq(k)                     # one branch each: four terminal k-mers per component and strand
            out += [s, fork]
        return out
    if shape == "path":             # one long path with SNP bubbles along it: deep union-find trees
        s = seq(6000)
        alt = list(s)
        for i in range(100, 5900, 150):
            alt[i] = "A" if alt[i] != "A" else "C"
        return tiled(s, 200, 50) + tiled("".join(alt), 200, 50)
    if shape == "cycle":            # a perfect cycle (no terminal k-mer at all) beside a small forked component
        c = seq(500)
        s = seq(3 * k)
        return tiled(c + c[:250], 200, 25) + [s, s[:2 * k] + seq(k)]
    # singletons: isolated k-mers that survive the filter, beside branching components that lose their thin arms to it
    out = []
    for _ in range(30):
        out += [seq(k)] * 2
    for _ in range(10):
        s = seq(4 * k)
        out += [s, s, s[:2 * k] + seq(k), s[:2 * k] + seq(k), s[:k + 3] + seq(k)]
    return out


@pytest.mark.parametrize("find", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", ["equal", "path", "cycle", "singletons"])
@pytest.mark.parametrize("k", [15, 31, 47])
def test_component_link_variants(ctx, k, shape, find):
    """cc_find 0 / 1 / 2 / 3 (k_cc_link's four ways of shortening paths): the number of components, their sizes and the graph
    after retainLargest are the oracle's.  The switch has no echo: the forms write different parent pointers and must give the
    same partition, so the comparison is the check."""
    reads = _cc_reads(k, shape)
    binb = dna.reads_to_bin(reads)
    rounds = 2 if shape == "singletons" else 1
    ref = O.PMap(k, 1)
    m = HipDNAMap(ctx, k, 0)
    assert m.count_reads(binb, len(reads)) == ref.count_reads(binb, len(reads))
    m.deleteAll_lt(rounds); ref.delete_lt(rounds)
    g, og = buildGraph(k, m), O.Graph(ref)
    assert g.canonical() == _oracle_graph(og, k)
    want_sizes = _component_sizes(og, k)
    assert len(want_sizes) == og.num_components()
    with forced(ctx, cc_find=find):
        nodes_pc, _ = g.componentStats()
        assert sorted(int(x) for x in nodes_pc) == want_sizes
        kept, comps = g.retainLargest()
    assert comps == og.num_components() == len(want_sizes)
    assert kept == og.retain_largest() == (want_sizes[-1] if want_sizes else 0)
    assert g.canonical() == _oracle_graph(og, k)
    assert g.counts()[0] == kept
    g.close(); m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) switches drawn at random beside the input
# ---------------------------------------------------------------------------------------------------------------------------
def _switch(values):
    """the default with probability about one half"""
    return st.one_of(st.none(), st.sampled_from(values))


SWITCHES = st.fixed_dictionaries({
    "p4_wide": _switch([0, 1, 2]), "fine_exact": _switch([0, 1]), "p4_direct": _switch([1]), "p2_sorted": _switch([0, 1]), "p2_wide": _switch([1]),
    "p45_stripes": _switch([2, 4, 16]), "p4_grid": _switch([1, 8]), "p24_pieces": _switch([8]), "min_lnb1": _switch([9, 10]),
    "part_exact": _switch([1]), "host_ragged": _switch([1]), "filter_classic": _switch([0, 1]), "cc_find": _switch([0, 1, 2]),
    "target_load_pct": _switch([30, 75]), "graph_load_pct": _switch([25, 40, 60, 75]), "graph_mbt": _switch([1]), "graph_mbt_keys": _switch([16, 100])})


@settings(max_examples=int(os.environ.get("GK_FUZZ_EXAMPLES", "60")), deadline=None, derandomize="GK_FUZZ_EXAMPLES" not in os.environ,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.function_scoped_fixture])
@given(seed=st.integers(0, 10**6), k=st.sampled_from([9, 21, 31, 34, 35, 55, 63, 64]), path=st.sampled_from(["auto", "partitioned"]),
       batches=st.integers(1, 3), rounds=st.integers(1, 3), hint=st.sampled_from([0, 64, 20000, 3_000_000]), switches=SWITCHES)
def test_random_switch_assignments_match_the_oracle(ctx, seed, k, path, batches, rounds, hint, switches):
    """count -> filter -> count -> graph -> bubbles -> simplify -> retain under a random assignment of the switches above (each
    at its default about half the time), input drawn as tests/test_fuzz_gpu.py draws it."""
    opts = {n: v for n, v in switches.items() if v is not None}
    rnd = random.Random(seed)
    glen = rnd.randint(max(k + 5, 40), 400)
    reads = _reads(rnd, rnd.randint(1, 160), k, glen, 0.01, 1)
    cut = sorted(rnd.randrange(len(reads) + 1) for _ in range(batches - 1))
    parts = [reads[a:b] for a, b in zip([0] + cut, cut + [len(reads)])]
    ref = O.PMap(k, 1)
    with forced(ctx, **opts):
        m = HipDNAMap(ctx, k, hint)
        m.set_insert_path(path)
        for p in parts:
            b = R.reads_to_bin(p)
            assert m.count_reads(b, len(p)) == ref.count_reads(b, len(p))
        assert_same_table(m.sorted_items(), ref.export_sorted())
        m.deleteAll_lt(rounds); ref.delete_lt(rounds)
        assert_same_table(m.sorted_items(), ref.export_sorted())
        b = R.reads_to_bin(parts[0])
        assert m.count_reads(b, len(parts[0])) == ref.count_reads(b, len(parts[0]))
        assert_same_table(m.sorted_items(), ref.export_sorted())
        assert m.verify()[1] == 0
        g, og = buildGraph(k, m), O.Graph(ref)
        _graph_steps(g, og, k)
        kept, comps = g.retainLargest()
        assert comps == og.num_components() and kept == og.retain_largest()
        assert g.canonical() == _oracle_graph(og, k)
        g.close(); m.close()
