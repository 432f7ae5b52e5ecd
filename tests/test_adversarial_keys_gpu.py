"""Tables filled with keys that share a stored word and a home slot (-m gpu).

Every slot layout but the 16-byte one stores a key as two separately claimed words (gk_device.h: CSlot, Slot<2>, and for k = 64
the tag in the slot address), and the claim protocol — claim w0, then w1; the loser of w1 moves on; a lookup walks past a slot
whose w0 matches and whose w1 does not — only ever matters for keys of ONE probe chain with ONE first word.  Random genomes
never produce those.  tests/slot_ref.py constructs them: groups of keys with one first stored word and one start position, one
group at the last position of a segment (the chain wraps), two groups whose chains run into each other, and per group 16
siblings of the same kind that are never inserted and must never be found.

Expected answers are a Python Counter and oracle.PMap, never a second device run.  Every test asserts that it IS adversarial
in the table as it stands: with S slots per segment, every group holds at least 8 * slots / S keys, so by pigeonhole at least
8 keys of every group share first word, start position AND segment whatever the geometry (`_adversarial`).
"""
from collections import Counter

import numpy as np
import pytest

import slot_ref as SR
from genome_amd import dna
from genome_amd.dist import DistDNAMap, HipDist, unique_id
from genome_amd.dnamap import Context, HipDNAMap, HipValueMap
from genome_amd.partitioned import PartitionedDNAMap, owner_of
from oracle import oracle as O
from spectrum_ref import spectrum_of
from test_variants_gpu import EXACT_VARIANTS, VARIANTS, forced

pytestmark = pytest.mark.gpu

CASES = [(k, name) for name in ("count12", "slot24", "tagged", "slot16") for k in SR.KS[name]]
IDS = [f"{name}-k{k}" for k, name in CASES]
SLOT_BYTES = {"count12": 12, "slot16": 16, "slot24": 24, "tagged": 24}
SLOT_NAME = {"count12": "count12", "slot16": "slot16", "slot24": "slot24", "tagged": "slot24"}
# groups x keys (the issue's sizes), and a capacity hint under which two batches of these keys, each up to 9 times, never make
# the table grow: 4 segments of 8-byte keys (need 32 <= 64), 4 of 16-byte keys (32 <= 32), 2 tagged (16 <= 16)
SHAPE = {1: (8, 64), 2: (8, 32), 64: (8, 16)}
ROOMY = {1: 5000, 2: 2600, 64: 900}
_FOUND = {}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _w(k):
    return 64 if k == 64 else SR.words_for_k(k)


def _groups(k, canonical_only=False, size=None, extra_groups=1):
    """the groups of a case, found once: SHAPE[k] groups, and `extra_groups` more for batches that bring fresh keys"""
    n, sz = SHAPE[_w(k)]
    key = (k, canonical_only, size or sz, extra_groups)
    if key not in _FOUND:
        _FOUND[key] = SR.find_groups(k, n + extra_groups, size or sz, canonical_only, seed=11)
    return _FOUND[key]


def _new_map(ctx, k, layout, hint, path=None):
    """an empty table of the layout the case is named for.  slot16 = what deleteAll_lt leaves of a count table: one throw-away
    key counted once and filtered away (the filter widens the 12-byte slots whatever route it takes).  The filter also sizes the
    table for its survivors -- none: one segment -- so where a test wants room (hint > 1000) the 16-byte table comes from
    gk_map_create_for_graph instead, the same slot type at the same number of slots as the count table of that hint."""
    if layout == "slot16" and hint > 1000:
        m = HipDNAMap(ctx, k, int(hint / 0.65 * 0.25), for_graph=True)
        assert m.stats()["slot_bytes"] == 16
    else:
        m = HipDNAMap(ctx, k, hint)
        if layout == "slot16":
            m.update_inc((np.array([5], np.uint64), np.zeros(1, np.uint64)))
            m.deleteAll_lt(2)
            assert m.size() == 0 and m.stats()["slot_bytes"] == 16
    if path:
        m.set_insert_path(path)
    return m


def _adversarial(slots, k, group_sizes):
    """the precondition: every group holds at least 8 * slots / S live keys"""
    S = SR.seg_slots(k)
    assert slots % S == 0
    need = 8 * slots // S
    assert min(group_sizes) >= need, f"not adversarial: {slots} slots = {slots // S} segments need {need} keys per group, the smallest has {min(group_sizes)}"


def _live_per_group(groups, cnt):
    return [sum(1 for kk in g.keys if cnt.get(kk, 0) > 0) for g in groups if any(cnt.get(kk, 0) > 0 for kk in g.keys)]


def _sorted_table(cnt):
    items = sorted(((hi, lo, c) for (lo, hi), c in cnt.items() if c > 0))
    return (np.array([a for _, a, _ in items], np.uint64), np.array([b for b, _, _ in items], np.uint64),
            np.array([c for _, _, c in items], np.int32))


def _check(m, k, layout, cnt, absent, groups, adversarial=True):
    """the table is the Counter: serialisation, invariants, point lookups of every key and of every key that must be absent"""
    cnt = Counter({kk: c for kk, c in cnt.items() if c > 0})
    got, want = m.sorted_items(), _sorted_table(cnt)
    for name, a, b in zip(("lo", "hi", "count"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), name
    live, bad, total = m.verify()
    assert bad == 0 and live == len(cnt) == m.size() and total == sum(cnt.values())
    keys = list(cnt)
    if keys:
        assert m.apply_batch(SR.arrays(keys)).tolist() == [cnt[kk] for kk in keys]
    if absent:
        assert (m.apply_batch(SR.arrays(absent)) == -1).all()
    st = m.stats()
    assert st["slot_bytes"] == SLOT_BYTES[layout]
    if adversarial:
        _adversarial(st["slots"], k, _live_per_group(groups, cnt))
    return st


def _reads_of(k, keys):
    """one read of exactly k bases per key, as a `.bin` stream (fixed stride 1 + ceil(k / 4))"""
    return dna.reads_to_bin([dna.unpack(lo, hi, k) for lo, hi in keys])


def _dev_keys(k, keys):
    lo, hi = SR.arrays(keys)
    return lo if SR.words_for_k(k) == 1 else np.stack([lo, hi], axis=1).reshape(-1)


class _Feed:
    """how a batch of keys (with repeats) reaches the map: 'keys' = key arrays, 'reads' = reads of k bases; host or device"""

    def __init__(self, ctx, k, kind):
        self.ctx, self.k, self.kind = ctx, k, kind

    def put(self, m, keys, dev):
        ctx, k = self.ctx, self.k
        if self.kind == "keys" and not dev:
            m.update_inc(SR.arrays(keys))
            return
        buf = _dev_keys(k, keys).view(np.uint8) if self.kind == "keys" else np.frombuffer(_reads_of(k, keys), np.uint8)
        if self.kind == "reads" and not dev:
            assert m.count_reads(buf, len(keys)) == len(keys)
            return
        d = ctx.alloc(buf.size + 64)
        try:
            ctx.upload(d, buf)
            if self.kind == "keys":
                m.update_inc_dev(d, len(keys))
            else:
                assert m.count_reads_dev(d, len(keys), k) == len(keys)
        finally:
            ctx.free(d)


def _batch(keys, seed):
    """every key r times, r drawn from 1..9 per key, shuffled: lanes race for the same slots"""
    rng = np.random.default_rng(seed)
    reps = rng.integers(1, 10, len(keys))
    out = [kk for kk, r in zip(keys, reps) for _ in range(int(r))]
    return [out[i] for i in rng.permutation(len(out))]


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the restatement is the device's
# ---------------------------------------------------------------------------------------------------------------------------
def _export(m):
    lo, hi, _ = m.items()
    return list(zip(lo.tolist(), hi.tolist()))


def _one_by_one(ctx, k, layout, keys):
    m = _new_map(ctx, k, layout, 64)
    assert m.stats()["slots"] == SR.seg_slots(k)
    for kk in keys:
        m.update_inc(SR.arrays([kk]))
    st = m.stats()
    assert st["slots"] == SR.seg_slots(k) and st["grows"] == 0 and st["slot_bytes"] == SLOT_BYTES[layout]
    out = _export(m)
    assert m.verify()[:2] == (len(keys), 0)
    m.close()
    return out


@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_start_position_chain_order_and_wrap_are_the_restated_ones(ctx, k, layout):
    """One segment, one key per batch; gk_map_export gives live keys in ascending slot index.  A group away from the segment's
    end comes out in insertion order (one chain, one start); the group at the LAST start position comes out with its first key
    last (the chain wraps to slot 0, or to the tag's slot of the first 4-slot group); three keys with distinct restated starts,
    inserted in descending order, come out ascending.  This pins seg_pos, the tagged start and the wrap without a hook."""
    G = _groups(k)
    n, sz = SHAPE[_w(k)]
    _adversarial(SR.seg_slots(k), k, [sz])
    inner = G.groups[3]
    assert inner.start + 4 * sz < G.S
    assert _one_by_one(ctx, k, layout, inner.keys) == inner.keys
    last = G.groups[0]
    assert last.start // (4 if k == 64 else 1) == (G.S // 4 if k == 64 else G.S) - 1
    assert _one_by_one(ctx, k, layout, last.keys) == last.keys[1:] + last.keys[:1]
    three = sorted((G.groups[i] for i in (3, 4, 6)), key=lambda g: -g.start)
    assert len({g.start for g in three}) == 3
    assert _one_by_one(ctx, k, layout, [g.keys[0] for g in three]) == [g.keys[0] for g in reversed(three)]
    # the two chains that run into each other, interleaved key by key: still every key once, in a slot its chain reaches
    a, b = (G.groups[1], G.groups[5]) if k == 64 else (G.groups[1], G.groups[2])
    mixed = [kk for pair in zip(a.keys, b.keys) for kk in pair]
    assert sorted(_one_by_one(ctx, k, layout, mixed)) == sorted(mixed)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) racing claims, every insert route; (g) the readers that sit on the table
# ---------------------------------------------------------------------------------------------------------------------------
def _two_batches(ctx, k, layout, path, kind, seed=3):
    """a shuffled batch with every key 1..9 times into the empty table, then the same keys and a fresh group on top"""
    canonical = kind == "reads"
    G = _groups(k, canonical)
    n, _ = SHAPE[_w(k)]
    first, fresh = G.groups[:n], G.groups[n:]
    absent = G.siblings()
    feed = _Feed(ctx, k, kind)
    m = _new_map(ctx, k, layout, ROOMY[_w(k)], path)
    ref = O.PMap(k, 1) if canonical else None
    cnt = Counter()
    st0 = m.stats()
    for step, groups in enumerate((first, first + fresh)):
        keys = [kk for g in groups for kk in g.keys]
        batch = _batch(keys, seed + step)
        # direct: host arrays first, device arrays on top; partitioned: device arrays (host key arrays have no partitioned form),
        # reads from host memory first (the ragged walk), device records on top
        feed.put(m, batch, dev=(step == 1) if (path == "direct" or kind == "reads") else True)
        cnt.update(batch)
        st = _check(m, k, layout, cnt, absent + ([kk for g in fresh for kk in g.keys] if step == 0 else []), G.groups)
        if ref is not None:
            b = _reads_of(k, batch)
            assert ref.count_reads(b, len(batch)) == len(batch)
            for x, y in zip(m.sorted_items(), ref.export_sorted()):
                assert np.array_equal(x, y)
        # the route is the one asked for: no quiet fall-back to the direct path (these batches are far below the spill list's
        # capacity), the segments built in the named slot type, and the table never grown (ROOMY)
        assert st["grows"] == 0 and st["retries_direct"] == 0
        if path == "partitioned":
            assert st["partitioned_launches"] > st0["partitioned_launches"] and st["direct_launches"] == 0, st
            assert st["last_slot"] == SLOT_NAME[layout]
        else:
            assert st["partitioned_launches"] == 0
        st0 = st
    return m, cnt


@pytest.mark.parametrize("kind", ["keys", "reads"])
@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_racing_claims_on_every_insert_route(ctx, k, layout, path, kind):
    """update_inc / update_inc_dev of key arrays and count_reads / count_reads_dev of k-base reads holding canonical keys, on the
    direct and on the partitioned path: after each of two batches the table is the Counter (and the oracle's, for reads), every
    key has its exact count, no sibling is found.  Then the readers: export is the Counter, the spectrum is the reference's."""
    m, cnt = _two_batches(ctx, k, layout, path, kind)
    lo, hi, c = m.items()
    assert Counter(dict(zip(zip(lo.tolist(), hi.tolist()), c.tolist()))) == cnt and len(lo) == len(cnt)
    for bins in (4, 16):
        sp = m.spectrum(bins)
        assert np.array_equal(sp["hist"], spectrum_of(list(cnt.values()), bins))
        assert (sp["distinct"], sp["occurrences"], sp["max_count"]) == (len(cnt), sum(cnt.values()), max(cnt.values()))
    m.close()


@pytest.mark.parametrize("kind", ["keys", "reads"])
@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_racing_claims_under_every_partitioned_variant(ctx, k, layout, kind):
    """The same two batches under each switchable member of the P2 / P4 / P5 families (tests/test_variants_gpu.py's lists), and
    the exact-level members also with every chunk walked (host_ragged) and behind P1's histogram (part_exact)."""
    runs = [v for v in VARIANTS] + [dict(base, **v) for base in ({"host_ragged": 1}, {"part_exact": 1}) for v in EXACT_VARIANTS]
    for opts in runs:
        try:
            with forced(ctx, **opts):
                m, _ = _two_batches(ctx, k, layout, "partitioned", kind)
                m.close()
        except Exception as e:
            raise AssertionError(f"variant {opts} k={k} {layout} input={kind}: {e!r}") from e


# ---------------------------------------------------------------------------------------------------------------------------
# (c) filter, then reuse
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_filter_between_survivors_that_share_a_word_then_reuse(ctx, k, layout, classic):
    """Counts 1, 2, 3, 1, 2, 3, ... along every chain (the keys go in index by index, so chain order is index order): what
    deleteAll_lt(2) and then deleteAll_lt(3) delete sits between survivors with the same first word.  Streaming rebuild
    (k_compact_seg) and tombstones + k_rehash, by name; then a batch that brings deleted keys back and repeats survivors."""
    G = _groups(k)
    n, sz = SHAPE[_w(k)]
    groups = G.groups[:n]
    absent = G.siblings() + G.groups[n].keys
    want_name = "classic" if classic or k == 64 else "streaming"
    with forced(ctx, filter_classic=classic):
        m = _new_map(ctx, k, layout, {1: 600, 2: 300, 64: 200}[_w(k)])
        cnt = Counter()
        for i in range(sz):
            col = [g.keys[i] for g in groups]
            m.update_inc(SR.arrays(col))
            cnt.update(col)
        extra = [(g.keys[i], i % 3) for g in groups for i in range(sz) if i % 3]
        lo, hi = SR.arrays([kk for kk, _ in extra])
        m.add_counts(lo, hi, [c for _, c in extra])
        for kk, c in extra:
            cnt[kk] += c
        assert sorted(Counter(cnt.values()).items()) == [(1, n * len(range(0, sz, 3))), (2, n * len(range(1, sz, 3))), (3, n * len(range(2, sz, 3)))]
        _check(m, k, layout, cnt, absent, groups)
        for rounds in (2, 3):
            assert m.stats()["slots"] <= 4096          # (the route is then fixed: tests/test_variants_gpu.py test_filter_variants)
            m.deleteAll_lt(rounds)
            assert m.stats()["last_filter"] == want_name
            deleted = [kk for kk, c in cnt.items() if c < rounds]
            assert deleted
            cnt = Counter({kk: c for kk, c in cnt.items() if c >= rounds})
            after = "slot16" if layout == "count12" else layout            # the filter widens count slots
            if rounds == 2:
                _check(m, k, after, cnt, absent + deleted, groups)
            else:       # (a third of every group is left: the comparison is complete, the precondition is the table before this filter)
                for a, b in zip(m.sorted_items(), _sorted_table(cnt)):
                    assert np.array_equal(a, b)
                assert m.verify() == (len(cnt), 0, sum(cnt.values()))
                assert (m.apply_batch(SR.arrays(absent + deleted)) == -1).all()
                assert m.apply_batch(SR.arrays(list(cnt))).tolist() == list(cnt.values())
        # deleted keys come back (even indices 0, 4, 6, 10, ...), survivors repeat (2, 8, 14, ...)
        again = [g.keys[i] for g in groups for i in range(0, sz, 2)]
        assert any(kk in cnt for kk in again) and any(kk not in cnt for kk in again)
        m.update_inc(SR.arrays(again))
        cnt.update(again)
        _check(m, k, after, cnt, absent, groups)
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) growth
# ---------------------------------------------------------------------------------------------------------------------------
GROW = {1: 384, 2: 192, 64: 112}       # keys per group: the third of four batches passes the growth limit of one segment


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_growth_moves_every_key_once(ctx, k, layout, path):
    """From a hint of 64 (one segment) in four batches: the table grows with the chains in it and ends as the Counter.  The
    precondition is asserted on the table every growth MOVES (what k_rehash / the streaming rebuild read), and on the direct path
    on the final table too.  Not on the partitioned path's final table: a batch that does not fit a table of fewer than 256
    segments makes that path grow it to 512 segments at once (gk_table.hip insert_batch: the L1 bucket of a key must survive a
    mid-batch growth), where a group would need 4096 keys — more than k = 27 has per start position."""
    G = _groups(k, size=GROW[_w(k)], extra_groups=0)
    keys = G.keys()
    rng = np.random.default_rng(k)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    feed = _Feed(ctx, k, "keys")
    m = _new_map(ctx, k, layout, 64, path)
    st = m.stats()
    assert st["slots"] == G.S
    cnt = Counter()
    q = len(keys) // 4
    for b in range(4):
        part = keys[b * q:(b + 1) * q] + keys[:q // 4]         # (and some keys of the first batch again)
        before = (st["slots"], st["grows"], _live_per_group(G.groups, cnt))
        feed.put(m, part, dev=path == "partitioned" or b % 2 == 1)
        cnt.update(part)
        for a, c in zip(m.sorted_items(), _sorted_table(cnt)):
            assert np.array_equal(a, c)
        st = m.stats()
        if st["grows"] > before[1] and before[2]:
            _adversarial(before[0], k, before[2])
    st = _check(m, k, layout, cnt, G.siblings(), G.groups, adversarial=path == "direct")
    assert st["grows"] >= 1 and st["slots"] > G.S
    m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) merges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,layout", CASES, ids=IDS)
def test_add_map_adds_the_counts_of_shared_groups(ctx, k, layout):
    """gk_map_add_map of two maps that share whole groups into a third, empty one and into one that holds them already"""
    G = _groups(k)
    n, _ = SHAPE[_w(k)]
    parts = (G.groups[:n - 2], G.groups[2:n])
    maps, cnts = [], []
    for i, gs in enumerate(parts):
        m = _new_map(ctx, k, layout, ROOMY[_w(k)])
        batch = _batch([kk for g in gs for kk in g.keys], 20 + i)
        m.update_inc(SR.arrays(batch))
        maps.append(m); cnts.append(Counter(batch))
    absent = G.siblings() + G.groups[n].keys
    for i, m in enumerate(maps):
        _check(m, k, layout, cnts[i], absent, G.groups)
    total = cnts[0] + cnts[1]
    into = _new_map(ctx, k, layout, ROOMY[_w(k)])
    into.add_map(maps[0]); into.add_map(maps[1])
    _check(into, k, layout, total, absent, G.groups)
    maps[0].add_map(maps[1])
    _check(maps[0], k, layout, total, absent, G.groups)
    _check(maps[1], k, layout, cnts[1], absent, G.groups)             # the source is unchanged
    for m in maps + [into]:
        m.close()


MERGE = {1: 64, 2: 32, 64: 32}          # keys per group: the largest of three partitions' shares of a group is then >= 8


@pytest.mark.parametrize("k", [27, 31, 47, 63, 64])
def test_partitions_and_their_merge_into_a_graph_table(ctx, k):
    """PartitionedDNAMap(ctx, k, 3) fed k-base reads of canonical keys; its partitions merged into a gk_map_create_for_graph
    table (gk_map_add_map); and the gather of a one-rank DistDNAMap (k_add_unique: claims without a count atomic)."""
    n, _ = SHAPE[_w(k)]
    G = _groups(k, True, size=MERGE[_w(k)])
    groups = G.groups[:n]
    rng = np.random.default_rng(k)
    keys = [kk for g in groups for kk in g.keys]
    batch = [kk for kk in keys for _ in range(int(rng.integers(1, 4)))]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    cnt = Counter(batch)
    absent = G.siblings() + G.groups[n].keys
    binb = _reads_of(k, batch)
    ref = O.PMap(k, 3)
    assert ref.count_reads(binb, len(batch)) == len(batch)
    pm = PartitionedDNAMap(ctx, k, 3)
    assert pm.count_reads(binb, len(batch)) == len(batch)
    for a, b, c in zip(pm.sorted_items(), _sorted_table(cnt), ref.export_sorted()):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    live, bad, total, _ = pm.verify()
    assert (live, bad, total) == (len(cnt), 0, len(batch)) and pm.foreign_keys() == 0
    assert (pm.apply_batch(SR.arrays(absent)) == -1).all()
    assert pm.apply_batch(SR.arrays(keys)).tolist() == [cnt[kk] for kk in keys]
    # adversarial inside a partition: every group has a partition holding 8 * (its slots / S) of its keys
    own = {kk: owner_of(k, kk[0], kk[1], 3) for kk in keys}
    for g in groups:
        assert any(sum(1 for kk in g.keys if own[kk] == p) >= 8 * pm.parts[p].stats()["slots"] // G.S for p in range(3)), g.start
    merged = pm.merged()
    _check(merged, k, "slot16" if k <= 31 else "slot24", cnt, absent, groups)
    merged.close(); pm.close(); ref.close()
    # one rank's gather
    dctx = Context(0)
    hd = HipDist(dctx, 0, 1, unique_id())
    dm = DistDNAMap(hd, k, len(cnt))
    dm.local.update_inc(SR.arrays(batch))
    full = dm.gathered()
    _check(full, k, "slot16" if k <= 31 else "slot24", cnt, absent, groups)
    assert full.verify_checksum() == dm.local.verify_checksum()
    full.close(); dm.close(); hd.close(); dctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# (f) the multimap
# ---------------------------------------------------------------------------------------------------------------------------
def _plan_slots(k, want_slots):
    """gk_internal.h plan_segments for small tables (no forced fan-out): the slots a table of at least want_slots gets"""
    S = SR.seg_slots(k)
    want_seg = max(1, -(-want_slots // S))
    l = 0
    while l < 8 and (2 << l) <= want_seg:
        l += 1
    return (-(-want_seg // (1 << l)) << l) * S


def _vmap_slots(k, batches):
    """gk_vmap.hip's sizing replayed: created for max(hint, 1024) entries at its target load, grown before a batch that would pass
    its limit (0.7, sized for 0.5; tagged 0.5, sized for 0.35) -> the slots after the batches.  A value map has no stats call, so
    this follows gk_vmap_create / vm_reserve by hand: a change of their sizing rule must be made here too (noted beside vm_reserve)."""
    limit, target = (0.5, 0.35) if k == 64 else (0.7, 0.5)
    cap, size = _plan_slots(k, int(1024 / target) + 1), 0
    for n in batches:
        if size + n > limit * cap:
            cap = _plan_slots(k, max(int((size + n) / target) + 1, cap + cap // 2))
        size += n
    return cap


VMAP = {False: {1: 64, 2: 32, 64: 32}, True: {1: 256, 2: 128, 64: 128}}       # keys per group: without and with growth


@pytest.mark.parametrize("grow", [False, True], ids=["fits", "grows"])
@pytest.mark.parametrize("k", [31, 47, 63, 64])
def test_multimap_keeps_every_keys_own_values(ctx, k, grow):
    """HipValueMap.putNew of the groups, every key 1..3 times (the value says which key and which copy): getAll returns exactly
    the key's own values, a sibling has none, size() is the number of entries; once more in batches that make the table grow."""
    n, _ = SHAPE[_w(k)]
    G = _groups(k, size=VMAP[grow][_w(k)])
    groups = G.groups[:n]
    keys = [kk for g in groups for kk in g.keys]
    rng = np.random.default_rng(k + grow)
    entries = [(i, c) for i in range(len(keys)) for c in range(3 if grow else int(rng.integers(1, 4)))]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    nb = 4 if grow else 1
    cuts = [len(entries) * b // nb for b in range(nb + 1)]
    vm = HipValueMap(ctx, k, 16)
    for a, b in zip(cuts, cuts[1:]):
        part = entries[a:b]
        vm.putNew_batch(SR.arrays([keys[i] for i, _ in part]), np.array([i * 4 + c for i, c in part], np.uint64))
    slots = _vmap_slots(k, [b - a for a, b in zip(cuts, cuts[1:])])
    assert (slots > _vmap_slots(k, [])) == grow
    _adversarial(slots, k, [len(g.keys) for g in groups])
    assert vm.size() == len(entries)
    want = {}
    for i, c in entries:
        want.setdefault(i, set()).add(i * 4 + c)
    got = vm.getAll_batch(SR.arrays(keys))
    for i, g in enumerate(got):
        assert len(g) == len(want[i]) and set(int(x) for x in g) == want[i], i
    v, f = vm.apply_batch(SR.arrays(keys))
    assert f.all() and all(int(x) in want[i] for i, x in enumerate(v))
    absent = G.siblings() + G.groups[n].keys
    assert not vm.apply_batch(SR.arrays(absent))[1].any()
    assert all(len(g) == 0 for g in vm.getAll_batch(SR.arrays(absent)))
    lo, hi, val = vm.items()
    assert sorted(zip(lo.tolist(), hi.tolist(), val.tolist())) == sorted((*keys[i], i * 4 + c) for i, c in entries)
    vm.close()
