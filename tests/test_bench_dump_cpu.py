"""bench.py --dump-outputs (bench.dump_outputs) without a GPU: a stand-in map with the same export interface.  The files must not
depend on the table's slot order (two builds lay the table out differently), must be float64, must hold genuine stored keys
with their counts, and must stay under DUMP_MAX_BYTES."""
import os

import numpy as np

import bench


class _FakeMap:
    def __init__(self, lo, hi, cnt, perm):
        self.lo, self.hi, self.cnt, self.perm = lo, hi, cnt, perm

    def verify_checksum(self):
        return len(self.lo), 0, int(self.cnt.sum()), 0xFEEDFACE12345678

    def items(self):
        return self.lo[self.perm], self.hi[self.perm], self.cnt[self.perm]

    def size(self):
        return len(self.lo)


def _table(n=400_000, seed=3):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    hi = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    cnt = rng.integers(1, 50, n).astype(np.int32)
    return lo, hi, cnt, rng


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_layout_independent_float64_and_genuine(tmp_path):
    lo, hi, cnt, rng = _table()
    bench.dump_outputs(str(tmp_path / "a"), _FakeMap(lo, hi, cnt, np.arange(len(lo))), 123, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), _FakeMap(lo, hi, cnt, rng.permutation(len(lo))), 123, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["count_sum", "distinct_kmers", "occurrences", "sample_counts", "sample_keys", "table_checksum"]
    for name in a:
        assert a[name].dtype == np.float64, name
        assert np.array_equal(a[name], b[name]), name
    assert a["occurrences"].tolist() == [123] and a["distinct_kmers"].tolist() == [len(lo)]
    assert a["count_sum"].tolist() == [float(cnt.sum())]
    assert a["table_checksum"].tolist() == [0x12345678, 0xFEEDFACE]
    keys = a["sample_keys"].astype(np.uint64)
    n = len(keys)
    assert len(lo) / 128 * 0.8 < n < len(lo) / 128 * 1.2           # about 1 in 128
    klo = keys[:, 0] | (keys[:, 1] << np.uint64(32))
    khi = keys[:, 2] | (keys[:, 3] << np.uint64(32))
    assert np.all(np.diff(np.lexsort((klo, khi))) == 1)             # sorted by (hi, lo)
    where = {(int(x), int(y)): int(c) for x, y, c in zip(lo, hi, cnt)}
    assert all(where[(int(x), int(y))] == c for x, y, c in zip(klo, khi, a["sample_counts"].astype(np.int64)))


def test_dump_respects_the_size_cap(tmp_path, monkeypatch):
    lo, hi, cnt, _ = _table()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    bench.dump_outputs(str(tmp_path), _FakeMap(lo, hi, cnt, np.arange(len(lo))), 1, 0, 1)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 10
    assert 0 < len(np.load(tmp_path / "sample_counts.npy")) < len(lo) / 128
