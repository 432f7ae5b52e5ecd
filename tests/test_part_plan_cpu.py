"""The partitioned insert's choices on the CPU: gk_test_part_plan (the test build's echo of gk_partition.hip part_choose, the
function part_run takes every choice from) against literals worked out by hand from the rules as they stood before part_choose
existed.  No device.

The rules of P4's family need tables no test can build (256 / 512 / 1024 fine buckets per L1 bucket, LDS fits beside 256 / 512 /
1024-bucket L1 tables); here they are a function of three integers.  A form fits when
    16 nb2 + 8 W threads kpt + 4 threads / 64 + 2 threads kpt + 16      (ScatterLds::bytes)
  + 8 (4 nb1 + 1)                                                       (part_tables_bytes)
is at most 160 KiB = 163840.  With 8-byte keys that is 16 nb2 + 41008 (512 x 8), 82000 (1024 x 8), 122960 (1024 x 12); with
16-byte keys 16 nb2 + 73776 (512 x 8), 110672 (1024 x 6); the tables are 8200 bytes at lnb1 = 8 and 32776 at lnb1 = 10.
"""
import ctypes as C

import pytest

from genome_amd import _lib as L

LDS_PER_CU = 160 << 10
DEVICE, HOST, PREFETCHED, RAGGED, KEYS = range(5)
FORMS = {"sort4096": (512, 4096), "sort8192": (1024, 8192), "sort12288": (1024, 12288), "sort6144": (1024, 6144), "direct": (512, 4096)}


class In(C.Structure):
    _fields_ = [(n, C.c_uint32 if n == "nb2" else C.c_int32) for n in
                ("W", "lnb1", "nb2", "source", "max_windows", "from_empty", "estimate", "fine_exact", "verify_uniform", "part_exact",
                 "p4_wide", "p4_direct", "p2_wide", "p2_sorted", "p45_stripes", "p24_pieces", "p4_grid", "test_max_nb2")]


class Form(C.Structure):
    _fields_ = [("name", C.c_char * 16), ("chunk_keys", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint64)]


class Out(C.Structure):
    _fields_ = [("p4_op", Form), ("p4_exact", Form), ("p2", C.c_char * 16)] + \
               [(n, C.c_int32) for n in ("supported", "op1", "fine_exact", "sync_between", "pipelined", "stripes")]


def plan(W=1, lnb1=8, nb2=370, source=DEVICE, max_windows=120, from_empty=1, **kw):
    """every switch at its default (-1; 0 for the test switches) unless named"""
    v = dict(W=W, lnb1=lnb1, nb2=nb2, source=source, max_windows=max_windows, from_empty=from_empty, estimate=0, fine_exact=0,
             verify_uniform=0, part_exact=0, p4_wide=-1, p4_direct=-1, p2_wide=-1, p2_sorted=-1, p45_stripes=-1, p24_pieces=-1, p4_grid=-1,
             test_max_nb2=0)
    assert not set(kw) - set(v), kw
    v.update(kw)
    i, o = In(**v), Out()
    assert L.test_hook("gk_test_part_plan")(C.byref(i), C.byref(o)) == L.GK_OK
    return o


def p4(o, level):
    """the level's form by name, after the checks every row makes: it fits the CU, and chunk and threads are the name's"""
    f = o.p4_op if level == "op" else o.p4_exact
    name = f.name.decode()
    assert (f.threads, f.chunk_keys) == FORMS[name], name
    if name != "direct":
        assert f.lds_bytes <= LDS_PER_CU, (name, f.lds_bytes)
    return name


OP_ROWS = [(1, 8, 255, "sort4096"), (1, 8, 256, "sort12288"), (1, 8, 2042, "sort12288"), (1, 8, 2043, "sort8192"), (1, 8, 4096, "sort8192"),
           (1, 10, 506, "sort12288"), (1, 10, 507, "sort8192"), (1, 10, 3066, "sort8192"), (1, 10, 3067, "sort4096"),
           (2, 8, 255, "sort4096"), (2, 8, 256, "sort6144"), (2, 8, 2810, "sort6144"), (2, 8, 2811, "sort4096"),
           (2, 10, 1274, "sort6144"), (2, 10, 1275, "sort4096")]
EXACT_ROWS = [(1, 8, 511, "sort4096"), (1, 8, 512, "sort8192"), (1, 8, 1023, "sort8192"), (1, 8, 1024, "sort12288"), (1, 8, 2042, "sort12288"),
              (1, 8, 2043, "sort8192"),
              (1, 10, 1024, "sort8192"),           # the x 12 form does not fit: 16384 + 122960 + 32776
              (2, 8, 4096, "sort4096")]            # 16-byte keys take the wide form only when asked


@pytest.mark.parametrize("W,lnb1,nb2,want", OP_ROWS)
def test_auto_overprovisioned_level(W, lnb1, nb2, want):
    assert p4(plan(W=W, lnb1=lnb1, nb2=nb2), "op") == want


@pytest.mark.parametrize("W,lnb1,nb2,want", EXACT_ROWS)
def test_auto_exact_level(W, lnb1, nb2, want):
    assert p4(plan(W=W, lnb1=lnb1, nb2=nb2, fine_exact=1), "exact") == want


def test_lds_bytes_are_the_formula():
    for W, threads, kpt, name, level, nb2 in ((1, 512, 8, "sort4096", "op", 100), (1, 1024, 8, "sort8192", "exact", 600), (1, 1024, 12, "sort12288", "op", 300),
                                             (2, 512, 8, "sort4096", "exact", 4096), (2, 1024, 6, "sort6144", "op", 300)):
        for lnb1 in (8, 9):
            o = plan(W=W, lnb1=lnb1, nb2=nb2)
            f = o.p4_op if level == "op" else o.p4_exact
            assert f.name.decode() == name
            assert f.lds_bytes == 16 * nb2 + 8 * W * threads * kpt + 4 * threads // 64 + 2 * threads * kpt + 16 + 8 * (4 * (1 << lnb1) + 1)


@pytest.mark.parametrize("level", ["op", "exact"])
def test_forced_p4_wide(level):
    for lnb1, nb2 in ((8, 64), (8, 2042), (10, 506)):                       # the x 12 form fits
        assert p4(plan(lnb1=lnb1, nb2=nb2, p4_wide=1), level) == "sort8192"
        assert p4(plan(lnb1=lnb1, nb2=nb2, p4_wide=2), level) == "sort12288"
    for lnb1, nb2 in ((8, 2043), (10, 507), (10, 3066)):                    # only the x 8 form does
        assert p4(plan(lnb1=lnb1, nb2=nb2, p4_wide=1), level) == "sort8192"
        assert p4(plan(lnb1=lnb1, nb2=nb2, p4_wide=2), level) == "sort8192"
    for wide in (1, 2):
        assert p4(plan(lnb1=10, nb2=3067, p4_wide=wide), level) == "sort4096"      # neither
        assert p4(plan(W=2, nb2=64, p4_wide=wide), level) == "sort6144"
        assert p4(plan(W=2, lnb1=10, nb2=1274, p4_wide=wide), level) == "sort6144"
        assert p4(plan(W=2, lnb1=10, nb2=1275, p4_wide=wide), level) == "sort4096"
    for W, lnb1, nb2 in ((1, 8, 64), (1, 8, 1024), (1, 8, 4096), (1, 10, 300), (2, 8, 256), (2, 8, 4096)):
        assert p4(plan(W=W, lnb1=lnb1, nb2=nb2, p4_wide=0), level) == "sort4096"


def test_forced_p4_direct():
    for W in (1, 2):
        for wide in (-1, 0, 1, 2):
            o = plan(W=W, nb2=1525, p4_direct=1, p4_wide=wide)
            assert p4(o, "exact") == "direct" and o.p4_exact.lds_bytes == 4 * 1525
            assert p4(o, "op") == p4(plan(W=W, nb2=1525, p4_wide=wide), "op") != "direct"        # ignored there
        assert p4(plan(W=W, nb2=1525, p4_direct=0), "exact") == p4(plan(W=W, nb2=1525), "exact") != "direct"


def test_part_supported():
    assert plan(W=2, lnb1=10, nb2=3580).supported == 1             # 16 * 3580 + 73776 + 32776 = 163832
    assert plan(W=2, lnb1=10, nb2=3581).supported == 0
    for W in (1, 2):
        for lnb1 in (0, 8, 9, 10):
            assert plan(W=W, lnb1=lnb1, nb2=4097).supported == 0
            assert plan(W=W, lnb1=lnb1, nb2=1).supported == 1
    assert plan(W=1, lnb1=10, nb2=4096).supported == 1             # 65536 + 41008 + 32776
    assert plan(W=2, lnb1=8, nb2=4096).supported == 1              # 65536 + 73776 + 8200
    assert plan(nb2=100, test_max_nb2=100).supported == 1 and plan(nb2=101, test_max_nb2=100).supported == 0


def test_p2_forms():
    for W in (1, 2):
        auto_sorted = W == 2
        for lnb1 in (9, 10):                       # beyond 256 L1 buckets: sorted or plain, whatever p2_wide says
            for wide in (-1, 0, 1):
                assert plan(W=W, lnb1=lnb1, p2_wide=wide).p2 == (b"sorted" if auto_sorted else b"plain")
                assert plan(W=W, lnb1=lnb1, p2_wide=wide, p2_sorted=1).p2 == b"sorted"
                assert plan(W=W, lnb1=lnb1, p2_wide=wide, p2_sorted=0).p2 == b"plain"
        for lnb1 in (4, 8):
            assert plan(W=W, lnb1=lnb1).p2 == (b"sorted" if auto_sorted else b"plain")
            assert plan(W=W, lnb1=lnb1, p2_wide=1).p2 == (b"wide_sorted" if auto_sorted else b"wide")
            assert plan(W=W, lnb1=lnb1, p2_wide=0, p2_sorted=0).p2 == b"plain"
            assert plan(W=W, lnb1=lnb1, p2_wide=0, p2_sorted=1).p2 == b"sorted"
            assert plan(W=W, lnb1=lnb1, p2_wide=1, p2_sorted=0).p2 == b"wide"
            assert plan(W=W, lnb1=lnb1, p2_wide=1, p2_sorted=1).p2 == b"wide_sorted"
    # what is not a stream of equal-length records that fit the LDS key buffer (5632 words) has no such member
    assert plan(source=RAGGED, max_windows=0).p2 == b"exact" and plan(part_exact=1).p2 == b"exact"
    assert plan(max_windows=5632).p2 == b"plain" and plan(max_windows=5633).p2 == b"exact"
    assert plan(W=2, max_windows=2816).p2 == b"sorted" and plan(W=2, max_windows=2817).p2 == b"exact"
    assert plan(source=KEYS, max_windows=0).p2 == b"keys" and plan(source=KEYS, max_windows=0, part_exact=1).p2 == b"keys_exact"


def test_stripes():
    want = {(-1, 8): 1, (0, 8): 1, (1, 8): 1, (2, 8): 2, (3, 8): 2, (5, 8): 4, (7, 8): 4, (8, 8): 8, (16, 8): 16, (17, 8): 16, (100, 8): 16,
            (3, 1): 2, (4, 1): 2, (2, 0): 1, (16, 3): 8, (12, 10): 8}
    for (stripes, lnb1), n in want.items():
        assert plan(lnb1=lnb1, p45_stripes=stripes).stripes == n, (stripes, lnb1)
        assert plan(lnb1=lnb1, p45_stripes=stripes, fine_exact=1).stripes == 1          # the exact level always gets 1
        assert plan(lnb1=lnb1, p45_stripes=stripes, from_empty=0).stripes == 1


def test_first_choices():
    """op1, the first fine_exact, sync_between, pipelined: one row per term of each rule"""
    def flags(**kw):
        o = plan(**kw)
        return o.op1, o.fine_exact, o.sync_between, o.pipelined
    assert flags() == (1, 0, 0, 0)                                              # from empty, near-distinct: nothing comes back between the levels
    assert flags(from_empty=0) == (1, 1, 1, 0)                                  # a table that holds data: exact, and the overflow flag is read first
    assert flags(fine_exact=1) == (1, 1, 0, 0)
    assert flags(estimate=1) == (1, 0, 1, 0)
    assert flags(verify_uniform=1) == (1, 0, 0, 0) and flags(verify_uniform=1, from_empty=0) == (1, 1, 1, 0)
    assert flags(source=RAGGED, max_windows=0) == (0, 1, 0, 0) and flags(part_exact=1) == (0, 1, 0, 0)
    assert flags(source=KEYS, max_windows=0) == (1, 0, 0, 0) and flags(source=KEYS, max_windows=0, from_empty=0) == (1, 1, 1, 0)
    for source in (DEVICE, HOST, PREFETCHED):
        assert flags(source=source, p24_pieces=2) == (1, 0, 0, 1)
        assert flags(source=source, p24_pieces=1) == (1, 0, 0, 0)
        assert flags(source=source, p24_pieces=2, p45_stripes=2) == (1, 0, 0, 0)
        assert flags(source=source, p24_pieces=2, estimate=1) == (1, 0, 1, 0)
        assert flags(source=source, p24_pieces=2, fine_exact=1) == (1, 1, 0, 0)
    assert flags(source=KEYS, max_windows=0, p24_pieces=2) == (1, 0, 0, 0)


def test_invalid_arguments():
    f = L.test_hook("gk_test_part_plan")
    o = Out()
    assert f(None, C.byref(o)) == L.GK_E_INVALID and f(C.byref(In(W=1, lnb1=8, nb2=1)), None) == L.GK_E_INVALID
    for bad in (dict(W=0), dict(W=3), dict(lnb1=-1), dict(lnb1=11), dict(source=5), dict(source=-1)):
        v = dict(W=1, lnb1=8, nb2=1, source=0)
        v.update(bad)
        assert f(C.byref(In(**v)), C.byref(o)) == L.GK_E_INVALID, bad
