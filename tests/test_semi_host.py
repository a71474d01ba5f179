"""select_where_in / aggregate_where_in and the device entry points behind them: what holds on
any machine. The names are declared in the headers, exported by libmq.so and bound by mq.py;
the workspace size and the automatic path need no device; the numpy restatement the GPU tests
compare against agrees with a plain Python loop, and the named sets are what they claim; and
without a device every call answers MQ_ENODEV / ERROR (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import semicases as sc
import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_keyset_build", "mq_keyset_free", "mq_semi_workspace_bytes", "mq_semi_auto_path", "mq_semi_positions",
              "mq_semi_agg"]
DROPIN_API = ["select_where_in", "aggregate_where_in"]


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    qry_h = open(f"{mq.INCLUDE_DIR}/mq_query.h").read()
    assert all(f" {n}(" in dev_h for n in DEVICE_API)
    assert all(f" {n}(" in qry_h for n in DROPIN_API)
    assert "enum { MQ_SEMI_AUTO = 0, MQ_SEMI_LDS = 1, MQ_SEMI_GLOBAL = 2 };" in dev_h
    assert (mq.MQ_SEMI_AUTO, mq.MQ_SEMI_LDS, mq.MQ_SEMI_GLOBAL) == (0, 1, 2)
    assert "typedef struct mq_keyset mq_keyset;" in dev_h
    assert [(n, t) for n, t in mq.MqKeysetInfo._fields_] == [
        ("lo", C.c_int32), ("hi", C.c_int32), ("distinct", C.c_uint64), ("bytes", C.c_uint64)]
    assert C.sizeof(mq.MqKeysetInfo) == 24
    assert "GeneralizedColumn* keys, GeneralizedColumn* set_keys, bool anti," in qry_h


def test_workspace_and_path_need_no_device():
    lib = mq.load()
    last = 0
    for n in [0, 1, 31, 1023, 1024, 1025, 4096, 4097, 10**6, 10**6 + 1, 10**9, 2**31 - 1]:
        b = lib.mq_semi_workspace_bytes(n)
        assert b >= last and b > 0, n
        assert b >= n // 8, n  # one bit per row is part of it
        assert b == lib.mq_where_workspace_bytes(n), n  # the same scan and expansion behind it
        last = b
    assert lib.mq_semi_auto_path(16) == mq.MQ_SEMI_LDS
    assert lib.mq_semi_auto_path(512 << 20) == mq.MQ_SEMI_GLOBAL
    paths = [lib.mq_semi_auto_path(b) for b in [0, 16, 1024, 2**14, 2**15, 2**16, 2**17, 2**17 + 16, 2**20, 2**29]]
    assert set(paths) == {mq.MQ_SEMI_LDS, mq.MQ_SEMI_GLOBAL}
    assert paths == sorted(paths)  # monotone: LDS (1) up to a size, GLOBAL (2) above it
    assert lib.mq_semi_auto_path(160 * 1024) == mq.MQ_SEMI_GLOBAL  # more than a CU's LDS


def test_model_is_consistent():
    """The restatement against a plain Python loop: 300 rows, both ends of int32 as keys and
    as set keys, 0 to 3 ranges, semi and anti."""
    rng = np.random.default_rng(11)
    cols = [rng.integers(-20, 20, 300).astype(np.int32) for _ in range(3)]
    key = rng.integers(-8, 8, 300).astype(np.int32)
    key[3], key[4], key[290], key[291] = wc.I32_MIN, wc.I32_MAX, wc.I32_MIN, wc.I32_MAX
    val, pay = wc.values_of(300), wc.payload_of(300)
    sets = [[-3, 0, 5, 5, 7], [wc.I32_MIN, 2], [wc.I32_MAX], [wc.I32_MIN, wc.I32_MAX], [], list(range(-8, 8))]
    for ranges in ([], [(-5, 12)], [(-5, 12), (None, 9), (-15, None)], [(None, None), (3, 3), (0, 5)]):
        p = len(ranges)
        for s in sets:
            members = {int(x) for x in s}
            for anti in (False, True):
                rows = []
                for i in range(300):
                    ok = all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi)
                             for c, (lo, hi) in zip(cols[:p], ranges))
                    if ok and ((int(key[i]) in members) != anti):
                        rows.append(i)
                got = sc.positions(cols[:p], ranges, key, np.array(s, dtype=np.int32), anti)
                assert got.dtype == np.int32 and got.tolist() == rows, (ranges, s, anti)
                assert sc.positions(cols[:p], ranges, key, s, anti, pay).tolist() == [int(pay[i]) for i in rows]
                vs = [int(val[i]) for i in rows]
                want = (len(vs), sum(vs), min(vs), max(vs)) if vs else (0, 0, wc.I32_MAX, wc.I32_MIN)
                assert sc.aggregate(cols[:p], ranges, key, s, val, anti) == want
    assert sc.positions([], [], key, [], True).tolist() == list(range(300))  # NOT IN the empty set
    assert sc.span_bytes([]) == 0 and sc.span_bytes([5]) == 16 and sc.span_bytes([0, 127]) == 16
    assert sc.span_bytes([0, 128]) == 32 and sc.span_bytes([wc.I32_MIN, wc.I32_MAX]) == 512 << 20


def test_named_sets_are_what_they_claim():
    lib = mq.load()
    for n in wc.SIZES + [70_001]:
        for name in sc.SETS:
            key, s = sc.keyset(name, n)
            assert key.dtype == s.dtype == np.int32 and len(key) == n, name
    n = 8193
    frac = {name: sc.hit(*sc.keyset(name, n)).mean() for name in sc.SETS}
    for name in ("dense_small", "sparse_wide", "single", "negative", "min_edge", "max_edge", "dups"):
        assert 0.1 < frac[name] < 0.9, (name, frac[name])  # semi and anti both keep rows
    assert frac["every_key"] == 1.0 and frac["empty"] == 0.0
    assert len(sc.keyset("empty", n)[1]) == 0 and len(sc.keyset("every_key", 0)[1]) == 0
    key, s = sc.keyset("dense_small", n)
    assert key.min() < s.min() and key.max() > s.max()  # keys on both sides of the span
    assert lib.mq_semi_auto_path(sc.span_bytes(s)) == mq.MQ_SEMI_LDS
    key, s = sc.keyset("sparse_wide", n)
    assert key.min() < s.min() and key.max() > s.max()
    assert sc.span_bytes(s) == 2**22 // 8 and lib.mq_semi_auto_path(sc.span_bytes(s)) == mq.MQ_SEMI_GLOBAL
    key, s = sc.keyset("min_edge", n)
    assert s.min() == wc.I32_MIN + 1 and {wc.I32_MIN, wc.I32_MAX, int(s.min()), int(s.max()), int(s.max()) + 1} <= set(key.tolist())
    key, s = sc.keyset("max_edge", n)
    assert s.max() == wc.I32_MAX and {wc.I32_MIN, wc.I32_MAX, int(s.min()), int(s.min()) - 1} <= set(key.tolist())
    key, s = sc.keyset("negative", n)
    assert s.max() < 0 and key.min() < s.min() and key.max() > s.max()
    key, s = sc.keyset("dups", n)
    assert len(s) == 4097 and len(np.unique(s)) <= 50
    assert sc.case("uniform_10", n, 0) == ([], [])
    assert len(sc.case("uniform_10", n, 3)[0]) == 3


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    rng = (mq.MqRange * 1)(mq.MqRange(1, 0, 1, 5))
    ptrs = (C.c_void_p * 1)(None)
    ks, info = C.c_void_p(), mq.MqKeysetInfo()
    assert lib.mq_keyset_build(None, 0, 0, 0, 0, C.byref(ks), C.byref(info), None) == mq.MQ_ENODEV
    assert lib.mq_keyset_build(None, 10, 1, 0, 5, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_keyset_free(None) == mq.MQ_ENODEV
    assert lib.mq_semi_positions(ptrs, rng, 1, None, None, 0, 0, None, 0, None, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_semi_positions(None, None, 0, None, None, 1, 2, None, 10, None, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_semi_agg(ptrs, rng, 1, None, None, 0, 0, None, 0, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_semi_agg(None, None, 0, None, None, 1, 7, None, 10, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_semi_workspace_bytes(10) > 0
    col = make_column(np.arange(8, dtype=np.int32))
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(g))
    lows = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(2)))
    highs = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(6)))
    for anti in (False, True):
        st = mq.Status(0, None)
        assert not lib.select_where_in(gp, lows, highs, 1, C.byref(g), C.byref(g), anti, None, C.byref(st))
        assert st.code == mq.ERROR
        assert "libmq" in capfd.readouterr().err
        st = mq.Status(0, None)
        assert not lib.aggregate_where_in(None, None, None, 0, C.byref(g), C.byref(g), anti, C.byref(g), C.byref(st))
        assert st.code == mq.ERROR
        assert "libmq" in capfd.readouterr().err
