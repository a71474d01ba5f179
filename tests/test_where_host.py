"""select_where / aggregate_where and the device entry points behind them: what holds on any
machine. The names are declared in the headers, exported by libmq.so and bound by mq.py;
the workspace size needs no device; the numpy restatement the GPU tests compare against
agrees with a plain Python loop, and the named sets are what they claim; and without a
device every call answers MQ_ENODEV / ERROR (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_where_workspace_bytes", "mq_where_positions", "mq_where_agg"]
DROPIN_API = ["select_where", "aggregate_where"]


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
    assert "Result* select_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols," in qry_h
    assert "Result** aggregate_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols," in qry_h
    assert f"enum {{ MQ_WHERE_MAX_COLS = {mq.MQ_WHERE_MAX_COLS} }};" in dev_h
    assert mq.MQ_WHERE_MAX_COLS == 8 == wc.MAX_COLS
    assert "typedef struct mq_range { int32_t has_low, low, has_high, high; } mq_range;" in dev_h
    assert [(n, t) for n, t in mq.MqRange._fields_] == [
        ("has_low", C.c_int32), ("low", C.c_int32), ("has_high", C.c_int32), ("high", C.c_int32)]
    assert C.sizeof(mq.MqRange) == 16
    assert "MOST SELECTIVE PREDICATE FIRST" in dev_h  # the caller is told what the order costs


def test_workspace_bytes_need_no_device():
    lib = mq.load()
    last = 0
    for n in [0, 1, 31, 1023, 1024, 1025, 4096, 4097, 10**6, 10**6 + 1, 10**9, 2**31 - 1]:
        b = lib.mq_where_workspace_bytes(n)
        assert b >= last and b > 0, n
        assert b >= n // 8, n  # one bit per row is part of it
        last = b
    assert lib.mq_where_workspace_bytes(10**9) < 10**9 // 4  # and not much more than that


def test_model_is_consistent():
    """The restatement against a plain Python loop: 300 rows x 3 columns, negatives, both
    ends of int32, every kind of bound."""
    rng = np.random.default_rng(7)
    cols = [rng.integers(-20, 20, 300).astype(np.int32) for _ in range(3)]
    cols[1][5], cols[1][6] = wc.I32_MIN, wc.I32_MAX
    val, pay = wc.values_of(300), wc.payload_of(300)
    for ranges in ([(-5, 12), (None, 9), (-15, None)], [(None, None), (wc.I32_MIN, wc.I32_MAX), (0, 1)],
                   [(3, 3), (None, None), (None, None)], [(None, wc.I32_MIN), (0, 5), (0, 5)],
                   [(-20, 20), (wc.I32_MAX, None), (None, None)]):
        rows = []
        for i in range(300):
            ok = True
            for c, (lo, hi) in zip(cols, ranges):
                x = int(c[i])
                ok = ok and (lo is None or x >= lo) and (hi is None or x < hi)
            if ok:
                rows.append(i)
        for p in (1, 2, 3):
            r = [i for i in range(300) if all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi)
                                              for c, (lo, hi) in zip(cols[:p], ranges[:p]))]
            assert wc.positions(cols[:p], ranges[:p]).tolist() == r
        got = wc.positions(cols, ranges)
        assert got.dtype == np.int32 and got.tolist() == rows
        assert wc.positions(cols, ranges, pay).tolist() == [int(pay[i]) for i in rows]
        vs = [int(val[i]) for i in rows]
        want = (len(vs), sum(vs), min(vs), max(vs)) if vs else (0, 0, wc.I32_MAX, wc.I32_MIN)
        assert wc.aggregate(cols, ranges, val) == want
    assert wc.aggregate(cols, [(None, None)] * 3, val)[0] == 300


def test_named_sets_are_what_they_claim():
    L = wc.LINE
    for n in (8193, wc.BIG):
        lines = (n + L - 1) // L
        for ncols in wc.NCOLS:
            for name in wc.CASES:
                cols, ranges = wc.case(name, n, ncols)
                assert len(cols) == len(ranges) == ncols, name
                assert all(c.dtype == np.int32 and len(c) == n for c in cols), name
            sel = lambda name, p=ncols: wc.mask(*wc.case(name, n, p))  # noqa: E731
            lead = lambda name: wc.in_range(wc.case(name, n, ncols)[0][0], *wc.case(name, n, ncols)[1][0])  # noqa: E731
            for name, frac in (("uniform_0p1", 0.001), ("uniform_1", 0.01), ("uniform_10", 0.1), ("uniform_50", 0.5)):
                f = lead(name).mean()
                assert 0.5 * frac < f < 1.6 * frac + 2 / n, (name, f)
            m = lead("sorted_lead")
            idx = np.flatnonzero(m)
            assert len(idx) > n // 4 and np.all(np.diff(idx) == 1) and idx[0] > 0 and idx[-1] < n - 1
            m = lead("clustered_lead")
            edges = np.flatnonzero(np.diff(m.astype(np.int8))) + 1
            runs = np.diff(np.concatenate(([0], edges, [n])))
            assert runs.min() == 1 and runs.max() == 4097 and np.any(edges % L != 0)
            per_line = lambda m: np.add.reduceat(m.astype(np.int64), np.arange(0, n, L))  # noqa: E731
            for name, where in (("islands_first", lambda k: 0 * k), ("islands_last", lambda k: 0 * k + L - 1),
                                ("islands_alt", lambda k: (L - 1) * (k & 1))):
                m = lead(name)
                c = per_line(m)
                k = np.arange(lines)
                rows = k * L + where(k)
                rows = rows[rows < n]
                assert np.array_equal(np.flatnonzero(m), rows), name
                assert np.all(c[:n // L] == 1), name  # exactly one survivor per whole line
            assert np.array_equal(np.flatnonzero(lead("every_257")), np.arange(0, n, 257))
            assert np.array_equal(np.flatnonzero(lead("tail_only")), np.arange(n - n % L, n)) and n % L
            assert np.flatnonzero(lead("ends_only")).tolist() == [0, n - 1]
            assert lead("first_all").all() and wc.case("first_all", n, ncols)[1][0] != (None, None)
            assert not lead("first_none").any() and not sel("first_none").any()
            cols, ranges = wc.case("last_kills", n, ncols)
            assert all(wc.in_range(c, *r).all() for c, r in zip(cols[:-1], ranges[:-1]))
            assert 0 < sel("last_kills").sum() < n
            assert wc.case("unbounded_middle", n, ncols)[1][min(1, ncols - 1)] == (None, None)
            assert sel("unbounded_middle").all() == (ncols == 1)
            lo, hi = wc.case("empty_range", n, ncols)[1][-1]
            assert lo >= hi and not sel("empty_range").any()
            assert (None, wc.I32_MIN) in wc.case("empty_high_min", n, ncols)[1] and not sel("empty_high_min").any()
            cols, ranges = wc.case("extreme_bounds", n, ncols)
            assert all(c.min() == wc.I32_MIN and c.max() == wc.I32_MAX for c in cols)
            assert all(lo in (None, wc.I32_MIN, wc.I32_MIN + 1) and hi in (None, wc.I32_MAX) for lo, hi in ranges)
            assert 0 < sel("extreme_bounds").sum() < n or ncols == 1
            cols, ranges = wc.case("same_twice", n, ncols)
            if ncols > 1:
                assert cols[1] is cols[0] and ranges[:2] == [(100, None), (None, 600)]
                assert 0 < sel("same_twice").sum() < wc.in_range(cols[0], 100, None).sum()
    for n in wc.SIZES:  # every size is constructible, also the empty one
        for name in wc.CASES:
            cols, ranges = wc.case(name, n, 3)
            assert len(wc.mask(cols, ranges)) == n
    assert len(np.unique(wc.payload_of(4097))) == 4097
    v = wc.values_of(4097)
    assert v.min() == wc.I32_MIN and v.max() == wc.I32_MAX


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    rng = (mq.MqRange * 2)(mq.MqRange(1, 0, 1, 5), mq.MqRange(0, 0, 0, 0))
    ptrs = (C.c_void_p * 2)(None, None)
    assert lib.mq_where_positions(ptrs, rng, 2, None, 0, None, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_where_positions(ptrs, rng, 2, None, 10, None, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_where_agg(ptrs, rng, 1, None, 0, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_where_agg(None, None, 0, None, 10, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_where_workspace_bytes(10) > 0
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(g))
    lows = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(2)))
    highs = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(6)))
    st = mq.Status(0, None)
    assert not lib.select_where(gp, lows, highs, 1, None, C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
    st = mq.Status(0, None)
    assert not lib.aggregate_where(gp, lows, highs, 1, C.byref(g), C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
