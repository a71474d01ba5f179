"""group_aggregate_by and the device entry points behind it: what holds on any machine. The
names are declared in the headers, exported by libmq.so and bound by mq.py; the path rule
(mq_group_by_auto_path) needs no device; the numpy restatement the GPU tests compare against
agrees with a row-by-row loop; and without a device every call answers MQ_ENODEV / ERROR (no
CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import groupbycases as gb
import groupcases as gc
from refapi import make_column, mq

DEVICE_API = ["mq_group_by_auto_path", "mq_group_by_plan", "mq_group_by_write"]
DROPIN_API = ["group_aggregate_by"]


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    qry_h = open(f"{mq.INCLUDE_DIR}/mq_query.h").read()
    assert all(f"int {n}(" in dev_h for n in DEVICE_API)
    assert ("Result** group_aggregate_by(GeneralizedColumn** keys, int nkeys, GeneralizedColumn* values, "
            "Status* ret_status);") in qry_h
    assert "enum { MQ_GROUP_MAX_KEYS = 4 };" in dev_h
    assert mq.MQ_GROUP_MAX_KEYS == 4 == gb.MAX_KEYS


def test_model_is_consistent():
    """The restatement against a row-by-row dict loop: 300 rows, negative keys, repeated
    tuples; with one key column it is groupcases.group."""
    rng = np.random.default_rng(13)
    n = 300
    cols = [rng.integers(-3, 3, n).astype(np.int32), rng.integers(-2, 2, n).astype(np.int32),
            rng.integers(-1, 2, n).astype(np.int32)]
    vals = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    for nkeys in (1, 2, 3):
        table = {}
        for i in range(n):
            t, v = tuple(int(c[i]) for c in cols[:nkeys]), int(vals[i])
            c, s, lo, hi = table.get(t, (0, 0, v, v))
            table[t] = (c + 1, s + v, min(lo, v), max(hi, v))
        order = sorted(table)  # Python orders tuples lexicographically, the first component first
        ks, cnt, sm, mn, mx = gb.group_by(cols[:nkeys], vals)
        assert list(zip(*[k.tolist() for k in ks])) == order and len(order) < n and order[0][0] < 0
        assert cnt.tolist() == [table[t][0] for t in order]
        assert sm.tolist() == [table[t][1] for t in order]
        assert mn.tolist() == [table[t][2] for t in order]
        assert mx.tolist() == [table[t][3] for t in order]
        assert [k.dtype for k in ks] == [np.int32] * nkeys
        assert (cnt.dtype, sm.dtype, mn.dtype, mx.dtype) == (np.uint64, np.int64, np.int32, np.int32)
    one = gb.group_by(cols[:1], vals)
    for got, want in zip([one[0][0], *one[1:]], gc.group(cols[0], vals)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    empty = gb.group_by([cols[0][:0], cols[1][:0]], vals[:0])
    assert len(empty[0]) == 2 and all(len(a) == 0 for a in empty[0] + list(empty[1:]))


def test_tuple_sets_are_what_they_say():
    s = 2048
    for nkeys in (2, 3, 4):
        sp = lambda name, n=4097: gb.space_of(gb.bounds_of(gb.tuples_of(name, n, nkeys, s)))
        assert sp("space_S") == s and sp("space_S_plus_1") == s + 1 and sp("ends_x_one") == 2**32
        assert sp("one_tuple") == 1 and sp("skewed") <= s
        assert len(gb.group_by(gb.tuples_of("seven_shuffled", 4097, nkeys, s), np.zeros(4097, np.int32))[1]) == 7
        first = gb.tuples_of("seven_sorted", 4097, nkeys, s)[0]
        assert np.all(np.diff(first) >= 0)
        cols = gb.tuples_of("all_distinct", 1025, nkeys, s)
        assert len(gb.group_by(cols, cols[0])[1]) == 1025 and all(len(np.unique(c)) < 1025 for c in cols)
        hot = gb.group_by(gb.tuples_of("skewed", 70_001, nkeys, s), np.zeros(70_001, np.int32))[1].max()
        assert 0.88 * 70_001 < hot < 0.92 * 70_001
        for name, j in (("last_differs", nkeys - 1), ("first_differs", 0)):
            cols = gb.tuples_of(name, 4097, nkeys, s)
            assert [len(np.unique(c)) > 1 for c in cols] == [i == j for i in range(nkeys)]
        cols = gb.tuples_of("first_two_last_many", 4097, nkeys, s)
        ks = gb.group_by(cols, cols[0])[0]
        assert np.all(np.diff(ks[0]) >= 0) and not np.all(np.diff(ks[-1]) >= 0)


def _auto(lib, bounds, nkeys=None):
    b = (C.c_int32 * max(len(bounds), 1))(*bounds)
    space = C.c_uint64(99)
    rc = lib.mq_group_by_auto_path(b, len(bounds) // 2 if nkeys is None else nkeys, C.byref(space))
    return rc, space.value


def test_auto_path_needs_no_device():
    lib = mq.load()
    S = lib.mq_group_dense_slots()
    D, SORT, EINVAL = mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT, mq.MQ_EINVAL
    assert _auto(lib, [0, S - 1, 5, 5]) == (D, S)
    side = int(np.floor(np.sqrt(S)))  # 45 for S = 2048: 45 x 45 fits, 46 x 45 does not
    assert side * side <= S < (side + 1) * side
    assert _auto(lib, [0, side - 1, 0, side - 1]) == (D, side * side)
    assert _auto(lib, [0, side, 0, side - 1]) == (SORT, (side + 1) * side)
    assert _auto(lib, [-7, -7 + S, 3, 3]) == (SORT, S + 1)
    assert _auto(lib, [gc.I32_MIN, gc.I32_MAX, 7, 7]) == (SORT, 2**32)
    assert _auto(lib, [gc.I32_MIN, gc.I32_MAX, 0, 1]) == (EINVAL, 2**33)
    assert _auto(lib, [gc.I32_MIN, gc.I32_MAX] * 4) == (EINVAL, 2**63)  # 2^128, saturated
    assert _auto(lib, [gc.I32_MIN, gc.I32_MAX, 0, 2**31 - 1, 0, 0]) == (EINVAL, 2**63)  # exactly 2^63
    assert _auto(lib, [0, 3, 0, 2, -1, 0, 5, 9]) == (D, 4 * 3 * 2 * 5)
    assert _auto(lib, [3, 3]) == (D, 1)
    assert _auto(lib, [0, 9, 5, 4])[0] == EINVAL and _auto(lib, [1, 0, 0, 9])[0] == EINVAL  # lo > hi
    assert _auto(lib, [], nkeys=0)[0] == EINVAL
    assert _auto(lib, [0, 1] * 5, nkeys=5)[0] == EINVAL
    assert lib.mq_group_by_auto_path(None, 2, None) == EINVAL
    b = (C.c_int32 * 4)(0, 9, 0, 9)
    assert lib.mq_group_by_auto_path(b, 2, None) == D  # the space may be left out


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    h, groups, path = C.c_void_p(), C.c_uint64(), C.c_int()
    keys = (C.c_void_p * 2)(None, None)
    assert lib.mq_group_by_plan(keys, 2, None, 0, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups), C.byref(path),
                                None) == mq.MQ_ENODEV
    assert lib.mq_group_by_write(None, None, None, None, None, None, None) == mq.MQ_ENODEV
    b = (C.c_int32 * 4)(0, 9, 0, 9)
    assert lib.mq_group_by_auto_path(b, 2, None) == mq.MQ_GROUP_DENSE  # the exception: no device needed
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    arr = (C.POINTER(mq.GeneralizedColumn) * 2)(C.pointer(g), C.pointer(g))
    st = mq.Status(0, None)
    assert not lib.group_aggregate_by(arr, 2, C.byref(g), C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
