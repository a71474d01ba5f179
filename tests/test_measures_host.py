"""group_aggregate_measures and the device entry points behind it: what holds on any machine. The
names are declared, exported and bound; mq_measure is the 24 bytes the header says; the dense
capacity per number of measures is the largest power of two of (4 + 24 * nmeas)-byte slots in
40 KiB and mq_group_measures_auto_path switches exactly there; and the numpy restatement the GPU
tests compare against agrees with hand-computed cases (the extremes of int32 among them) and with
a loop over Python integers.
"""
import ctypes as C

import numpy as np
import pytest

import measurecases as mc
import starcases as sc
import wherecases as wc
from refapi import mq

DEVICE_API = ["mq_group_measures_dense_slots", "mq_group_measures_auto_path", "mq_group_measures_plan",
              "mq_group_measures_write", "mq_group_measures_free"]
DROPIN_API = ["group_aggregate_measures"]
I32_MIN, I32_MAX = mc.I32_MIN, mc.I32_MAX


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
    assert "enum { MQ_GROUP_MAX_MEASURES = 4 };" in dev_h and mq.MQ_GROUP_MAX_MEASURES == 4 == mc.MAX_MEASURES
    assert "enum { MQ_MEAS_COL = 0, MQ_MEAS_ADD = 1, MQ_MEAS_SUB = 2, MQ_MEAS_MUL = 3 };" in dev_h
    assert (mq.MQ_MEAS_COL, mq.MQ_MEAS_ADD, mq.MQ_MEAS_SUB, mq.MQ_MEAS_MUL) == tuple(mc.OPS[o] for o in ("col", "add", "sub", "mul"))


def test_measure_struct_layout():
    assert C.sizeof(mq.MqMeasure) == 24
    assert [n for n, _ in mq.MqMeasure._fields_] == ["d_a", "d_b", "op", "reserved"]
    assert [getattr(mq.MqMeasure, n).offset for n, _ in mq.MqMeasure._fields_] == [0, 8, 16, 20]


def test_dense_slots():
    lib = mq.load()
    assert [lib.mq_group_measures_dense_slots(k) for k in (1, 2, 3, 4)] == [1024, 512, 512, 256]
    assert lib.mq_group_measures_dense_slots(0) == 0 and lib.mq_group_measures_dense_slots(5) == 0
    for nmeas in (1, 2, 3, 4):
        s = lib.mq_group_measures_dense_slots(nmeas)
        assert s == mc.SLOTS[nmeas] and s & (s - 1) == 0
        assert s * mc.slot_bytes(nmeas) <= mc.LDS_BYTES < 2 * s * mc.slot_bytes(nmeas)
    assert lib.mq_group_dense_slots() == 2048  # the single-value plans keep theirs


@pytest.mark.parametrize("nmeas", [1, 2, 3, 4])
def test_auto_path_switches_at_the_capacity(nmeas):
    lib = mq.load()
    cap = mc.SLOTS[nmeas]

    def auto(bounds, nkeys, nm=nmeas):
        space = C.c_uint64(777)
        return lib.mq_group_measures_auto_path((C.c_int32 * len(bounds))(*bounds), nkeys, nm, C.byref(space)), space.value

    assert auto([5, 5 + cap - 1], 1) == (mq.MQ_GROUP_DENSE, cap)
    assert auto([5, 5 + cap], 1) == (mq.MQ_GROUP_SORT, cap + 1)
    assert auto([-3, -2, 100, 100 + cap // 2 - 1], 2) == (mq.MQ_GROUP_DENSE, cap)
    assert auto([0, cap, -7, -7], 2) == (mq.MQ_GROUP_SORT, cap + 1)
    assert auto([I32_MIN, I32_MAX], 1) == (mq.MQ_GROUP_SORT, 1 << 32)
    assert auto([I32_MIN, I32_MAX, 0, 1], 2)[0] == mq.MQ_EINVAL and b"mq_group_measures_auto_path" in lib.mq_last_error()
    assert auto([1, 0], 1) == (mq.MQ_EINVAL, 0)
    assert auto([0, 1], 0)[0] == mq.MQ_EINVAL and auto([0, 1] * 5, 5)[0] == mq.MQ_EINVAL
    assert auto([0, 1], 1, 0)[0] == mq.MQ_EINVAL and auto([0, 1], 1, 5)[0] == mq.MQ_EINVAL
    assert lib.mq_group_measures_auto_path(None, 1, nmeas, None) == mq.MQ_EINVAL


def i32(*v):
    return np.array(v, dtype=np.int32)


def test_model_by_hand():
    """Six rows, a range that drops one, a filtering set that drops another, two groups."""
    k = i32(2, 1, 2, 1, 2, 9)
    a = i32(10, -3, 7, 5, 100, 1000)
    b = i32(2, 4, -1, 5, 100, 1000)
    sel = i32(1, 1, 1, 1, 0, 1)   # the range [1, 2) drops row 4
    fk = i32(5, 5, 6, 5, 5, 77)   # the set {5, 6} drops row 5
    terms = [sc.Term("plain", k), sc.Term("ks", fk, i32(5, 6))]
    meas = [mc.Measure("col", a), mc.Measure("add", a, b), mc.Measure("sub", a, b), mc.Measure("mul", a, b)]
    keys, count, aggs = mc.model([sel], [(1, 2)], terms, meas)
    assert keys[0].tolist() == [1, 2] and count.tolist() == [2, 2] and count.dtype == np.uint64
    want = [([2, 17], [-3, 7], [5, 10]), ([11, 18], [1, 6], [10, 12]), ([-7, 16], [-7, 8], [0, 8]), ([13, 13], [-12, -7], [25, 20])]
    for (s, mn, mx), (ws, wmn, wmx) in zip(aggs, want):
        assert (s.tolist(), mn.tolist(), mx.tolist()) == (ws, wmn, wmx)
        assert s.dtype == mn.dtype == mx.dtype == np.int64


def test_model_extremes():
    one = [sc.Term("plain", i32(0, 0, 0, 0))]
    lo4, hi4 = np.full(4, I32_MIN, np.int32), np.full(4, I32_MAX, np.int32)
    (s, mn, mx), = mc.model([], [], one, [mc.Measure("mul", lo4, lo4)])[2]
    assert (s.tolist(), mn.tolist(), mx.tolist()) == ([0], [1 << 62], [1 << 62])  # 4 * 2^62 = 2^64
    two = [sc.Term("plain", i32(0, 0))]
    (s, mn, mx), = mc.model([], [], two, [mc.Measure("mul", lo4[:2], lo4[:2])])[2]
    assert s.tolist() == [mc.I64_MIN]                                           # 2 * 2^62 wraps to INT64_MIN
    (s, mn, mx), = mc.model([], [], two, [mc.Measure("mul", lo4[:2], hi4[:2])])[2]
    p = I32_MIN * I32_MAX
    assert (s.tolist(), mn.tolist(), mx.tolist()) == ([2 * p], [p], [p])
    (s, mn, mx), = mc.model([], [], two, [mc.Measure("sub", lo4[:2], hi4[:2])])[2]
    assert mn.tolist() == [-4294967295] == mx.tolist() and s.tolist() == [-8589934590]
    (s, mn, mx), = mc.model([], [], two, [mc.Measure("add", hi4[:2], hi4[:2])])[2]
    assert mn.tolist() == [4294967294] == mx.tolist() and s.tolist() == [8589934588]


@pytest.mark.parametrize("layout", ["km", "ks_km", "km_plain_km", "ks_km_plain_km"])
def test_model_agrees_with_python_integers(layout):
    n = 300
    kinds = sc.LAYOUTS[layout]
    cards = (3,) * sc.nkeys_of(kinds)
    terms = sc.make(layout, cards, n, seed=5)
    for big in (False, True):
        ops = mc.columns(n, seed=1, big=big)
        meas = mc.q1_measures(ops, 4) + [mc.Measure("mul", ops[0], ops[0])]
        for ncols in (0, 2):
            cols, ranges = sc.case("uniform_50", n, ncols)
            got, want = mc.model(cols, ranges, terms, meas), mc.brute(cols, ranges, terms, meas)
            assert [k.tolist() for k in got[0]] == [k.tolist() for k in want[0]]
            assert got[1].tolist() == want[1].tolist() and len(got[1]) > 1
            for g, w in zip(got[2], want[2]):
                assert all(a.dtype == np.int64 and a.tolist() == b.tolist() for a, b in zip(g, w))
            one = sc.model(cols, ranges, terms, ops[1])  # a plain column is starcases' value column
            assert got[2][1][0].tolist() == one[2].tolist() and got[2][1][1].tolist() == one[3].tolist()
            assert int(got[1].sum()) == int(sc.joined(cols, ranges, terms).sum()) < n
    assert wc.I32_MIN == I32_MIN
