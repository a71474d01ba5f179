"""group_aggregate and the device entry points behind it: what holds on any machine.
The names are declared in the headers, exported by libmq.so and bound by mq.py; the dense
path's slot limit needs no device; the numpy restatement the GPU tests compare against
agrees with a row-by-row loop; and without a device every call answers MQ_ENODEV / ERROR
(no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import groupcases as gc
from refapi import make_column, mq

DEVICE_API = ["mq_group_dense_slots", "mq_group_plan", "mq_group_write", "mq_group_free"]
DROPIN_API = ["group_aggregate"]


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
    assert "Result** group_aggregate(GeneralizedColumn* keys, GeneralizedColumn* values, Status* ret_status);" in qry_h
    assert "enum { MQ_GROUP_AUTO = 0, MQ_GROUP_DENSE = 1, MQ_GROUP_SORT = 2 };" in dev_h
    assert (mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT) == (0, 1, 2)


def test_dense_slots_is_a_positive_constant():
    lib = mq.load()
    s = lib.mq_group_dense_slots()
    assert s > 0 and lib.mq_group_dense_slots() == s


def test_model_is_consistent():
    """The restatement against a row-by-row dict loop: 300 rows, negative keys, repeats."""
    rng = np.random.default_rng(11)
    keys = rng.integers(-20, 9, 300).astype(np.int32)
    vals = rng.integers(-2**31, 2**31 - 1, 300).astype(np.int32)
    table = {}
    for k, v in zip(keys.tolist(), vals.tolist()):
        c, s, lo, hi = table.get(k, (0, 0, v, v))
        table[k] = (c + 1, s + v, min(lo, v), max(hi, v))
    order = sorted(table)
    gk, gc_, gs, gmn, gmx = gc.group(keys, vals)
    assert gk.tolist() == order and len(order) < 300 and order[0] < 0
    assert gc_.tolist() == [table[k][0] for k in order]
    assert gs.tolist() == [table[k][1] for k in order]
    assert gmn.tolist() == [table[k][2] for k in order]
    assert gmx.tolist() == [table[k][3] for k in order]
    assert (gk.dtype, gc_.dtype, gs.dtype, gmn.dtype, gmx.dtype) == (np.int32, np.uint64, np.int64, np.int32, np.int32)
    assert all(len(a) == 0 for a in gc.group(keys[:0], vals[:0]))
    # the named sets are what they say
    s = 2048
    assert gc.key_range(gc.keys_of("range_S", 4097, s)) == s
    assert gc.key_range(gc.keys_of("range_S_plus_1", 4097, s)) == s + 1
    assert gc.key_range(gc.keys_of("int32_ends", 65, s)) == 2**32
    assert len(np.unique(gc.keys_of("all_distinct", 1025, s))) == 1025
    assert np.all(np.diff(gc.keys_of("seven_sorted", 4097, s)) >= 0)
    assert int(gc.group(gc.keys_of("one_key", 70_001, s), gc.values_of("all_max", np.zeros(70_001, np.int32)))[2][0]) > 2**47


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    h, groups, path = C.c_void_p(), C.c_uint64(), C.c_int()
    assert lib.mq_group_plan(None, None, 0, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups), C.byref(path),
                             None) == mq.MQ_ENODEV
    assert lib.mq_group_write(None, None, None, None, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_group_free(None) == mq.MQ_ENODEV
    assert lib.mq_group_dense_slots() > 0
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    st = mq.Status(0, None)
    assert not lib.group_aggregate(C.byref(g), C.byref(g), C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
