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

DEVICE_API = ["mq_group_dense_slots", "mq_group_sort_geometry", "mq_group_plan", "mq_group_write", "mq_group_free"]
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


def _sort_geometry(lib, n):
    b, c = C.c_uint32(77), C.c_uint64(77)
    lib.mq_group_sort_geometry(n, C.byref(b), C.byref(c))
    return b.value, c.value


def test_sort_geometry_needs_no_device():
    """(blocks, chunk rows) of the sort path's fixed grid, pinned: chunks() of
    mq_scan_common.h with 1024-row tiles and at most 2048 blocks. A block takes a second
    tile from 2 097 153 rows on."""
    lib = mq.load()
    assert _sort_geometry(lib, 4_195_333) == (1366, 3072)
    assert _sort_geometry(lib, 2_097_152) == (2048, 1024)
    assert _sort_geometry(lib, 2_097_153) == (1025, 2048)
    assert _sort_geometry(lib, 300_001) == (293, 1024)  # the largest of gc.SIZES: one tile a block
    assert _sort_geometry(lib, 1) == (1, 1024) and _sort_geometry(lib, 0) == (1, 1024)
    lib.mq_group_sort_geometry(5000, None, None)  # either output may be NULL
    assert (gc.SORT_N, gc.SORT_N_TWO_TILES) == (4_195_333, 2_097_153)


def test_sort_run_sets_are_what_they_say():
    """groupcases.runs_of / keys_from_runs / planted_values at a small size: the run
    lengths sum to n, a stable sort of the keys has exactly those runs, both INT32 ends are
    keys, and the values carry both extremes at tile edges of the sorted sequence."""
    n, chunk = 20_011, 3 * gc.SEG_TILE
    for name in gc.RUN_SETS:
        runs = gc.runs_of(name, n, chunk)
        assert runs.sum() == n and runs.min() >= 1, name
        keys, order = gc.keys_from_runs(runs, seed=3)
        k, count = gc.group(keys, keys)[:2]
        assert np.array_equal(count, runs.astype(np.uint64)), name
        assert k[0] == gc.I32_MIN and (len(k) == 1 or k[-1] == gc.I32_MAX), name
        assert np.array_equal(keys[order], np.repeat(k, runs)), name
        sv = gc.planted_values(runs, order, seed=4)[order]
        assert {int(sv[gc.SEG_TILE - 1]), int(sv[gc.SEG_TILE])} == {gc.I32_MIN, gc.I32_MAX}, name
    starts = lambda name: np.concatenate([[0], np.cumsum(gc.runs_of(name, n, chunk))[:-1]])
    assert np.all(starts("tile_runs") % gc.SEG_TILE == 0)
    assert np.all(starts("tile_runs_plus_1")[1:] % gc.SEG_TILE == 1)
    assert np.all(starts("tile_runs_minus_1")[1:] % gc.SEG_TILE == gc.SEG_TILE - 1)
    assert np.all(starts("chunk_runs_plus_1")[1:] % chunk == 1)
    assert np.all(starts("chunk_runs_minus_1")[1:] % chunk == chunk - 1)
    assert gc.runs_of("skewed", n, chunk).max() == n * 9 // 10
    assert set(gc.runs_of("mixed", n, chunk)[:-1].tolist()) <= set(gc.MIXED_RUNS)


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
