"""group_count_distinct and mq_group_distinct_plan behind it: what holds on any machine. The names
are declared in the headers, exported by libmq.so and bound by mq.py; the three functions that
need no device answer without one; AUTO's size rule at its edges; and the numpy model the GPU
tests compare against agrees with a set of Python tuples.
"""
import ctypes as C

import numpy as np
import pytest

import distinctcases as dc
from refapi import mq

DEVICE_API = ["mq_group_distinct_lds_bytes", "mq_group_distinct_bitmap_bytes", "mq_group_distinct_auto_path",
              "mq_group_distinct_plan", "mq_group_distinct_write", "mq_group_distinct_free"]
DROPIN_API = ["group_count_distinct"]
FULL = [dc.I32_MIN, dc.I32_MAX]


def auto(lib, kb, vb, nkeys=None):
    """(return code, *h_bitmap_bytes)"""
    b = C.c_uint64(77)
    k = (C.c_int32 * max(len(kb), 1))(*kb)
    v = (C.c_int32 * 2)(*vb)
    return lib.mq_group_distinct_auto_path(k, len(kb) // 2 if nkeys is None else nkeys, v, C.byref(b)), b.value


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    assert (mq.MQ_GDISTINCT_AUTO, mq.MQ_GDISTINCT_LDS, mq.MQ_GDISTINCT_BITMAP, mq.MQ_GDISTINCT_SORT) == (0, 1, 2, 3)
    assert (dc.AUTO, dc.LDS, dc.BITMAP, dc.SORT) == (0, 1, 2, 3)
    assert [f for f, _ in mq.MqGdistinctInfo._fields_] == ["path", "space", "span", "bitmap_bytes", "rows", "pairs"]
    assert C.sizeof(mq.MqGdistinctInfo) == 48
    # the drop-in takes what group_aggregate_by_where takes
    assert mq._SIGS["group_count_distinct"] == mq._SIGS["group_aggregate_by_where"]


def test_constants_need_no_device():
    lib = mq.load()
    lds, bitmap = lib.mq_group_distinct_lds_bytes(), lib.mq_group_distinct_bitmap_bytes()
    assert 0 < lds <= 64 * 1024 and lds % 4 == 0  # two blocks fit a CU's 160 KiB
    assert bitmap == 512 * 2**20


def test_auto_rule_at_its_edges():
    lib = mq.load()
    lds, bitmap = lib.mq_group_distinct_lds_bytes(), lib.mq_group_distinct_bitmap_bytes()
    words = lds // 4
    # 4 P R equal to the LDS constant, and one word more: R = 1 (P rows of one word), then P = 1 (one row of R words)
    assert auto(lib, [0, words - 1], [5, 5]) == (dc.LDS, lds)
    assert auto(lib, [0, words], [5, 5]) == (dc.BITMAP, lds + 4)
    assert auto(lib, [7, 7], [0, 32 * words - 1]) == (dc.LDS, lds)
    assert auto(lib, [7, 7], [0, 32 * words]) == (dc.BITMAP, lds + 4)
    # R's rounding: W = 32 / 33 and 64 / 65 with P = words / 2 rows
    half = words // 2
    assert auto(lib, [1, half], [-16, 15]) == (dc.LDS, 4 * half)
    assert auto(lib, [1, half], [-16, 16]) == (dc.LDS, 8 * half)
    assert auto(lib, [1, half], [-32, 31]) == (dc.LDS, 8 * half)
    assert auto(lib, [1, half], [-32, 32]) == (dc.BITMAP, 12 * half)
    for w, r in ((1, 1), (31, 1), (32, 1), (33, 2), (64, 2), (65, 3)):
        assert auto(lib, [0, 9, 0, 9], [100, 100 + w - 1]) == (dc.LDS, 400 * r), w
        assert dc.shape([0, 9, 0, 9], [100, 100 + w - 1]) == (100, w, r, 400 * r)
    # P = 1 with W = 2^32: BITMAP exactly at 512 MiB; P = 2: SORT; P = 2^32 with W = 1: SORT
    assert auto(lib, [3, 3], FULL) == (dc.BITMAP, bitmap)
    assert auto(lib, [3, 4], FULL) == (dc.SORT, 2 * bitmap)
    assert auto(lib, FULL, [0, 0]) == (dc.SORT, 4 * 2**32)
    assert auto(lib, [0, 0] + FULL + [5, 5, -1, -1], [0, 0]) == (dc.SORT, 4 * 2**32)
    assert auto(lib, [0, 2**15 - 1, 0, 2**15 - 1], [0, 2**20 - 1]) == (dc.SORT, 4 * 2**30 * 2**15)
    for kb, vb in (([0, 9, 0, 9], [0, 64]), ([3, 3], FULL), ([0, 2**20 - 1], [0, 0])):
        a, ok = dc.paths_of(kb, vb, lds, bitmap)
        assert auto(lib, kb, vb) == (a, dc.shape(kb, vb)[3]) and ok[0] == a and ok[-1] == dc.SORT


def test_auto_refusals():
    lib = mq.load()
    who = b"mq_group_distinct_auto_path"
    assert auto(lib, FULL + [0, 1], [0, 0]) == (mq.MQ_EINVAL, 2**64 - 1) and b"2^32" in lib.mq_last_error()  # P = 2^33
    assert auto(lib, FULL + FULL + FULL + FULL, [0, 0])[0] == mq.MQ_EINVAL
    assert auto(lib, [1, 0], [0, 0]) == (mq.MQ_EINVAL, 0) and who in lib.mq_last_error()  # lo > hi
    assert auto(lib, [0, 1, 5, 4], [0, 0])[0] == mq.MQ_EINVAL
    assert auto(lib, [0, 1], [1, 0]) == (mq.MQ_EINVAL, 0)
    for nkeys in (0, 5, -1):
        assert auto(lib, [0, 1] * 5, [0, 0], nkeys=nkeys) == (mq.MQ_EINVAL, 0), nkeys
    v = (C.c_int32 * 2)(0, 0)
    assert lib.mq_group_distinct_auto_path(None, 1, v, None) == mq.MQ_EINVAL
    assert lib.mq_group_distinct_auto_path(v, 1, None, None) == mq.MQ_EINVAL
    assert lib.mq_group_distinct_auto_path(v, 1, v, None) == dc.LDS  # the byte count is optional


def test_model_against_a_set_of_tuples():
    """Tiny inputs: 1 to 4 key columns, 0 to 3 predicates, both int32 ends among keys and values,
    a key that is the value column, and a mask that matches nothing."""
    rng = np.random.default_rng(31)
    n = 200
    cols = [rng.integers(-20, 20, n).astype(np.int32) for _ in range(3)]
    keys = [rng.integers(-2, 2, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32),
            rng.integers(-1, 1, n).astype(np.int32), rng.integers(5, 7, n).astype(np.int32)]
    keys[0][5], keys[0][6], keys[1][7] = dc.I32_MIN, dc.I32_MAX, dc.I32_MAX
    vals = rng.integers(-3, 4, n).astype(np.int32)
    vals[5], vals[9] = dc.I32_MAX, dc.I32_MIN
    seen_empty = False
    for nkeys in (1, 2, 3, 4):
        for ranges in ([], [(-5, 12)], [(-5, 12), (None, 9), (-15, None)], [(3, 3), (None, None)], [(0, 5), (100, 200)]):
            for ks, v in ((keys[:nkeys], vals), (keys[:nkeys - 1] + [vals], vals)):
                got_keys, counts, rows, pairs = dc.model(cols[:len(ranges)], ranges, ks, v)
                order, want = dc.brute(cols[:len(ranges)], ranges, ks, v)
                assert list(zip(*[k.tolist() for k in got_keys])) == order
                assert counts.tolist() == want and counts.dtype == np.uint64
                assert [k.dtype for k in got_keys] == [np.int32] * nkeys
                assert pairs == sum(want) and rows == int(dc.mask(cols[:len(ranges)], ranges, n).sum())
                seen_empty |= len(order) == 0
    assert seen_empty
    # a key that is the value column: every count is 1
    assert set(dc.model([], [], [vals], vals)[1].tolist()) == {1}


def test_generators_are_what_they_claim():
    for span in dc.SPANS:
        keys, vals = dc.table(1025, [3, 4], -7, span, seed=span)
        ks, counts, rows, pairs = dc.model([], [], keys, vals)
        assert counts[0] == span and (ks[0][0], ks[1][0]) == (0, -2)
        assert vals.min() == -7 and vals.max() == -7 + span - 1
    assert dc.ROWS == sorted(dc.ROWS) and {0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 70_001} == set(dc.ROWS)


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device():
    lib = mq.load()
    h, groups = C.c_void_p(), C.c_uint64()
    ptrs = (C.c_void_p * 2)(None, None)
    assert lib.mq_group_distinct_plan(None, None, 0, ptrs, 2, None, 0, None, None, 0, C.byref(h), C.byref(groups), None,
                                      None) == mq.MQ_ENODEV
    assert lib.mq_group_distinct_write(None, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_group_distinct_free(None) == mq.MQ_ENODEV
