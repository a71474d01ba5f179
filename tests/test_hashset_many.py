"""J4 bulk inserts on the host path: mq_hashset_insert_many and mq_hashset_insert_result
below MQ_HASHSET_GPU_MIN keys run insert_hashset's loop, so the table must equal
refcpu.hashset_table, the key-by-key insert_hashset table and, where the reference
defines the case, the reference's own loop. Every list of test_hashset.py, in one call
and in three consecutive calls into one set."""
import ctypes as C

import numpy as np
import pytest

from hashsetcases import LISTS, expected_table, thirds
from refapi import free_result_struct, make_result, mq
from test_hashset import _bind, _elements, _table


@pytest.fixture(scope="module")
def lib():
    return _bind(mq.load())


def _many(lib, hs, keys):
    a = np.asarray(keys, dtype=np.int32)
    assert lib.mq_hashset_insert_many(hs, a.ctypes.data if len(a) else None, len(a)) == 0


def _result(lib, hs, keys):
    r = make_result(np.asarray(keys, dtype=np.int32))
    assert lib.mq_hashset_insert_result(hs, C.byref(r)) == 0
    free_result_struct(r)


def _one_by_one(lib, size, keys):
    hs = lib.create_hashset(size)
    for k in keys:
        lib.insert_hashset(hs, int(k))
    t = _table(hs)
    lib.free_hashset(hs)
    return t


@pytest.mark.parametrize("insert", [_many, _result], ids=["many", "result"])
@pytest.mark.parametrize("calls", [1, 3])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_bulk_insert_host_path(lib, refcpu, name, calls, insert):
    size, keys = LISTS[name]
    want = expected_table(refcpu, size, keys)
    hs = lib.create_hashset(size)
    for batch in ([keys] if calls == 1 else thirds(keys)):
        insert(lib, hs, batch)
    t = _table(hs)
    assert np.array_equal(t, want), name
    assert np.array_equal(t, _one_by_one(lib, size, keys)), name
    for k in set(keys) | {0, 1, size, 2 * size + 1}:
        assert bool(lib.lookup_hashset(hs, k)) == refcpu.hashset_lookup(want, k), (name, k)
    assert np.array_equal(_elements(lib, hs), refcpu.hashset_elements(want)), name
    lib.free_hashset(hs)


def test_bulk_insert_arguments(lib):
    hs = lib.create_hashset(8)
    keys = np.array([3, 11, 19], dtype=np.int32)
    assert lib.mq_hashset_insert_many(None, keys.ctypes.data, 3) == mq.MQ_EINVAL
    assert lib.mq_hashset_insert_many(hs, None, 3) == mq.MQ_EINVAL
    assert lib.mq_hashset_insert_many(hs, None, 0) == 0
    assert lib.mq_hashset_insert_result(hs, None) == mq.MQ_EINVAL
    r = make_result(np.array([1.5], dtype=np.float64), mq.DOUBLE)
    assert lib.mq_hashset_insert_result(hs, C.byref(r)) == mq.MQ_EINVAL
    free_result_struct(r)
    assert not _table(hs).any()  # nothing above stored a key
    empty = make_result(np.empty(0, dtype=np.int32))
    assert lib.mq_hashset_insert_result(hs, C.byref(empty)) == 0
    free_result_struct(empty)
    assert not _table(hs).any()
    lib.free_hashset(hs)
