"""J4 bulk insert on the device: mq_hashset_insert must leave exactly the slots of the
sequential insert_hashset loop (refcpu.hashset_table; the reference's own loop where it
defines the case), whatever order the blocks run in, and mq_hashset_insert_many /
mq_hashset_insert_result must give the same table on the GPU path as on the host path."""
import ctypes as C

import numpy as np
import pytest

from hashsetcases import LISTS, expected_table, thirds
from refapi import _libc, free_result_struct, make_column, make_result, mq, take
from test_hashset import _bind, _elements, _table

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2**31, 2**31 - 1


@pytest.fixture(scope="module")
def lib():
    lib = _bind(mq.load())
    mq.check(lib.mq_init(0), "mq_init")
    return lib


class DevTable:
    """A `size`-slot table in HBM with the workspace for batches of up to max_n keys."""

    def __init__(self, lib, size: int, max_n: int, start=None):
        from devbuf import Dev
        self.lib, self.size = lib, size
        self.tab = Dev.of(np.zeros(size, np.int32) if start is None else np.asarray(start, np.int32))
        self.ws_bytes = lib.mq_hashset_insert_workspace_bytes(size, max_n)
        self.ws = Dev(self.ws_bytes)
        self.stored = Dev(8)

    def insert(self, keys) -> int:
        """One mq_hashset_insert of keys; returns *d_stored."""
        from devbuf import Dev
        keys = np.asarray(keys, dtype=np.int32)
        dk = Dev.of(keys)
        mq.check(self.lib.mq_hashset_insert(self.tab.ptr, self.size, dk.ptr, len(keys), self.stored.ptr,
                                            self.ws.ptr, self.ws_bytes, None), "mq_hashset_insert")
        stored = int(self.stored.get(np.uint64, 1)[0])  # syncs: dk may go now
        dk.free()
        return stored

    def table(self) -> np.ndarray:
        return self.tab.get(np.int32, self.size)


def _check(lib, refcpu, size, batches, want=None):
    """Insert the batches into one zeroed device table; the table after each batch and
    *d_stored against the restatement of the keys so far. Returns the final table."""
    dt = DevTable(lib, size, max(1, max(len(b) for b in batches)))
    sofar = []
    for b in batches:
        sofar += [int(k) for k in b]
        stored = dt.insert(b)
        t = dt.table()
        exp = refcpu.hashset_table(sofar, size)
        assert np.array_equal(t, exp), (size, len(sofar))
        assert stored == np.count_nonzero(exp)
    if want is not None:
        assert np.array_equal(t, want)
    return t


@pytest.mark.parametrize("calls", [1, 3])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_existing_lists(lib, refcpu, name, calls):
    size, keys = LISTS[name]
    want = expected_table(refcpu, size, keys)
    _check(lib, refcpu, size, [keys] if calls == 1 else thirds(keys), want)


def test_one_cluster_with_wrap_around(lib, refcpu):
    """Every key's home is slot 250 of 257: one cluster of 200 that wraps past the last
    slot, in a shuffled order with every fifth key repeated later."""
    size = 257
    rng = np.random.default_rng(3)
    keys = (257 * np.arange(1, 201) + 250).astype(np.int32)
    rng.shuffle(keys)
    keys = np.concatenate([keys, keys[::5]])
    rng.shuffle(keys[100:])
    want = expected_table(refcpu, size, keys.tolist())
    t = _check(lib, refcpu, size, [keys], want)
    assert np.count_nonzero(t) == 200 and t[250] == keys[0]


def test_heavy_duplicates(lib, refcpu):
    """4096 keys over 600 distinct values (0, negatives, INT32_MIN and INT32_MAX among
    them) into 1009 slots: without the reduction to first occurrences a later copy is
    evicted past a slot its earlier copy then settles in, and the key is stored twice."""
    size = 1009
    rng = np.random.default_rng(5)
    special = [0, I32_MIN, I32_MAX, -1, -1009, 1009]
    values = np.setdiff1d(np.concatenate([rng.integers(I32_MIN, I32_MAX, 700, dtype=np.int64),
                                          rng.integers(-3000, 3000, 200, dtype=np.int64)]), special)
    values = np.concatenate([special, rng.permutation(values)])[:600]
    assert len(np.unique(values)) == 600
    keys = values[rng.integers(0, 600, 4096)].astype(np.int32)
    keys[:600] = values  # every value occurs
    rng.shuffle(keys)
    t = _check(lib, refcpu, size, [keys])
    nz = t[t != 0]
    assert len(np.unique(nz)) == len(nz) == 599  # no value in two slots; 0 not stored


def test_overfull(lib, refcpu):
    size = 61
    rng = np.random.default_rng(7)
    keys = rng.permutation(np.arange(-100, 100))[:200].astype(np.int32)
    keys = keys[keys != 0]
    keys = np.concatenate([keys, [12345]])[:200].astype(np.int32)
    assert len(np.unique(keys)) == 200
    dt = DevTable(lib, size, 200)
    stored = dt.insert(keys)
    t = dt.table()
    assert np.array_equal(t, refcpu.hashset_table(keys.tolist(), size))
    assert stored == 61 and set(t.tolist()) == set(keys[:61].tolist())  # the first 61 distinct keys


def test_incremental(lib, refcpu):
    """Three batches into one device table = one batch; a batch that repeats resident
    keys and an all-zero batch change nothing."""
    size = 509
    rng = np.random.default_rng(9)
    keys = rng.integers(-5000, 5000, 330, dtype=np.int64).astype(np.int32)
    a, b, c = keys[:110], np.concatenate([keys[60:110], keys[110:220]]), keys[220:]
    whole = np.concatenate([a, b, c])
    one = _check(lib, refcpu, size, [whole])
    dt = DevTable(lib, size, 512)
    for batch in (a, b, c):
        dt.insert(batch)
    t = dt.table()
    assert np.array_equal(t, one)
    nz = np.count_nonzero(t)
    assert dt.insert(rng.permutation(t[t != 0])) == nz and np.array_equal(dt.table(), t)  # resident keys again
    assert dt.insert(np.zeros(300, np.int32)) == nz and np.array_equal(dt.table(), t)
    assert dt.insert(np.empty(0, np.int32)) == nz and np.array_equal(dt.table(), t)  # n = 0 counts only


def test_many_blocks_contending(lib, refcpu):
    """50,000 keys (about 10 % duplicates) over ~200 blocks into 65537 slots: the table,
    a lookup of every input key, and a second build byte for byte."""
    from devbuf import Dev
    size = 65537
    rng = np.random.default_rng(13)
    keys = rng.integers(I32_MIN, I32_MAX, 50_000, dtype=np.int64).astype(np.int32)
    dup = rng.choice(50_000, 5000, replace=False)
    keys[dup] = keys[rng.integers(0, 50_000, 5000)]
    keys[::997] = 0
    want = refcpu.hashset_table(keys.tolist(), size)
    tables = []
    for _ in range(2):
        dt = DevTable(lib, size, len(keys))
        stored = dt.insert(keys)
        tables.append(dt.table())
        assert stored == np.count_nonzero(want)
    assert np.array_equal(tables[0], want)
    assert tables[0].tobytes() == tables[1].tobytes()
    dk, df = Dev.of(keys), Dev(len(keys))
    mq.check(lib.mq_hashset_lookup(dt.tab.ptr, size, dk.ptr, len(keys), df.ptr, None))
    assert np.array_equal(df.get(np.uint8, len(keys)).astype(bool), keys != 0)


def test_arguments(lib):
    from devbuf import Dev
    size = 16
    start = np.zeros(size, np.int32)
    start[3] = 3
    dt = DevTable(lib, size, 4, start)
    dk = Dev.of(np.array([1, 2, 3, 4], np.int32))
    ins = lib.mq_hashset_insert
    ws, wsb = dt.ws.ptr, dt.ws_bytes
    assert ins(dt.tab.ptr, size, None, 0, None, None, 0, None) == mq.MQ_OK  # n = 0: no keys, no workspace
    assert ins(dt.tab.ptr, size, dk.ptr, 0, dt.stored.ptr, ws, wsb, None) == mq.MQ_OK
    assert int(dt.stored.get(np.uint64, 1)[0]) == 1
    assert ins(dt.tab.ptr, 0, dk.ptr, 4, None, ws, wsb, None) == mq.MQ_EINVAL
    assert ins(dt.tab.ptr, -5, dk.ptr, 4, None, ws, wsb, None) == mq.MQ_EINVAL
    assert ins(None, size, dk.ptr, 4, None, ws, wsb, None) == mq.MQ_EINVAL
    assert ins(dt.tab.ptr, size, None, 4, None, ws, wsb, None) == mq.MQ_EINVAL
    assert ins(dt.tab.ptr, size, dk.ptr, 2**32 - 1, None, ws, wsb, None) == mq.MQ_EINVAL
    assert ins(dt.tab.ptr, size, dk.ptr, 4, None, ws, wsb - 1, None) == mq.MQ_EINVAL
    assert ins(dt.tab.ptr, size, dk.ptr, 4, None, None, wsb, None) == mq.MQ_EINVAL
    assert b"mq_hashset_insert" in lib.mq_last_error()
    assert np.array_equal(dt.table(), start)  # none of the above touched the table
    assert ins(dt.tab.ptr, size, dk.ptr, 4, None, ws, wsb, None) == mq.MQ_OK  # d_stored may be NULL
    assert np.array_equal(dt.table(), [0, 1, 2, 3, 4] + [0] * 11)
    assert lib.mq_hashset_insert_workspace_bytes(size, 4) >= size * 8 + 8 * 8


def _drop_in_keys():
    rng = np.random.default_rng(17)
    keys = rng.integers(I32_MIN, I32_MAX, 40_000, dtype=np.int64).astype(np.int32)
    keys[1::7] = keys[::7][: len(keys[1::7])]  # duplicates
    keys[::501] = 0
    return keys


def test_drop_in_gpu_path(lib, refcpu, monkeypatch):
    """mq_hashset_insert_many with the threshold lowered (MQ_HASHSET_GPU_MIN is read per
    call) against the same call on the host path, in two calls into one set; the GPU
    path moves the table over PCIe (mq_transfer_seconds), the host path moves nothing."""
    size = 65537
    keys = _drop_in_keys()
    tables = {}
    for path, gpu_min in (("gpu", "1"), ("host", str(2**40))):
        monkeypatch.setenv("MQ_HASHSET_GPU_MIN", gpu_min)
        hs = lib.create_hashset(size)
        lib.mq_transfer_seconds(1)
        for part in (keys[:25_000], keys[25_000:]):
            assert lib.mq_hashset_insert_many(hs, part.ctypes.data, len(part)) == 0
        assert (lib.mq_transfer_seconds(1) > 0) == (path == "gpu")
        tables[path] = _table(hs)
        monkeypatch.setenv("MQ_HASHSET_GPU_MIN", "32768")  # the listing on the GPU for both
        assert np.array_equal(_elements(lib, hs), refcpu.hashset_elements(tables[path]))
        lib.free_hashset(hs)
    assert np.array_equal(tables["gpu"], tables["host"])
    assert np.array_equal(tables["gpu"], refcpu.hashset_table(keys.tolist(), size))


def test_drop_in_result_from_fetch(lib, refcpu, monkeypatch):
    """mq_hashset_insert_result of a fetch_column's output: the keys come from the
    Result's HBM shadow when one is resident (no second upload), and the table equals
    the host path's."""
    size = 1_000_003
    rng = np.random.default_rng(19)
    data = rng.integers(I32_MIN, I32_MAX, 400_000, dtype=np.int64).astype(np.int32)
    data[::11] = data[5]
    col = make_column(data)
    pos = make_result(np.arange(0, 400_000, dtype=np.int32))
    st = mq.Status(0, None)
    r = lib.fetch_column(C.byref(col), C.byref(pos), C.byref(st))
    assert st.code == mq.OK and r and r.contents.num_tuples == 400_000
    monkeypatch.setenv("MQ_HASHSET_GPU_MIN", "1")
    tiny = make_result(np.array([1, 2], dtype=np.int32))
    assert take(lib.min(C.byref(tiny), C.byref(st)))[0] == 1  # another operator: what only fetch_column could use is gone
    free_result_struct(tiny)
    resident = bool(lib.mq_result_device_ptr(r))  # a guarded shadow outlives its operator
    before = mq.residency(lib)["result_uploads"]
    hs = lib.create_hashset(size)
    assert lib.mq_hashset_insert_result(hs, r) == 0
    assert mq.residency(lib)["result_uploads"] - before == (0 if resident else 1)
    got = _table(hs)
    lib.free_hashset(hs)
    monkeypatch.setenv("MQ_HASHSET_GPU_MIN", str(2**40))
    hs = lib.create_hashset(size)
    assert lib.mq_hashset_insert_result(hs, r) == 0
    assert np.array_equal(got, _table(hs))
    nz = got[got != 0]
    assert len(np.unique(nz)) == len(nz) == len(np.unique(data[data != 0]))
    lib.free_hashset(hs)
    lib.mq_column_invalidate(C.byref(col))
    _libc.free(r.contents.payload)
    _libc.free(C.cast(r, C.c_void_p))
    free_result_struct(pos)
