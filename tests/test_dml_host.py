"""relational_delete / relational_update and the device entry points behind them:
what holds on any machine. The names are declared in the headers, exported by
libmq.so and bound by mq.py; the numpy restatement the GPU tests compare against
agrees with itself; and without a device both operators answer ERROR and leave every
column, count and index as they were (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import dmlcases as dc
from refapi import make_result, free_result_struct, mq

DEVICE_API = ["mq_delete_workspace_bytes", "mq_dml_geometry", "mq_delete_plan", "mq_delete_columns", "mq_delete_index",
              "mq_update_rows"]
DROPIN_API = ["relational_delete", "relational_update"]


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
    assert all(f"void {n}(" in qry_h for n in DROPIN_API)


def test_workspace_size_needs_no_device():
    lib = mq.load()
    sizes = [lib.mq_delete_workspace_bytes(n) for n in (0, 1, 4096, 4097, 10**6, 2**31 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    # one bit per row and one u32 per 64 rows, plus a fixed part
    assert sizes[-1] < (2**31) * 3 // 16 + (1 << 20)


def _geometry(lib, n):
    pb, pc, ib, ic_ = C.c_uint32(77), C.c_uint64(77), C.c_uint32(77), C.c_uint64(77)
    lib.mq_dml_geometry(n, C.byref(pb), C.byref(pc), C.byref(ib), C.byref(ic_))
    return (pb.value, pc.value), (ib.value, ic_.value)


def test_geometry_needs_no_device():
    """(blocks, chunk) of the word prefix and of the index pass, pinned: chunks() of
    mq_scan_common.h over the bitmap words + 1 in 256-word steps on at most 1024 blocks,
    and over the entries in 1024-entry steps on at most 2048 blocks. The prefix takes a
    second step a block from 16 773 121 rows on, the index pass from 2 097 153."""
    lib = mq.load()
    assert _geometry(lib, 16_773_120)[0] == (1024, 256)
    assert _geometry(lib, 16_773_121)[0] == (513, 512)
    assert _geometry(lib, 2**24 + 5) == ((513, 512), (1821, 9216))
    assert _geometry(lib, 2_097_152)[1] == (2048, 1024)
    assert _geometry(lib, 2_097_153)[1] == (1025, 2048)
    assert _geometry(lib, 4_195_333)[1] == (1366, 3072)
    assert _geometry(lib, 2**20 + 5) == ((65, 256), (1025, 1024))  # the largest of dc.SIZES: one step a block
    assert _geometry(lib, 0) == ((1, 256), (1, 1024))
    lib.mq_dml_geometry(5000, None, None, None, None)  # any output may be NULL
    assert dc.BIG_N == 2**24 + 5 and dc.INDEX_N == [2_097_153, 4_195_333]


def test_big_cases_are_what_they_say():
    """dmlcases.big_delete_set / big_index at a small size with a two-step chunk: in the
    picked chunks first_steps deletes every row of the first step's words and none of the
    second's, second_steps is its complement, and big_index is a sorted index with ties
    over a permutation."""
    cw = 2 * dc.PREFIX_STEP
    n = 8 * cw * 64 + 77
    first, second = dc.big_delete_set("first_steps", n, cw), dc.big_delete_set("second_steps", n, cw)
    assert np.array_equal(np.sort(np.concatenate([first, second])), np.arange(n))
    gone = np.zeros(n, dtype=bool)
    gone[first] = True
    step = dc.PREFIX_STEP * 64
    for c in (0, 1, 7, 4, 6):
        assert gone[c * 2 * step:c * 2 * step + step].all() and not gone[c * 2 * step + step:(c + 1) * 2 * step].any()
    assert 0.2 < gone[2 * 2 * step:3 * 2 * step].mean() < 0.4
    for name, frac in (("random_50pct", 0.5), ("random_1pct", 0.01)):
        ids = dc.big_delete_set(name, n, cw)
        assert np.all(np.diff(ids) > 0) and abs(len(ids) / n - frac) < 0.01
    v, p = dc.big_index(n, clustered=False)
    assert np.all(v[1:] >= v[:-1]) and len(np.unique(v)) == 1000
    assert np.array_equal(np.sort(p), np.arange(n, dtype=np.uint64)) and not np.array_equal(p, np.arange(n))
    assert np.array_equal(dc.big_index(n, clustered=True)[1], np.arange(n, dtype=np.uint64))


def test_model_is_consistent():
    """The restatement against a row-by-row Python loop, on a small table."""
    cols = dc.table(300, 3)
    ids = dc.delete_sets(300)["random_50pct"]
    keep = [r for r in range(300) if r not in set(ids.tolist())]
    for order in dc.ORDERS:
        pos = dc.position_list(ids, order, seed=1)
        assert len(pos) == 2 * len(ids) and set(pos.tolist()) == set(ids.tolist())
        assert np.array_equal(dc.delete_rows(cols, pos), cols[:, keep])
    v, p = dc.index_of(cols[0])
    nv, np_ = dc.delete_index(v, p, ids, 300)
    new_col = cols[0][keep]
    assert np.all(nv[1:] >= nv[:-1]) and np.array_equal(new_col[np_.astype(np.int64)], nv)
    assert np.array_equal(np.sort(np_), np.arange(len(keep), dtype=np.uint64))
    up = dc.update_rows(cols[1], [3, 3, 299, -1, 300], 8)
    assert up[3] == up[299] == 8 and np.array_equal(np.delete(up, [3, 299]), np.delete(cols[1], [3, 299]))


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device_nothing_changes(capfd):
    lib = mq.load()
    model = dc.tbl5(500)
    bufs = [np.ascontiguousarray(c) for c in model.copy()]
    db, t, cs = dc.make_db(bufs, index_col=0)
    # an index as build_index would leave it (malloc'd arrays are not needed: never freed here)
    v, p = dc.index_of(bufs[0])
    v, p = np.ascontiguousarray(v), np.ascontiguousarray(p.astype(np.uintp))
    ix = mq.ColumnIndex(v.ctypes.data_as(C.POINTER(C.c_int)), p.ctypes.data_as(C.POINTER(C.c_size_t)))
    cs[0].index = C.pointer(ix)
    v0, p0 = v.copy(), p.copy()
    r = make_result(np.array([1, 2, 3], np.int32))
    assert lib.mq_delete_plan(None, 0, 0, None, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_update_rows(None, 0, None, 0, 0, None, None) == mq.MQ_ENODEV
    for call in (lambda st: lib.relational_delete(C.byref(t), C.byref(r), C.byref(st)),
                 lambda st: lib.relational_update(C.byref(cs[1]), C.byref(r), -10, C.byref(st)),
                 lambda st: lib.relational_update(C.byref(cs[0]), C.byref(r), -10, C.byref(st))):
        st = mq.Status(0, None)
        call(st)
        assert st.code == mq.ERROR
        assert "libmq" in capfd.readouterr().err
        assert t.row_count == 500 and all(cs[j].row_count == 500 for j in range(4))
        assert np.array_equal(np.stack(bufs), model)
        assert np.array_equal(v, v0) and np.array_equal(p, p0)
        assert (cs[1].min, cs[1].max) == (int(model[1].min()), int(model[1].max()))
    free_result_struct(r)
