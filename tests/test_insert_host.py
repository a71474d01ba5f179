"""relational_insert and the device entry points behind it: what holds on any machine.
The names are declared in the headers, exported by libmq.so and bound by mq.py; the
workspace size needs no device; the numpy restatement the GPU tests compare against
agrees with a row-by-row loop; and without a device the operator answers ERROR and leaves
every row, count, min / max and index array as it was (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import dmlcases as dc
import insertcases as ic
from refapi import mq

DEVICE_API = ["mq_insert_workspace_bytes", "mq_insert_points", "mq_insert_plan", "mq_insert_columns",
              "mq_insert_index", "mq_insert_slots", "mq_insert_positions"]
DROPIN_API = ["relational_insert"]


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
    assert not hasattr(lib, "insert_row")  # the server's db_manager.o defines it


def test_workspace_size_needs_no_device():
    lib = mq.load()
    ns = (0, 1, 4096, 4097, 10**6, 2**30)
    for k in (0, 1, 4097, 2**30 - 1):
        sizes = [lib.mq_insert_workspace_bytes(n, k) for n in ns]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
        sizes = [lib.mq_insert_workspace_bytes(k, n) for n in ns]
        assert sizes == sorted(sizes)
        # one bit per output slot and one u32 per 64 slots, plus a fixed part
        assert all(lib.mq_insert_workspace_bytes(n, k) < 3 * (n + k) // 16 + (1 << 20) for n in ns)


def test_model_is_consistent():
    """The restatement against a row-by-row Python loop, on a 300-row table."""
    n, k = 300, 120
    rng = np.random.default_rng(3)
    cols = dc.table(n, 3)
    cols[0] = np.sort(rng.integers(0, 40, n)).astype(np.int32)  # the clustered keys, with repeats
    cols[1] = rng.integers(0, 25, n)
    new = np.stack([rng.integers(-3, 44, k), rng.integers(-2, 27, k), rng.integers(0, 9, k)]).astype(np.int32)
    # append: insert_row k times
    rows = [list(r) for r in cols.T]
    for r in new.T:
        rows.append(list(r))
    assert np.array_equal(ic.insert_rows(cols, None, new), np.array(rows, dtype=np.int32).T)
    # sorted insert: each new row lands after every row (old, or inserted before it) with key <= its own
    rows, slot_of = [list(r) for r in cols.T], []
    tags = [("old", i) for i in range(n)]
    for b, r in enumerate(new.T):
        at = max([i + 1 for i, q in enumerate(rows) if q[0] <= r[0]], default=0)
        rows.insert(at, list(r))
        tags.insert(at, ("new", b))
    want = np.array(rows, dtype=np.int32).T
    got = ic.insert_rows(cols, cols[0], new, key_col=0)
    assert np.array_equal(got, want) and np.all(got[0][1:] >= got[0][:-1])
    points, slots = ic.new_slots(cols[0], new[0])
    assert np.all(points[1:] >= points[:-1]) and points.max() <= n
    assert [tags.index(("new", b)) for b in range(k)] == slots.tolist()
    order = np.argsort(new[0], kind="stable")
    for j in range(3):  # the same interleave from the insertion points, as the device expands it
        assert np.array_equal(ic.expand(cols[j], points, new[j][order]), want[j])
    # an unclustered index on column 1: merged one entry at a time, renumbered and not
    v, p = dc.index_of(cols[1])
    old_slot = np.array([tags.index(("old", i)) for i in range(n)], dtype=np.uint64)
    for new_pos, ren, old_pos in ((slots, points, old_slot[p.astype(np.int64)]),
                                  (np.arange(n, n + k, dtype=np.uint64), None, p)):
        ev, ep = v.tolist(), old_pos.tolist()
        for b in range(k):
            at = max([i + 1 for i, q in enumerate(ev) if q <= new[1][b]], default=0)
            ev.insert(at, int(new[1][b]))
            ep.insert(at, int(new_pos[b]))
        gv, gp = ic.insert_index(v, p, new[1], new_pos, ren)
        assert gv.tolist() == ev and gp.tolist() == ep
        table = want if ren is not None else ic.insert_rows(cols, None, new)
        assert np.array_equal(table[1][gp.astype(np.int64)], gv)
        assert np.array_equal(np.sort(gp), np.arange(n + k, dtype=np.uint64))


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device_nothing_changes(capfd):
    lib = mq.load()
    model = dc.tbl5(500)
    bufs = [np.ascontiguousarray(np.concatenate([c, np.full(100, 7, np.int32)])) for c in model]
    before = np.stack(bufs).copy()
    db, t, cs = ic.make_db(bufs, 500, index_col=0)
    # an index as build_index would leave it (malloc'd arrays are not needed: never freed here)
    v, p = dc.index_of(bufs[0][:500])
    v, p = np.ascontiguousarray(v), np.ascontiguousarray(p.astype(np.uintp))
    ix = mq.ColumnIndex(v.ctypes.data_as(C.POINTER(C.c_int)), p.ctypes.data_as(C.POINTER(C.c_size_t)))
    cs[0].index = C.pointer(ix)
    v0, p0 = v.copy(), p.copy()
    assert lib.mq_insert_points(None, 0, None, 0, None, None) == mq.MQ_ENODEV
    assert lib.mq_insert_plan(None, 0, 0, None, None, 0, None) == mq.MQ_ENODEV
    assert lib.mq_insert_columns(None, None, None, 0, None, None) == mq.MQ_ENODEV
    assert lib.mq_insert_index(None, None, None, None, None, None, 0, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_insert_slots(None, None, 0, None, None) == mq.MQ_ENODEV
    assert lib.mq_insert_positions(None, 0, None, 0, None, None) == mq.MQ_ENODEV
    rows = np.ascontiguousarray(ic.MILESTONE5_ROWS)
    for k in (1, 5):
        st = mq.Status(0, None)
        lib.relational_insert(C.byref(db), C.byref(t), rows.ctypes.data_as(C.POINTER(C.c_int)), k, C.byref(st))
        assert st.code == mq.ERROR
        assert "libmq" in capfd.readouterr().err
        assert t.row_count == 500 and t.table_length == 600 and all(cs[j].row_count == 500 for j in range(4))
        assert np.array_equal(np.stack(bufs), before)
        assert np.array_equal(v, v0) and np.array_equal(p, p0)
        assert all((cs[j].min, cs[j].max) == (int(model[j].min()), int(model[j].max())) for j in range(4))
