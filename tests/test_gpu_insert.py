"""Batched row inserts on gfx950 (csrc/mq_dml.hip; relational_insert in mq_query.c), every
comparison exact equality with the numpy restatement in insertcases.py: the reference's
insert_row (db_manager.c:164-199) issued once per row, with the clustered order and the
sorted indexes maintained as the workload generator expects (milestone5.py:40-78).

Which regime each size reaches: ic.SIZES (up to 2^20 + 5 old rows) cover the expansion's
tiles and alignments with one step a block in the plan's word prefix. At n + k = 2^24 + 5
slots every block of the prefix takes two steps (asserted from mq_dml_geometry), for
mq_insert_columns and mq_insert_index alike. The grid-stride kernels (k_ins_points,
k_ins_slots, k_ins_positions, k_ins_index) take one loop step at every size here; past one
step they run in test_gpu_regimes.py under a CU limit.
"""
import ctypes as C

import numpy as np
import pytest

import dmlcases as dc
import insertcases as ic
from devbuf import Dev
from refapi import make_result, free_result_struct, mq, take
from test_gpu_dml import (FILL32, FILL64, Tbl, check_index, filled, lib, memfd_array, ptr_array,  # noqa: F401 (lib: fixture)
                          two_prefix_steps)

pytestmark = pytest.mark.gpu


def plan(L, ws, points: np.ndarray, n: int):
    d = Dev.of(points.astype(np.uint32))
    bad = C.c_uint64(~0)
    rc = L.mq_insert_plan(d.ptr, len(points), n, C.byref(bad), ws.ptr, ws.nbytes, None)
    return rc, bad.value


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

def expand_and_check(L, cols, points, new, in_off=lambda j: 0, out_off=lambda j: j % 4, tag=()):
    ncols, n = cols.shape
    k = len(points)
    m = n + k
    ws = Dev(L.mq_insert_workspace_bytes(n, k))
    rc, bad = plan(L, ws, points, n)
    assert (rc, bad) == (mq.MQ_OK, 0), tag
    dold = [Dev.of(cols[j], offset_elems=in_off(j)) for j in range(ncols)]
    dnew = [Dev.of(new[j], offset_elems=(in_off(j) * 3) % 4) for j in range(ncols)]
    outs = [Dev.of(np.full(m + 8, -7, np.int32), offset_elems=out_off(j)) for j in range(ncols)]
    mq.check(L.mq_insert_columns(ws.ptr, ptr_array(dold), ptr_array(dnew), ncols, ptr_array(outs), None),
             "mq_insert_columns")
    for j in range(ncols):
        got = outs[j].get(np.int32, m + 8)
        assert np.array_equal(got[:m], ic.expand(cols[j], points, new[j])), tag + (j,)
        assert np.all(got[m:] == -7), tag + (j, "wrote past the end")


@pytest.mark.parametrize("ncols", ic.NCOLS)
@pytest.mark.parametrize("n", ic.SIZES)
def test_insert_columns(lib, n, ncols):
    """Every insertion pattern: each column bit-equal to the restatement. Column 1 (old
    and new values) sits 4 bytes off a 16-byte boundary, and the outputs start 0, 1, 2, 3
    dwords off one."""
    cols = dc.table(n, ncols)
    for name, points in ic.insertion_points(n).items():
        new = dc.table(len(points), ncols, seed=1)
        expand_and_check(lib, cols, points, new, in_off=lambda j: 1 if j == 1 else 0, tag=(name,))


def test_insert_columns_70(lib):
    """More columns than one launch carries pointers for (64)."""
    n = 5000
    points = ic.insertion_points(n)["random_50pct"]
    expand_and_check(lib, dc.table(n, 70), points, dc.table(len(points), 70, seed=1), in_off=lambda j: j % 4)


@pytest.mark.parametrize("n", [0, 1, 5, 64, 4097, 100_003])
def test_insert_points(lib, n):
    rng = np.random.default_rng(n)
    lo, hi = -2**31, 2**31 - 1
    old = rng.integers(-40, 40, n) * 3  # duplicates
    if n >= 5:
        old[:2], old[-2:] = lo, hi
    old = np.sort(old).astype(np.int32)
    new = np.concatenate([rng.integers(-130, 130, 300), [lo, lo, hi, hi, -121, 121, 0]])  # below, above, between
    new = np.sort(new).astype(np.int32)
    dold, dnew, dins = Dev.of(old), Dev.of(new), Dev.of(np.full(len(new) + 2, 77, np.uint32))
    mq.check(lib.mq_insert_points(dold.ptr if n else None, n, dnew.ptr, len(new), dins.ptr, None), "mq_insert_points")
    got = dins.get(np.uint32, len(new) + 2)
    assert np.array_equal(got[:-2], np.searchsorted(old, new, side="right"))
    assert np.all(got[-2:] == 77)
    assert np.all(got[1:-2] >= got[:-3])


@pytest.mark.parametrize("n", [0, 1, 65, 4097, 100_003])
def test_insert_index(lib, n):
    """An index with many equal values, the positions among them shuffled; the new entries
    carry rows n.. (an append) or their slots of a sorted insert, whose points renumber the
    old positions. mq_insert_slots / mq_insert_positions give those rows."""
    check_insert_index(lib, n, max(n // 3, 7))


def check_insert_index(lib, n, k):
    rng = np.random.default_rng(n)
    key = (rng.permutation(n) % 11).astype(np.int32)
    shuf = rng.permutation(n)
    p = shuf[np.argsort(key[shuf], kind="stable")]
    v, p = key[p], p.astype(np.uint64)
    new_v = rng.integers(-2, 13, k).astype(np.int32)            # the indexed column's new values, batch order
    tkeys_old = np.sort(rng.integers(0, 50, n)).astype(np.int32)  # the table's clustered keys
    tkeys_new = rng.integers(-5, 55, k).astype(np.int32)
    tpoints, slots = ic.new_slots(tkeys_old, tkeys_new)
    torder = np.argsort(tkeys_new, kind="stable").astype(np.uint64)
    order = np.argsort(new_v, kind="stable").astype(np.uint64)    # mq_index_build's positions
    points = np.searchsorted(v, new_v[order.astype(np.int64)], side="right").astype(np.uint32)
    ws = Dev(lib.mq_insert_workspace_bytes(n, k))
    assert plan(lib, ws, points, n) == (mq.MQ_OK, 0)
    dv, dp, dnv = Dev.of(v), Dev.of(p), Dev.of(new_v[order.astype(np.int64)])
    dtp, dto, dord = Dev.of(tpoints), Dev.of(torder), Dev.of(order)
    dslots, dnp = Dev.of(np.full(k + 1, 5, np.uint64)), Dev.of(np.full(k + 1, 5, np.uint64))
    mq.check(lib.mq_insert_slots(dtp.ptr, dto.ptr, k, dslots.ptr, None), "mq_insert_slots")
    got = dslots.get(np.uint64, k + 1)
    assert np.array_equal(got[:k], slots) and got[k] == 5
    for d_slots, new_rows, ren, kren in ((dslots.ptr, slots, tpoints, k),
                                         (None, np.arange(n, n + k, dtype=np.uint64), None, 0)):
        mq.check(lib.mq_insert_positions(d_slots, n, dord.ptr, k, dnp.ptr, None), "mq_insert_positions")
        got = dnp.get(np.uint64, k + 1)
        assert np.array_equal(got[:k], new_rows[order.astype(np.int64)]) and got[k] == 5
        ov, op = Dev.of(np.full(n + k + 2, -7, np.int32)), Dev.of(np.full(n + k + 2, 7, np.uint64))
        mq.check(lib.mq_insert_index(ws.ptr, dv.ptr, dp.ptr, dnv.ptr, dnp.ptr, dtp.ptr if kren else None, kren,
                                     ov.ptr, op.ptr, None), "mq_insert_index")
        wv, wp = ic.insert_index(v, p, new_v, new_rows, ren)
        gv, gp = ov.get(np.int32, n + k + 2), op.get(np.uint64, n + k + 2)
        assert np.array_equal(gv[:n + k], wv) and np.array_equal(gp[:n + k], wp)
        assert np.all(gv[n + k:] == -7) and np.all(gp[n + k:] == 7)
        assert np.array_equal(np.sort(gp[:n + k]), np.arange(n + k, dtype=np.uint64))


# ---------------------------------------------------------------------------
# past one step a block
#
# mq_insert_plan shares the delete's word prefix (k_dml_word_sums / _prefix) over the
# n + k output slots. At every size of ic.SIZES a block's chunk of bitmap words is one
# step long; at n + k = dc.BIG_N every block takes two and `base += total` carries the
# first step's count into the second (mq_dml_geometry, asserted by two_prefix_steps).
# ---------------------------------------------------------------------------
BIG_K = {"front": 1000, "append": 1000, "random": 1000, "half": ic.BIG_HALF_K}


@pytest.mark.parametrize("name", list(BIG_K))
def test_insert_columns_two_prefix_steps(lib, name):
    """mq_insert_plan + mq_insert_columns at n + k = dc.BIG_N slots: 1000 new rows at the
    front, appended and at random points, and k = n / 2 at sorted random points; one
    aligned column and one 4 bytes off, each equal to the restatement, nothing written past
    the end."""
    k = BIG_K[name]
    n = dc.BIG_N - k
    two_prefix_steps(lib, n + k)
    points = ic.big_points(name, n, k)
    expand_and_check(lib, dc.table(n, 2), points, dc.table(k, 2, seed=1), in_off=lambda j: j, tag=(name,))


@pytest.mark.parametrize("name", ["random", "half"])
def test_insert_index_two_prefix_steps(lib, name):
    """mq_insert_index with renumbering at n + k = dc.BIG_N entries, on dc.big_index's tied
    values and permuted positions, against ic.insert_index. The table's rows were
    interleaved by a sorted insert of their own (mq_insert_slots gives the new rows' slots,
    mq_insert_positions files them in the index's order)."""
    k = BIG_K[name]
    n = dc.BIG_N - k
    m = n + k
    two_prefix_steps(lib, m)
    rng = np.random.default_rng(k)
    v, p = dc.big_index(n, clustered=False)
    # the indexed column's new values, batch order; for k = n / 2 already ascending, so that
    # neither the test nor the model sorts millions of rows
    new_v = rng.integers(-2, 1002, k).astype(np.int32)
    if name == "half":
        new_v.sort()
    order = np.argsort(new_v, kind="stable").astype(np.uint64)
    points = np.searchsorted(v, new_v[order.astype(np.int64)], side="right").astype(np.uint32)
    # the table's clustered keys: ascending old keys, new keys in batch order
    tkeys_old = (np.arange(n, dtype=np.int64) * 50 // n).astype(np.int32)
    tkeys_new = rng.integers(-5, 55, k).astype(np.int32)
    tpoints, slots = ic.new_slots(tkeys_old, tkeys_new)
    torder = np.argsort(tkeys_new, kind="stable").astype(np.uint64)
    ws = Dev(lib.mq_insert_workspace_bytes(n, k))
    assert plan(lib, ws, points, n) == (mq.MQ_OK, 0)
    dv, dp, dnv = Dev.of(v), Dev.of(p), Dev.of(new_v[order.astype(np.int64)])
    dtp, dto, dord = Dev.of(tpoints), Dev.of(torder), Dev.of(order)
    dslots, dnp = Dev.of(np.full(k + 1, 5, np.uint64)), Dev.of(np.full(k + 1, 5, np.uint64))
    mq.check(lib.mq_insert_slots(dtp.ptr, dto.ptr, k, dslots.ptr, None), "mq_insert_slots")
    got = dslots.get(np.uint64, k + 1)
    assert np.array_equal(got[:k], slots) and got[k] == 5
    mq.check(lib.mq_insert_positions(dslots.ptr, n, dord.ptr, k, dnp.ptr, None), "mq_insert_positions")
    got = dnp.get(np.uint64, k + 1)
    assert np.array_equal(got[:k], slots[order.astype(np.int64)]) and got[k] == 5
    ov, op = filled(lib, m + 4, np.int32), filled(lib, m + 4, np.uint64)
    mq.check(lib.mq_insert_index(ws.ptr, dv.ptr, dp.ptr, dnv.ptr, dnp.ptr, dtp.ptr, k, ov.ptr, op.ptr, None),
             "mq_insert_index")
    wv, wp = ic.insert_index(v, p, new_v, slots, tpoints)
    gv, gp = ov.get(np.int32, m + 4), op.get(np.uint64, m + 4)
    assert np.array_equal(gv[:m], wv) and np.array_equal(gp[:m], wp)
    assert np.all(gv[m:].view(np.uint32) == FILL32) and np.all(gp[m:] == FILL64)


def test_error_codes(lib):
    n, k = 1000, 4
    ws = Dev(lib.mq_insert_workspace_bytes(n, k))
    old, new = Dev.of(np.arange(n, dtype=np.int32)), Dev.of(np.arange(k, dtype=np.int32))
    out = Dev.of(np.full(n + k, -7, np.int32))
    p64, o64 = Dev.of(np.arange(n, dtype=np.uint64)), Dev.of(np.full(n + k, 7, np.uint64))
    n64 = Dev.of(np.arange(k, dtype=np.uint64))
    cols = lambda: lib.mq_insert_columns(ws.ptr, ptr_array([old]), ptr_array([new]), 1, ptr_array([out]), None)
    index = lambda: lib.mq_insert_index(ws.ptr, old.ptr, p64.ptr, new.ptr, n64.ptr, None, 0, out.ptr, o64.ptr, None)
    # descending points, or points > n: counted, and no plan is left (not an earlier one
    # either): the apply steps refuse, outputs untouched
    for points, nbad in (([3, 2, 5, 4], 2), ([1, 2, 3, n + 1], 1), ([n + 5, 0, 0, 0], 2)):
        rc, bad = plan(lib, ws, np.array(points, np.uint32), n)
        assert (rc, bad) == (mq.MQ_EINVAL, nbad)
        assert cols() == mq.MQ_EINVAL and index() == mq.MQ_EINVAL
        assert np.all(out.get(np.int32, n + k) == -7) and np.all(o64.get(np.uint64, n + k) == 7)
    ins = Dev.of(np.array([0, 5, 5, n], np.uint32))
    bad = C.c_uint64()
    assert lib.mq_insert_plan(None, k, n, C.byref(bad), ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_insert_plan(ins.ptr, k, n, None, ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), None, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), ws.ptr, ws.nbytes - 1, None) == mq.MQ_EINVAL
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), ws.ptr + 4, ws.nbytes, None) == mq.MQ_EINVAL
    # n + k >= 2^31: refused on the arguments alone (nothing of that size exists)
    assert lib.mq_insert_workspace_bytes(2**31 - 5, 4) > 2**28
    assert lib.mq_insert_plan(ins.ptr, k, 2**31 - k, C.byref(bad), ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_insert_points(old.ptr, 2**31 - k, new.ptr, k, ins.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_points(None, n, new.ptr, k, ins.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_points(old.ptr, n, None, k, ins.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_points(old.ptr, n, new.ptr, k, None, None) == mq.MQ_EINVAL
    assert lib.mq_insert_slots(None, None, k, o64.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_positions(None, 0, None, k, o64.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), ws.ptr, ws.nbytes, None) == mq.MQ_OK and bad.value == 0
    pa = ptr_array
    assert lib.mq_insert_columns(ws.ptr, None, pa([new]), 1, pa([out]), None) == mq.MQ_EINVAL
    assert lib.mq_insert_columns(ws.ptr, pa([old]), None, 1, pa([out]), None) == mq.MQ_EINVAL
    assert lib.mq_insert_columns(ws.ptr, pa([old]), pa([new]), 1, pa([old]), None) == mq.MQ_EINVAL
    assert lib.mq_insert_columns(None, pa([old]), pa([new]), 1, pa([out]), None) == mq.MQ_EINVAL
    assert lib.mq_insert_columns(ws.ptr, pa([old]), pa([new]), 1025, pa([out]), None) == mq.MQ_EINVAL
    assert lib.mq_insert_index(ws.ptr, None, None, new.ptr, n64.ptr, None, 0, out.ptr, o64.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_insert_index(ws.ptr, old.ptr, p64.ptr, new.ptr, n64.ptr, None, 0, None, o64.ptr, None) == mq.MQ_EINVAL
    assert np.all(out.get(np.int32, n + k) == -7)
    # a delete plan on the same workspace ends the insert plan
    dws = Dev(max(lib.mq_delete_workspace_bytes(n), ws.nbytes))
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), dws.ptr, dws.nbytes, None) == mq.MQ_OK
    deleted, pos = C.c_uint64(), Dev.of(np.array([1], np.int32))
    assert lib.mq_delete_plan(pos.ptr, 1, n, C.byref(deleted), C.byref(bad), dws.ptr, dws.nbytes, None) == mq.MQ_OK
    assert lib.mq_insert_columns(dws.ptr, pa([old]), pa([new]), 1, pa([out]), None) == mq.MQ_EINVAL
    # the valid plan on ws is this thread's last insert plan no more: plan again, then apply
    assert lib.mq_insert_plan(ins.ptr, k, n, C.byref(bad), ws.ptr, ws.nbytes, None) == mq.MQ_OK
    mq.check(cols())
    want = ic.expand(np.arange(n, dtype=np.int32), np.array([0, 5, 5, n]), np.arange(k, dtype=np.int32))
    assert np.array_equal(out.get(np.int32, n + k), want)


# ---------------------------------------------------------------------------
# drop-in level: a 4-column table of 10,000 rows (the reference suite's tbl5)
# ---------------------------------------------------------------------------

FILL = 0x5A5A5A5A  # what the spare capacity holds before rows arrive


class ITbl(Tbl):
    """test_gpu_dml.Tbl over buffers with `spare` rows of capacity beyond the table's."""

    def __init__(self, lib, cols: np.ndarray, spare: int, index_cols=(), clustered_col=None, build=True):
        self.lib = lib
        n = cols.shape[1]
        self.bufs = [memfd_array(np.concatenate([c, np.full(spare, FILL, np.int32)])) for c in cols]
        self.db, self.t, self.cs = ic.make_db(self.bufs, n)
        for j in index_cols:
            self.cs[j].has_index, self.cs[j].sorted, self.cs[j].clustered = True, True, j == clustered_col
        if index_cols and build:
            lib.build_index(C.byref(self.db))

    def insert(self, rows: np.ndarray, db=True):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        st = mq.Status(0, None)
        self.lib.relational_insert(C.byref(self.db) if db else None, C.byref(self.t),
                                   rows.ctypes.data_as(C.POINTER(C.c_int)), len(rows), C.byref(st))
        return st.code

    def index(self, j):
        n = self.cs[j].row_count
        ix = self.cs[j].index.contents
        return (np.ctypeslib.as_array(ix.values, shape=(n,)).copy(),
                np.ctypeslib.as_array(ix.positions, shape=(n,)).astype(np.uint64))

    def check_counts(self, model: np.ndarray, minmax):
        n = model.shape[1]
        assert self.t.row_count == n and all(self.cs[j].row_count == n for j in range(len(model)))
        assert np.array_equal(self.rows(), model)
        assert [(self.cs[j].min, self.cs[j].max) for j in range(len(model))] == minmax


@pytest.fixture
def itbl(lib):
    made = []

    def make(cols, spare, **kw):
        made.append(ITbl(lib, cols, spare, **kw))
        return made[-1]
    yield make
    for t in made:
        t.close()


def widen(minmax, batch):
    return [(min(lo, int(batch[:, j].min())), max(hi, int(batch[:, j].max()))) for j, (lo, hi) in enumerate(minmax)]


def check_histogram(t: ITbl, j: int):
    """The histogram as index_one builds it (index.c:63-84): bin_size from min / max, the
    bin starts, and a count per bin; rows whose bin lies past the 100th are in none (the
    reference writes those past its array)."""
    c = t.cs[j]
    data = t.bufs[j][:c.row_count].astype(np.int64)
    h = C.cast(c.histogram, C.POINTER(dc.Histogram)).contents
    assert h.bin_size == int((c.max - c.min) / 99)
    assert list(h.values) == [(b * h.bin_size) for b in range(100)]
    bins = (data - c.min) // h.bin_size
    assert list(h.counts) == np.bincount(bins[bins < 100], minlength=100).tolist()


def check_index_exact(t: ITbl, j: int, want_v, want_p, lo, hi):
    """check_index's properties (ascending values, a permutation mapping to them, an index
    select returning the scan's set) and the model's arrays exactly."""
    n = t.cs[j].row_count
    data = t.bufs[j][:n]
    v, p = t.index(j)
    assert np.all(v[1:] >= v[:-1])
    assert np.array_equal(np.sort(p), np.arange(n, dtype=np.uint64))
    assert np.array_equal(data[p.astype(np.int64)], v)
    assert np.array_equal(v, want_v) and np.array_equal(p, want_p)
    check_histogram(t, j)
    via_index = take(t.select(j, lo, hi))
    scan = take(t.select(j, lo, hi, scan=True))
    assert np.array_equal(np.sort(via_index), scan)
    assert np.array_equal(scan, np.flatnonzero((data >= lo) & (data < hi)).astype(np.int32))


def test_milestone5_sequence(lib, itbl):
    """tbl5 with a clustered index on col1 and an unclustered one on col2, both built by
    build_index; the generator's five one-row inserts, then a batch of 1000 rows with
    repeated keys. After every step the rows, counts, min / max, both indexes and selects
    and fetches through them equal the model."""
    t = itbl(dc.tbl5(), 2000, index_cols=(0, 1), clustered_col=0)
    model = t.rows().copy()  # build_index reordered the other columns
    keys, ones = t.index(0)
    uv, up = t.index(1)
    assert np.array_equal(ones, np.arange(10_000, dtype=np.uint64))
    minmax = [(t.cs[j].min, t.cs[j].max) for j in range(4)]
    batch = ic.random_batch(1000)
    batch[0, 1] = 1034  # col2 then spans -55 .. 1034 = 99 * 11: every row falls in a bin
    steps = [ic.MILESTONE5_ROWS[i:i + 1] for i in range(5)] + [batch]
    for rows in steps:
        assert t.insert(rows) == mq.OK
        points, slots = ic.new_slots(keys, rows[:, 0])
        uv, up = ic.insert_index(uv, up, rows[:, 1], slots, points)
        model = ic.insert_rows(model, keys, rows.T, key_col=0)
        keys = np.sort(np.concatenate([keys, rows[:, 0]]), kind="stable")
        minmax = widen(minmax, rows)
        n = model.shape[1]
        t.check_counts(model, minmax)
        assert t.t.table_length == 12_000
        # the clustered index: sorted values, identity positions
        gv, gp = t.index(0)
        assert np.array_equal(gv, keys) and np.array_equal(gp, np.arange(n, dtype=np.uint64))
        check_index_exact(t, 1, uv, up, 100, 300)
        # select + fetch through both indexes against a scan of the model
        s = t.select(0, -1, 5000)  # bounds that are keys: -1 arrives with the first row
        pos = take(s, free=False)
        assert np.array_equal(pos, np.flatnonzero((keys >= -1) & (keys < 5000)))
        for j in (1, 2, 3):
            assert np.array_equal(t.fetch(j, s), model[j][pos])
        take(s)
        s = t.select(1, -11, 40)
        pos = take(s, free=False)
        assert np.array_equal(np.sort(pos), np.flatnonzero((model[1] >= -11) & (model[1] < 40)))
        assert np.array_equal(t.fetch(3, s), model[3][pos])
        take(s)
    check_index(t, 1, 0, 500)  # with the histogram counting every row


def test_append_table_stays_resident(lib, itbl):
    """No clustered index: the rows are appended, the resident copies are extended on the
    device (no column upload, by the insert or after it), the unclustered index on col1 has
    the new entries merged in; a delete of the inserted rows then restores everything."""
    start = dc.tbl5()
    n, k = 10_000, 1000
    t = itbl(start, 3000, index_cols=(0,))
    v0, p0 = t.index(0)
    for j, (lo, hi) in enumerate([(0, n), (0, 1000), (-500, 500), (0, 2**30)]):
        take(t.select(j, lo, hi, scan=True))  # every column resident before the insert
    batch = ic.random_batch(k)
    batch[:, 0] = np.random.default_rng(1).integers(0, n, k)  # repeats of old keys, inside the old min / max
    res = mq.residency(lib)
    assert t.insert(batch, db=False) == mq.OK  # db may be NULL while the table need not grow
    model = ic.insert_rows(start, None, batch.T)
    t.check_counts(model, widen([(int(c.min()), int(c.max())) for c in start], batch))
    assert t.t.table_length == 13_000
    assert all(np.all(b[n + k:] == FILL) for b in t.bufs)
    wv, wp = ic.insert_index(v0, p0, batch[:, 0], np.arange(n, n + k, dtype=np.uint64))
    check_index_exact(t, 0, wv, wp, 2000, 4000)
    check_index(t, 0, 2000, 4000)
    s = t.select(3, 2**28, 2**29, scan=True)
    pos = take(s, free=False)
    assert np.array_equal(pos, np.flatnonzero((model[3] >= 2**28) & (model[3] < 2**29)))
    for j in range(4):
        assert np.array_equal(t.fetch(j, s), model[j][pos])
    take(s)
    every = make_result(np.arange(n + k, dtype=np.int32))
    for j in range(4):
        assert np.array_equal(t.fetch(j, C.byref(every)), model[j])
    free_result_struct(every)
    after = mq.residency(lib)
    assert (after["column_uploads"], after["column_bytes"]) == (res["column_uploads"], res["column_bytes"])
    # the round trip with relational_delete
    gone = make_result(np.arange(n, n + k, dtype=np.int32))
    assert t.delete(C.byref(gone)) == mq.OK
    free_result_struct(gone)
    assert t.t.row_count == n and np.array_equal(t.rows(), start)
    gv, gp = t.index(0)
    assert np.array_equal(gv, v0) and np.array_equal(gp, p0)


def test_delete_after_sorted_insert_restores(lib, itbl):
    t = itbl(dc.tbl5(3000), 500, index_cols=(0, 1), clustered_col=0)
    start = t.rows().copy()
    before = [t.index(0), t.index(1)]
    batch = ic.random_batch(300, seed=4)
    assert t.insert(batch) == mq.OK
    _, slots = ic.new_slots(before[0][0], batch[:, 0])
    gone = make_result(slots.astype(np.int32))
    assert t.delete(C.byref(gone)) == mq.OK
    free_result_struct(gone)
    assert t.t.row_count == 3000 and np.array_equal(t.rows(), start)
    for j in (0, 1):
        gv, gp = t.index(j)
        assert np.array_equal(gv, before[j][0]) and np.array_equal(gp, before[j][1])


def test_growth_needs_the_servers_hooks(lib, itbl, capfd):
    """row_count + nrows > table_length with no save_data / start_data linked: ERROR,
    nothing changed (load_db answers the same way)."""
    start = dc.tbl5(2000)
    t = itbl(start, 3, index_cols=(0,))
    v0, p0 = t.index(0)
    minmax = [(t.cs[j].min, t.cs[j].max) for j in range(4)]
    capfd.readouterr()
    assert t.insert(ic.MILESTONE5_ROWS[:4]) == mq.ERROR
    assert "libmq: relational_insert" in capfd.readouterr().err
    t.check_counts(start, minmax)
    assert t.t.table_length == 2003 and all(np.all(b[2000:] == FILL) for b in t.bufs)
    gv, gp = t.index(0)
    assert np.array_equal(gv, v0) and np.array_equal(gp, p0)
    assert t.insert(ic.MILESTONE5_ROWS[:3]) == mq.OK  # exactly full
    assert t.t.row_count == 2003 and np.array_equal(t.rows(), ic.insert_rows(start, None, ic.MILESTONE5_ROWS[:3].T))


def test_attached_column_is_detached_not_written(lib, itbl):
    model = dc.tbl5(4000)
    t = itbl(model, 100)
    mine = [Dev.of(model[j]) for j in range(4)]
    for j in range(4):
        mq.check(lib.mq_column_attach(C.byref(t.cs[j]), mine[j].ptr), "attach")
    assert t.insert(ic.MILESTONE5_ROWS) == mq.OK
    want = ic.insert_rows(model, None, ic.MILESTONE5_ROWS.T)
    assert np.array_equal(t.rows(), want)
    assert np.array_equal(take(t.select(1, -60, 0, scan=True)), np.arange(4000, 4005))
    for j in range(4):  # the caller's buffers keep their old content
        assert np.array_equal(mine[j].get(np.int32, 4000), model[j])


def test_refused_inserts_change_nothing(lib, itbl, capfd):
    model = dc.tbl5(5000)
    t = itbl(model, 50, index_cols=(0,))
    v0, p0 = t.index(0)
    minmax = [(t.cs[j].min, t.cs[j].max) for j in range(4)]
    rows = ic.MILESTONE5_ROWS

    def unchanged():
        t.check_counts(model, minmax)
        gv, gp = t.index(0)
        assert np.array_equal(gv, v0) and np.array_equal(gp, p0)
        assert all(np.all(b[5000:] == FILL) for b in t.bufs)

    assert t.insert(rows[:0]) == mq.OK  # nrows == 0
    unchanged()
    st = mq.Status(0, None)
    lib.relational_insert(C.byref(t.db), None, rows.ctypes.data_as(C.POINTER(C.c_int)), 5, C.byref(st))
    assert st.code == mq.ERROR
    st = mq.Status(0, None)
    lib.relational_insert(C.byref(t.db), C.byref(t.t), None, 5, C.byref(st))
    assert st.code == mq.ERROR
    t.cs[2].row_count = 4999  # a column out of step with its table
    assert t.insert(rows) == mq.ERROR
    t.cs[2].row_count = 5000
    unchanged()
    big = 2**31 - 3  # row_count + nrows >= 2^31: refused before anything is touched
    t.t.row_count = big
    for j in range(4):
        t.cs[j].row_count = big
    assert t.insert(rows) == mq.ERROR
    t.t.row_count = 5000
    for j in range(4):
        t.cs[j].row_count = 5000
    assert capfd.readouterr().err.count("libmq: relational_insert") == 4
    unchanged()
    assert t.insert(rows) == mq.OK
    assert np.array_equal(t.rows(), ic.insert_rows(model, None, rows.T))
