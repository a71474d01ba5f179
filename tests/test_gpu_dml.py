"""Row deletes and updates on gfx950 (csrc/mq_dml.hip; relational_delete and
relational_update in mq_query.c), every comparison exact equality with the numpy
restatement in dmlcases.py (the workload generator's pandas statements,
milestone5.py:127-142, 186-202; the reference itself has neither command).

Which regime each size reaches: dc.SIZES (up to 2^20 + 5 rows) cover the compaction's
tiles and alignments with one step a block in the word prefix and in the index pass, both
of which run on fixed grids. 2 097 153 and 4 195 333 rows are the first with 2 and 3 steps
a block in the index pass (k_dml_index_count / _write); 2^24 + 5 rows give 2 steps a block
in the word prefix (k_dml_word_sums / _prefix) and 9 in the index pass, so the bases both
carry from step to step are exercised. Those tests assert their regime from
mq_dml_geometry first. mq_update_rows past one grid-stride step is in test_gpu_regimes.py.
"""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

import dmlcases as dc
from devbuf import Dev
from refapi import make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # The drop-in's first operator pins glibc's mmap threshold at 1 MB (mq_query.c ready()),
    # which is what lets a large Result payload be write-guarded. Run one before this
    # module's multi-megabyte numpy temporaries come and go: freed while the threshold is
    # still dynamic they would raise it and leave tens of MB free at the top of the heap,
    # from where a later module's 40 MB payload would be served (unguardable).
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    return L


def ptr_array(devs):
    return (C.c_void_p * max(len(devs), 1))(*[d.ptr for d in devs])


def plan(L, ws, pos: np.ndarray, n: int):
    d = Dev.of(pos)
    deleted, bad = C.c_uint64(~0), C.c_uint64(~0)
    rc = L.mq_delete_plan(d.ptr, len(pos), n, C.byref(deleted), C.byref(bad), ws.ptr, ws.nbytes, None)
    return rc, deleted.value, bad.value


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ncols", dc.NCOLS)
@pytest.mark.parametrize("n", dc.SIZES)
def test_delete_columns_and_index(lib, n, ncols):
    """Every delete set, the position list ascending, reversed and shuffled with every
    id twice: h_deleted counts distinct rows, every column and both index forms equal
    the restatement."""
    cols = dc.table(n, ncols)
    # column 1 sits 4 bytes off a 16-byte boundary: the loads that cannot be dwordx4
    dcols = [Dev.of(cols[j], offset_elems=1 if j == 1 else 0) for j in range(ncols)]
    rng = np.random.default_rng(n)
    # many equal values, and among equal values the positions in shuffled order
    key = (rng.permutation(n) % 7).astype(np.int32)
    shuf = rng.permutation(n)
    p = shuf[np.argsort(key[shuf], kind="stable")]
    indexes = [(key[p], p.astype(np.uint64)), dc.index_of(key, clustered=True)]
    dix = [(Dev.of(v), Dev.of(q)) for v, q in indexes]
    ws = Dev(lib.mq_delete_workspace_bytes(n))
    for name, ids in dc.delete_sets(n).items():
        left = n - len(ids)
        want = dc.delete_rows(cols, ids)
        want_ix = [dc.delete_index(v, q, ids, n) for v, q in indexes]
        for order in dc.ORDERS:
            tag = (name, order)
            rc, deleted, bad = plan(lib, ws, dc.position_list(ids, order, seed=n), n)
            assert (rc, deleted, bad) == (mq.MQ_OK, len(ids), 0), tag
            # outputs start 0, 1, 2, 3 dwords off a 16-byte boundary
            outs = [Dev.of(np.full(left + 8, -7, np.int32), offset_elems=j % 4) for j in range(ncols)]
            mq.check(lib.mq_delete_columns(ws.ptr, ptr_array(dcols), ncols, ptr_array(outs), None), "mq_delete_columns")
            for j in range(ncols):
                got = outs[j].get(np.int32, left + 8)
                assert np.array_equal(got[:left], want[j]), tag + (j,)
                assert np.all(got[left:] == -7), tag + (j, "wrote past the end")
            if order != "shuffled" and n > 9000:
                continue  # the index step does not depend on the list's order
            for (dv, dq), (wv, wq) in zip(dix, want_ix):
                ov, oq = Dev.of(np.full(left + 2, -7, np.int32)), Dev.of(np.full(left + 2, 7, np.uint64))
                mq.check(lib.mq_delete_index(ws.ptr, dv.ptr, dq.ptr, ov.ptr, oq.ptr, None), "mq_delete_index")
                gv, gq = ov.get(np.int32, left + 2), oq.get(np.uint64, left + 2)
                assert np.array_equal(gv[:left], wv) and np.array_equal(gq[:left], wq), tag
                assert np.all(gv[left:] == -7) and np.all(gq[left:] == 7), tag + ("wrote past the end",)


# ---------------------------------------------------------------------------
# past one step a block
#
# The word prefix and the index pass run on fixed grids (mq_dml_geometry). At every size
# of dc.SIZES a block's chunk is one step long, so `base += total` (k_dml_word_prefix) and
# `base += run` (k_dml_index_write) never carry anything. dc.BIG_N gives two prefix steps
# and nine index steps a block; dc.INDEX_N are the first sizes with 2 and 3 index steps.
# ---------------------------------------------------------------------------
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # what mq_memset(0x5A) leaves


def dml_geometry(L, n):
    """((prefix blocks, prefix chunk words), (index blocks, index chunk rows))"""
    pb, pc, ib, ic_ = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    L.mq_dml_geometry(n, C.byref(pb), C.byref(pc), C.byref(ib), C.byref(ic_))
    return (pb.value, pc.value), (ib.value, ic_.value)


def filled(L, count, dtype, offset_elems=0):
    """A device buffer of `count` entries of dtype, every byte 0x5A, starting offset_elems
    entries into its allocation."""
    size = np.dtype(dtype).itemsize
    d = Dev((count + offset_elems) * size + 16)
    mq.check(L.mq_memset(d.p, 0x5A, d.nbytes, None), "mq_memset")
    d.off = offset_elems * size
    return d


def two_prefix_steps(L, n):
    """The prefix chunk in words at n rows, after asserting two steps a block there and
    several index steps a block."""
    (pb, pc), (ib, ic_) = dml_geometry(L, n)
    assert pc % dc.PREFIX_STEP == 0 and pc // dc.PREFIX_STEP >= 2 and pb >= 2, (n, pb, pc)
    assert ic_ % dc.INDEX_STEP == 0 and ic_ // dc.INDEX_STEP >= 2 and ib >= 2, (n, ib, ic_)
    return pc


_big = {}


def big_case(L, name):
    """The delete set `name` at dc.BIG_N rows and its plan's position list (shuffled, every
    id twice) on the device; one set is kept at a time."""
    if name not in _big:
        _big.clear()
        ids = dc.big_delete_set(name, dc.BIG_N, two_prefix_steps(L, dc.BIG_N))
        _big[name] = (ids, Dev.of(dc.position_list(ids, "shuffled", seed=dc.BIG_N)))
    return _big[name]


def plan_on_device(L, ws, dpos, k, n):
    deleted, bad = C.c_uint64(~0), C.c_uint64(~0)
    rc = L.mq_delete_plan(dpos.ptr, k, n, C.byref(deleted), C.byref(bad), ws.ptr, ws.nbytes, None)
    return rc, deleted.value, bad.value


@pytest.fixture(scope="module")
def big_table():
    """Two full-range columns of dc.BIG_N rows, column 1 placed 4 bytes off a 16-byte line."""
    cols = dc.table(dc.BIG_N, 2)
    return cols, [Dev.of(cols[0]), Dev.of(cols[1], offset_elems=1)]


@pytest.fixture(scope="module")
def big_ws(lib):
    return Dev(lib.mq_delete_workspace_bytes(dc.BIG_N))


def check_delete_index(L, ws, n, ids, clustered, tag):
    """mq_delete_index on the plan in ws against dc.delete_index, outputs pre-filled."""
    v, q = dc.big_index(n, clustered)
    wv, wq = dc.delete_index(v, q, ids, n)
    left = n - len(ids)
    assert len(wv) == left
    dv, dq = Dev.of(v), Dev.of(q)
    ov, oq = filled(L, left + 4, np.int32), filled(L, left + 4, np.uint64)
    mq.check(L.mq_delete_index(ws.ptr, dv.ptr, dq.ptr, ov.ptr, oq.ptr, None), "mq_delete_index")
    gv, gq = ov.get(np.int32, left + 4), oq.get(np.uint64, left + 4)
    assert np.array_equal(gv[:left], wv), tag + ("values",)
    assert np.array_equal(gq[:left], wq), tag + ("positions",)
    assert np.all(gv[left:].view(np.uint32) == FILL32) and np.all(gq[left:] == FILL64), tag + ("wrote past the end",)


@pytest.mark.parametrize("name", dc.BIG_SETS)
def test_delete_columns_two_prefix_steps(lib, big_table, big_ws, name):
    """mq_delete_plan + mq_delete_columns at dc.BIG_N rows, where every block of the word
    prefix takes two steps: h_deleted and h_bad, both columns equal np.delete, nothing
    written past n - deleted. first_steps / second_steps make one step's total full and
    the other's zero in six chunks."""
    n = dc.BIG_N
    ids, dpos = big_case(lib, name)
    cols, dcols = big_table
    left = n - len(ids)
    assert plan_on_device(lib, big_ws, dpos, 2 * len(ids), n) == (mq.MQ_OK, len(ids), 0), name
    outs = [filled(lib, left + 8, np.int32, offset_elems=3 * j) for j in range(2)]
    mq.check(lib.mq_delete_columns(big_ws.ptr, ptr_array(dcols), 2, ptr_array(outs), None), "mq_delete_columns")
    want = dc.delete_rows(cols, ids)
    for j in range(2):
        got = outs[j].get(np.int32, left + 8)
        assert np.array_equal(got[:left], want[j]), (name, j)
        assert np.all(got[left:].view(np.uint32) == FILL32), (name, j, "wrote past the end")


@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("name", dc.BIG_SETS)
def test_delete_index_two_prefix_steps(lib, big_ws, name, clustered):
    """mq_delete_index at dc.BIG_N rows on the same plans: the renumbering reads the word
    prefix past its first step, and every block of the index pass takes nine steps. The
    secondary form has tied values and the positions (i * 1 000 003) mod n; the clustered
    form the identity."""
    n = dc.BIG_N
    ids, dpos = big_case(lib, name)
    assert plan_on_device(lib, big_ws, dpos, 2 * len(ids), n) == (mq.MQ_OK, len(ids), 0), name
    check_delete_index(lib, big_ws, n, ids, clustered, (name, clustered))


@pytest.mark.parametrize("n,steps", [(dc.INDEX_N[0], 2), (dc.INDEX_N[1], 3)])
def test_delete_index_first_sizes_past_one_step(lib, n, steps):
    """mq_delete_index at the first sizes where a block of the index pass takes 2 and 3
    steps (today the last chunk holds 1 row and 2053 rows: a lone row, two whole steps and
    a ragged one), half of the rows deleted."""
    (_, _), (ib, ic_) = dml_geometry(lib, n)
    assert ic_ % dc.INDEX_STEP == 0 and ic_ // dc.INDEX_STEP >= steps and ib >= 2, (n, ib, ic_)
    assert (n - (ib - 1) * ic_) % dc.INDEX_STEP != 0, (n, ib, ic_)  # the last chunk ends in a ragged step
    assert dml_geometry(lib, dc.INDEX_N[0] - 1)[1][1] == dc.INDEX_STEP  # one row fewer: one step a block
    ids = dc.big_delete_set("random_50pct", n, 0)
    ws = Dev(lib.mq_delete_workspace_bytes(n))
    dpos = Dev.of(dc.position_list(ids, "shuffled", seed=n))
    assert plan_on_device(lib, ws, dpos, 2 * len(ids), n) == (mq.MQ_OK, len(ids), 0)
    for clustered in (False, True):
        check_delete_index(lib, ws, n, ids, clustered, (n, clustered))


@pytest.mark.parametrize("n", [1, 64, 257, 8193, 100_003])
def test_update_rows(lib, n):
    rng = np.random.default_rng(n)
    col = dc.table(n, 1)[0]
    ids = rng.integers(0, n, 3 * n // 4 + 1).astype(np.int32)
    ids = np.concatenate([ids, ids[::3]])  # repeats
    d, dp, bad = Dev.of(col), Dev.of(ids), Dev.of(np.array([99], np.uint64))
    mq.check(lib.mq_update_rows(d.ptr, n, dp.ptr, len(ids), -10, bad.ptr, None), "mq_update_rows")
    assert np.array_equal(d.get(np.int32, n), dc.update_rows(col, ids, -10))
    assert bad.get(np.uint64, 1)[0] == 0
    # out-of-range ids are skipped and counted; d_bad may be NULL
    wild = np.concatenate([ids, [-1, n, n + 1, 2**31 - 1, -2**31]]).astype(np.int32)
    rng.shuffle(wild)
    d, dp = Dev.of(np.concatenate([col, [4242, 4242]]).astype(np.int32)), Dev.of(wild)
    mq.check(lib.mq_update_rows(d.ptr, n, dp.ptr, len(wild), 77, bad.ptr, None), "mq_update_rows")
    got = d.get(np.int32, n + 2)
    assert np.array_equal(got[:n], dc.update_rows(col, ids, 77)) and np.all(got[n:] == 4242)
    assert bad.get(np.uint64, 1)[0] == 5
    mq.check(lib.mq_update_rows(d.ptr, n, dp.ptr, len(wild), 78, None, None), "mq_update_rows")
    assert np.array_equal(d.get(np.int32, n), dc.update_rows(col, ids, 78))


def test_error_codes(lib):
    n = 1000
    ws = Dev(lib.mq_delete_workspace_bytes(n))
    for wrong in (-1, n):
        rc, _, bad = plan(lib, ws, np.array([3, wrong, 5, wrong], np.int32), n)
        assert (rc, bad) == (mq.MQ_EINVAL, 2)
        # no plan is left behind
        col, out = Dev.of(np.arange(n, dtype=np.int32)), Dev(n * 4)
        assert lib.mq_delete_columns(ws.ptr, ptr_array([col]), 1, ptr_array([out]), None) == mq.MQ_EINVAL
    pos = Dev.of(np.array([1, 2], np.int32))
    deleted, bad = C.c_uint64(), C.c_uint64()
    args = (C.byref(deleted), C.byref(bad))
    assert lib.mq_delete_plan(None, 2, n, *args, ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_delete_plan(pos.ptr, 2, n, *args, None, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_delete_plan(pos.ptr, 2, n, None, C.byref(bad), ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_delete_plan(pos.ptr, 2, n, *args, ws.ptr, ws.nbytes - 1, None) == mq.MQ_EINVAL
    assert lib.mq_delete_plan(pos.ptr, 2, 2**31, *args, ws.ptr, ws.nbytes, None) == mq.MQ_EINVAL
    assert lib.mq_delete_plan(pos.ptr, 2, n, *args, ws.ptr, ws.nbytes, None) == mq.MQ_OK
    col, out = Dev.of(np.arange(n, dtype=np.int32)), Dev(n * 4)
    assert lib.mq_delete_columns(ws.ptr, None, 1, ptr_array([out]), None) == mq.MQ_EINVAL
    assert lib.mq_delete_columns(ws.ptr, ptr_array([col]), 1, ptr_array([col]), None) == mq.MQ_EINVAL
    assert lib.mq_delete_columns(None, ptr_array([col]), 1, ptr_array([out]), None) == mq.MQ_EINVAL
    assert lib.mq_delete_columns(ws.ptr, ptr_array([col]), 1025, ptr_array([out]), None) == mq.MQ_EINVAL
    assert lib.mq_delete_index(ws.ptr, None, None, out.ptr, out.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_update_rows(None, n, pos.ptr, 2, 0, None, None) == mq.MQ_EINVAL
    assert lib.mq_update_rows(col.ptr, n, None, 2, 0, None, None) == mq.MQ_EINVAL
    assert lib.mq_update_rows(col.ptr, 2**31, pos.ptr, 2, 0, None, None) == mq.MQ_EINVAL
    # the valid plan above is still in place
    mq.check(lib.mq_delete_columns(ws.ptr, ptr_array([col]), 1, ptr_array([out]), None))
    assert np.array_equal(out.get(np.int32, n - 2), np.delete(np.arange(n, dtype=np.int32), [1, 2]))


# ---------------------------------------------------------------------------
# drop-in level: a 4-column table of 10,000 rows (the reference suite's tbl5)
# ---------------------------------------------------------------------------

def memfd_array(values: np.ndarray):
    """The rows in a MAP_SHARED file mapping, as the reference's start_data maps a
    column (db_manager.c:736-790): memory a write guard can cover."""
    fd = os.memfd_create("mqcol")
    os.ftruncate(fd, max(values.nbytes, 4))
    m = mmap.mmap(fd, max(values.nbytes, 4), mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE)
    os.close(fd)
    a = np.frombuffer(m, dtype=np.int32)[:len(values)]
    a[:] = values
    return a


class Tbl:
    def __init__(self, lib, cols: np.ndarray, index_col=None, clustered=False, build=True):
        self.lib = lib
        self.bufs = [memfd_array(c) for c in cols]
        self.db, self.t, self.cs = dc.make_db(self.bufs, index_col, clustered)
        if index_col is not None and build:
            lib.build_index(C.byref(self.db))

    def rows(self):
        return np.stack([b[:self.cs[j].row_count] for j, b in enumerate(self.bufs)])

    def select(self, j, lo, hi, scan=False):
        st = mq.Status(0, None)
        fn = self.lib.select_column_scan if scan else self.lib.select_column
        rp = fn(C.byref(self.cs[j]), C.pointer(C.c_int(lo)), C.pointer(C.c_int(hi)), C.byref(st))
        assert st.code == mq.OK and rp
        return rp

    def fetch(self, j, rp):
        st = mq.Status(0, None)
        out = self.lib.fetch_column(C.byref(self.cs[j]), rp, C.byref(st))
        assert st.code == mq.OK and out
        return take(out)

    def delete(self, rp):
        st = mq.Status(0, None)
        self.lib.relational_delete(C.byref(self.t), rp, C.byref(st))
        return st.code

    def update(self, j, rp, value):
        st = mq.Status(0, None)
        self.lib.relational_update(C.byref(self.cs[j]), rp, value, C.byref(st))
        return st.code

    def close(self):
        self.lib.mq_release_all()  # lifts the guards before the mappings go


@pytest.fixture
def tbl(lib):
    made = []

    def make(cols, **kw):
        made.append(Tbl(lib, cols, **kw))
        return made[-1]
    yield make
    for t in made:
        t.close()


def check_index(t: Tbl, j: int, lo: int, hi: int):
    """The index of column j after an edit: ascending values, positions a permutation of
    the rows that maps to them, the histogram counting every row, and a select through
    it returning the scan's set."""
    n = t.cs[j].row_count
    data = t.bufs[j][:n]
    ix = t.cs[j].index.contents
    v = np.ctypeslib.as_array(ix.values, shape=(n,))
    p = np.ctypeslib.as_array(ix.positions, shape=(n,))
    assert np.all(v[1:] >= v[:-1])
    assert np.array_equal(np.sort(p), np.arange(n, dtype=np.uint64))
    assert np.array_equal(data[p.astype(np.int64)], v)
    h = C.cast(t.cs[j].histogram, C.POINTER(dc.Histogram)).contents
    assert sum(h.counts[:]) == n
    via_index = take(t.select(j, lo, hi))
    scan = take(t.select(j, lo, hi, scan=True))
    assert np.array_equal(np.sort(via_index), scan)
    assert np.array_equal(scan, np.flatnonzero((data >= lo) & (data < hi)).astype(np.int32))


def test_milestone5_sequence(lib, tbl):
    """select -> relational_update of another column; select -> relational_delete;
    select + fetch afterwards; then an update of the indexed column. One unclustered
    index (col1), built by build_index before the edits."""
    model = dc.tbl5()
    t = tbl(model, index_col=0)
    n = model.shape[1]
    take(t.select(1, 0, 1000, scan=True))  # col2 .. col4 resident before the edits
    take(t.select(2, -500, 500, scan=True))
    take(t.select(3, 0, 2**30, scan=True))

    # u1=select(db1.tbl5.col2,100,150); relational_update(db1.tbl5.col3,u1,-10)
    u1 = t.select(1, 100, 150)
    ids = take(u1, free=False)
    assert np.array_equal(ids, np.flatnonzero((model[1] >= 100) & (model[1] < 150)))
    up = mq.residency(lib)["column_uploads"]
    assert t.update(2, u1, -10) == mq.OK
    model[2] = dc.update_rows(model[2], ids, -10)
    assert np.array_equal(t.rows(), model)
    got = take(t.select(2, -10, -9))
    assert np.array_equal(got, np.flatnonzero(model[2] == -10))
    assert mq.residency(lib)["column_uploads"] == up, "the updated column was uploaded again"
    assert (t.cs[2].min, t.cs[2].max) == (min(int(dc.tbl5()[2].min()), -10), int(dc.tbl5()[2].max()))
    take(u1)

    # d1=select(db1.tbl5.col2,300,420); relational_delete(db1.tbl5,d1)
    d1 = t.select(1, 300, 420)
    ids = take(d1, free=False)
    assert 0 < len(ids) < n
    up = mq.residency(lib)["column_uploads"]
    assert t.delete(d1) == mq.OK
    take(d1)
    model = dc.delete_rows(model, ids)
    left = n - len(ids)
    assert t.t.row_count == left and all(t.cs[j].row_count == left for j in range(4))
    assert t.t.table_length == n
    assert np.array_equal(t.rows(), model)
    # select + fetch afterwards: the device copies hold the same rows as the host
    s = t.select(3, 2**28, 2**29)
    pos = take(s, free=False)
    assert np.array_equal(pos, np.flatnonzero((model[3] >= 2**28) & (model[3] < 2**29)))
    for j in (1, 2, 3):
        assert np.array_equal(t.fetch(j, s), model[j][pos])
    take(s)
    every = make_result(np.arange(left, dtype=np.int32))
    for j in range(4):
        assert np.array_equal(t.fetch(j, C.byref(every)), model[j])
    free_result_struct(every)
    assert mq.residency(lib)["column_uploads"] == up, "a compacted column was uploaded again"
    check_index(t, 0, 2000, 4000)

    # an update of the indexed column: the index is built again
    u2 = t.select(1, 500, 520, scan=True)
    ids = take(u2, free=False)
    assert t.update(0, u2, -10) == mq.OK
    take(u2)
    model[0] = dc.update_rows(model[0], ids, -10)
    assert np.array_equal(t.rows(), model)
    assert t.cs[0].min == -10
    check_index(t, 0, -10, 3000)

    # a second delete, through the sorted index's value-ordered positions, empties a range
    d2 = t.select(0, -10, 5000)
    ids = take(d2, free=False)
    assert not np.all(ids[1:] > ids[:-1])  # value order, not row order
    assert t.delete(d2) == mq.OK
    take(d2)
    model = dc.delete_rows(model, ids)
    assert np.array_equal(t.rows(), model) and t.t.row_count == model.shape[1]
    check_index(t, 0, 5000, 7000)
    assert len(take(t.select(0, -10, 5000, scan=True))) == 0


def test_delete_nothing_and_everything(lib, tbl):
    model = dc.tbl5(2000)
    t = tbl(model, index_col=0)
    empty = make_result(np.zeros(0, np.int32))
    assert t.delete(C.byref(empty)) == mq.OK
    free_result_struct(empty)
    assert t.t.row_count == 2000 and np.array_equal(t.rows(), model)
    allrows = make_result(np.arange(2000, dtype=np.int32)[::-1])
    assert t.delete(C.byref(allrows)) == mq.OK
    free_result_struct(allrows)
    assert t.t.row_count == 0 and all(t.cs[j].row_count == 0 for j in range(4))
    assert len(take(t.select(1, 0, 1000, scan=True))) == 0


def test_clustered_table(lib, tbl):
    """The clustered column itself answers ERROR to an update; the other columns update
    normally, and a delete keeps the clustered index's identity positions."""
    t = tbl(dc.tbl5(3000), index_col=0, clustered=True)
    model = t.rows().copy()  # build_index reordered the other columns
    n = 3000
    s = t.select(1, 0, 100, scan=True)
    ids = take(s, free=False)
    assert t.update(0, s, 5) == mq.ERROR
    assert np.array_equal(t.rows(), model)
    assert t.update(3, s, 5) == mq.OK
    model[3] = dc.update_rows(model[3], ids, 5)
    assert np.array_equal(t.rows(), model)
    ix = t.cs[0].index.contents
    v0 = np.ctypeslib.as_array(ix.values, shape=(n,)).copy()
    assert t.delete(s) == mq.OK
    take(s)
    model = dc.delete_rows(model, ids)
    left = n - len(ids)
    assert np.array_equal(t.rows(), model)
    assert np.array_equal(np.ctypeslib.as_array(ix.values, shape=(left,)), np.delete(v0, ids))
    assert np.array_equal(np.ctypeslib.as_array(ix.positions, shape=(left,)), np.arange(left, dtype=np.uint64))
    got = take(t.select(0, 1000, 2000))
    want = np.flatnonzero((np.delete(v0, ids) >= 1000) & (np.delete(v0, ids) < 2000))
    assert np.array_equal(got, want)


def test_out_of_range_id_changes_nothing(lib, tbl):
    model = dc.tbl5(5000)
    t = tbl(model, index_col=0)
    ix = t.cs[0].index.contents
    v0 = np.ctypeslib.as_array(ix.values, shape=(5000,)).copy()
    p0 = np.ctypeslib.as_array(ix.positions, shape=(5000,)).copy()
    for wrong in (5000, -1):
        r = make_result(np.array([1, 2, wrong, 3], np.int32))
        assert t.delete(C.byref(r)) == mq.ERROR
        assert t.update(1, C.byref(r), 9) == mq.ERROR
        free_result_struct(r)
        assert t.t.row_count == 5000 and all(t.cs[j].row_count == 5000 for j in range(4))
        assert np.array_equal(t.rows(), model)
        assert np.array_equal(np.ctypeslib.as_array(ix.values, shape=(5000,)), v0)
        assert np.array_equal(np.ctypeslib.as_array(ix.positions, shape=(5000,)), p0)
    r = make_result(np.array([1.0, 2.0]), mq.DOUBLE)
    assert t.delete(C.byref(r)) == mq.ERROR and t.update(1, C.byref(r), 9) == mq.ERROR
    free_result_struct(r)
    t.cs[2].row_count = 4999  # a column out of step with its table
    r = make_result(np.array([1], np.int32))
    assert t.delete(C.byref(r)) == mq.ERROR
    free_result_struct(r)
    t.cs[2].row_count = 5000
    assert np.array_equal(t.rows(), model)


def test_attached_column_is_detached_not_written(lib, tbl):
    model = dc.tbl5(4000)
    t = tbl(model)
    mine = [Dev.of(model[j]) for j in range(4)]
    for j in range(4):
        mq.check(lib.mq_column_attach(C.byref(t.cs[j]), mine[j].ptr), "attach")
    r = make_result(np.array([5, 6, 7, 3999], np.int32))
    assert t.update(1, C.byref(r), -3) == mq.OK
    want = model.copy()
    want[1] = dc.update_rows(model[1], [5, 6, 7, 3999], -3)
    assert np.array_equal(t.rows(), want)
    assert np.array_equal(take(t.select(1, -3, -2, scan=True)), [5, 6, 7, 3999])
    assert t.delete(C.byref(r)) == mq.OK
    free_result_struct(r)
    want = dc.delete_rows(want, np.array([5, 6, 7, 3999]))
    assert np.array_equal(t.rows(), want)
    assert np.array_equal(take(t.select(3, 0, 2**30, scan=True)), np.arange(3996))
    for j in range(4):  # the caller's buffers keep their old content
        assert np.array_equal(mine[j].get(np.int32, 4000), model[j])
