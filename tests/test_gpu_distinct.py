"""group_count_distinct on gfx950 (mq_group_distinct_plan in csrc/mq_distinct.hip; group_count_distinct
in mq_query.c), every comparison exact equality: with the numpy model of distinctcases.py, with
mq_group_by_where_plan's keys, with mq_keyset_build's COUNT(DISTINCT), and with the chain
mq_group_by_where_plan over (keys.., v) -> mq_group_by_plan over its tuples.

Every case runs on every path whose size rule it satisfies, plus AUTO, without bounds and with
them, and asserts the path taken.
"""
import ctypes as C

import numpy as np
import pytest

import distinctcases as dc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, LDS, BITMAP, SORT = dc.AUTO, dc.LDS, dc.BITMAP, dc.SORT
PAD = 8
KEY_SENT, CNT_SENT = -7, 7777
WHO = b"mq_group_distinct_plan"


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # the drop-in's first operator pins glibc's mmap threshold (see test_gpu_group.py)
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    yield L
    L.mq_test_set_cu_limit(0)


@pytest.fixture(scope="module")
def caps(lib):
    return lib.mq_group_distinct_lds_bytes(), lib.mq_group_distinct_bitmap_bytes()


def c_ranges(ranges):
    return (mq.MqRange * max(len(ranges), 1))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in ranges])


def c_ptrs(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def c_i32(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def upload(arrays, offs=(0,)):
    """One device copy per distinct array object, the k-th distinct one offs[k % len(offs)] dwords
    off a 16-byte boundary."""
    devs, ptrs = {}, []
    for a in arrays:
        if id(a) not in devs:
            devs[id(a)] = Dev.of(a, offset_elems=offs[len(devs) % len(offs)])
        ptrs.append(devs[id(a)].ptr)
    return ptrs, devs


def plan(L, pc, ranges, dks, dv, n, path, kb=None, vb=None, ncols=None, nkeys=None, null_preds=False):
    """(rc, handle, groups, info)"""
    h, groups, info = C.c_void_p(77), C.c_uint64(12345), mq.MqGdistinctInfo()
    rc = L.mq_group_distinct_plan(None if null_preds else c_ptrs(pc), None if null_preds else c_ranges(ranges),
                                  len(pc) if ncols is None else ncols, c_ptrs(dks), len(dks) if nkeys is None else nkeys, dv, n,
                                  c_i32(kb), c_i32(vb), path, C.byref(h), C.byref(groups), C.byref(info), None)
    return rc, h.value, groups.value, info


def written(L, h, g, nkeys, skip_keys=(), skip_count=False, keys_null=False):
    """The outputs of one write into sentinel-filled buffers (None where skipped)."""
    keys = [None if j in skip_keys else Dev.of(np.full(g + PAD, KEY_SENT, np.int32)) for j in range(nkeys)]
    cnt = None if skip_count else Dev.of(np.full(g + PAD, CNT_SENT, np.uint64))
    arr = None if keys_null else (C.c_void_p * nkeys)(*[k.ptr if k else None for k in keys])
    mq.check(L.mq_group_distinct_write(h, arr, cnt.ptr if cnt else None, None), "mq_group_distinct_write")
    return [k.get(np.int32, g + PAD) if k else None for k in keys], cnt.get(np.uint64, g + PAD) if cnt else None


def check_written(got, want, g, tag, keys_written=True):
    keys, cnt = got
    for j, k in enumerate(keys):
        if k is None:
            continue
        if keys_written:
            assert np.array_equal(k[:g], want[0][j]), tag + ("key", j)
            assert np.all(k[g:] == KEY_SENT), tag + ("key", j, "wrote past the groups")
        else:
            assert np.all(k == KEY_SENT), tag + ("key", j, "written though the key array was NULL")
    if cnt is not None:
        assert np.array_equal(cnt[:g], want[1]), tag + ("count",)
        assert np.all(cnt[g:] == CNT_SENT), tag + ("count", "wrote past the groups")


def run(L, pc, ranges, dks, dv, n, path, want, tag, kb=None, vb=None, expect=None, null_preds=False):
    """Plan, check the info, write, compare, free. Returns the info."""
    rc, h, g, info = plan(L, pc, ranges, dks, dv, n, path, kb, vb, null_preds=null_preds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[1]), tag + ("groups", g)
    if expect is not None:
        assert info.path == expect, tag + ("path", info.path)
    if g:
        assert (info.rows, info.pairs) == (want[2], want[3]), tag + ("rows, pairs", info.rows, info.pairs)
    check_written(written(L, h, g, len(dks)), want, g, tag)
    mq.check(L.mq_group_distinct_free(h), "mq_group_distinct_free")
    return info


def refused(L, *args, **kw):
    rc, h, g, _ = plan(L, *args, **kw)
    return (rc, h, g) == (mq.MQ_EINVAL, None, 0) and WHO in L.mq_last_error()


def run_paths(L, caps, cols, ranges, keys, vals, tag, offs=(0,), wide=None, only=None):
    """Every path the bounds allow plus AUTO, without bounds (the plan finds the exact ones) and
    with bounds (the exact ones, or `wide` = (key bounds, value bounds)), against the model."""
    n = len(vals)
    want = dc.model(cols, ranges, keys, vals)
    ptrs, keep = upload(list(cols) + list(keys) + [vals], offs)
    pc, dks, dv = ptrs[:len(cols)], ptrs[len(cols):len(cols) + len(keys)], ptrs[-1]
    exact = dc.matching_bounds(cols, ranges, keys, vals)
    if exact is None:  # no matching row: every path plans nothing
        for path in (AUTO, LDS, BITMAP, SORT):
            assert run(L, pc, ranges, dks, dv, n, path, want, tag + (path,), expect=path or LDS).pairs == 0
        return want
    for kb, vb in ((None, None), wide or exact, (exact[0], None), (None, exact[1])):
        ub = ((kb or exact[0]), (vb or exact[1]))
        auto, ok = dc.paths_of(ub[0], ub[1], *caps)
        for path in [AUTO] + ok:
            if only and path not in only:
                continue
            info = run(L, pc, ranges, dks, dv, n, path, want, tag + (path, kb, vb), kb, vb, expect=path or auto)
            p, w, r, b = dc.shape(*ub)
            assert (info.space, info.span, info.bitmap_bytes) == (p, w, 0 if info.path == SORT else b), tag + (path, kb, vb)
        for path in (LDS, BITMAP):
            if path not in ok:
                assert refused(L, pc, ranges, dks, dv, n, path, kb, vb), tag + ("forced past its rule", path, kb, vb)
    return want


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", dc.ROWS)
def test_rows(lib, caps, n):
    """Wave, tile and unrolled-step edges and several blocks: two predicates, two key columns of
    3 x 4 tuples, 33 values."""
    cols, ranges = dc.predicates(n, 2, seed=n)
    keys, vals = dc.table(n, [3, 4], -5, 33, seed=n)
    run_paths(lib, caps, cols, ranges, keys, vals, ("rows", n))


@pytest.mark.parametrize("n", [1025, 8193])
def test_every_column_off_by_one_element(lib, caps, n):
    cols, ranges = dc.predicates(n, 2, seed=3)
    keys, vals = dc.table(n, [5, 2, 3], 100, 65, seed=4)
    run_paths(lib, caps, cols, ranges, keys, vals, ("offset", n), offs=(1,))


@pytest.mark.parametrize("span", dc.SPANS)
def test_value_span(lib, caps, span):
    """W at R's rounding edges, vlo and vhi present, one group holding all W values: its count is
    W, so no padding bit is counted; bounds one wider on each side change nothing."""
    n = 4097
    keys, vals = dc.table(n, [2, 3], -span // 2, span, seed=span)
    want = run_paths(lib, caps, [], [], keys, vals, ("span", span))
    assert want[1][0] == span and vals.min() == -span // 2 and vals.max() == -span // 2 + span - 1
    run_paths(lib, caps, [], [], keys, vals, ("span", span, "wider"), wide=([-1, 2, -3, 1], [int(vals.min()) - 1, int(vals.max()) + 1]))


def test_equal_rows_and_distinct_rows(lib, caps):
    n = 8193
    keys = [np.full(n, 4, np.int32), np.full(n, -9, np.int32)]
    vals = np.full(n, 123, np.int32)
    want = run_paths(lib, caps, [], [], keys, vals, ("equal",))
    assert want[1].tolist() == [1]
    run_paths(lib, caps, [], [], keys, vals, ("equal", "wide"), wide=([0, 9, -10, -5], [100, 200]))
    # every row a different pair: 7 tuples x 1170 values, shuffled
    i = np.random.default_rng(8).permutation(7 * 1170)
    keys = [np.ascontiguousarray(i % 7, dtype=np.int32), np.zeros(len(i), np.int32)]
    vals = np.ascontiguousarray(i // 7 - 500, dtype=np.int32)
    want = run_paths(lib, caps, [], [], keys, vals, ("distinct",))
    assert want[3] == len(i) and want[1].tolist() == [1170] * 7


def test_wide_bounds_leave_empty_rows_out(lib, caps):
    n = 8193
    cols, ranges = dc.predicates(n, 2, seed=11)
    rng = np.random.default_rng(12)
    keys = [np.ascontiguousarray(rng.choice([3, 17, 40], n), dtype=np.int32), np.ascontiguousarray(rng.choice([-2, 2], n), dtype=np.int32)]
    vals = np.ascontiguousarray(rng.choice([0, 31, 32, 95], n), dtype=np.int32)
    want = run_paths(lib, caps, cols, ranges, keys, vals, ("wide",), wide=([0, 49, -4, 4], [-10, 120]))
    assert len(want[1]) == 6 and set(want[1].tolist()) == {4}
    # a key space of 2^20 rows of one word: many rows a wave in the count kernel
    low = np.ascontiguousarray(vals & 31)
    run_paths(lib, caps, cols, ranges, keys, low, ("wide", "2^20 x 1"), wide=([0, 1023, -512, 511], [0, 31]), only=(AUTO, BITMAP))
    # rows of 17 and of 5000 words: a wave a row, and a row in two pieces
    run_paths(lib, caps, cols, ranges, keys, vals, ("wide", "17 words"), wide=([0, 49, -4, 4], [-1, 32 * 17 - 2]), only=(BITMAP,))
    run_paths(lib, caps, cols, ranges, keys, vals, ("wide", "5000 words"), wide=([0, 49, -4, 4], [-60_000, 99_999]), only=(BITMAP,))


def test_extreme_keys(lib, caps):
    """Keys and values at both int32 ends: a key range of 2^32 beside a constant key, either way
    round (a stride of 2^32 that the code holds as 0)."""
    n = 4097
    rng = np.random.default_rng(13)
    ends = np.ascontiguousarray(rng.choice([dc.I32_MIN, dc.I32_MIN + 1, -1, 0, dc.I32_MAX], n), dtype=np.int32)
    const = np.full(n, -77, np.int32)
    vals = np.ascontiguousarray(rng.choice([dc.I32_MIN, 5, dc.I32_MAX], n), dtype=np.int32)
    cols, ranges = dc.predicates(n, 2, seed=14)
    for keys in ([ends, const], [const, ends], [ends]):
        want = run_paths(lib, caps, cols, ranges, keys, vals, ("ends", len(keys)))
        assert want[1].tolist() == [3] * 5
    small = np.ascontiguousarray(rng.integers(0, 3, n), dtype=np.int32)
    ptrs, keep = upload([ends, small, vals])
    assert refused(lib, [], [], ptrs[:2], ptrs[2], n, AUTO) and b"2^32" in lib.mq_last_error()


def test_full_span_is_the_512_mib_bitmap(lib, caps):
    """P = 1 and values over the whole of int32: BITMAP exactly at its cap, one row over many blocks."""
    n = 8193
    vals = np.ascontiguousarray(np.random.default_rng(15).integers(dc.I32_MIN, dc.I32_MAX, n, endpoint=True), dtype=np.int32)
    vals[7], vals[8000], vals[9] = dc.I32_MIN, dc.I32_MAX, vals[10]
    keys = [np.full(n, 42, np.int32)]
    want = dc.model([], [], keys, vals)
    assert want[1].tolist() == [len(np.unique(vals))]
    ptrs, keep = upload(keys + [vals])
    full = [dc.I32_MIN, dc.I32_MAX]
    for path, vb in ((AUTO, None), (BITMAP, full), (SORT, full)):
        info = run(lib, [], [], ptrs[:1], ptrs[1], n, path, want, ("full span", path), [42, 42] if vb else None, vb,
                   expect=path or BITMAP)
        assert info.span == 2**32 and info.bitmap_bytes == (0 if path == SORT else caps[1])
    assert refused(lib, [], [], ptrs[:1], ptrs[1], n, LDS, [42, 42], full)
    assert refused(lib, [], [], ptrs[:1], ptrs[1], n, BITMAP, [42, 43], full)  # P = 2: past the cap


@pytest.mark.parametrize("ncols", [0, 2, 8])
def test_predicates_and_rows_that_fail_them(lib, caps, ncols):
    """A key and a value far outside the given bounds on a row that fails a predicate is fine; on a
    matching row it is MQ_EINVAL, and a later plan still works."""
    n = 8215
    cols, ranges = dc.predicates(n, ncols, seed=20 + ncols)
    keys, vals = dc.table(n, [4, 3], 10, 40, seed=21)
    m = dc.mask(cols, ranges, n)
    kb, vb = [0, 3, -2, 0], [10, 49]
    dead = np.flatnonzero(~m)
    for i, row in enumerate(dead):  # every failing row carries a stray component
        j, kind = i % 3, (i // 3) % 4
        stray = [kb[2 * j] - 1 if j < 2 else vb[0] - 1, kb[2 * j + 1] + 1 if j < 2 else vb[1] + 1, dc.I32_MIN, dc.I32_MAX][kind]
        (keys[j] if j < 2 else vals)[row] = stray
    want = run_paths(lib, caps, cols, ranges, keys, vals, ("dead rows", ncols), wide=(kb, vb)) if ncols else None
    ptrs, keep = upload(cols + keys + [vals])
    pc, dks, dv = ptrs[:ncols], ptrs[ncols:ncols + 2], ptrs[-1]
    if not ncols:  # NULL predicate arrays
        want = dc.model([], [], keys, vals)
        for path in (AUTO, LDS, BITMAP, SORT):
            run(lib, pc, ranges, dks, dv, n, path, want, ("no predicates", path), kb, vb, expect=path or LDS, null_preds=True)
            run(lib, pc, ranges, dks, dv, n, path, want, ("no predicates", path, "NULL bounds"), null_preds=True)
    live = np.flatnonzero(m)
    for which, stray in ((0, 4), (1, -3), (2, 50), (2, 9)):
        k2, v2 = [k.copy() for k in keys], vals.copy()
        (k2[which] if which < 2 else v2)[live[len(live) // 2]] = stray
        p2, keep2 = upload(k2 + [v2])
        for path in (AUTO, LDS, BITMAP, SORT):
            assert refused(lib, pc, ranges, p2[:2], p2[2], n, path, kb, vb), (ncols, which, stray, path)
        run(lib, pc, ranges, p2[:2], p2[2], n, AUTO, dc.model(cols, ranges, k2, v2), ("NULL bounds", which, stray))
    run(lib, pc, ranges, dks, dv, n, AUTO, want, ("after the errors", ncols), kb, vb)


def test_empty_outcomes(lib, caps):
    n = 4097
    cols, _ = dc.predicates(n, 2, seed=30)
    keys, vals = dc.table(n, [4, 3], 10, 40, seed=31)
    for ranges in ([(2000, 3000), (None, None)], [(7, 7), (None, None)], [(None, None), (None, dc.I32_MIN)]):
        want = run_paths(lib, caps, cols, ranges, keys, vals, ("empty", ranges))
        assert len(want[1]) == 0
        ptrs, keep = upload(cols + keys + [vals])
        for path in (AUTO, SORT):  # given bounds change nothing
            run(lib, ptrs[:2], ranges, ptrs[2:4], ptrs[4], n, path, want, ("empty", "bounds", path), [0, 3, -2, 0], [10, 49])
    e = np.empty(0, np.int32)
    want = dc.model([], [], [e, e], e)
    for path in (AUTO, LDS, BITMAP, SORT):
        rc, h, g, info = plan(lib, [None], [(0, 5)], [None, None], None, 0, path, kb=[3, 1, 0, 0])  # NULL columns, any bounds
        assert (rc, g, info.path) == (mq.MQ_OK, 0, path or LDS) and h
        mq.check(lib.mq_group_distinct_write(h, None, None, None), "write")
        mq.check(lib.mq_group_distinct_free(h), "free")


@pytest.mark.parametrize("nkeys", [1, 3, 4])
def test_nkeys_and_aliased_columns(lib, caps, nkeys):
    n = 8193
    cols, ranges = dc.predicates(n, 2, seed=40)
    cols[0] = np.ascontiguousarray(cols[0] % 12, dtype=np.int32)
    ranges[0] = (2, 11)
    keys, vals = dc.table(n, [3, 2, 4, 2][:nkeys], -8, 20, seed=41)
    run_paths(lib, caps, cols, ranges, keys, vals, ("nkeys", nkeys))
    want = run_paths(lib, caps, cols, ranges, keys[:-1] + [vals], vals, ("the last key is the value column", nkeys))
    assert set(want[1].tolist()) == {1}
    run_paths(lib, caps, cols, ranges, [cols[0]] + keys[1:], vals, ("the first key is a predicate column", nkeys))
    run_paths(lib, caps, cols, ranges, keys, cols[0], ("the values are a predicate column", nkeys))


@pytest.fixture
def one_cu(lib):
    """One CU for the geometry during the test; the hardware count is back afterwards."""
    mq.check(lib.mq_device_sync(), "mq_device_sync")
    mq.check(lib.mq_test_set_cu_limit(1), "mq_test_set_cu_limit")
    try:
        yield
    finally:
        lib.mq_device_sync()
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_many_blocks_one_bit(lib, caps, one_cu):
    """300 007 rows on one limited CU: a block takes many steps, and several blocks merge the same
    LDS words: a few hot pairs that every block sees, and a sprinkle of others."""
    n = dc.LONG_N
    blocks, rpb = C.c_uint32(), C.c_uint64()
    lib.mq_scan_geometry(n, C.byref(blocks), C.byref(rpb))
    assert blocks.value <= 8 and rpb.value >= 3 * 8192, (blocks.value, rpb.value)
    cols, ranges = dc.predicates(n, 2, seed=50)
    rng = np.random.default_rng(51)
    hot = rng.random(n) < 0.9
    keys = [np.ascontiguousarray(np.where(hot, 1, rng.integers(0, 3, n)), dtype=np.int32),
            np.ascontiguousarray(np.where(hot, 5, rng.integers(4, 8, n)), dtype=np.int32)]
    vals = np.ascontiguousarray(np.where(hot, 17, rng.integers(0, 100, n)), dtype=np.int32)
    run_paths(lib, caps, cols, ranges, keys, vals, ("one cu",), offs=(0, 1, 0))


def test_sort_path_chunk_edges(lib, caps):
    """One group longer than a chunk of the sort path's passes, with equal pairs across the chunk
    boundaries; then groups and pairs that end exactly at a boundary."""
    n = 5000
    blocks, chunk = C.c_uint32(), C.c_uint64()
    lib.mq_group_sort_geometry(n, C.byref(blocks), C.byref(chunk))
    chunk = chunk.value
    assert blocks.value >= 3 and chunk < n // 2
    for cut in (0, 1, 7):
        # sorted by (key, value): rows [0, 10) one small group; then one group of 2 * chunk + 50 rows whose value
        # changes `cut` rows after each chunk boundary it spans; then single rows
        long_end = 10 + 2 * chunk + 50
        key = np.empty(n, np.int32)
        key[:10], key[10:long_end] = -4, 3
        key[long_end:] = 100 + np.arange(n - long_end) // 3
        vals = np.zeros(n, np.int32)
        vals[:10] = np.arange(10) // 2
        i = np.arange(10, long_end)
        vals[10:long_end] = (i >= chunk + cut).astype(np.int32) + (i >= 2 * chunk + cut)
        vals[long_end:] = np.arange(n - long_end) % 2
        perm = np.random.default_rng(cut).permutation(n)
        keys = [np.ascontiguousarray(key[perm]), np.ascontiguousarray(-key[perm])]
        v = np.ascontiguousarray(vals[perm] * 1000)
        want = run_paths(lib, caps, [], [], keys, v, ("chunk edges", cut), only=(SORT,))
        assert want[1][1] == 3 and want[1][0] == 5
    # group edges at the chunk boundaries: groups of exactly chunk rows, each of 2 values
    key = (np.arange(n) // chunk).astype(np.int32)
    v = ((np.arange(n) % chunk) >= chunk // 2).astype(np.int32)
    perm = np.random.default_rng(9).permutation(n)
    run_paths(lib, caps, [], [], [np.ascontiguousarray(key[perm])], np.ascontiguousarray(v[perm]), ("edges at boundaries",), only=(SORT,))


def test_only_the_sort_path_can_take_it(lib, caps):
    """Two key columns of range 2^15 each and values over 2^20."""
    n = 70_001
    rng = np.random.default_rng(60)
    pool = rng.integers(0, 2**15, (500, 2))
    pick = rng.integers(0, 500, n)
    keys = [np.ascontiguousarray(pool[pick, j], dtype=np.int32) for j in range(2)]
    keys[0][0], keys[0][1], keys[1][2], keys[1][3] = 0, 2**15 - 1, 0, 2**15 - 1
    vals = np.ascontiguousarray(rng.integers(0, 2**20, n) // 4096 * 4096 + rng.integers(0, 3, n), dtype=np.int32)
    vals[4], vals[5] = 0, 2**20 - 1
    cols, ranges = dc.predicates(n, 1, seed=61)
    cols[0][:6] = 500
    kb, vb = dc.matching_bounds(cols, ranges, keys, vals)
    assert dc.shape(kb, vb)[:2] == (2**30, 2**20) and dc.paths_of(kb, vb, *caps) == (SORT, [SORT])
    want = run_paths(lib, caps, cols, ranges, keys, vals, ("sort only",))
    assert len(want[1]) > 400 and want[1].max() > 10


def test_write_null_outputs_and_repeats(lib, caps):
    n = 4097
    cols, ranges = dc.predicates(n, 2, seed=70)
    keys, vals = dc.table(n, [3, 2, 2], 0, 70, seed=71)
    want = dc.model(cols, ranges, keys, vals)
    ptrs, keep = upload(cols + keys + [vals])
    for path in (LDS, BITMAP, SORT):
        rc, h, g, info = plan(lib, ptrs[:2], ranges, ptrs[2:5], ptrs[5], n, path)
        assert rc == mq.MQ_OK and g == len(want[1]) and info.path == path
        first = written(lib, h, g, 3)
        check_written(first, want, g, (path, "all"))
        for j in range(3):
            check_written(written(lib, h, g, 3, skip_keys=(j,)), want, g, (path, "no key", j))
        check_written(written(lib, h, g, 3, skip_keys=(0, 1, 2)), want, g, (path, "no keys"))
        check_written(written(lib, h, g, 3, keys_null=True), want, g, (path, "NULL key array"), keys_written=False)
        check_written(written(lib, h, g, 3, skip_count=True), want, g, (path, "no count"))
        mq.check(lib.mq_group_distinct_write(h, None, None, None), "a write of nothing")
        again = written(lib, h, g, 3)
        assert b"".join(a.tobytes() for a in first[0] + [first[1]]) == b"".join(a.tobytes() for a in again[0] + [again[1]])
        mq.check(lib.mq_group_distinct_free(h), "free")
    assert lib.mq_group_distinct_write(None, None, None, None) == mq.MQ_EINVAL
    mq.check(lib.mq_group_distinct_free(None), "free(NULL)")


def test_errors_allocate_nothing(lib, caps):
    n = 1025
    cols, ranges = dc.predicates(n, 2, seed=80)
    keys, vals = dc.table(n, [4, 3], 10, 40, seed=81)
    ptrs, keep = upload(cols + keys + [vals])
    pc, dks, dv = ptrs[:2], ptrs[2:4], ptrs[4]
    kb, vb = [0, 3, -2, 0], [10, 49]
    assert refused(lib, pc, ranges, dks, dv, 2**31, AUTO)
    assert refused(lib, [pc[0], None], ranges, dks, dv, n, AUTO)
    assert refused(lib, [pc[0], pc[1] + 2], ranges, dks, dv, n, AUTO)
    assert refused(lib, pc, ranges, [dks[0], None], dv, n, AUTO)
    assert refused(lib, pc, ranges, [dks[0] + 1, dks[1]], dv, n, AUTO)
    assert refused(lib, pc, ranges, dks, None, n, AUTO)
    assert refused(lib, pc, ranges, dks, dv + 2, n, AUTO)
    for path in (4, -1):
        assert refused(lib, pc, ranges, dks, dv, n, path)
    assert refused(lib, pc, ranges, dks, dv, n, AUTO, [0, 3, 1, 0], vb)
    assert refused(lib, pc, ranges, dks, dv, n, AUTO, kb, [5, 4])
    assert refused(lib, pc, ranges, dks, dv, n, AUTO, [0, 3, 1, 0])           # checked though the value bounds are missing
    assert refused(lib, pc, ranges, dks, dv, n, AUTO, [dc.I32_MIN, dc.I32_MAX, 0, 1], vb) and b"2^32" in lib.mq_last_error()
    assert refused(lib, pc, ranges, dks, dv, n, LDS, [0, 2**12, -2, 0], vb)    # a forced path past its rule
    assert refused(lib, pc, ranges, dks, dv, n, BITMAP, [0, 2**26, -2, 0], vb)
    for ncols in (-1, 9):
        assert refused(lib, (pc * 5)[:9], (ranges * 5)[:9], dks, dv, n, AUTO, ncols=ncols)
    for nkeys in (0, -1, 5):
        assert refused(lib, pc, ranges, (dks * 3)[:5], dv, n, AUTO, nkeys=nkeys)
    h, groups = C.c_void_p(77), C.c_uint64(77)
    cp, cr, ck = c_ptrs(pc), c_ranges(ranges), c_ptrs(dks)
    for args in ((None, cr, 2, ck), (cp, None, 2, ck), (cp, cr, 2, None)):
        h.value, groups.value = 77, 77
        assert lib.mq_group_distinct_plan(*args, 2, dv, n, None, None, AUTO, C.byref(h), C.byref(groups), None, None) == mq.MQ_EINVAL
        assert (h.value, groups.value) == (None, 0)
    assert lib.mq_group_distinct_plan(cp, cr, 2, ck, 2, dv, n, None, None, AUTO, None, C.byref(groups), None, None) == mq.MQ_EINVAL
    assert lib.mq_group_distinct_plan(cp, cr, 2, ck, 2, dv, n, None, None, AUTO, C.byref(h), None, None, None) == mq.MQ_EINVAL
    assert h.value is None
    # h_info may be NULL; and the operator still works
    assert lib.mq_group_distinct_plan(cp, cr, 2, ck, 2, dv, n, None, None, AUTO, C.byref(h), C.byref(groups), None, None) == mq.MQ_OK
    want = dc.model(cols, ranges, keys, vals)
    assert groups.value == len(want[1])
    mq.check(lib.mq_group_distinct_free(h), "free")
    run(lib, pc, ranges, dks, dv, n, AUTO, want, ("after the errors",))


# ---------------------------------------------------------------------------
# against the operators that are there already
# ---------------------------------------------------------------------------

def by_where(L, pc, ranges, dks, dv, n, nkeys):
    """mq_group_by_where_plan -> (groups, key outputs, counts)"""
    h, groups = C.c_void_p(), C.c_uint64()
    mq.check(L.mq_group_by_where_plan(c_ptrs(pc), c_ranges(ranges), len(pc), c_ptrs(dks), nkeys, dv, n, None, mq.MQ_GROUP_AUTO,
                                      C.byref(h), C.byref(groups), None, None, None), "mq_group_by_where_plan")
    g = groups.value
    keys = [Dev.of(np.zeros(g + 1, np.int32)) for _ in range(nkeys)]
    cnt = Dev.of(np.zeros(g + 1, np.uint64))
    mq.check(L.mq_group_by_write(h, (C.c_void_p * nkeys)(*[k.ptr for k in keys]), cnt.ptr, None, None, None, None), "write")
    out = [k.get(np.int32, g) for k in keys], cnt.get(np.uint64, g)
    mq.check(L.mq_group_free(h), "free")
    return g, out[0], out[1], keys


@pytest.mark.parametrize("nkeys", [1, 2, 3])
def test_against_group_by_where_and_the_chain(lib, caps, nkeys):
    """The key outputs are mq_group_by_where_plan's on the same inputs; and the result is that of
    the chain: mq_group_by_where_plan over (keys.., v) as one more key, then mq_group_by_plan over
    those tuples' key part for their count."""
    n = 70_001
    cols, ranges = dc.predicates(n, 2, seed=90)
    keys, vals = dc.table(n, [5, 7, 3][:nkeys], -100, 300, seed=91)
    want = dc.model(cols, ranges, keys, vals)
    ptrs, keep = upload(cols + keys + [vals], (0, 1))
    pc, dks, dv = ptrs[:2], ptrs[2:2 + nkeys], ptrs[-1]
    g0, ref_keys, _, _ = by_where(lib, pc, ranges, dks, dv, n, nkeys)
    g1, tuples, _, tuple_devs = by_where(lib, pc, ranges, dks + [dv], dv, n, nkeys + 1)
    assert g1 == want[3]
    h, groups = C.c_void_p(), C.c_uint64()
    tp = [d.ptr for d in tuple_devs[:nkeys]]
    mq.check(lib.mq_group_by_plan(c_ptrs(tp), nkeys, tp[0], g1, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups), None, None)
             if nkeys > 1 else
             lib.mq_group_plan(tp[0], tp[0], g1, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups), None, None), "chain")
    chain_cnt = Dev.of(np.zeros(groups.value + 1, np.uint64))
    mq.check(lib.mq_group_by_write(h, None, chain_cnt.ptr, None, None, None, None), "chain write")
    chain = chain_cnt.get(np.uint64, groups.value)
    mq.check(lib.mq_group_free(h), "free")
    for path in (AUTO, BITMAP, SORT):
        rc, h, g, info = plan(lib, pc, ranges, dks, dv, n, path)
        assert rc == mq.MQ_OK and g == g0 == groups.value
        got_keys, got_cnt = written(lib, h, g, nkeys)
        assert all(np.array_equal(a[:g], b) for a, b in zip(got_keys, ref_keys)), (nkeys, path)
        assert np.array_equal(got_cnt[:g], chain) and np.array_equal(chain, want[1]), (nkeys, path)
        mq.check(lib.mq_group_distinct_free(h), "free")


def test_one_constant_key_is_the_key_set_count(lib, caps):
    n = 70_001
    vals = np.ascontiguousarray(np.random.default_rng(95).integers(-5000, 5000, n), dtype=np.int32)
    keys = [np.full(n, 9, np.int32)]
    ptrs, keep = upload(keys + [vals], (1,))
    ks, ki = C.c_void_p(), mq.MqKeysetInfo()
    mq.check(lib.mq_keyset_build(ptrs[1], n, 0, 0, 0, C.byref(ks), C.byref(ki), None), "mq_keyset_build")
    mq.check(lib.mq_keyset_free(ks), "mq_keyset_free")
    assert ki.distinct == len(np.unique(vals))
    for path in (AUTO, LDS, BITMAP, SORT):
        rc, h, g, info = plan(lib, [], [], ptrs[:1], ptrs[1], n, path, null_preds=True)
        assert rc == mq.MQ_OK and g == 1 and info.pairs == ki.distinct and info.rows == n
        assert written(lib, h, g, 1)[1][0] == ki.distinct
        mq.check(lib.mq_group_distinct_free(h), "free")


# ---------------------------------------------------------------------------
# the drop-in
# ---------------------------------------------------------------------------

def gcol(obj):
    g = mq.GeneralizedColumn()
    if isinstance(obj, mq.Column):
        g.column_type = mq.COLUMN
        g.column_pointer.column = C.pointer(obj)
    else:
        g.column_type = mq.RESULT
        g.column_pointer.result = obj if isinstance(obj, C.POINTER(mq.Result)) else C.pointer(obj)
    return g


def _b(v):
    return None if v is None else C.pointer(C.c_int(int(v)))


def dropin(L, objs, ranges, keys, values, ncols=None, nkeys=None, null_preds=False):
    """group_count_distinct -> (status, the nkeys + 1 Results as (data_type, numpy array) or None)"""
    gs = [gcol(o) for o in objs]
    m = max(len(gs), 1)
    gp = (C.POINTER(mq.GeneralizedColumn) * m)(*[C.pointer(g) for g in gs])
    lows = (C.POINTER(C.c_int) * m)(*[_b(lo) for lo, _ in ranges])
    highs = (C.POINTER(C.c_int) * m)(*[_b(hi) for _, hi in ranges])
    gks, gv, st = [gcol(k) for k in keys], gcol(values), mq.Status(0, None)
    arr = (C.POINTER(mq.GeneralizedColumn) * max(len(gks), 1))(*[C.pointer(g) for g in gks])
    nkeys = len(keys) if nkeys is None else nkeys
    if null_preds:
        gp = lows = highs = None
    rpp = L.group_count_distinct(gp, lows, highs, len(objs) if ncols is None else ncols, arr, nkeys, C.byref(gv), C.byref(st))
    if not rpp:
        return st.code, None
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(nkeys + 1)]
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def check_results(out, want, tag):
    nkeys = len(want[0])
    assert [t for t, _ in out] == [mq.INT] * nkeys + [mq.LONG], tag
    for i, ((_, got), w) in enumerate(zip(out, list(want[0]) + [want[1]])):
        assert len(got) == len(w) and np.array_equal(got, w.astype(got.dtype)), tag + (i,)


def test_dropin_equals_the_device_api(lib, caps):
    n = 70_001
    cols, ranges = dc.predicates(n, 3, seed=100)
    keys, vals = dc.table(n, [6, 5, 2], -40, 500, seed=101)
    want = dc.model(cols, ranges, keys, vals)
    ptrs, keep = upload(cols + keys + [vals])
    rc, h, g, info = plan(lib, ptrs[:3], ranges, ptrs[3:6], ptrs[6], n, AUTO)
    assert rc == mq.MQ_OK
    dev_keys, dev_cnt = written(lib, h, g, 3)
    mq.check(lib.mq_group_distinct_free(h), "free")
    cc, ck, cv = [make_column(c) for c in cols], [make_column(k) for k in keys], make_column(vals)
    code, out = dropin(lib, cc, ranges, ck, cv)
    assert code == mq.OK
    check_results(out, want, ("columns",))
    assert all(np.array_equal(o[1], d[:g]) for o, d in zip(out, dev_keys)) and np.array_equal(out[3][1].astype(np.uint64), dev_cnt[:g])
    # INT Results: two with an HBM shadow, one of the caller's own
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    f1 = lib.fetch_column(C.byref(cc[1]), C.byref(every), C.byref(st))
    fk = lib.fetch_column(C.byref(ck[0]), C.byref(every), C.byref(st))
    assert st.code == mq.OK and f1 and fk
    rv = make_result(vals)
    code, out = dropin(lib, [cc[0], f1, cc[2]], ranges, [fk] + ck[1:], rv)
    assert code == mq.OK
    check_results(out, want, ("results",))
    # no predicates: NULL arrays
    full = dc.model([], [], keys[:2], vals)
    for null_preds in (True, False):
        code, out = dropin(lib, [], [], ck[:2], cv, null_preds=null_preds)
        assert code == mq.OK
        check_results(out, full, ("ncols == 0", null_preds))
    code, out = dropin(lib, cc, ranges, ck[:1], ck[0])  # the values are the key
    assert code == mq.OK
    check_results(out, dc.model(cols, ranges, keys[:1], keys[0]), ("values = key",))
    for r in (f1, fk):
        take(r)
    for r in (every, rv):
        free_result_struct(r)
    for c in cc + ck + [cv]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_outcomes_and_errors(lib, caps, capfd):
    n = 1000
    cols, ranges = dc.predicates(n, 2, seed=110)
    keys, vals = dc.table(n, [4, 3], 0, 50, seed=111)
    cc, ck, cv = [make_column(c) for c in cols], [make_column(k) for k in keys], make_column(vals)
    empty = dc.model(cols, [(7, 7), (None, None)], keys, vals)
    for none in ([(7, 7), (None, None)], [(2000, 3000), (0, 1000)]):
        code, out = dropin(lib, cc, none, ck, cv)
        assert code == mq.OK
        check_results(out, empty, ("empty", none))
    e = np.empty(0, np.int32)
    ce = make_column(e)
    code, out = dropin(lib, [ce, ce], ranges, [ce, ce, ce], ce)
    assert code == mq.OK
    check_results(out, dc.model([], [], [e, e, e], e), ("no rows",))
    short = make_column(cols[0][:999].copy())
    lng = make_result(cols[0].astype(np.int64), mq.LONG)
    ends = make_column(np.ascontiguousarray(np.where(np.arange(n) % 2, dc.I32_MIN, dc.I32_MAX), dtype=np.int32))
    capfd.readouterr()

    def refused_dropin(call):
        return call == (mq.ERROR, None) and "libmq" in capfd.readouterr().err

    assert refused_dropin(dropin(lib, cc, ranges, ck, cv, ncols=-1))
    assert refused_dropin(dropin(lib, cc * 5, ranges * 5, ck, cv, ncols=9))
    assert refused_dropin(dropin(lib, cc, ranges, ck * 3, cv, nkeys=0))
    assert refused_dropin(dropin(lib, cc, ranges, ck * 3, cv, nkeys=5))
    assert refused_dropin(dropin(lib, [cc[0], short], ranges, ck, cv))   # different lengths
    assert refused_dropin(dropin(lib, cc, ranges, [ck[0], short], cv))
    assert refused_dropin(dropin(lib, cc, ranges, ck, short))
    assert refused_dropin(dropin(lib, [cc[0], lng], ranges, ck, cv))     # a LONG Result as a column
    assert refused_dropin(dropin(lib, cc, ranges, [lng, ck[1]], cv))     # ... as a key
    assert refused_dropin(dropin(lib, cc, ranges, ck, lng))              # ... as values
    code, out = dropin(lib, cc, [(None, None), (None, None)], [ends, ck[0]], cv)  # a key space wider than 2^32
    err = capfd.readouterr().err
    assert (code, out) == (mq.ERROR, None) and "libmq" in err and "2^32" in err
    gks = [gcol(k) for k in ck]
    arr = (C.POINTER(mq.GeneralizedColumn) * 2)(*[C.pointer(g) for g in gks])
    st = mq.Status(0, None)
    assert not lib.group_count_distinct(None, None, None, 0, arr, 2, None, C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_count_distinct(None, None, None, 0, None, 2, C.byref(gks[0]), C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_count_distinct(None, None, None, 2, arr, 2, C.byref(gks[0]), C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 3
    code, out = dropin(lib, cc, ranges, ck, cv)  # and the operator still works
    assert code == mq.OK
    check_results(out, dc.model(cols, ranges, keys, vals), ("after the errors",))
    free_result_struct(lng)
    for c in cc + ck + [cv, ce, short, ends]:
        lib.mq_column_invalidate(C.byref(c))
