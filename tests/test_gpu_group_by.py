"""GROUP BY over two to four key columns on gfx950 (mq_group_by_plan / _write in
csrc/mq_group.hip; group_aggregate_by in mq_query.c), every comparison exact equality with
the numpy restatement in groupbycases.py (the reference has no such operator).

gc.SIZES (up to 300 001 rows) reach both paths, the ragged last tile, several blocks and the
tail tiles of a chunk; on the whole device a block of k_group_by_dense or k_group_by_pack gets
too few rows there to run its unrolled loop more than once, so the long-chunk tests lower the
CU count the geometry uses (mq_test_set_cu_limit) and assert their regime first.
"""
import ctypes as C

import numpy as np
import pytest

import groupbycases as gb
import groupcases as gc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PAD = 8
KEY_SENT = -7
SENT = {"count": 7, "sum": -77, "min": -777, "max": 777}
DTYPE = {"count": np.uint64, "sum": np.int64, "min": np.int32, "max": np.int32}
AGGS = ["count", "sum", "min", "max"]


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # pin glibc's mmap threshold through the drop-in's first operator (see test_gpu_group.py)
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    yield L
    L.mq_test_set_cu_limit(0)


@pytest.fixture(scope="module")
def S(lib):
    return lib.mq_group_dense_slots()


def auto_path(L, bounds):
    b = (C.c_int32 * len(bounds))(*bounds)
    return L.mq_group_by_auto_path(b, len(bounds) // 2, None)


def plan(L, dks, dv, n, path, bounds=None, stream=None):
    """(rc, handle, groups, path taken); dks: the key columns' device pointers"""
    h, groups, taken = C.c_void_p(), C.c_uint64(12345), C.c_int(-1)
    keys = (C.c_void_p * len(dks))(*dks)
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    rc = L.mq_group_by_plan(keys, len(dks), dv, n, b, path, C.byref(h), C.byref(groups), C.byref(taken), stream)
    return rc, h.value, groups.value, taken.value


def out_buffers(g, nkeys, skip_keys=(), skip=()):
    """Sentinel-filled device buffers, PAD entries longer than the groups: one per key column
    (None where skipped) and one per aggregate."""
    keys = [None if j in skip_keys else Dev.of(np.full(g + PAD, KEY_SENT, np.int32)) for j in range(nkeys)]
    aggs = {nm: None if nm in skip else Dev.of(np.full(g + PAD, SENT[nm], DTYPE[nm])) for nm in AGGS}
    return keys, aggs


def write(L, h, keys, aggs, keys_null=False, stream=None):
    arr = None if keys_null else (C.c_void_p * len(keys))(*[k.ptr if k else None for k in keys])
    return L.mq_group_by_write(h, arr, *[aggs[nm].ptr if aggs[nm] else None for nm in AGGS], stream)


def check_outputs(keys, aggs, g, want, tag, keys_written=True):
    for j, (k, w) in enumerate(zip(keys, want[0])):
        if k is None:
            continue
        got = k.get(np.int32, g + PAD)
        if keys_written:
            assert np.array_equal(got[:g], w), tag + ("key", j)
            assert np.all(got[g:] == KEY_SENT), tag + ("key", j, "wrote past the groups")
        else:
            assert np.all(got == KEY_SENT), tag + ("key", j, "written though the key array was NULL")
    for nm, w in zip(AGGS, want[1:]):
        if aggs[nm] is None:
            continue
        got = aggs[nm].get(DTYPE[nm], g + PAD)
        assert np.array_equal(got[:g], w), tag + (nm,)
        assert np.all(got[g:] == SENT[nm]), tag + (nm, "wrote past the groups")


def run(L, dks, dv, n, path, want, tag, bounds=None, skip_keys=(), skip=(), keys_null=False):
    rc, h, g, taken = plan(L, dks, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (mq.load().mq_last_error(),)
    assert g == len(want[1]), tag
    keys, aggs = out_buffers(g, len(dks), skip_keys, skip)
    mq.check(write(L, h, keys, aggs, keys_null), "mq_group_by_write")
    check_outputs(keys, aggs, g, want, tag, keys_written=not keys_null)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


def paths_for(L, S, bounds):
    """The paths a key space allows and the one AUTO takes."""
    space = gb.space_of(bounds)
    assert space <= 2**32
    auto = DENSE if space <= S else SORT
    assert auto_path(L, bounds) == auto
    return ((AUTO, DENSE, SORT) if auto == DENSE else (AUTO, SORT)), auto


# ---------------------------------------------------------------------------
# 1. the paths against the restatement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", gc.SIZES)
@pytest.mark.parametrize("tset", gb.TUPLE_SETS)
def test_paths_agree_with_the_restatement(lib, S, tset, n):
    """nkeys = 2, 3, 4 under every path the key space allows, in three layouts: everything
    16-byte aligned (the dwordx4 kernels); key columns and values 0 or 1 dword off a 16-byte
    boundary independently (the dword kernels); and the value column being the last key
    column, the same pointer. The same exact answer, nothing written past the groups, and
    the path reported is the one mq_group_by_auto_path predicts from the columns' ranges."""
    for nkeys in (2, 3, 4):
        cols = gb.tuples_of(tset, n, nkeys, S)
        vals = gc.values_of("uniform", cols[0])
        bounds = gb.bounds_of(cols)
        paths, auto = paths_for(lib, S, bounds) if n else ((AUTO, DENSE, SORT), DENSE)
        if tset == "space_S" and n >= 2:
            assert auto == DENSE and gb.space_of(bounds) == S
        if tset in ("space_S_plus_1", "ends_x_one") and n >= 2:
            assert auto == SORT and gb.space_of(bounds) == (S + 1 if tset == "space_S_plus_1" else 2**32)
        offs = [(n + nkeys + j) & 1 for j in range(nkeys)]
        if not any(offs):
            offs[-1] = 1
        for layout, koffs, voff in (("aligned", [0] * nkeys, 0), ("offset", offs, (n >> 1) & 1), ("vals_is_key", offs, None)):
            dks = [Dev.of(c, offset_elems=o) for c, o in zip(cols, koffs)]
            dv = dks[-1] if voff is None else Dev.of(vals, offset_elems=voff)
            want = gb.group_by(cols, cols[-1] if voff is None else vals)
            for path in paths:
                tag = (tset, n, nkeys, layout, path)
                taken = run(lib, [d.ptr for d in dks], dv.ptr, n, path, want, tag)
                if n:
                    assert taken == (path if path != AUTO else auto), tag
            if n and auto == SORT:
                rc, h, g, _ = plan(lib, [d.ptr for d in dks], dv.ptr, n, DENSE)
                assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), (tset, n, nkeys, layout, "DENSE forced past S")


# ---------------------------------------------------------------------------
# 2. every component is checked against its own bounds
# ---------------------------------------------------------------------------

def _in_bounds(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(2, 8, n).astype(np.int32), rng.integers(1, 9, n).astype(np.int32)]


@pytest.mark.parametrize("stray", [(3, 12), (3, -1)])
@pytest.mark.parametrize("where", ["full_tile", "ragged_tile", "whole_wave_tile"])
def test_component_wise_bounds(lib, stray, where):
    """Bounds {0,9, 0,9} and one row whose tuple is (3, 12) or (3, -1): the summed slot, 42 or
    29, lies inside the 100-slot table, the second component does not lie in its bounds. Both
    paths must refuse the plan. The stray row sits in a full tile, in the ragged last tile, or
    fills a whole 256-row wave tile (which the dense kernel folds as a run)."""
    n = 4097
    bounds = [0, 9, 0, 9]
    assert 0 <= stray[0] * 10 + stray[1] < 100
    cols = _in_bounds(n, 3)
    rows = {"full_tile": slice(1000, 1001), "ragged_tile": slice(n - 1, n), "whole_wave_tile": slice(1024, 1280)}[where]
    cols[0][rows], cols[1][rows] = stray
    vals = gc.values_of("uniform", cols[0])
    dks, dv = [Dev.of(c) for c in cols], Dev.of(vals)
    for path in (DENSE, SORT, AUTO):
        rc, h, g, _ = plan(lib, [d.ptr for d in dks], dv.ptr, n, path, bounds=bounds)
        assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), (stray, where, path)
    # without bounds the same rows are fine
    want = gb.group_by(cols, vals)
    run(lib, [d.ptr for d in dks], dv.ptr, n, AUTO, want, (stray, where, "NULL bounds"))


def test_wider_bounds_give_the_same_result(lib, S):
    n = 4097
    cols = _in_bounds(n, 4)
    vals = gc.values_of("uniform", cols[0])
    want = gb.group_by(cols, vals)
    devs, dv = [Dev.of(c) for c in cols], Dev.of(vals)
    dks = [d.ptr for d in devs]
    for path in (AUTO, DENSE, SORT):
        for bounds in (None, gb.bounds_of(cols), [0, 9, 0, 9], [-30, 10, -1, 20]):
            assert run(lib, dks, dv.ptr, n, path, want, (path, bounds), bounds=bounds) == (path or DENSE)
        if path != DENSE:  # the path rule applies to the bounds given
            assert run(lib, dks, dv.ptr, n, path, want, (path, "wide"), bounds=[0, S, 0, 9]) == SORT
            assert run(lib, dks, dv.ptr, n, path, want, (path, "2^32"), bounds=[-2**15, 2**15 - 1, -2**15, 2**15 - 1]) == SORT
    rc, h, g, _ = plan(lib, dks, dv.ptr, n, DENSE, bounds=[0, S, 0, 9])
    assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), "DENSE forced past S"
    for bad in ([5, 4, 0, 9], [0, 9, 9, 0], [3, 7, 1, 8], [2, 7, 2, 8], [gc.I32_MIN, gc.I32_MAX, 0, 9]):
        rc, h, g, _ = plan(lib, dks, dv.ptr, n, AUTO, bounds=bad)  # lo > hi; a key excluded; wider than 2^32
        assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), bad
    assert "2^32" in lib.mq_last_error().decode()


def test_argument_errors_and_no_rows(lib):
    n = 100
    cols = _in_bounds(n, 5)
    dks, dv = [Dev.of(c) for c in cols], Dev.of(cols[0])
    p = [d.ptr for d in dks]
    for args in ((p, dv.ptr, n, 3), (p, dv.ptr, 2**31, AUTO), ([p[0], p[1] + 2], dv.ptr, n, AUTO), (p, dv.ptr + 1, n, AUTO),
                 ([p[0], None], dv.ptr, n, AUTO), (p, None, n, AUTO)):
        rc, h, g, _ = plan(lib, *args)
        assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), args
    h, groups = C.c_void_p(), C.c_uint64(5)
    keys5 = (C.c_void_p * 5)(*([p[0]] * 5))
    for nkeys in (0, 5, -1):
        assert lib.mq_group_by_plan(keys5, nkeys, dv.ptr, n, None, AUTO, C.byref(h), C.byref(groups), None, None) == mq.MQ_EINVAL
        assert h.value is None and groups.value == 0
    assert lib.mq_group_by_plan(keys5, 2, dv.ptr, n, None, AUTO, None, C.byref(groups), None, None) == mq.MQ_EINVAL
    assert lib.mq_group_by_plan(None, 2, dv.ptr, n, None, AUTO, C.byref(h), C.byref(groups), None, None) == mq.MQ_EINVAL
    # no rows: any bounds, zero groups, a handle to free
    for path in (AUTO, DENSE, SORT):
        rc, h, g, taken = plan(lib, [None, None], None, 0, path, bounds=[3, 1, 0, 0])
        assert (rc, g) == (mq.MQ_OK, 0) and h and taken == (SORT if path == SORT else DENSE)
        mq.check(lib.mq_group_by_write(h, None, None, None, None, None, None), "mq_group_by_write")
        mq.check(lib.mq_group_free(h), "mq_group_free")


# ---------------------------------------------------------------------------
# 3. one key column is mq_group_plan
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("keyset", ["uniform_100", "all_distinct", "int32_ends"])
def test_one_key_is_mq_group_plan(lib, S, keyset):
    n = 70_001
    keys = gc.keys_of(keyset, n, S)
    vals = gc.values_of("uniform", keys)
    dk, dv = Dev.of(keys, offset_elems=1), Dev.of(vals)
    for path in (AUTO, SORT):
        h, groups, taken = C.c_void_p(), C.c_uint64(), C.c_int(-1)
        mq.check(lib.mq_group_plan(dk.ptr, dv.ptr, n, None, path, C.byref(h), C.byref(groups), C.byref(taken), None))
        g = groups.value
        ref = {nm: Dev.of(np.full(g + PAD, 0x55, dt)) for nm, dt in [("keys", np.int32)] + list(DTYPE.items())}
        mq.check(lib.mq_group_write(h.value, *[ref[nm].ptr for nm in ["keys"] + AGGS], None))
        mq.check(lib.mq_group_free(h.value))
        rc, h2, g2, taken2 = plan(lib, [dk.ptr], dv.ptr, n, path)
        assert (rc, g2, taken2) == (mq.MQ_OK, g, taken.value) and h2
        got = {nm: Dev.of(np.full(g + PAD, 0x55, dt)) for nm, dt in [("keys", np.int32)] + list(DTYPE.items())}
        mq.check(write(lib, h2, [got["keys"]], got))
        for nm, dt in [("keys", np.int32)] + list(DTYPE.items()):
            assert np.array_equal(got[nm].get(dt, g + PAD), ref[nm].get(dt, g + PAD)), (keyset, path, nm)
        # mq_group_write serves the handle too, keys included: it is a one-key handle
        mq.check(lib.mq_group_write(h2, got["keys"].ptr, None, None, None, None, None))
        mq.check(lib.mq_group_free(h2))
    want = gc.group(keys, vals)
    assert np.array_equal(ref["keys"].get(np.int32, g), want[0]) and np.array_equal(ref["sum"].get(np.int64, g), want[2])


# ---------------------------------------------------------------------------
# 4. outputs left out
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("tset", ["seven_shuffled", "skewed", "all_distinct"])
def test_null_outputs(lib, S, tset):
    n, nkeys = 4097, 3
    cols = gb.tuples_of(tset, n, nkeys, S)
    vals = gc.values_of("uniform", cols[0])
    want = gb.group_by(cols, vals)
    devs, dv = [Dev.of(c) for c in cols], Dev.of(vals, offset_elems=1)
    dks = [d.ptr for d in devs]
    paths = (DENSE, SORT) if gb.space_of(gb.bounds_of(cols)) <= S else (SORT,)
    for path in paths:
        for j in range(nkeys):  # each key output NULL in turn
            run(lib, dks, dv.ptr, n, path, want, (tset, path, "no key", j), skip_keys=(j,))
        run(lib, dks, dv.ptr, n, path, want, (tset, path, "no keys"), skip_keys=(0, 1, 2))
        run(lib, dks, dv.ptr, n, path, want, (tset, path, "NULL key array"), keys_null=True)
        for skip in [("count",), ("sum",), ("min",), ("max",), ("count", "sum", "min", "max"), ("sum", "min", "max")]:
            run(lib, dks, dv.ptr, n, path, want, (tset, path, skip), skip=skip)
        # mq_group_write on the multi-key handle: the aggregates without keys; keys are refused
        rc, h, g, _ = plan(lib, dks, dv.ptr, n, path)
        assert rc == mq.MQ_OK and g == len(want[1])
        keys, aggs = out_buffers(g, 1)
        mq.check(lib.mq_group_write(h, None, *[aggs[nm].ptr for nm in AGGS], None), "mq_group_write")
        check_outputs([], aggs, g, want, (tset, path, "mq_group_write"))
        keys, aggs = out_buffers(g, 1)
        assert lib.mq_group_write(h, keys[0].ptr, *[aggs[nm].ptr for nm in AGGS], None) == mq.MQ_EINVAL
        assert np.all(keys[0].get(np.int32, g + PAD) == KEY_SENT)
        for nm in AGGS:
            assert np.all(aggs[nm].get(DTYPE[nm], g + PAD) == SENT[nm]), (tset, path, nm, "written by a refused call")
        mq.check(lib.mq_group_free(h), "mq_group_free")


# ---------------------------------------------------------------------------
# 5. long chunks: the unrolled loops past one step a block
# ---------------------------------------------------------------------------
LONG_N = 300_007


def _geometry(L, n):
    b, r = C.c_uint32(), C.c_uint64()
    L.mq_scan_geometry(n, C.byref(b), C.byref(r))
    return b.value, r.value


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


@pytest.mark.parametrize("nkeys", [2, 4])
@pytest.mark.parametrize("tset", ["seven_sorted", "one_tuple", "space_S"])
def test_long_chunks(lib, S, one_cu, tset, nkeys):
    """One limited CU and 300 007 rows: a block of k_group_by_dense (at most 4 a CU) and of
    k_group_by_pack (at most 8) gets at least 3 x 8192 rows, so the unrolled loop runs several
    times, the tail tiles and the ragged last tile all occur, and runs of wave-uniform tiles
    (seven_sorted, one_tuple) are flushed mid-chunk; space_S makes every row an LDS atomic.
    Both paths over the same rows."""
    n = LONG_N
    blocks, rpb = _geometry(lib, n)
    assert blocks <= 8 and rpb >= 3 * 8192, (blocks, rpb)
    cols = gb.tuples_of(tset, n, nkeys, S)
    if tset == "seven_sorted":
        uniform = np.ones(n // 256, dtype=bool)  # wave tiles whose 256 tuples are equal
        for c in cols:
            tiles = c[: n // 256 * 256].reshape(-1, 256)
            uniform &= tiles.min(axis=1) == tiles.max(axis=1)
        assert uniform.sum() > len(uniform) // 2
    vals = gc.values_of("uniform", cols[0])
    want = gb.group_by(cols, vals)
    assert gb.space_of(gb.bounds_of(cols)) <= S
    for koff, voff in ((0, 0), (1, 0), (0, 1)):
        dks = [Dev.of(c, offset_elems=koff if j == nkeys - 1 else 0) for j, c in enumerate(cols)]
        dv = Dev.of(vals, offset_elems=voff)
        for path in (AUTO, SORT):
            assert run(lib, [d.ptr for d in dks], dv.ptr, n, path, want, (tset, nkeys, koff, voff, path)) == (path or DENSE)


# ---------------------------------------------------------------------------
# 6. the drop-in
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


def aggregate_by(L, keys, values, nkeys=None):
    """group_aggregate_by -> (status, the nkeys + 4 Results as (data_type, numpy array) or None)"""
    gks, gv, st = [gcol(k) for k in keys], gcol(values), mq.Status(0, None)
    arr = (C.POINTER(mq.GeneralizedColumn) * len(gks))(*[C.pointer(g) for g in gks])
    nkeys = len(keys) if nkeys is None else nkeys
    rpp = L.group_aggregate_by(arr, nkeys, C.byref(gv), C.byref(st))
    if not rpp:
        return st.code, None
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(nkeys + 4)]  # take() free()s the payloads
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def check_results(out, want, tag):
    nkeys = len(want[0])
    assert [t for t, _ in out] == [mq.INT] * nkeys + [mq.LONG, mq.LONG, mq.INT, mq.INT], tag
    for i, ((_, got), w) in enumerate(zip(out, list(want[0]) + list(want[1:]))):
        assert len(got) == len(w) and np.array_equal(got, w.astype(got.dtype)), tag + (i,)


@pytest.mark.parametrize("n", [4097, 70_001])
def test_dropin_column_and_result_arguments(lib, S, n):
    for nkeys, tset in ((2, "skewed"), (3, "all_distinct"), (4, "seven_shuffled"), (2, "ends_x_one"), (1, "skewed")):
        cols = gb.tuples_of(tset, n, max(nkeys, 2), S)[:nkeys]
        vals = gc.values_of("uniform", cols[0])
        want = gb.group_by(cols, vals)
        ccols, cv = [make_column(c) for c in cols], make_column(vals)
        code, out = aggregate_by(lib, ccols, cv)
        assert code == mq.OK
        check_results(out, want, (n, nkeys, tset, "columns"))
        # INT Results with an HBM shadow (fetch_column's outputs) for the first key and the values
        st, rpos = mq.Status(0, None), make_result(np.arange(n, dtype=np.int32))
        fk = lib.fetch_column(C.byref(ccols[0]), C.byref(rpos), C.byref(st))
        fv = lib.fetch_column(C.byref(cv), C.byref(rpos), C.byref(st))
        assert st.code == mq.OK and fk and fv
        code, out = aggregate_by(lib, [fk] + ccols[1:], fv)
        assert code == mq.OK
        check_results(out, want, (n, nkeys, tset, "results"))
        code, out = aggregate_by(lib, ccols, ccols[-1])  # the values are a key column, the same object
        assert code == mq.OK
        check_results(out, gb.group_by(cols, cols[-1]), (n, nkeys, tset, "values = last key"))
        for r in (fk, fv):
            take(r)
        free_result_struct(rpos)
        for c in ccols + [cv]:
            lib.mq_column_invalidate(C.byref(c))


def test_dropin_empty_and_errors(lib, capfd):
    empty = np.empty(0, np.int32)
    ce = make_column(empty)
    for nkeys in (1, 2, 4):
        code, out = aggregate_by(lib, [ce] * nkeys, ce)
        assert code == mq.OK
        check_results(out, gb.group_by([empty] * nkeys, empty), ("empty", nkeys))
    lib.mq_column_invalidate(C.byref(ce))
    small = np.arange(100, dtype=np.int32)
    ck = make_column(small)
    capfd.readouterr()
    short = make_result(small[:99])
    for keys, vals in (([ck, ck], short), ([ck, short], ck)):  # different lengths
        code, out = aggregate_by(lib, keys, vals)
        assert (code, out) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err
    lng = make_result(small.astype(np.int64), mq.LONG)
    for keys, vals in (([ck, lng], ck), ([ck, ck], lng)):  # a LONG Result on either side
        code, out = aggregate_by(lib, keys, vals)
        assert (code, out) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err
    for nkeys in (0, 5):
        code, out = aggregate_by(lib, [ck] * 5, ck, nkeys=nkeys)
        assert (code, out) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err
    ends = gc.keys_of("int32_ends", 100, 0)
    cends = make_column(ends)
    code, out = aggregate_by(lib, [cends, ck], ck)  # 2^32 x 100: a key space wider than 2^32
    assert (code, out) == (mq.ERROR, None)
    err = capfd.readouterr().err
    assert "libmq" in err and "2^32" in err
    code, out = aggregate_by(lib, [ck, ck], ck)
    assert code == mq.OK and np.array_equal(out[0][1], small) and np.array_equal(out[1][1], small)
    free_result_struct(short)
    free_result_struct(lng)
    for c in (ck, cends):
        lib.mq_column_invalidate(C.byref(c))
