"""Grouped aggregates on gfx950 (csrc/mq_group.hip; group_aggregate in mq_query.c), every
comparison exact equality with the numpy restatement in groupcases.py (the reference has
no such operator).

Which regime each size reaches: gc.SIZES (up to 300 001 rows) cover both paths, the dense
path's tiles and the sort path with one 1024-row tile a block of its fixed grid, where no
run is carried from tile to tile. 2 097 153 rows are the first with two tiles a block (a
last chunk of one row), 4 195 333 rows give three (a last chunk that ends in a 5-row
tile): there k_group_seg_write carries the open run across tiles, meets tiles with no
head, and closes carried runs with a plain store or with atomics. Each of those tests
asserts its regime from mq_group_sort_geometry first.
"""
import ctypes as C

import numpy as np
import pytest

import groupcases as gc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PAD = 8
SENT = {"keys": -7, "count": 7, "sum": -77, "min": -777, "max": 777}
DTYPE = {"keys": np.int32, "count": np.uint64, "sum": np.int64, "min": np.int32, "max": np.int32}
NAMES = ["keys", "count", "sum", "min", "max"]


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # The drop-in's first operator pins glibc's mmap threshold at 1 MB (mq_query.c ready()),
    # which is what lets a large Result payload be write-guarded. Run one before this
    # module's multi-megabyte numpy temporaries come and go (see test_gpu_dml.py).
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    return L


@pytest.fixture(scope="module")
def S(lib):
    return lib.mq_group_dense_slots()


def plan(L, dk, dv, n, path, bounds=None, stream=None):
    """(rc, handle, groups, path taken)"""
    h, groups, taken = C.c_void_p(), C.c_uint64(12345), C.c_int(-1)
    b = None if bounds is None else (C.c_int32 * 2)(*bounds)
    rc = L.mq_group_plan(dk, dv, n, b, path, C.byref(h), C.byref(groups), C.byref(taken), stream)
    return rc, h.value, groups.value, taken.value


def out_buffers(g, skip=()):
    """One sentinel-filled device buffer per output, PAD entries longer than the groups."""
    return {nm: None if nm in skip else Dev.of(np.full(g + PAD, SENT[nm], DTYPE[nm])) for nm in NAMES}


def write(L, h, outs, stream=None):
    return L.mq_group_write(h, *[outs[nm].ptr if outs[nm] else None for nm in NAMES], stream)


def check_outputs(outs, g, want, tag):
    for nm, w in zip(NAMES, want):
        if outs[nm] is None:
            continue
        got = outs[nm].get(DTYPE[nm], g + PAD)
        assert np.array_equal(got[:g], w), tag + (nm,)
        assert np.all(got[g:] == SENT[nm]), tag + (nm, "wrote past the groups")


def run(L, dk, dv, n, path, want, tag, bounds=None, skip=()):
    rc, h, g, taken = plan(L, dk, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (mq.load().mq_last_error(),)
    assert g == len(want[0]), tag
    outs = out_buffers(g, skip)
    mq.check(write(L, h, outs), "mq_group_write")
    check_outputs(outs, g, want, tag)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", gc.SIZES)
@pytest.mark.parametrize("keyset", gc.KEY_SETS)
def test_paths_agree_with_the_restatement(lib, S, keyset, n):
    """Every value set under every path the key range allows, keys and values 0 and 1
    dword off a 16-byte boundary independently: the same exact answer, nothing written
    past the groups, and AUTO takes the dense path exactly when the range fits."""
    keys = gc.keys_of(keyset, n, S)
    dense_ok = gc.key_range(keys) <= S
    for i, vset in enumerate(gc.VALUE_SETS):
        ko, vo = i & 1, (i >> 1) & 1
        if vset == "keys":
            ko = n & 1
        vals = gc.values_of(vset, keys)
        want = gc.group(keys, vals)
        dk = Dev.of(keys, offset_elems=ko)
        dv = dk if vset == "keys" else Dev.of(vals, offset_elems=vo)  # values = keys: the same pointer
        for path in (AUTO, DENSE, SORT) if dense_ok else (AUTO, SORT):
            tag = (keyset, n, vset, path)
            taken = run(lib, dk.ptr, dv.ptr, n, path, want, tag)
            if n:
                assert taken == (path if path != AUTO else DENSE if dense_ok else SORT), tag
        if n and not dense_ok:
            rc, h, g, _ = plan(lib, dk.ptr, dv.ptr, n, DENSE)
            assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), (keyset, n, vset, "DENSE forced past S")


@pytest.mark.parametrize("keyset", ["uniform_100", "seven_sorted", "all_distinct"])
def test_null_outputs(lib, S, keyset):
    """Each aggregate left out in turn (and all four): the others are still right."""
    n = 4097
    keys = gc.keys_of(keyset, n, S)
    vals = gc.values_of("uniform", keys)
    want = gc.group(keys, vals)
    dk, dv = Dev.of(keys), Dev.of(vals, offset_elems=1)
    paths = (DENSE, SORT) if gc.key_range(keys) <= S else (SORT,)
    for path in paths:
        for skip in [("count",), ("sum",), ("min",), ("max",), ("count", "sum", "min", "max"), ("sum", "min", "max")]:
            run(lib, dk.ptr, dv.ptr, n, path, want, (keyset, path, skip), skip=skip)


def test_key_bounds(lib, S):
    n = 70_001
    keys = gc.keys_of("uniform_100", n, S)
    vals = gc.values_of("uniform", keys)
    want = gc.group(keys, vals)
    lo, hi = int(keys.min()), int(keys.max())
    dk, dv = Dev.of(keys), Dev.of(vals)
    for path in (AUTO, DENSE, SORT):
        assert run(lib, dk.ptr, dv.ptr, n, path, want, ("exact", path), bounds=(lo, hi)) == (path or DENSE)
        # wider bounds: the same result; the path rule applies to the range given
        assert run(lib, dk.ptr, dv.ptr, n, path, want, ("wider", path), bounds=(lo - 5, lo - 5 + S - 1)) == (path or DENSE)
        if path != DENSE:
            assert run(lib, dk.ptr, dv.ptr, n, path, want, ("wide", path), bounds=(lo - 5, lo - 5 + S)) == SORT
            assert run(lib, dk.ptr, dv.ptr, n, path, want, ("all", path), bounds=(gc.I32_MIN, gc.I32_MAX)) == SORT
        # a pair that excludes one key, at either end; lo > hi
        for bad in [(lo + 1, hi), (lo, hi - 1), (hi + 1, hi + 3), (hi, lo)]:
            rc, h, g, _ = plan(lib, dk.ptr, dv.ptr, n, path, bounds=bad)
            assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), (path, bad)
    rc, h, g, _ = plan(lib, dk.ptr, dv.ptr, n, DENSE, bounds=(lo, lo + S))
    assert (rc, h, g) == (mq.MQ_EINVAL, None, 0), "DENSE forced past S"
    # no rows: any bounds, zero groups, a handle to free
    rc, h, g, _ = plan(lib, None, None, 0, AUTO, bounds=(3, 1))
    assert (rc, g) == (mq.MQ_OK, 0) and h
    mq.check(lib.mq_group_write(h, None, None, None, None, None, None), "mq_group_write")
    mq.check(lib.mq_group_free(h), "mq_group_free")


def test_32_plans_on_32_streams(lib, S):
    """32 handles alive at once, dense and sort mixed, their writes queued on 32 streams
    with no host sync in between; all exact. Then every handle is freed and a further
    plan runs on the pool blocks they gave back."""
    n, nstreams = 70_001, 32
    sets = ["uniform_100", "all_distinct", "seven_sorted", "skewed", "int32_ends"]
    data = {}
    for ks in sets:
        keys = gc.keys_of(ks, n, S)
        vals = gc.values_of("uniform", keys)
        data[ks] = (Dev.of(keys), Dev.of(vals, offset_elems=1), gc.group(keys, vals), gc.key_range(keys) <= S)
    streams = []
    for _ in range(nstreams):
        sp = C.c_void_p()
        mq.check(lib.mq_stream_create(C.byref(sp)))
        streams.append(sp.value)
    jobs = []
    for s in range(nstreams):
        ks = sets[s % len(sets)]
        dk, dv, want, dense_ok = data[ks]
        path = (AUTO, SORT, DENSE)[s % 3] if dense_ok else (AUTO, SORT)[s % 2]
        rc, h, g, taken = plan(lib, dk.ptr, dv.ptr, n, path, stream=streams[s])
        assert rc == mq.MQ_OK and g == len(want[0]), (s, ks, path)
        jobs.append((s, ks, h, g, out_buffers(g), want, taken))
    assert {j[6] for j in jobs} == {DENSE, SORT}
    for s, ks, h, g, outs, want, _ in jobs:
        mq.check(write(lib, h, outs, streams[s]), "mq_group_write")
    for sp in streams:
        mq.check(lib.mq_stream_sync(sp))
    for s, ks, h, g, outs, want, taken in jobs:
        check_outputs(outs, g, want, (s, ks, taken))
        mq.check(lib.mq_group_free(h), "mq_group_free")
    for ks in ("all_distinct", "uniform_100"):
        dk, dv, want, _ = data[ks]
        run(lib, dk.ptr, dv.ptr, n, AUTO, want, ("after the frees", ks))
    for sp in streams:
        mq.check(lib.mq_stream_destroy(sp))


# ---------------------------------------------------------------------------
# the sort path past one tile a block
#
# k_group_heads / k_group_seg_write run on a fixed grid (mq_group_sort_geometry): up to
# 2 097 152 rows a block's chunk is one 1024-row tile, so the sizes above never carry a run
# from one tile to the next. gc.SORT_N gives every block three tiles (the last chunk a
# ragged one), gc.SORT_N_TWO_TILES is the first size with two.
# ---------------------------------------------------------------------------
FILL = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}  # what mq_memset(0x5A) leaves in an entry


def sort_geometry(L, n):
    b, c = C.c_uint32(), C.c_uint64()
    L.mq_group_sort_geometry(n, C.byref(b), C.byref(c))
    return b.value, c.value


def run_filled(L, dk, dv, n, path, want, tag, skip=()):
    """run() with the outputs pre-filled with 0x5A bytes on the device; returns the path."""
    rc, h, g, taken = plan(L, dk, dv, n, path)
    assert rc == mq.MQ_OK and h, tag + (mq.load().mq_last_error(),)
    assert g == len(want[0]), tag
    outs = {nm: None if nm in skip else Dev((g + PAD) * np.dtype(DTYPE[nm]).itemsize) for nm in NAMES}
    for o in outs.values():
        if o:
            mq.check(L.mq_memset(o.ptr, 0x5A, o.nbytes, None), "mq_memset")
    mq.check(write(L, h, outs), "mq_group_write")
    for nm, w in zip(NAMES, want):
        if outs[nm] is None:
            continue
        got = outs[nm].get(DTYPE[nm], g + PAD)
        assert np.array_equal(got[:g], w), tag + (nm,)
        assert np.all(got[g:].view(f"u{got.itemsize}") == FILL[got.itemsize]), tag + (nm, "wrote past the groups")
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


def sort_regime(L, n, tiles):
    """The chunk of the sort path at n rows, after asserting `tiles` tiles a block, more
    than one block and a last chunk that ends in a ragged tile."""
    blocks, chunk = sort_geometry(L, n)
    assert chunk % gc.SEG_TILE == 0 and chunk // gc.SEG_TILE >= tiles and blocks >= 2, (n, blocks, chunk)
    last = n - (blocks - 1) * chunk
    assert 0 < last <= chunk and last % gc.SEG_TILE != 0, (n, blocks, chunk, last)
    return chunk


@pytest.mark.parametrize("runset", gc.RUN_SETS)
def test_sort_path_three_tiles_a_block(lib, runset):
    """SORT forced at gc.SORT_N rows: keys, count, sum, min, max and the plan's group count
    equal the restatement, nothing is written past the groups. The key columns are built
    from the run lengths of the sorted keys (groupcases.runs_of): one key (every chunk after
    the first has no head and emits with atomics onto group 0), all distinct (1024 heads a
    tile), runs of exactly one tile and of exactly one chunk starting on, one row after and
    one row before the edges, mixed lengths, and one run over 90 % of the rows. Values are
    full-range with INT32_MIN / INT32_MAX planted around every tile edge; the one-key column
    also sums all-INT32_MAX and all-INT32_MIN values (|sum| about 9e15). all_distinct under
    AUTO reports SORT; mixed also runs without the count and sum outputs."""
    n = gc.SORT_N
    chunk = sort_regime(lib, n, 3)
    runs = gc.runs_of(runset, n, chunk)
    keys, order = gc.keys_from_runs(runs, seed=n + len(runset))
    assert len(keys) == n
    dk = Dev.of(keys)
    vsets = [gc.planted_values(runs, order, seed=7)]
    if runset == "one_key":
        vsets += [gc.values_of("all_max", keys), gc.values_of("all_min", keys)]
    for i, vals in enumerate(vsets):
        want = gc.group(keys, vals)
        assert len(want[0]) == len(runs) and np.array_equal(want[1], runs.astype(np.uint64))
        dv = Dev.of(vals, offset_elems=i & 1)
        assert run_filled(lib, dk.ptr, dv.ptr, n, SORT, want, (runset, i)) == SORT
        if runset == "all_distinct":
            assert run_filled(lib, dk.ptr, dv.ptr, n, AUTO, want, (runset, "AUTO")) == SORT
        if runset == "mixed":
            run_filled(lib, dk.ptr, dv.ptr, n, SORT, want, (runset, "no count, no sum"), skip=("count", "sum"))
    if runset == "one_key":
        assert abs(int(want[2][0])) > 9 * 10**15


def test_sort_path_first_size_with_two_tiles(lib):
    """gc.SORT_N_TWO_TILES rows: two tiles a block and a last chunk of one row, on the
    mixed run lengths."""
    n = gc.SORT_N_TWO_TILES
    chunk = sort_regime(lib, n, 2)
    blocks, _ = sort_geometry(lib, n)
    assert n - (blocks - 1) * chunk == 1 and sort_geometry(lib, n - 1)[1] == gc.SEG_TILE
    runs = gc.runs_of("mixed", n, chunk)
    keys, order = gc.keys_from_runs(runs, seed=n)
    vals = gc.planted_values(runs, order, seed=8)
    want = gc.group(keys, vals)
    assert len(want[0]) == len(runs)
    dk, dv = Dev.of(keys, offset_elems=1), Dev.of(vals)
    assert run_filled(lib, dk.ptr, dv.ptr, n, SORT, want, ("mixed", n)) == SORT


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


def aggregate(L, keys, values):
    """group_aggregate -> (status, the five Results as (data_type, numpy array) or None)"""
    gk, gv, st = gcol(keys), gcol(values), mq.Status(0, None)
    rpp = L.group_aggregate(C.byref(gk), C.byref(gv), C.byref(st))
    if not rpp:
        return st.code, None
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(5)]
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def check_results(out, want, tag):
    assert [t for t, _ in out] == [mq.INT, mq.LONG, mq.LONG, mq.INT, mq.INT], tag
    for (_, got), w, nm in zip(out, want, NAMES):
        assert len(got) == len(w) and np.array_equal(got, w.astype(got.dtype)), tag + (nm,)


@pytest.fixture(scope="module")
def table(S):
    n = 300_001
    keys = gc.keys_of("skewed", n, S)
    wide = gc.keys_of("all_distinct", n, S)
    vals = gc.values_of("uniform", keys)
    return n, keys, wide, vals


def test_dropin_column_and_result_arguments(lib, table):
    n, keys, wide, vals = table
    ck, cw, cv = make_column(keys), make_column(wide), make_column(vals)
    api_pos = np.arange(n, dtype=np.int32)
    st = mq.Status(0, None)
    rpos = make_result(api_pos)
    fk = lib.fetch_column(C.byref(ck), C.byref(rpos), C.byref(st))  # a Result with an HBM shadow
    fv = lib.fetch_column(C.byref(cv), C.byref(rpos), C.byref(st))
    assert st.code == mq.OK and fk and fv
    for kname, kh in (("dense", keys), ("sort", wide)):
        want = gc.group(kh, vals)
        kc = ck if kname == "dense" else cw
        code, out = aggregate(lib, kc, cv)
        assert code == mq.OK
        check_results(out, want, (kname, "column x column"))
        code, out = aggregate(lib, kc, fv)
        assert code == mq.OK
        check_results(out, want, (kname, "column x result"))
    code, out = aggregate(lib, fk, fv)
    assert code == mq.OK
    check_results(out, gc.group(keys, vals), ("result x result",))
    code, out = aggregate(lib, ck, ck)  # the same object twice
    assert code == mq.OK
    check_results(out, gc.group(keys, keys), ("keys x keys",))
    for r in (fk, fv):
        take(r)
    free_result_struct(rpos)
    for c in (ck, cw, cv):
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_empty_and_errors(lib, table, capfd):
    n, keys, wide, vals = table
    empty = np.empty(0, np.int32)
    ce = make_column(empty)
    code, out = aggregate(lib, ce, ce)
    assert code == mq.OK
    check_results(out, gc.group(empty, empty), ("empty",))
    lib.mq_column_invalidate(C.byref(ce))
    small = np.arange(100, dtype=np.int32)
    ck = make_column(small)
    capfd.readouterr()
    short = make_result(small[:99])
    code, out = aggregate(lib, ck, short)  # length mismatch
    assert (code, out) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err
    lng = make_result(small.astype(np.int64), mq.LONG)
    for a, b in ((ck, lng), (lng, ck)):  # a LONG Result on either side
        code, out = aggregate(lib, a, b)
        assert (code, out) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err
    code, out = aggregate(lib, ck, ck)
    assert code == mq.OK and np.array_equal(out[0][1], small)
    free_result_struct(short)
    free_result_struct(lng)
    lib.mq_column_invalidate(C.byref(ck))


def test_dropin_chain_select_fetch_group_print(lib, table):
    """select_column -> two fetch_column -> group_aggregate -> print of keys and sums."""
    n, keys, wide, vals = table
    ck, cv = make_column(keys), make_column(vals)
    st = mq.Status(0, None)
    low, high = 10, 1500
    pos = lib.select_column(C.byref(ck), C.pointer(C.c_int(low)), C.pointer(C.c_int(high)), C.byref(st))
    fk = lib.fetch_column(C.byref(ck), pos, C.byref(st))
    fv = lib.fetch_column(C.byref(cv), pos, C.byref(st))
    assert st.code == mq.OK and pos and fk and fv
    gk, gv = gcol(fk), gcol(fv)
    rpp = lib.group_aggregate(C.byref(gk), C.byref(gv), C.byref(st))
    assert st.code == mq.OK and rpp
    arr = (C.POINTER(mq.Result) * 2)(rpp[0], rpp[2])
    p = lib.print(arr, 2, C.byref(st))
    text = C.string_at(p).decode()
    _libc.free(p)
    sel = (keys >= low) & (keys < high)
    wk, _, ws, _, _ = gc.group(keys[sel], vals[sel])
    assert len(wk) > 1000
    assert text == "\n".join(map(str, wk.tolist())) + "," + "\n".join(map(str, ws.tolist()))
    for i in range(5):
        take(rpp[i])
    _libc.free(C.cast(rpp, C.c_void_p))
    for r in (pos, fk, fv):
        take(r)
    for c in (ck, cv):
        lib.mq_column_invalidate(C.byref(c))
