"""group_aggregate_where on gfx950 (mq_group_where_plan and k_group_where_dense in
csrc/mq_group.hip; group_aggregate_where in mq_query.c), every comparison exact equality:
with the composed numpy model (groupcases.group over wherecases.mask), with mq_group_plan
on the same columns, and with the chain select -> fetch x 2 -> group run through libmq.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import groupcases as gc
import groupwherecases as gw
import wherecases as wc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PAD = 8
NAMES = ["keys", "count", "sum", "min", "max"]
DTYPE = {"keys": np.int32, "count": np.uint64, "sum": np.int64, "min": np.int32, "max": np.int32}
FILL = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}  # what mq_memset(0x5A) leaves in an entry


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
    return L


@pytest.fixture(scope="module")
def S(lib):
    return lib.mq_group_dense_slots()


def c_ranges(ranges):
    return (mq.MqRange * len(ranges))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in ranges])


def c_ptrs(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def upload(arrays, offs=(0,)):
    """One device copy per distinct array object (identity kept: the same array twice is the
    same pointer twice), the k-th distinct one offs[k % len(offs)] dwords off a 16-byte
    boundary. Returns (pointers in the order given, the buffers to keep alive)."""
    devs, ptrs = {}, []
    for a in arrays:
        if id(a) not in devs:
            devs[id(a)] = Dev.of(a, offset_elems=offs[len(devs) % len(offs)])
        ptrs.append(devs[id(a)].ptr)
    return ptrs, devs


def wplan(L, ptrs, ranges, dk, dv, n, path, bounds=None, stream=None):
    """(rc, handle, groups, path taken, matching rows)"""
    h, groups, taken, rows = C.c_void_p(), C.c_uint64(12345), C.c_int(-1), C.c_uint64(54321)
    b = None if bounds is None else (C.c_int32 * 2)(*bounds)
    rc = L.mq_group_where_plan(c_ptrs(ptrs), c_ranges(ranges), len(ptrs), dk, dv, n, b, path, C.byref(h), C.byref(groups),
                               C.byref(taken), C.byref(rows), stream)
    return rc, h.value, groups.value, taken.value, rows.value


def filled_outputs(L, g, stream=None):
    outs = {nm: Dev((g + PAD) * np.dtype(DTYPE[nm]).itemsize) for nm in NAMES}
    for o in outs.values():
        mq.check(L.mq_memset(o.ptr, 0x5A, o.nbytes, stream), "mq_memset")
    return outs


def write(L, h, outs, stream=None):
    return L.mq_group_write(h, *[outs[nm].ptr for nm in NAMES], stream)


def check_outputs(outs, g, want, tag):
    for nm, w in zip(NAMES, want):
        got = outs[nm].get(DTYPE[nm], g + PAD)
        assert np.array_equal(got[:g], w), tag + (nm,)
        assert np.all(got[g:].view(f"u{got.itemsize}") == FILL[got.itemsize]), tag + (nm, "wrote past the groups")


def run(L, ptrs, ranges, dk, dv, n, path, want, tag, bounds=None):
    """Plan, write into 0x5A-filled outputs, compare, free. Returns the path taken."""
    rc, h, g, taken, rows = wplan(L, ptrs, ranges, dk, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[0]), tag + ("groups", g)
    assert rows == int(want[1].sum()), tag + ("rows", rows)
    outs = filled_outputs(L, g)
    mq.check(write(L, h, outs), "mq_group_write")
    check_outputs(outs, g, want, tag)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


def refused(L, ptrs, ranges, dk, dv, n, path, bounds=None):
    rc, h, g, _, rows = wplan(L, ptrs, ranges, dk, dv, n, path, bounds)
    return (rc, h, g, rows) == (mq.MQ_EINVAL, None, 0, 0) and bool(L.mq_last_error())


def run_paths(L, S, cols, ranges, keys, vals, tag, offs=(0,), values_are_keys=False):
    """Every path the matching key range allows, against the model; AUTO's choice and the
    refusal of DENSE on a wider range are asserted."""
    n = len(keys)
    m = wc.mask(cols, ranges)
    want = gc.group(keys[m], vals[m])
    assert int(want[1].sum()) == int(m.sum())
    ptrs, keep = upload(list(cols) + [keys] + ([] if values_are_keys else [vals]), offs)
    dk = ptrs[len(cols)]
    dv = dk if values_are_keys else ptrs[-1]
    dense_ok = gc.key_range(keys[m]) <= S
    for path in (AUTO, DENSE, SORT) if dense_ok else (AUTO, SORT):
        taken = run(L, ptrs[:len(cols)], ranges, dk, dv, n, path, want, tag + (path,))
        assert taken == (path if path != AUTO else DENSE if dense_ok else SORT), tag + (path, taken)
    if not dense_ok:
        assert refused(L, ptrs[:len(cols)], ranges, dk, dv, n, DENSE), tag + ("DENSE forced past S",)
    return want


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.CASES)
def test_matrix_agrees_with_the_model(lib, S, name):
    """The rotation of groupwherecases.matrix: this predicate set at ncols 1, 2, 3 and 8, at
    0, 1025, 8193 rows and rotating further sizes, key and value sets rotating along, columns
    0 and 1 dword off a 16-byte boundary in turn."""
    ci = wc.CASES.index(name)
    for q, (ncols, n, ks, vs) in enumerate(gw.matrix(ci)):
        cols, ranges = wc.case(name, n, ncols)
        keys = gc.keys_of(ks, n, S)
        vals = gc.values_of(vs, keys)
        offs = [(0,), (0, 1), (1, 0, 0), (1,)][(ci + q) % 4]
        run_paths(lib, S, cols, ranges, keys, vals, (name, ncols, n, ks, vs), offs, values_are_keys=vs == "keys")


@pytest.mark.parametrize("name", gw.POISON_SETS)
def test_dead_rows_are_never_looked_at(lib, S, name):
    """Every failing row, in live lines and in whole dead lines, carries a key outside the
    bounds given (the exact min and max of the matching keys): the plan succeeds on DENSE
    and equals the model. One matching row with a key out of bounds is MQ_EINVAL."""
    cols, ranges, keys, vals, bounds = gw.poisoned(name, S)
    n = len(keys)
    m = wc.mask(cols, ranges)
    want = gc.group(keys[m], vals[m])
    for offs in ((0,), (1, 0)):
        ptrs, keep = upload(cols + [keys, vals], offs)
        for path in (DENSE, AUTO):
            assert run(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, path, want, (name, offs, path), bounds) == DENSE
        assert run(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, SORT, want, (name, offs, SORT), bounds) == SORT
    live = np.flatnonzero(m)
    for row, key in ((live[len(live) // 2], bounds[1] + 1), (live[0], bounds[0] - 1), (live[-1], gc.I32_MAX)):
        planted = keys.copy()
        planted[row] = key
        ptrs, keep = upload(cols + [planted, vals])
        for path in (DENSE, AUTO, SORT):
            assert refused(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, path, bounds), (name, row, key, path)


def test_the_filter_narrows_the_range(lib, S):
    """all_distinct keys over 8193 rows that are predicate column 0 too: a range of `slots`
    values lands on DENSE under AUTO without bounds, one more value on SORT, and DENSE
    forced there is MQ_EINVAL."""
    cols, ranges, keys, vals = gw.narrow(S, 0)
    assert gc.key_range(keys) > S
    ptrs, keep = upload(cols + [vals])
    want = gw.model(cols, ranges, keys, vals)
    assert len(want[0]) == S
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), AUTO, want, ("narrow", AUTO)) == DENSE
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), DENSE, want, ("narrow", DENSE)) == DENSE
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), SORT, want, ("narrow", SORT)) == SORT
    cols, ranges, keys, vals = gw.narrow(S, 1)
    want = gw.model(cols, ranges, keys, vals)
    assert len(want[0]) == S + 1
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), AUTO, want, ("narrow + 1", AUTO)) == SORT
    assert refused(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), DENSE)
    # bounds that are wider than the matching keys but fit: DENSE again
    lo = gw.NARROW_LOW
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), AUTO, want, ("narrow + 1", "bounds"),
               bounds=(lo, lo + S)) == SORT
    ranges[0] = (lo, lo + S - 5)
    want = gw.model(cols, ranges, keys, vals)
    assert run(lib, ptrs[:2], ranges, ptrs[0], ptrs[2], len(keys), AUTO, want, ("narrow - 5", "bounds"),
               bounds=(lo - 3, lo + S - 4)) == DENSE


@pytest.mark.parametrize("pred", ["first_all", "sorted_lead", "clustered_lead", "last_kills"])
@pytest.mark.parametrize("keyset", ["seven_sorted", "one_key"])
def test_the_run_fold(lib, S, keyset, pred):
    """Wave tiles whose 256 rows all survive and share one key are folded in registers:
    fully live columns, one long live stretch, live stretches of 1 to 4097 rows that start
    and stop inside tiles, and a last predicate that leaves scattered rows."""
    for n, ncols, vs in ((8193, 2, "uniform"), (70_001, 3, "all_min"), (70_001, 1, "keys")):
        cols, ranges = wc.case(pred, n, ncols)
        keys = gc.keys_of(keyset, n, S)
        vals = gc.values_of(vs, keys)
        run_paths(lib, S, cols, ranges, keys, vals, (keyset, pred, n, ncols, vs), (n & 1, 0), values_are_keys=vs == "keys")


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("pred", ["uniform_10", "clustered_lead", "islands_alt"])
def test_many_iterations_a_block(lib, S, pred, limit):
    """wc.BIG rows on a grid of 1 or 2 CUs' blocks: many iterations a block, sums past 2^47."""
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        n = wc.BIG
        for keyset, ncols in (("uniform_100", 2), ("seven_sorted", 3)):
            cols, ranges = wc.case(pred, n, ncols)
            keys = gc.keys_of(keyset, n, S)
            vals = gc.values_of("all_max", keys)
            m = wc.mask(cols, ranges)
            want = gc.group(keys[m], vals[m])
            ptrs, keep = upload(cols + [keys, vals], (limit - 1, 0, 1))
            for path in (AUTO, DENSE):
                assert run(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, path, want, (pred, limit, keyset, path)) == DENSE
            if keyset == "uniform_100":
                assert run(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, SORT, want, (pred, limit, keyset, SORT)) == SORT
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


@pytest.mark.parametrize("n", [1025, 8193])
def test_alignment(lib, S, n):
    """One predicate column, the keys and the values each 0 and 1 dword off a 16-byte
    boundary, independently."""
    cols, ranges = wc.case("uniform_50", n, 1)
    keys = gc.keys_of("uniform_100", n, S)
    vals = gc.values_of("uniform", keys)
    want = gw.model(cols, ranges, keys, vals)
    for oc, ok, ov in itertools.product((0, 1), repeat=3):
        dc, dk, dv = Dev.of(cols[0], offset_elems=oc), Dev.of(keys, offset_elems=ok), Dev.of(vals, offset_elems=ov)
        for path in (DENSE, SORT):
            assert run(lib, [dc.ptr], ranges, dk.ptr, dv.ptr, n, path, want, (n, oc, ok, ov, path)) == path


def test_aliasing(lib, S):
    """Keys is a predicate column, values is keys, and the same column twice."""
    n = 8193
    cols, ranges = wc.case("same_twice", n, 3)
    assert cols[1] is cols[0]
    keys = cols[0]  # uniform in [0, 1000): fits the dense path
    for vals, alias in ((keys, True), (cols[2], False)):
        want = gw.model(cols, ranges, keys, vals)
        assert len(want[0]) > 100
        ptrs, keep = upload(cols, (1, 0))
        assert ptrs[0] == ptrs[1]
        dv = ptrs[0] if alias else ptrs[2]
        for path in (AUTO, DENSE, SORT):
            assert run(lib, ptrs, ranges, ptrs[0], dv, n, path, want, ("same_twice", alias, path)) == (path or DENSE)
    # keys a later predicate column, values the first one
    cols, ranges = wc.case("uniform_50", n, 3)
    want = gw.model(cols, ranges, cols[2], cols[0])
    ptrs, keep = upload(cols)
    for path in (AUTO, SORT):
        run(lib, ptrs, ranges, ptrs[2], ptrs[0], n, path, want, ("keys = column 2", path))


def group_outputs(L, plan_call):
    """The five outputs (and the group count) of a planned handle, as raw arrays."""
    rc, h, g = plan_call()
    assert rc == mq.MQ_OK and h, L.mq_last_error()
    outs = filled_outputs(L, g)
    mq.check(write(L, h, outs), "mq_group_write")
    got = [outs[nm].get(DTYPE[nm], g + PAD) for nm in NAMES]
    mq.check(L.mq_group_free(h), "mq_group_free")
    return g, got


def plain_plan(L, dk, dv, n, path):
    h, groups = C.c_void_p(), C.c_uint64()
    rc = L.mq_group_plan(dk, dv, n, None, path, C.byref(h), C.byref(groups), None, None)
    return rc, h.value, groups.value


@pytest.mark.parametrize("keyset", ["uniform_100", "seven_sorted", "all_distinct"])
def test_identities(lib, S, keyset):
    n = 70_001
    keys = gc.keys_of(keyset, n, S)
    vals = gc.values_of("uniform", keys)
    cols, ranges = wc.case("uniform_50", n, 3)
    ptrs, keep = upload(cols + [keys, vals], (0, 1))
    dk, dv = ptrs[3], ptrs[4]
    paths = (DENSE, SORT) if gc.key_range(keys) <= S else (SORT,)
    # all ranges unbounded: mq_group_plan's outputs on the same columns
    for path in paths:
        g0, ref = group_outputs(lib, lambda: plain_plan(lib, dk, dv, n, path))
        g1, got = group_outputs(lib, lambda: wplan(lib, ptrs[:3], [(None, None)] * 3, dk, dv, n, path)[:3])
        assert g0 == g1 and all(np.array_equal(a, b) for a, b in zip(ref, got)), (keyset, path)
    # one predicate: mq_select_positions -> mq_fetch x 2 -> mq_group_plan
    lo, hi = ranges[0]
    sws = lib.mq_scan_workspace_bytes(n)
    ws, pos, cnt = Dev(sws), Dev(4 * n), Dev(16)
    mq.check(lib.mq_select_positions(ptrs[0], None, n, *mq.bounds(lo, hi), pos.ptr, cnt.ptr, ws.ptr, sws, None), "select")
    k = int(cnt.get(np.uint64, 1)[0])
    assert 0 < k < n
    fk, fv = Dev(4 * k), Dev(4 * k)
    mq.check(lib.mq_fetch(dk, pos.ptr, k, fk.ptr, None), "fetch")
    mq.check(lib.mq_fetch(dv, pos.ptr, k, fv.ptr, None), "fetch")
    m1 = wc.in_range(cols[0], lo, hi)
    for path in (AUTO, SORT):
        g0, ref = group_outputs(lib, lambda: plain_plan(lib, fk.ptr, fv.ptr, k, path))
        rc, h, g, taken, rows = wplan(lib, ptrs[:1], ranges[:1], dk, dv, n, path)
        assert rows == k
        mq.check(lib.mq_group_free(h), "mq_group_free")
        g1, got = group_outputs(lib, lambda: wplan(lib, ptrs[:1], ranges[:1], dk, dv, n, path)[:3])
        assert g0 == g1 and all(np.array_equal(a, b) for a, b in zip(ref, got)), (keyset, path, "chain")
        assert np.array_equal(got[0][:g1], gc.group(keys[m1], vals[m1])[0])
    # permuting the predicates changes nothing
    want = gw.model(cols, ranges, keys, vals)
    for perm in itertools.permutations(range(3)):
        for path in paths:
            run(lib, [ptrs[i] for i in perm], [ranges[i] for i in perm], dk, dv, n, path, want, (keyset, perm, path))


@pytest.mark.parametrize("name", ["first_none", "empty_range", "empty_high_min", "no_rows"])
def test_empty_outcomes(lib, S, name):
    """Zero groups, MQ_OK, a handle that frees, and a write that leaves the sentinels."""
    n = 0 if name == "no_rows" else 4097
    cols, ranges = wc.case("uniform_50" if name == "no_rows" else name, n, 3)
    keys = gc.keys_of("uniform_100", n, S)
    vals = gc.values_of("uniform", keys)
    ptrs, keep = upload(cols + [keys, vals])
    for path in (AUTO, DENSE, SORT):
        for bounds in (None, (-5, 5), (gc.I32_MIN, gc.I32_MAX)):
            if bounds == (gc.I32_MIN, gc.I32_MAX) and path == DENSE and n and name == "first_none":
                assert refused(lib, ptrs[:3], ranges, ptrs[3], ptrs[4], n, path, bounds)  # the range rule comes first
                continue
            rc, h, g, taken, rows = wplan(lib, ptrs[:3], ranges, ptrs[3], ptrs[4], n, path, bounds)
            assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h, (name, path, bounds, lib.mq_last_error())
            outs = filled_outputs(lib, 0)
            mq.check(write(lib, h, outs), "mq_group_write")
            check_outputs(outs, 0, gc.group(keys[:0], vals[:0]), (name, path, bounds))
            mq.check(lib.mq_group_free(h), "mq_group_free")
    if n == 0:  # NULL columns are fine without rows
        rc, h, g, taken, rows = wplan(lib, [None, None], ranges[:2], None, None, 0, AUTO)
        assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h
        mq.check(lib.mq_group_free(h), "mq_group_free")


def test_sort_path_past_one_tile_a_block(lib):
    """4 195 333 rows, about 60 % matching: K > 2 097 152 puts k_group_seg_write on two
    tiles a block; mixed run lengths over the matching rows, SORT forced."""
    _, m = gw.sort_big_mask()
    k = int(m.sum())
    blocks, chunk = C.c_uint32(), C.c_uint64()
    lib.mq_group_sort_geometry(k, C.byref(blocks), C.byref(chunk))
    assert k > 2_097_152 and chunk.value >= 2 * gc.SEG_TILE
    cols, ranges, keys, vals, runs = gw.sort_big(chunk.value)
    want = gc.group(keys[m], vals[m])
    assert len(want[0]) == len(runs)
    ptrs, keep = upload(cols + [keys, vals], (0, 1, 0))
    assert run(lib, ptrs[:1], ranges, ptrs[1], ptrs[2], len(keys), SORT, want, ("sort big",)) == SORT


def test_sixteen_handles_on_sixteen_streams(lib, S):
    """Dense and sort mixed, each with its own predicates, all planned before any is written."""
    n = 70_001
    streams = []
    for _ in range(16):
        sp = C.c_void_p()
        mq.check(lib.mq_stream_create(C.byref(sp)), "mq_stream_create")
        streams.append(sp.value)
    try:
        jobs = []
        keysets = ["uniform_100", "all_distinct", "seven_sorted", "skewed", "int32_ends"]
        for i, sp in enumerate(streams):
            name, ncols = wc.CASES[(3 * i) % len(wc.CASES)], wc.NCOLS[i % 4]
            cols, ranges = wc.case(name, n, ncols)
            keys = gc.keys_of(keysets[i % len(keysets)], n, S)
            vals = gc.values_of("uniform", keys)
            want = gw.model(cols, ranges, keys, vals)
            ptrs, keep = upload(cols + [keys, vals], (i & 1, 0))
            jobs.append((i, sp, ptrs, keep, ranges, want, name))
        mq.check(lib.mq_device_sync(), "device sync")  # the uploads (null stream) are done
        planned = []
        for i, sp, ptrs, keep, ranges, want, name in jobs:
            path = (AUTO, SORT)[i % 2]
            rc, h, g, taken, rows = wplan(lib, ptrs[:-2], ranges, ptrs[-2], ptrs[-1], n, path, stream=sp)
            assert rc == mq.MQ_OK and g == len(want[0]) and rows == int(want[1].sum()), (i, name, lib.mq_last_error())
            planned.append((h, g, taken, filled_outputs(lib, g, sp)))
        assert {p[2] for p in planned} == {DENSE, SORT}
        for (i, sp, *_), (h, g, taken, outs) in zip(jobs, planned):
            mq.check(write(lib, h, outs, sp), "mq_group_write")
        for sp in streams:
            mq.check(lib.mq_stream_sync(sp), "sync")
        for (i, sp, ptrs, keep, ranges, want, name), (h, g, taken, outs) in zip(jobs, planned):
            check_outputs(outs, g, want, (i, name, taken))
            mq.check(lib.mq_group_free(h), "mq_group_free")
    finally:
        mq.check(lib.mq_device_sync(), "device sync")
        for sp in streams:
            lib.mq_stream_destroy(sp)


def test_errors_write_nothing(lib, S):
    n = 1025
    cols, ranges = wc.case("uniform_50", n, 2)
    keys = gc.keys_of("uniform_100", n, S)
    vals = gc.values_of("uniform", keys)
    ptrs, keep = upload(cols + [keys, vals])
    p2, dk, dv = ptrs[:2], ptrs[2], ptrs[3]
    assert refused(lib, p2, ranges, dk, dv, 2**31, AUTO)                       # 2^31 rows (never read)
    assert refused(lib, [p2[0], None], ranges, dk, dv, n, AUTO)                # a NULL column
    assert refused(lib, [p2[0], p2[1] + 2], ranges, dk, dv, n, AUTO)           # not 4-byte aligned
    assert refused(lib, p2, ranges, None, dv, n, AUTO)
    assert refused(lib, p2, ranges, dk, None, n, AUTO)
    assert refused(lib, p2, ranges, dk + 1, dv, n, AUTO)
    assert refused(lib, p2, ranges, dk, dv + 2, n, AUTO)
    assert refused(lib, p2, ranges, dk, dv, n, 3)                              # no such path
    assert refused(lib, p2, ranges, dk, dv, n, -1)
    assert refused(lib, p2, ranges, dk, dv, n, AUTO, bounds=(5, 4))            # lo > hi
    assert refused(lib, p2, ranges, dk, dv, n, DENSE, bounds=(0, S))           # S + 1 values
    assert refused(lib, (p2 * 5)[:9], (ranges * 5)[:9], dk, dv, n, AUTO)       # nine predicates
    L = lib
    h, groups, taken, rows = C.c_void_p(77), C.c_uint64(77), C.c_int(-1), C.c_uint64(77)
    cp, cr = c_ptrs(p2), c_ranges(ranges)
    tail = (C.byref(h), C.byref(groups), C.byref(taken), C.byref(rows), None)
    for ncols in (0, -1, 9):
        h.value, groups.value, rows.value = 77, 77, 77
        assert L.mq_group_where_plan(cp, cr, ncols, dk, dv, n, None, AUTO, *tail) == mq.MQ_EINVAL
        assert (h.value, groups.value, rows.value) == (None, 0, 0)
    assert L.mq_group_where_plan(None, cr, 2, dk, dv, n, None, AUTO, *tail) == mq.MQ_EINVAL
    assert L.mq_group_where_plan(cp, None, 2, dk, dv, n, None, AUTO, *tail) == mq.MQ_EINVAL
    assert L.mq_group_where_plan(cp, cr, 2, dk, dv, n, None, AUTO, None, C.byref(groups), None, None, None) == mq.MQ_EINVAL
    assert L.mq_group_where_plan(cp, cr, 2, dk, dv, n, None, AUTO, C.byref(h), None, None, None, None) == mq.MQ_EINVAL
    assert h.value is None
    # h_path and h_rows may be NULL; and the operator still works
    assert L.mq_group_where_plan(cp, cr, 2, dk, dv, n, None, AUTO, C.byref(h), C.byref(groups), None, None, None) == mq.MQ_OK
    want = gw.model(cols, ranges, keys, vals)
    assert groups.value == len(want[0])
    mq.check(L.mq_group_free(h), "mq_group_free")
    run(lib, p2, ranges, dk, dv, n, AUTO, want, ("after the errors",))


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


def where_args(objs, ranges):
    gs = [gcol(o) for o in objs]
    n = max(len(gs), 1)
    gp = (C.POINTER(mq.GeneralizedColumn) * n)(*[C.pointer(g) for g in gs])
    lows = (C.POINTER(C.c_int) * n)(*[_b(lo) for lo, _ in ranges])
    highs = (C.POINTER(C.c_int) * n)(*[_b(hi) for _, hi in ranges])
    return gs, gp, lows, highs


def five(rpp):
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(5)]
    _libc.free(C.cast(rpp, C.c_void_p))
    return out


def fused(L, objs, ranges, keys, values, ncols=None):
    """group_aggregate_where -> (status, the five Results as (data_type, numpy array) or None)"""
    keep = where_args(objs, ranges)
    gk, gv, st = gcol(keys), gcol(values), mq.Status(0, None)
    rpp = L.group_aggregate_where(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, C.byref(gk),
                                  C.byref(gv), C.byref(st))
    return (st.code, five(rpp)) if rpp else (st.code, None)


def chain(L, objs, ranges, keys_c, vals_c):
    """select_where -> fetch_column x 2 -> group_aggregate through libmq."""
    keep = where_args(objs, ranges)
    st = mq.Status(0, None)
    pos = L.select_where(keep[1], keep[2], keep[3], len(objs), None, C.byref(st))
    assert st.code == mq.OK and pos
    fk = L.fetch_column(C.byref(keys_c), pos, C.byref(st))
    fv = L.fetch_column(C.byref(vals_c), pos, C.byref(st))
    assert st.code == mq.OK and fk and fv
    gk, gv = gcol(fk), gcol(fv)
    rpp = L.group_aggregate(C.byref(gk), C.byref(gv), C.byref(st))
    assert st.code == mq.OK and rpp
    out = five(rpp)
    for r in (pos, fk, fv):
        take(r)
    return out


def check_results(out, want, tag):
    assert [t for t, _ in out] == [mq.INT, mq.LONG, mq.LONG, mq.INT, mq.INT], tag
    for (_, got), w, nm in zip(out, want, NAMES):
        assert len(got) == len(w) and np.array_equal(got, w.astype(got.dtype)), tag + (nm,)


@pytest.mark.parametrize("keyset", ["skewed", "all_distinct"])
def test_dropin_equals_the_chain(lib, S, keyset):
    """Columns and INT Results as arguments; equal to select_where -> fetch_column x 2 ->
    group_aggregate through libmq and to the model, on the dense and on the sort path."""
    n = 70_001
    cols, ranges = wc.case("uniform_50", n, 3)
    keys = gc.keys_of(keyset, n, S)
    vals = gc.values_of("uniform", keys)
    want = gw.model(cols, ranges, keys, vals)
    assert len(want[0]) > 500
    cc, ck, cv = [make_column(c) for c in cols], make_column(keys), make_column(vals)
    ref = chain(lib, cc, ranges, ck, cv)
    check_results(ref, want, (keyset, "chain"))
    code, out = fused(lib, cc, ranges, ck, cv)
    assert code == mq.OK
    check_results(out, want, (keyset, "columns"))
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(out, ref))
    # INT Results: one with an HBM shadow, one of the caller's own
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    f1 = lib.fetch_column(C.byref(cc[1]), C.byref(every), C.byref(st))
    fk = lib.fetch_column(C.byref(ck), C.byref(every), C.byref(st))
    assert st.code == mq.OK and f1 and fk
    rv = make_result(vals)
    code, out = fused(lib, [cc[0], f1, cc[2]], ranges, fk, rv)
    assert code == mq.OK
    check_results(out, want, (keyset, "results"))
    code, out = fused(lib, cc, ranges, ck, ck)  # values = keys
    assert code == mq.OK
    check_results(out, gw.model(cols, ranges, keys, keys), (keyset, "keys x keys"))
    code, out = fused(lib, cc[:1], ranges[:1], cc[0], cv)  # keys = the predicate column
    assert code == mq.OK
    check_results(out, gw.model(cols[:1], ranges[:1], cols[0], vals), (keyset, "keys = column 0"))
    for r in (f1, fk):
        take(r)
    for r in (every, rv):
        free_result_struct(r)
    for c in cc + [ck, cv]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_outcomes_and_errors(lib, S, capfd):
    n = 1000
    cols, ranges = wc.case("uniform_50", n, 2)
    keys = gc.keys_of("uniform_100", n, S)
    vals = gc.values_of("uniform", keys)
    cc, ck, cv = [make_column(c) for c in cols], make_column(keys), make_column(vals)
    full = [(None, None), (0, 1000)]
    code, out = fused(lib, cc, full, ck, cv)
    assert code == mq.OK
    check_results(out, gc.group(keys, vals), ("full",))
    for none in ([(7, 7), (None, None)], [(2000, 3000), (0, 1000)]):
        code, out = fused(lib, cc, none, ck, cv)
        assert code == mq.OK
        check_results(out, gc.group(keys[:0], vals[:0]), ("empty", none))
    e = np.empty(0, np.int32)
    ce = make_column(e)
    code, out = fused(lib, [ce, ce], ranges, ce, ce)
    assert code == mq.OK
    check_results(out, gc.group(e, e), ("no rows",))
    short = make_column(cols[0][:999].copy())
    lng = make_result(cols[0].astype(np.int64), mq.LONG)
    capfd.readouterr()

    def refused_dropin(call):
        return call == (mq.ERROR, None) and "libmq" in capfd.readouterr().err

    assert refused_dropin(fused(lib, cc, ranges, ck, cv, ncols=0))
    assert refused_dropin(fused(lib, cc * 5, ranges * 5, ck, cv, ncols=9))
    assert refused_dropin(fused(lib, [cc[0], short], ranges, ck, cv))   # different lengths
    assert refused_dropin(fused(lib, cc, ranges, short, cv))
    assert refused_dropin(fused(lib, cc, ranges, ck, short))
    assert refused_dropin(fused(lib, [cc[0], lng], ranges, ck, cv))     # a LONG Result as a column
    assert refused_dropin(fused(lib, cc, ranges, lng, cv))              # ... as keys
    assert refused_dropin(fused(lib, cc, ranges, ck, lng))              # ... as values
    keep = where_args(cc, ranges)
    st, gk = mq.Status(0, None), gcol(ck)
    assert not lib.group_aggregate_where(keep[1], keep[2], keep[3], 2, C.byref(gk), None, C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_aggregate_where(keep[1], keep[2], keep[3], 2, None, C.byref(gk), C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_aggregate_where(None, keep[2], keep[3], 2, C.byref(gk), C.byref(gk), C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 3
    code, out = fused(lib, cc, ranges, ck, cv)  # and the operator still works
    assert code == mq.OK
    check_results(out, gw.model(cols, ranges, keys, vals), ("after the errors",))
    free_result_struct(lng)
    for c in cc + [ck, cv, ce, short]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_under_row_shards(lib, S):
    """MQ_SHARDS = 2 on device 0: columns held as row shards give the same bytes (the operator
    runs on the calling device) and are split again by the next sharded operator."""
    n = wc.BIG
    cols, ranges = wc.case("clustered_lead", n, 3)
    keys = gc.keys_of("skewed", n, S)
    vals = gc.values_of("uniform", keys)
    cc, ck, cv = [make_column(c) for c in cols], make_column(keys), make_column(vals)
    code, before = fused(lib, cc, ranges, ck, cv)
    assert code == mq.OK
    check_results(before, gw.model(cols, ranges, keys, vals), ("unsharded",))
    for c in cc + [ck, cv]:
        lib.mq_column_invalidate(C.byref(c))
    devs = (C.c_int * 2)(0, 0)
    assert lib.mq_shard_config(2, devs, 2, 0) == 0
    try:
        st = mq.Status(0, None)
        for c, (lo, hi) in ((cc[0], ranges[0]), (ck, (10, 1500))):  # splits the column
            first = lib.select_column(C.byref(c), _b(lo), _b(hi), C.byref(st))
            assert st.code == mq.OK and first
            take(first)
        code, out = fused(lib, cc, ranges, ck, cv)
        assert code == mq.OK
        assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(out, before))
        again = lib.select_column(C.byref(ck), _b(10), _b(1500), C.byref(st))
        assert st.code == mq.OK and np.array_equal(take(again), np.flatnonzero((keys >= 10) & (keys < 1500)).astype(np.int32))
    finally:
        for c in cc + [ck, cv]:
            lib.mq_column_invalidate(C.byref(c))
        assert lib.mq_shard_config(0, None, 0, 0) == 0
