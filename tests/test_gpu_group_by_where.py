"""group_aggregate_by_where on gfx950 (mq_group_by_where_plan, k_group_by_where_dense,
k_group_by_where_bounds and k_group_by_pack_pos in csrc/mq_group.hip; group_aggregate_by_where
in mq_query.c), every comparison exact equality: with the composed numpy model
(groupbycases.group_by over wherecases.mask), with mq_group_where_plan and mq_group_by_plan on
the same columns, and with the chain select_where -> fetch_column x (nkeys + 1) ->
group_aggregate_by run through libmq.

wc.SIZES (0 .. 8193) cover a 32-row line, a 256-row wave tile, the 1024-row tile and the ragged
tail; 70 001 and 300 001 rows several blocks; 300 007 rows on one limited CU a block that runs
its unrolled loop more than once (the regime is asserted first).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import groupbycases as gb
import groupbywherecases as gbw
import groupcases as gc
import wherecases as wc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PAD = 8
KEY_SENT = -7
SENT = {"count": 7, "sum": -77, "min": -777, "max": 777}
DTYPE = {"count": np.uint64, "sum": np.int64, "min": np.int32, "max": np.int32}
AGGS = ["count", "sum", "min", "max"]
WHO = b"mq_group_by_where_plan"


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
def S(lib):
    return lib.mq_group_dense_slots()


def c_ranges(ranges):
    return (mq.MqRange * max(len(ranges), 1))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in ranges])


def c_ptrs(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def upload(arrays, offs=(0,)):
    """One device copy per distinct array object (the same array twice is the same pointer
    twice), the k-th distinct one offs[k % len(offs)] dwords off a 16-byte boundary."""
    devs, ptrs = {}, []
    for a in arrays:
        if id(a) not in devs:
            devs[id(a)] = Dev.of(a, offset_elems=offs[len(devs) % len(offs)])
        ptrs.append(devs[id(a)].ptr)
    return ptrs, devs


def plan(L, ptrs, ranges, dks, dv, n, path, bounds=None, stream=None, ncols=None, nkeys=None):
    """(rc, handle, groups, path taken, matching rows)"""
    h, groups, taken, rows = C.c_void_p(77), C.c_uint64(12345), C.c_int(-1), C.c_uint64(54321)
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    rc = L.mq_group_by_where_plan(c_ptrs(ptrs), c_ranges(ranges), len(ptrs) if ncols is None else ncols, c_ptrs(dks),
                                  len(dks) if nkeys is None else nkeys, dv, n, b, path, C.byref(h), C.byref(groups),
                                  C.byref(taken), C.byref(rows), stream)
    return rc, h.value, groups.value, taken.value, rows.value


def out_buffers(g, nkeys, skip_keys=(), skip=()):
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


def run(L, ptrs, ranges, dks, dv, n, path, want, tag, bounds=None, skip_keys=(), skip=(), keys_null=False):
    """Plan, write into sentinel-filled outputs, compare, free. Returns the path taken."""
    rc, h, g, taken, rows = plan(L, ptrs, ranges, dks, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[1]), tag + ("groups", g)
    assert rows == int(want[1].sum()), tag + ("rows", rows)
    keys, aggs = out_buffers(g, len(dks), skip_keys, skip)
    mq.check(write(L, h, keys, aggs, keys_null), "mq_group_by_write")
    check_outputs(keys, aggs, g, want, tag, keys_written=not keys_null)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


def refused(L, *args, **kw):
    rc, h, g, _, rows = plan(L, *args, **kw)
    return (rc, h, g, rows) == (mq.MQ_EINVAL, None, 0, 0) and WHO in L.mq_last_error()


def auto_path(L, bounds):
    b = (C.c_int32 * len(bounds))(*bounds)
    return L.mq_group_by_auto_path(b, len(bounds) // 2, None)


def run_paths(L, S, cols, ranges, keys, vals, tag, offs=(0,), vals_is_last_key=False):
    """Every path the matching rows' key space allows, without bounds and with the exact ones,
    against the model; AUTO's choice is mq_group_by_auto_path's on the matching rows' bounds,
    and DENSE forced on a wider space is refused."""
    n, nkeys = len(vals), len(keys)
    m = wc.mask(cols, ranges)
    v = keys[-1] if vals_is_last_key else vals
    want = gb.group_by([k[m] for k in keys], v[m])
    assert int(want[1].sum()) == int(m.sum())
    ptrs, keep = upload(list(cols) + list(keys) + ([] if vals_is_last_key else [vals]), offs)
    pc, dks = ptrs[:len(cols)], ptrs[len(cols):len(cols) + nkeys]
    dv = dks[-1] if vals_is_last_key else ptrs[-1]
    exact = gb.bounds_of([k[m] for k in keys])
    if not exact:  # no matching row: every path plans nothing
        for path in (AUTO, DENSE, SORT):
            assert run(L, pc, ranges, dks, dv, n, path, want, tag + (path,)) == (SORT if path == SORT else DENSE)
        return want
    space = gb.space_of(exact)
    assert space <= 2**32
    auto = DENSE if space <= S else SORT
    assert auto_path(L, exact) == auto
    for path in (AUTO, DENSE, SORT) if auto == DENSE else (AUTO, SORT):
        for bounds in (None, exact):
            taken = run(L, pc, ranges, dks, dv, n, path, want, tag + (path, bounds), bounds)
            assert taken == (path if path != AUTO else auto), tag + (path, bounds, taken)
    if auto == SORT:
        for bounds in (None, exact):
            assert refused(L, pc, ranges, dks, dv, n, DENSE, bounds), tag + ("DENSE forced past S", bounds)
    return want


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.CASES)
def test_matrix_agrees_with_the_model(lib, S, name):
    """The rotation of groupbywherecases.matrix: this predicate set at ncols 1, 2, 3 and 8 with
    2, 3 and 4 key columns, at 0, 1025, 8193 rows and rotating further sizes, tuple and value
    sets rotating along, columns 0 and 1 dword off a 16-byte boundary in turn."""
    ci = wc.CASES.index(name)
    for q, (ncols, nkeys, n, ts, vs) in enumerate(gbw.matrix(ci)):
        cols, ranges = wc.case(name, n, ncols)
        keys = gb.tuples_of(ts, n, nkeys, S)
        vals = gc.values_of(vs, keys[0])
        offs = [(0,), (0, 1), (1, 0, 0), (1,)][(ci + q) % 4]
        run_paths(lib, S, cols, ranges, keys, vals, (name, ncols, nkeys, n, ts, vs), offs, vals_is_last_key=q % 5 == 4)


@pytest.mark.parametrize("n", [70_001, 300_001])
def test_several_blocks(lib, S, n):
    for pred, ncols, nkeys, ts in (("uniform_10", 2, 3, "skewed"), ("clustered_lead", 3, 2, "seven_shuffled"),
                                   ("islands_alt", 1, 4, "space_S")):
        cols, ranges = wc.case(pred, n, ncols)
        keys = gb.tuples_of(ts, n, nkeys, S)
        vals = gc.values_of("all_max", keys[0])
        run_paths(lib, S, cols, ranges, keys, vals, (pred, n, nkeys, ts), (n & 1, 0, 1))


@pytest.mark.parametrize("name", gbw.POISON_SETS)
def test_dead_rows_are_never_looked_at(lib, S, name):
    """Every failing row, in live lines and in whole dead lines, carries a component outside
    its column's bounds (the exact min and max over the matching rows), some of them with a
    summed code inside the table: the plan succeeds on both paths and equals the model."""
    for nkeys in gbw.NKEYS:
        cols, ranges, keys, vals, bounds = gbw.poisoned(name, nkeys)
        n = len(vals)
        want = gbw.model(cols, ranges, keys, vals)
        for offs in ((0,), (1, 0)):
            ptrs, keep = upload(cols + keys + [vals], offs)
            pc, dks, dv = ptrs[:2], ptrs[2:2 + nkeys], ptrs[-1]
            for path in (DENSE, AUTO):
                assert run(lib, pc, ranges, dks, dv, n, path, want, (name, nkeys, offs, path), bounds) == DENSE
            assert run(lib, pc, ranges, dks, dv, n, SORT, want, (name, nkeys, offs, SORT), bounds) == SORT
            assert run(lib, pc, ranges, dks, dv, n, AUTO, want, (name, nkeys, offs, "NULL bounds")) == DENSE


def _in_bounds(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(2, 8, n).astype(np.int32), rng.integers(1, 9, n).astype(np.int32)]


@pytest.mark.parametrize("stray", [(3, 12), (3, -1)])
@pytest.mark.parametrize("where", ["full_tile", "ragged_tile", "inside_uniform_tile", "lone_survivor_of_wave_tile"])
def test_component_wise_bounds_on_live_rows(lib, stray, where):
    """Bounds {0,9, 0,9} and one matching row whose tuple is (3, 12) or (3, -1): the summed
    slot, 42 or 29, lies inside the 100-slot table, the second component does not lie in its
    bounds. Both paths refuse the plan. The row sits in a full tile, in the ragged last tile,
    inside a wave tile whose other 255 rows share one tuple, or is the only survivor of its
    wave tile (which the dense kernel folds as a run). The same row failing the predicate is
    no error."""
    n = 4097
    bounds = [0, 9, 0, 9]
    assert 0 <= stray[0] * 10 + stray[1] < 100
    keys = _in_bounds(n, 3)
    lead = np.full(n, 5, dtype=np.int32)
    row = {"full_tile": 1000, "ragged_tile": n - 1, "inside_uniform_tile": 1100, "lone_survivor_of_wave_tile": 1100}[where]
    if where == "inside_uniform_tile":
        keys[0][1024:2048], keys[1][1024:2048] = 4, 6
    if where == "lone_survivor_of_wave_tile":
        lead[1024:1280] = -5
        lead[row] = 5
    keys[0][row], keys[1][row] = stray
    vals = gc.values_of("uniform", keys[0])
    ranges = [(0, 10)]
    ptrs, keep = upload([lead] + keys + [vals])
    for path in (DENSE, SORT, AUTO):
        assert refused(lib, ptrs[:1], ranges, ptrs[1:3], ptrs[3], n, path, bounds), (stray, where, path)
    # without bounds the same rows are fine
    run(lib, ptrs[:1], ranges, ptrs[1:3], ptrs[3], n, AUTO, gbw.model([lead], ranges, keys, vals), (stray, where, "NULL bounds"))
    # and so is the stray row where the predicate kills it
    lead[row] = -5
    ptrs, keep = upload([lead] + keys + [vals])
    want = gbw.model([lead], ranges, keys, vals)
    for path in (DENSE, SORT):
        assert run(lib, ptrs[:1], ranges, ptrs[1:3], ptrs[3], n, path, want, (stray, where, path, "dead"), bounds) == path


@pytest.mark.parametrize("nkeys", gbw.NKEYS)
def test_the_filter_narrows_the_key_space(lib, S, nkeys):
    """The key columns span 129 x 64 tuples; the predicates leave exactly S tuples in a space of
    S (DENSE under AUTO without bounds) and one tuple more (SORT, DENSE refused)."""
    cols, ranges, keys, vals = gbw.narrow(S, 0, nkeys)
    assert gb.space_of(gb.bounds_of(keys)) > S
    ptrs, keep = upload(cols + keys + [vals])
    pc, dks, dv, n = ptrs[:2], ptrs[2:2 + nkeys], ptrs[-1], len(vals)
    want = gbw.model(cols, ranges, keys, vals)
    assert len(want[1]) == S
    for path in (AUTO, DENSE, SORT):
        assert run(lib, pc, ranges, dks, dv, n, path, want, ("narrow", nkeys, path)) == (path or DENSE)
    cols, ranges, keys, vals = gbw.narrow(S, 1, nkeys)  # the same columns, one more code in the range
    want = gbw.model(cols, ranges, keys, vals)
    assert len(want[1]) == S + 1
    assert run(lib, pc, ranges, dks, dv, n, AUTO, want, ("narrow + 1", nkeys)) == SORT
    assert refused(lib, pc, ranges, dks, dv, n, DENSE)


@pytest.mark.parametrize("kill", ["nothing", "every_other_line", "one_row_a_wave_tile"])
def test_the_run_fold(lib, S, kill):
    """Sorted tuples, so that the surviving rows of most wave tiles share one slot: all rows
    surviving, every other 32-row line killed, and one dead row in every wave tile. The runs
    span tiles and are flushed where the slot changes."""
    for n, nkeys in ((8193, 2), (70_001, 4), (70_001, 3)):
        keys = gb.tuples_of("seven_sorted", n, nkeys, S)
        lead = np.full(n, 5, dtype=np.int32)
        if kill == "every_other_line":
            lead[(np.arange(n) // wc.LINE) % 2 == 1] = -5
        if kill == "one_row_a_wave_tile":
            t = np.arange(0, n, 256)
            rows = t + (17 * (t // 256)) % 256
            lead[rows[rows < n]] = -5
        other = np.ascontiguousarray(np.random.default_rng(n).integers(0, 1000, n), dtype=np.int32)
        cols, ranges = [lead, other], [(0, 10), (0, 1000)]
        uniform = np.ones(n // 256, dtype=bool)  # wave tiles whose surviving tuples are equal
        m = wc.mask(cols, ranges)
        for k in keys:
            tiles = np.where(m, k, k[0])[: n // 256 * 256].reshape(-1, 256)
            live = m[: n // 256 * 256].reshape(-1, 256)
            hi = np.where(live, tiles, gc.I32_MIN).max(axis=1)
            lo = np.where(live, tiles, gc.I32_MAX).min(axis=1)
            uniform &= hi == lo
        assert uniform.sum() > len(uniform) // 2
        vals = gc.values_of("uniform", keys[0])
        run_paths(lib, S, cols, ranges, keys, vals, (kill, n, nkeys), (n & 1, 0))


LONG_N = 300_007


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


@pytest.mark.parametrize("nkeys", [2, 3, 4])
@pytest.mark.parametrize("pred", ["uniform_50", "clustered_lead"])
def test_long_chunks(lib, S, one_cu, pred, nkeys):
    """One limited CU and 300 007 rows: a block gets at least 3 x 8192 rows, so the unrolled
    loops of the dense, the bounds and the mask kernels run several times, with the tail tiles
    and the ragged last tile; sums past 2^47."""
    n = LONG_N
    blocks, rpb = C.c_uint32(), C.c_uint64()
    lib.mq_scan_geometry(n, C.byref(blocks), C.byref(rpb))
    assert blocks.value <= 8 and rpb.value >= 3 * 8192, (blocks.value, rpb.value)
    cols, ranges = wc.case(pred, n, 2)
    for ts in ("seven_sorted", "space_S"):
        keys = gb.tuples_of(ts, n, nkeys, S)
        vals = gc.values_of("all_max", keys[0])
        want = gbw.model(cols, ranges, keys, vals)
        ptrs, keep = upload(cols + keys + [vals], (0, 1, 0))
        pc, dks, dv = ptrs[:2], ptrs[2:2 + nkeys], ptrs[-1]
        for path in (AUTO, SORT):
            assert run(lib, pc, ranges, dks, dv, n, path, want, (pred, nkeys, ts, path)) == (path or DENSE)


@pytest.mark.parametrize("n", [1025, 8193])
def test_alignment(lib, S, n):
    """One predicate column, each of two key columns and the values 0 and 1 dword off a 16-byte
    boundary, independently."""
    cols, ranges = wc.case("uniform_50", n, 1)
    keys = gb.tuples_of("seven_shuffled", n, 2, S)
    vals = gc.values_of("uniform", keys[0])
    want = gbw.model(cols, ranges, keys, vals)
    for oc, o0, o1, ov in itertools.product((0, 1), repeat=4):
        dc, d0, d1, dv = (Dev.of(a, offset_elems=o) for a, o in ((cols[0], oc), (keys[0], o0), (keys[1], o1), (vals, ov)))
        for path in (DENSE, SORT):
            assert run(lib, [dc.ptr], ranges, [d0.ptr, d1.ptr], dv.ptr, n, path, want, (n, oc, o0, o1, ov, path)) == path


def test_aliasing(lib, S):
    """A key that is a predicate column, values that are the last key, and one column as every key."""
    n = 8193
    cols, ranges = wc.case("same_twice", n, 3)
    assert cols[1] is cols[0]
    other = gb.tuples_of("seven_shuffled", n, 2, S)[1]
    keys = [cols[0], other]  # cols[0]: uniform in [0, 1000), under [100, 600)
    want = run_paths(lib, S, cols, ranges, keys, other, ("key = column 0, values = last key",), (1, 0), vals_is_last_key=True)
    assert len(want[1]) > 100
    for nkeys in (2, 3, 4):  # the same column for all keys: (x, x, ..)
        keys = [cols[2]] * nkeys
        for rng2 in ((250, 262), ranges[2]):  # 12^nkeys tuples' space fits the table with 2 and 3 keys
            r = [ranges[0], ranges[1], rng2]
            want = gbw.model(cols, r, keys, cols[0])
            assert all(np.array_equal(want[0][0], k) for k in want[0])
            ptrs, keep = upload(cols)
            dks = [ptrs[2]] * nkeys
            space = gb.space_of(gbw.matching_bounds(cols, r, keys))
            if space > 2**32:
                assert refused(lib, ptrs, r, dks, ptrs[0], n, AUTO)
                continue
            for path in (AUTO, SORT):
                taken = run(lib, ptrs, r, dks, ptrs[0], n, path, want, ("one column", nkeys, rng2, path))
                assert taken == (path or (DENSE if space <= S else SORT))


def raw_outputs(L, nkeys, planned, by_write=True):
    """The key and aggregate outputs (sentinels behind them included) of a planned handle."""
    rc, h, g = planned[:3]
    assert rc == mq.MQ_OK and h, L.mq_last_error()
    keys, aggs = out_buffers(g, nkeys)
    if by_write:
        mq.check(write(L, h, keys, aggs), "mq_group_by_write")
    else:
        mq.check(L.mq_group_write(h, keys[0].ptr, *[aggs[nm].ptr for nm in AGGS], None), "mq_group_write")
    got = [k.get(np.int32, g + PAD) for k in keys] + [aggs[nm].get(DTYPE[nm], g + PAD) for nm in AGGS]
    mq.check(L.mq_group_free(h), "mq_group_free")
    return g, got


def test_identities(lib, S):
    n = 70_001
    cols, ranges = wc.case("uniform_50", n, 3)
    pcols, keep0 = upload(cols, (0, 1))
    # one key column: mq_group_where_plan
    for keyset in ("uniform_100", "all_distinct"):
        k1 = gc.keys_of(keyset, n, S)
        vals = gc.values_of("uniform", k1)
        dk, dv = Dev.of(k1, offset_elems=1), Dev.of(vals)
        for path in (AUTO, SORT):
            h, groups, taken, rows = C.c_void_p(), C.c_uint64(), C.c_int(-1), C.c_uint64()
            rc = lib.mq_group_where_plan(c_ptrs(pcols), c_ranges(ranges), 3, dk.ptr, dv.ptr, n, None, path, C.byref(h),
                                         C.byref(groups), C.byref(taken), C.byref(rows), None)
            g0, ref = raw_outputs(lib, 1, (rc, h.value, groups.value), by_write=False)
            p = plan(lib, pcols, ranges, [dk.ptr], dv.ptr, n, path)
            assert p[3] == taken.value and p[4] == rows.value
            g1, got = raw_outputs(lib, 1, p)
            assert g0 == g1 and all(np.array_equal(a, b) for a, b in zip(ref, got)), (keyset, path)
    for ts, nkeys in (("skewed", 2), ("all_distinct", 3), ("seven_sorted", 4)):
        keys = gb.tuples_of(ts, n, nkeys, S)
        vals = gc.values_of("uniform", keys[0])
        ptrs, keep = upload(keys + [vals], (1, 0))
        dks, dv = ptrs[:nkeys], ptrs[-1]
        paths = (DENSE, SORT) if gb.space_of(gb.bounds_of(keys)) <= S else (SORT,)
        # every range unbounded: mq_group_by_plan's outputs on the same columns
        for path in paths:
            h, groups = C.c_void_p(), C.c_uint64()
            rc = lib.mq_group_by_plan(c_ptrs(dks), nkeys, dv, n, None, path, C.byref(h), C.byref(groups), None, None)
            g0, ref = raw_outputs(lib, nkeys, (rc, h.value, groups.value))
            p = plan(lib, pcols, [(None, None)] * 3, dks, dv, n, path)
            assert p[4] == n
            g1, got = raw_outputs(lib, nkeys, p)
            assert g0 == g1 and all(np.array_equal(a, b) for a, b in zip(ref, got)), (ts, path)
        # wider bounds give the same result; permuting the predicates changes nothing
        want = gbw.model(cols, ranges, keys, vals)
        exact = gbw.matching_bounds(cols, ranges, keys)
        wider = [b + (-3 if i % 2 == 0 else 2) for i, b in enumerate(exact)]
        full = gb.bounds_of(keys)
        for path in paths:
            for bounds in (wider, full):
                if gb.space_of(bounds) <= (S if path == DENSE else 2**32):
                    assert run(lib, pcols, ranges, dks, dv, n, path, want, (ts, path, bounds), bounds) == path
            base = None
            for perm in itertools.permutations(range(3)):
                g, got = raw_outputs(lib, nkeys, plan(lib, [pcols[i] for i in perm], [ranges[i] for i in perm], dks, dv, n, path))
                blob = b"".join(a.tobytes() for a in got)
                base = base or blob
                assert g == len(want[1]) and blob == base, (ts, path, perm)
            assert np.array_equal(got[nkeys][:g], want[1])


@pytest.mark.parametrize("name", ["first_none", "empty_range", "empty_high_min", "no_rows"])
def test_empty_outcomes(lib, S, name):
    """Zero groups, MQ_OK, a handle that frees, and a write that leaves the sentinels."""
    n = 0 if name == "no_rows" else 4097
    cols, ranges = wc.case("uniform_50" if name == "no_rows" else name, n, 3)
    keys = gb.tuples_of("seven_shuffled", n, 3, S)
    vals = gc.values_of("uniform", keys[0])
    ptrs, keep = upload(cols + keys + [vals])
    want = gb.group_by([k[:0] for k in keys], vals[:0])
    for path in (AUTO, DENSE, SORT):
        for bounds in (None, [-5, 5, 100, 103, -1000, -999], [gc.I32_MIN, gc.I32_MAX, 0, 0, 7, 7]):
            if bounds and gb.space_of(bounds) > S and path == DENSE and n:
                assert refused(lib, ptrs[:3], ranges, ptrs[3:6], ptrs[6], n, path, bounds)  # the arguments come first
                continue
            rc, h, g, taken, rows = plan(lib, ptrs[:3], ranges, ptrs[3:6], ptrs[6], n, path, bounds)
            assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h, (name, path, bounds, lib.mq_last_error())
            # AUTO reports what the given bounds pick once the columns are read (first_none: its ranges are
            # satisfiable); a plan that ends before that reports DENSE
            by_bounds = path == AUTO and bounds and name == "first_none" and gb.space_of(bounds) > S
            assert taken == (SORT if path == SORT or by_bounds else DENSE), (name, path, bounds, taken)
            kb, aggs = out_buffers(0, 3)
            mq.check(write(lib, h, kb, aggs), "mq_group_by_write")
            check_outputs(kb, aggs, 0, want, (name, path, bounds))
            mq.check(lib.mq_group_free(h), "mq_group_free")
    if n == 0:  # NULL columns and any bounds are fine without rows
        rc, h, g, taken, rows = plan(lib, [None, None], ranges[:2], [None, None], None, 0, AUTO, bounds=[3, 1, 0, 0])
        assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h
        mq.check(lib.mq_group_by_write(h, None, None, None, None, None, None), "mq_group_by_write")
        mq.check(lib.mq_group_free(h), "mq_group_free")


def test_errors_write_nothing(lib, S):
    n = 1025
    cols, ranges = wc.case("uniform_50", n, 2)
    keys = _in_bounds(n, 5)
    vals = gc.values_of("uniform", keys[0])
    ptrs, keep = upload(cols + keys + [vals])
    p2, dks, dv = ptrs[:2], ptrs[2:4], ptrs[4]
    assert refused(lib, p2, ranges, dks, dv, 2**31, AUTO)                          # 2^31 rows (never read)
    assert refused(lib, [p2[0], None], ranges, dks, dv, n, AUTO)                   # a NULL column
    assert refused(lib, [p2[0], p2[1] + 2], ranges, dks, dv, n, AUTO)              # not 4-byte aligned
    assert refused(lib, p2, ranges, [dks[0], None], dv, n, AUTO)
    assert refused(lib, p2, ranges, [dks[0] + 1, dks[1]], dv, n, AUTO)
    assert refused(lib, p2, ranges, dks, None, n, AUTO)
    assert refused(lib, p2, ranges, dks, dv + 2, n, AUTO)
    assert refused(lib, p2, ranges, dks, dv, n, 3)                                 # no such path
    assert refused(lib, p2, ranges, dks, dv, n, -1)
    assert refused(lib, p2, ranges, dks, dv, n, AUTO, bounds=[0, 9, 5, 4])         # lo > hi
    assert refused(lib, p2, ranges, dks, dv, n, AUTO, bounds=[9, 0, 0, 9])
    assert refused(lib, p2, ranges, dks, dv, n, DENSE, bounds=[0, S, 0, 9])        # P > slots, DENSE forced
    assert refused(lib, p2, ranges, dks, dv, n, AUTO, bounds=[gc.I32_MIN, gc.I32_MAX, 0, 9])  # P > 2^32
    assert b"2^32" in lib.mq_last_error()
    assert refused(lib, p2, ranges, dks, dv, n, AUTO, bounds=[3, 7, 1, 8])         # a matching key excluded
    assert refused(lib, (p2 * 5)[:9], (ranges * 5)[:9], dks, dv, n, AUTO)          # nine predicates
    for ncols in (0, -1, 9):
        assert refused(lib, p2, ranges, dks, dv, n, AUTO, ncols=ncols)
    for nkeys in (0, -1, 5):
        assert refused(lib, p2, ranges, (dks * 3)[:5], dv, n, AUTO, nkeys=nkeys)
    L = lib
    h, groups, rows = C.c_void_p(77), C.c_uint64(77), C.c_uint64(77)
    cp, cr, ck = c_ptrs(p2), c_ranges(ranges), c_ptrs(dks)
    tail = (C.byref(h), C.byref(groups), None, C.byref(rows), None)
    for args in ((None, cr, 2, ck), (cp, None, 2, ck), (cp, cr, 2, None)):
        h.value, groups.value, rows.value = 77, 77, 77
        assert L.mq_group_by_where_plan(*args, 2, dv, n, None, AUTO, *tail) == mq.MQ_EINVAL
        assert (h.value, groups.value, rows.value) == (None, 0, 0)
    assert L.mq_group_by_where_plan(cp, cr, 2, ck, 2, dv, n, None, AUTO, None, C.byref(groups), None, None, None) == mq.MQ_EINVAL
    assert L.mq_group_by_where_plan(cp, cr, 2, ck, 2, dv, n, None, AUTO, C.byref(h), None, None, None, None) == mq.MQ_EINVAL
    assert h.value is None
    # h_path and h_rows may be NULL; and the operator still works
    assert L.mq_group_by_where_plan(cp, cr, 2, ck, 2, dv, n, None, AUTO, C.byref(h), C.byref(groups), None, None, None) == mq.MQ_OK
    want = gbw.model(cols, ranges, keys, vals)
    assert groups.value == len(want[1])
    mq.check(L.mq_group_free(h), "mq_group_free")
    run(lib, p2, ranges, dks, dv, n, AUTO, want, ("after the errors",))


@pytest.mark.parametrize("ts", ["seven_shuffled", "all_distinct"])
def test_null_outputs(lib, S, ts):
    n, nkeys = 4097, 3
    cols, ranges = wc.case("uniform_50", n, 2)
    keys = gb.tuples_of(ts, n, nkeys, S)
    vals = gc.values_of("uniform", keys[0])
    want = gbw.model(cols, ranges, keys, vals)
    ptrs, keep = upload(cols + keys + [vals], (0, 1))
    pc, dks, dv = ptrs[:2], ptrs[2:5], ptrs[5]
    paths = (DENSE, SORT) if gb.space_of(gbw.matching_bounds(cols, ranges, keys)) <= S else (SORT,)
    for path in paths:
        for j in range(nkeys):  # each key output NULL in turn
            run(lib, pc, ranges, dks, dv, n, path, want, (ts, path, "no key", j), skip_keys=(j,))
        run(lib, pc, ranges, dks, dv, n, path, want, (ts, path, "no keys"), skip_keys=(0, 1, 2))
        run(lib, pc, ranges, dks, dv, n, path, want, (ts, path, "NULL key array"), keys_null=True)
        for skip in [("count",), ("sum", "min", "max"), ("count", "sum", "min", "max")]:
            run(lib, pc, ranges, dks, dv, n, path, want, (ts, path, skip), skip=skip)
        # mq_group_write on the multi-key handle: the aggregates without keys; keys are refused
        rc, h, g, _, _ = plan(lib, pc, ranges, dks, dv, n, path)
        assert rc == mq.MQ_OK and g == len(want[1])
        kb, aggs = out_buffers(g, 1)
        mq.check(lib.mq_group_write(h, None, *[aggs[nm].ptr for nm in AGGS], None), "mq_group_write")
        check_outputs([], aggs, g, want, (ts, path, "mq_group_write"))
        assert lib.mq_group_write(h, kb[0].ptr, *[aggs[nm].ptr for nm in AGGS], None) == mq.MQ_EINVAL
        assert np.all(kb[0].get(np.int32, g + PAD) == KEY_SENT)
        mq.check(lib.mq_group_free(h), "mq_group_free")


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
        tsets = ["seven_shuffled", "all_distinct", "seven_sorted", "skewed", "space_S_plus_1"]
        for i, sp in enumerate(streams):
            name, ncols, nkeys = wc.CASES[(3 * i) % len(wc.CASES)], wc.NCOLS[i % 4], gbw.NKEYS[i % 3]
            cols, ranges = wc.case(name, n, ncols)
            keys = gb.tuples_of(tsets[i % len(tsets)], n, nkeys, S)
            vals = gc.values_of("uniform", keys[0])
            want = gbw.model(cols, ranges, keys, vals)
            ptrs, keep = upload(cols + keys + [vals], (i & 1, 0))
            jobs.append((i, sp, ptrs, keep, ranges, want, name, ncols, nkeys))
        mq.check(lib.mq_device_sync(), "device sync")  # the uploads (null stream) are done
        planned = []
        for i, sp, ptrs, keep, ranges, want, name, ncols, nkeys in jobs:
            rc, h, g, taken, rows = plan(lib, ptrs[:ncols], ranges, ptrs[ncols:ncols + nkeys], ptrs[-1], n, (AUTO, SORT)[i % 2],
                                         stream=sp)
            assert rc == mq.MQ_OK and g == len(want[1]) and rows == int(want[1].sum()), (i, name, lib.mq_last_error())
            planned.append((h, g, taken, out_buffers(g, nkeys)))
        assert {p[2] for p in planned} == {DENSE, SORT}
        mq.check(lib.mq_device_sync(), "device sync")  # the sentinel uploads (null stream) are done
        for (i, sp, *_), (h, g, taken, (kb, aggs)) in zip(jobs, planned):
            mq.check(write(lib, h, kb, aggs, stream=sp), "mq_group_by_write")
        for sp in streams:
            mq.check(lib.mq_stream_sync(sp), "sync")
        for (i, sp, ptrs, keep, ranges, want, name, ncols, nkeys), (h, g, taken, (kb, aggs)) in zip(jobs, planned):
            check_outputs(kb, aggs, g, want, (i, name, taken))
            mq.check(lib.mq_group_free(h), "mq_group_free")
    finally:
        mq.check(lib.mq_device_sync(), "device sync")
        for sp in streams:
            lib.mq_stream_destroy(sp)


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


def results(rpp, count):
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(count)]
    _libc.free(C.cast(rpp, C.c_void_p))
    return out


def fused(L, objs, ranges, keys, values, ncols=None, nkeys=None):
    """group_aggregate_by_where -> (status, the nkeys + 4 Results as (data_type, numpy array) or None)"""
    keep = where_args(objs, ranges)
    gks, gv, st = [gcol(k) for k in keys], gcol(values), mq.Status(0, None)
    arr = (C.POINTER(mq.GeneralizedColumn) * max(len(gks), 1))(*[C.pointer(g) for g in gks])
    nkeys = len(keys) if nkeys is None else nkeys
    rpp = L.group_aggregate_by_where(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, arr, nkeys, C.byref(gv),
                                     C.byref(st))
    return (st.code, results(rpp, nkeys + 4)) if rpp else (st.code, None)


def chain(L, objs, ranges, key_cols, vals_c):
    """select_where -> fetch_column x (nkeys + 1) -> group_aggregate_by through libmq."""
    keep = where_args(objs, ranges)
    st = mq.Status(0, None)
    pos = L.select_where(keep[1], keep[2], keep[3], len(objs), None, C.byref(st))
    assert st.code == mq.OK and pos
    fetched = [L.fetch_column(C.byref(c), pos, C.byref(st)) for c in key_cols + [vals_c]]
    assert st.code == mq.OK and all(fetched)
    gks, gv = [gcol(f) for f in fetched[:-1]], gcol(fetched[-1])
    arr = (C.POINTER(mq.GeneralizedColumn) * len(gks))(*[C.pointer(g) for g in gks])
    rpp = L.group_aggregate_by(arr, len(gks), C.byref(gv), C.byref(st))
    assert st.code == mq.OK and rpp
    out = results(rpp, len(gks) + 4)
    for r in [pos] + fetched:
        take(r)
    return out


def check_results(out, want, tag):
    nkeys = len(want[0])
    assert [t for t, _ in out] == [mq.INT] * nkeys + [mq.LONG, mq.LONG, mq.INT, mq.INT], tag
    for i, ((_, got), w) in enumerate(zip(out, list(want[0]) + list(want[1:]))):
        assert len(got) == len(w) and np.array_equal(got, w.astype(got.dtype)), tag + (i,)


@pytest.mark.parametrize("ts,nkeys", [("skewed", 2), ("all_distinct", 3), ("seven_shuffled", 4)])
def test_dropin_equals_the_chain(lib, S, ts, nkeys):
    """Columns and INT Results as arguments; equal to select_where -> fetch_column x (nkeys + 1)
    -> group_aggregate_by through libmq and to the model, on the dense and on the sort path."""
    n = 70_001
    cols, ranges = wc.case("uniform_50", n, 3)
    keys = gb.tuples_of(ts, n, nkeys, S)
    vals = gc.values_of("uniform", keys[0])
    want = gbw.model(cols, ranges, keys, vals)
    cc, ck, cv = [make_column(c) for c in cols], [make_column(k) for k in keys], make_column(vals)
    ref = chain(lib, cc, ranges, ck, cv)
    check_results(ref, want, (ts, "chain"))
    code, out = fused(lib, cc, ranges, ck, cv)
    assert code == mq.OK
    check_results(out, want, (ts, "columns"))
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(out, ref))
    # INT Results: two with an HBM shadow, one of the caller's own
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    f1 = lib.fetch_column(C.byref(cc[1]), C.byref(every), C.byref(st))
    fk = lib.fetch_column(C.byref(ck[0]), C.byref(every), C.byref(st))
    assert st.code == mq.OK and f1 and fk
    rv = make_result(vals)
    code, out = fused(lib, [cc[0], f1, cc[2]], ranges, [fk] + ck[1:], rv)
    assert code == mq.OK
    check_results(out, want, (ts, "results"))
    code, out = fused(lib, cc, ranges, ck, ck[-1])  # values = the last key
    assert code == mq.OK
    check_results(out, gbw.model(cols, ranges, keys, keys[-1]), (ts, "values = last key"))
    code, out = fused(lib, cc[:1], ranges[:1], [cc[0]] + ck[1:], cv)  # the first key = the predicate column
    assert code == mq.OK
    check_results(out, gbw.model(cols[:1], ranges[:1], [cols[0]] + keys[1:], vals), (ts, "key 0 = column 0"))
    code, out = fused(lib, cc, ranges, ck[:1], cv)  # one key column: group_aggregate_where's answer
    assert code == mq.OK
    check_results(out, gbw.model(cols, ranges, keys[:1], vals), (ts, "one key"))
    for r in (f1, fk):
        take(r)
    for r in (every, rv):
        free_result_struct(r)
    for c in cc + ck + [cv]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_outcomes_and_errors(lib, S, capfd):
    n = 1000
    cols, ranges = wc.case("uniform_50", n, 2)
    keys = gb.tuples_of("seven_shuffled", n, 2, S)
    vals = gc.values_of("uniform", keys[0])
    cc, ck, cv = [make_column(c) for c in cols], [make_column(k) for k in keys], make_column(vals)
    code, out = fused(lib, cc, [(None, None), (0, 1000)], ck, cv)
    assert code == mq.OK
    check_results(out, gb.group_by(keys, vals), ("full",))
    for none in ([(7, 7), (None, None)], [(2000, 3000), (0, 1000)]):
        code, out = fused(lib, cc, none, ck, cv)
        assert code == mq.OK
        check_results(out, gb.group_by([k[:0] for k in keys], vals[:0]), ("empty", none))
    e = np.empty(0, np.int32)
    ce = make_column(e)
    code, out = fused(lib, [ce, ce], ranges, [ce, ce, ce], ce)
    assert code == mq.OK
    check_results(out, gb.group_by([e, e, e], e), ("no rows",))
    short = make_column(cols[0][:999].copy())
    lng = make_result(cols[0].astype(np.int64), mq.LONG)
    ends = make_column(gc.keys_of("int32_ends", n, 0))
    capfd.readouterr()

    def refused_dropin(call):
        return call == (mq.ERROR, None) and "libmq" in capfd.readouterr().err

    assert refused_dropin(fused(lib, cc, ranges, ck, cv, ncols=0))
    assert refused_dropin(fused(lib, cc * 5, ranges * 5, ck, cv, ncols=9))
    assert refused_dropin(fused(lib, cc, ranges, ck * 3, cv, nkeys=0))
    assert refused_dropin(fused(lib, cc, ranges, ck * 3, cv, nkeys=5))
    assert refused_dropin(fused(lib, [cc[0], short], ranges, ck, cv))   # different lengths
    assert refused_dropin(fused(lib, cc, ranges, [ck[0], short], cv))
    assert refused_dropin(fused(lib, cc, ranges, ck, short))
    assert refused_dropin(fused(lib, [cc[0], lng], ranges, ck, cv))     # a LONG Result as a column
    assert refused_dropin(fused(lib, cc, ranges, [lng, ck[1]], cv))     # ... as a key
    assert refused_dropin(fused(lib, cc, ranges, ck, lng))              # ... as values
    code, out = fused(lib, cc, [(None, None), (None, None)], [ends, ck[0]], cv)  # a key space wider than 2^32
    err = capfd.readouterr().err
    assert (code, out) == (mq.ERROR, None) and "libmq" in err and "2^32" in err
    keep = where_args(cc, ranges)
    gks = [gcol(k) for k in ck]
    arr = (C.POINTER(mq.GeneralizedColumn) * 2)(*[C.pointer(g) for g in gks])
    st = mq.Status(0, None)
    assert not lib.group_aggregate_by_where(keep[1], keep[2], keep[3], 2, arr, 2, None, C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_aggregate_by_where(keep[1], keep[2], keep[3], 2, None, 2, C.byref(gks[0]), C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.group_aggregate_by_where(None, keep[2], keep[3], 2, arr, 2, C.byref(gks[0]), C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 3
    code, out = fused(lib, cc, ranges, ck, cv)  # and the operator still works
    assert code == mq.OK
    check_results(out, gbw.model(cols, ranges, keys, vals), ("after the errors",))
    free_result_struct(lng)
    for c in cc + ck + [cv, ce, short, ends]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_under_row_shards(lib, S):
    """MQ_SHARDS = 2 on device 0: columns held as row shards give the same bytes (the operator
    runs on the calling device) and are split again by the next sharded operator."""
    n = wc.BIG
    cols, ranges = wc.case("clustered_lead", n, 3)
    keys = gb.tuples_of("skewed", n, 2, S)
    vals = gc.values_of("uniform", keys[0])
    cc, ck, cv = [make_column(c) for c in cols], [make_column(k) for k in keys], make_column(vals)
    code, before = fused(lib, cc, ranges, ck, cv)
    assert code == mq.OK
    check_results(before, gbw.model(cols, ranges, keys, vals), ("unsharded",))
    for c in cc + ck + [cv]:
        lib.mq_column_invalidate(C.byref(c))
    devs = (C.c_int * 2)(0, 0)
    assert lib.mq_shard_config(2, devs, 2, 0) == 0
    try:
        st = mq.Status(0, None)
        klo, khi = int(keys[0].min()), int(keys[0].min()) + 3
        for c, (lo, hi) in ((cc[0], ranges[0]), (ck[0], (klo, khi))):  # splits the column
            first = lib.select_column(C.byref(c), _b(lo), _b(hi), C.byref(st))
            assert st.code == mq.OK and first
            take(first)
        code, out = fused(lib, cc, ranges, ck, cv)
        assert code == mq.OK
        assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() for a, b in zip(out, before))
        again = lib.select_column(C.byref(ck[0]), _b(klo), _b(khi), C.byref(st))
        assert st.code == mq.OK
        assert np.array_equal(take(again), np.flatnonzero((keys[0] >= klo) & (keys[0] < khi)).astype(np.int32))
    finally:
        for c in cc + ck + [cv]:
            lib.mq_column_invalidate(C.byref(c))
        assert lib.mq_shard_config(0, None, 0, 0) == 0
