"""mq_group_top and the drop-in group_top_k on gfx950 (mq_group.hip, mq_topk64.hip, mq_query.c):
HAVING, ORDER BY an aggregate and LIMIT over the groups of a handle from each of the six plans, and
over the Results of group_aggregate and group_aggregate_measures. The check is the handle's own
mq_group_by_write of everything (the existing tests pin that against the models) followed by the
numpy restatement in topk64cases.py; every comparison is exact equality.
"""
import ctypes as C

import numpy as np
import pytest

import groupbycases as gb
import groupbywherecases as gbw  # noqa: F401  (the where cases below are its shapes)
import groupcases as gc
import groupjoincases as gj
import groupwherecases as gw  # noqa: F401
import measurecases as mc
import starcases as sc
import topk64cases as tc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take
from test_gpu_group_by_where import gcol, where_args
from test_gpu_group_where import c_ptrs, c_ranges
from test_gpu_star import gptrs

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
KEY, COUNT, SUM, MIN, MAX = range(5)
PAD = 8
SENT_BYTE = 0x5A
DT = {COUNT: np.uint64, SUM: np.int64, MIN: np.int32, MAX: np.int32}
N = 70_001  # several blocks of every plan's kernels; the sort path's chunks hold many runs


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # see test_gpu_topk.py: one drop-in operator before this module's numpy temporaries come and go
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    return L


# ---------------------------------------------------------------------------
# handles from the six plans: (handle, groups, nkeys, what to keep alive)
# ---------------------------------------------------------------------------

def _out():
    return C.c_void_p(), C.c_uint64(), C.c_int(-1), C.c_uint64()


def _pred(n):
    """Two predicate columns: about a third of the rows survive."""
    rng = np.random.default_rng(n + 1)
    cols = [np.ascontiguousarray(rng.integers(0, 100, n), np.int32) for _ in range(2)]
    return cols, [(10, 70), (None, 55)]


def plan_group(L, n, sort):
    keys = gc.keys_of("range_S_plus_1" if sort else "uniform_100", n, 2048)
    vals = gc.values_of("uniform", keys)
    dk, dv = Dev.of(keys), Dev.of(vals)
    h, g, p, _ = _out()
    mq.check(L.mq_group_plan(dk.ptr, dv.ptr, n, None, AUTO, C.byref(h), C.byref(g), C.byref(p), None), "mq_group_plan")
    return h, g.value, 1, p.value, (dk, dv)


def plan_where(L, n, sort):
    keys = gc.keys_of("all_distinct" if sort else "uniform_100", n, 2048)
    vals = gc.values_of("uniform", keys)
    cols, ranges = _pred(n)
    dc, dk, dv = [Dev.of(c) for c in cols], Dev.of(keys), Dev.of(vals)
    h, g, p, rows = _out()
    mq.check(L.mq_group_where_plan(c_ptrs([d.ptr for d in dc]), c_ranges(ranges), 2, dk.ptr, dv.ptr, n, None, AUTO, C.byref(h),
                                   C.byref(g), C.byref(p), C.byref(rows), None), "mq_group_where_plan")
    return h, g.value, 1, p.value, (dc, dk, dv)


def plan_by(L, n, sort, nkeys=3):
    keys = gb.tuples_of("all_distinct" if sort else "space_S", n, nkeys, 2048)
    vals = gc.values_of("uniform", keys[0])
    dks, dv = [Dev.of(k) for k in keys], Dev.of(vals)
    h, g, p, _ = _out()
    mq.check(L.mq_group_by_plan(c_ptrs([d.ptr for d in dks]), nkeys, dv.ptr, n, None, AUTO, C.byref(h), C.byref(g), C.byref(p),
                                None), "mq_group_by_plan")
    return h, g.value, nkeys, p.value, (dks, dv)


def plan_by_where(L, n, sort, nkeys=3):
    keys = gb.tuples_of("all_distinct" if sort else "space_S", n, nkeys, 2048)
    vals = gc.values_of("uniform", keys[0])
    cols, ranges = _pred(n)
    dc, dks, dv = [Dev.of(c) for c in cols], [Dev.of(k) for k in keys], Dev.of(vals)
    h, g, p, rows = _out()
    mq.check(L.mq_group_by_where_plan(c_ptrs([d.ptr for d in dc]), c_ranges(ranges), 2, c_ptrs([d.ptr for d in dks]), nkeys, dv.ptr,
                                      n, None, AUTO, C.byref(h), C.byref(g), C.byref(p), C.byref(rows), None),
             "mq_group_by_where_plan")
    return h, g.value, nkeys, p.value, (dc, dks, dv)


class Maps(list):
    """Key maps to free once the handle planned over them is gone."""


def free_maps(L, keep):
    mq.check(L.mq_device_sync(), "sync")
    for x in keep:
        if isinstance(x, Maps):
            for km in x:
                mq.check(L.mq_keymap_free(km), "mq_keymap_free")


def _keymap(L, card, seed):
    dk, da = sc.dimension(seed, card, -3)
    ddk, dda, km = Dev.of(dk), Dev.of(da), C.c_void_p()
    mq.check(L.mq_keymap_build(ddk.ptr, dda.ptr, len(dk), 0, 0, 0, C.byref(km), None, None), "mq_keymap_build")
    return dk, km, (ddk, dda)


def plan_join(L, n, sort):
    dk, km, keep = _keymap(L, 3000 if sort else 200, 3)
    fkey = gj.fact_keys("half_present", n, dk)
    vals = gc.values_of("uniform", fkey)
    cols, ranges = _pred(n)
    dc, df, dv = [Dev.of(c) for c in cols], Dev.of(fkey), Dev.of(vals)
    h, g, p, rows = _out()
    mq.check(L.mq_group_join_plan(c_ptrs([d.ptr for d in dc]), c_ranges(ranges), 2, df.ptr, km, dv.ptr, n, None, AUTO, C.byref(h),
                                  C.byref(g), C.byref(p), C.byref(rows), None), "mq_group_join_plan")
    return h, g.value, 1, p.value, (keep, dc, df, dv, Maps([km]))


def plan_star(L, n, sort):
    """km x plain x km: three key components."""
    cards = (40, 9, 300) if sort else (8, 16, 16)
    terms = sc.make("km_plain_km", cards, n, seed=4)
    vals = gc.values_of("uniform", terms[0].col)
    arr, keep, maps = (mq.MqStarTerm * 3)(), [], []
    for j, t in enumerate(terms):
        d = Dev.of(t.col)
        keep.append(d)
        km = None
        if t.kind == "km":
            ddk, dda, km = Dev.of(t.dim_keys), Dev.of(t.dim_attrs), C.c_void_p()
            mq.check(L.mq_keymap_build(ddk.ptr, dda.ptr, len(t.dim_keys), 0, 0, 0, C.byref(km), None, None), "mq_keymap_build")
            keep += [ddk, dda]
            maps.append(km)
        arr[j] = mq.MqStarTerm(d.ptr, km.value if km else None, None)
    dv = Dev.of(vals)
    h, g, p, rows = _out()
    mq.check(L.mq_group_star_plan(None, None, 0, arr, 3, dv.ptr, n, None, AUTO, C.byref(h), C.byref(g), C.byref(p), C.byref(rows),
                                  None), "mq_group_star_plan")
    return h, g.value, 3, p.value, (keep, dv, Maps(maps))


PLANS = {"group": plan_group, "where": plan_where, "by": plan_by, "by_where": plan_by_where, "join": plan_join, "star": plan_star}


def write_all(L, h, g, nkeys):
    """mq_group_by_write of everything: (key columns, {agg: column})."""
    dk = [Dev(4 * g) for _ in range(nkeys)]
    da = {a: Dev(np.dtype(DT[a]).itemsize * g) for a in DT}
    mq.check(L.mq_group_by_write(h, c_ptrs([d.ptr for d in dk]), da[COUNT].ptr, da[SUM].ptr, da[MIN].ptr, da[MAX].ptr, None),
             "mq_group_by_write")
    return [d.get(np.int32, g) for d in dk], {a: da[a].get(DT[a], g) for a in DT}


def order_of(order_by, desc, k, having_by=KEY, low=None, high=None, path=mq.MQ_TOPK_AUTO, cap=0):
    return mq.MqGroupOrder(order_by, int(desc), k, having_by, mq.MqRange64(low is not None, low or 0, high is not None, high or 0),
                           path, cap)


class TopOuts:
    def __init__(self, L, g, nkeys):
        self.L, self.g, self.nkeys = L, g, nkeys
        self.k = [Dev(4 * (g + PAD)) for _ in range(nkeys)]
        self.a = {a: Dev(np.dtype(DT[a]).itemsize * (g + PAD)) for a in DT}

    def reset(self):
        for d in self.k + list(self.a.values()):
            mq.check(self.L.mq_memset(d.ptr, SENT_BYTE, d.nbytes, None), "mq_memset")


def sent(dtype):
    return np.frombuffer(bytes([SENT_BYTE] * 8), dtype)[0]


def top(L, h, outs, o, full, tag, skip=()):
    """One mq_group_top checked against mq_group_by_write of everything followed by the model."""
    keys, aggs = full
    g = outs.g
    as64 = lambda a: None if a == KEY else aggs[a].astype(np.int64)
    idx = tc.topk64(as64(o.order_by), as64(o.having_by), (o.having.low if o.having.has_low else None,
                                                           o.having.high if o.having.has_high else None),
                    o.k, bool(o.descending), n=g)
    outs.reset()
    m, info = C.c_uint64(12345), mq.MqTopk64Info()
    kp = None if "keys" in skip else c_ptrs([d.ptr if j not in skip else None for j, d in enumerate(outs.k)])
    ap = [None if a in skip else outs.a[a].ptr for a in (COUNT, SUM, MIN, MAX)]
    rc = L.mq_group_top(h, C.byref(o), C.byref(m), kp, *ap, C.byref(info), None)
    assert rc == mq.MQ_OK, tag + (L.mq_last_error(),)
    assert m.value == len(idx) == info.m, tag + (m.value, len(idx))
    cap = min(o.k, g)
    for j, d in enumerate(outs.k):
        got = d.get(np.int32, g + PAD)
        if "keys" in skip or j in skip:
            assert np.all(got == sent(np.int32)), tag + ("key", j, "was not asked for")
        else:
            assert np.array_equal(got[:len(idx)], keys[j][idx]) and np.all(got[len(idx):] == sent(np.int32)), tag + ("key", j)
    for a in DT:
        got = outs.a[a].get(DT[a], g + PAD)
        if a in skip:
            assert np.all(got == sent(DT[a])), tag + (a, "was not asked for")
        else:
            assert np.array_equal(got[:len(idx)], aggs[a][idx]) and np.all(got[len(idx):] == sent(DT[a])), tag + ("agg", a)
    assert len(idx) <= cap
    return info


@pytest.mark.parametrize("sort", [False, True], ids=["dense", "sort"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_top_on_every_plan(lib, plan, sort):
    """Every order_by in both directions, each with a HAVING on a different aggregate, k in
    {1, 10, groups, no limit}; then the handle still writes all its groups, the same bytes."""
    h, g, nkeys, taken, keep = PLANS[plan](lib, N, sort)
    try:
        assert taken == (SORT if sort else DENSE) and g > 20, (plan, taken, g)
        full = write_all(lib, h, g, nkeys)
        keys, aggs = full
        outs = TopOuts(lib, g, nkeys)
        med = {a: int(np.sort(aggs[a].astype(np.int64))[g // 2]) for a in DT}
        i = 0
        for order_by in (KEY, COUNT, SUM, MIN, MAX):
            for desc in (False, True):
                for k in (1, 10, g, tc.K_ALL):
                    i += 1
                    having_by = (COUNT, SUM, MIN, MAX)[(order_by + i) % 4]
                    if having_by == order_by:
                        having_by = (COUNT, SUM, MIN, MAX)[(order_by + i + 1) % 4]
                    low, high = ((med[having_by], None), (None, med[having_by]), (None, None))[i % 3]
                    if low is None and high is None:
                        having_by = KEY
                    path, cap = ((mq.MQ_TOPK_AUTO, 0), (mq.MQ_TOPK_SELECT, 4), (mq.MQ_TOPK_SORT, 0))[i % 3 if i % 2 else 0]
                    o = order_of(order_by, desc, k, having_by, low, high, path, cap)
                    top(lib, h, outs, o, full, (plan, sort, order_by, desc, k, having_by, low, high, path))
        # a filter on the ordering aggregate itself, and one that nothing passes
        top(lib, h, outs, order_of(SUM, True, 10, SUM, med[SUM], None), full, (plan, "having sum"))
        info = top(lib, h, outs, order_of(COUNT, True, 10, COUNT, N + 1, None), full, (plan, "nothing passes"))
        assert (info.m, info.passed) == (0, 0)
        # only some outputs
        top(lib, h, outs, order_of(MAX, False, 7), full, (plan, "no keys"), skip=("keys", SUM))
        top(lib, h, outs, order_of(MIN, True, 7), full, (plan, "one key"), skip=tuple(range(1, nkeys)) + (COUNT, MIN, MAX))
        # the handle is as it was
        again = write_all(lib, h, g, nkeys)
        assert all(np.array_equal(a, b) for a, b in zip(keys, again[0])) and all(np.array_equal(aggs[a], again[1][a]) for a in DT)
        top(lib, h, outs, order_of(COUNT, False, 10), full, (plan, "after the write"))
    finally:
        mq.check(lib.mq_group_free(h), "mq_group_free")
        free_maps(lib, keep)


def test_ties_come_in_key_order(lib):
    """Counts repeat a lot: equal counts must come in ascending key order, in both directions."""
    h, g, nkeys, _, keep = plan_group(lib, N, False)
    try:
        full = write_all(lib, h, g, nkeys)
        assert len(np.unique(full[1][COUNT])) < g
        outs = TopOuts(lib, g, nkeys)
        for desc in (False, True):
            for path, cap in ((mq.MQ_TOPK_SELECT, 1), (mq.MQ_TOPK_SORT, 0)):
                info = top(lib, h, outs, order_of(COUNT, desc, g // 2, path=path, cap=cap), full, ("ties", desc, path))
                assert info.path == path
    finally:
        mq.check(lib.mq_group_free(h), "mq_group_free")


def test_no_groups_and_errors(lib):
    e = Dev(16)
    h, g, p, _ = _out()
    mq.check(lib.mq_group_plan(e.ptr, e.ptr, 0, None, AUTO, C.byref(h), C.byref(g), C.byref(p), None), "mq_group_plan")
    m, info = C.c_uint64(7), mq.MqTopk64Info()
    o = order_of(SUM, True, 10)
    assert lib.mq_group_top(h, C.byref(o), C.byref(m), None, None, None, None, None, C.byref(info), None) == mq.MQ_OK
    assert (g.value, m.value, info.m) == (0, 0, 0)
    mq.check(lib.mq_group_free(h), "mq_group_free")

    h, g, nkeys, _, keep = plan_group(lib, 4097, False)
    try:
        outs = TopOuts(lib, g, nkeys)
        outs.reset()
        ap = [outs.a[a].ptr for a in (COUNT, SUM, MIN, MAX)]
        kp = c_ptrs([outs.k[0].ptr])
        bad = [order_of(5, False, 10), order_of(-1, False, 10), order_of(SUM, False, 10, having_by=5), order_of(SUM, False, 10, -1),
               order_of(SUM, False, 10, path=3), order_of(SUM, False, 10, path=-1)]
        for o in bad:
            m = C.c_uint64(7)
            assert lib.mq_group_top(h, C.byref(o), C.byref(m), kp, *ap, C.byref(info), None) == mq.MQ_EINVAL
            assert m.value == 0 and b"mq_group_top" in lib.mq_last_error()
        o = order_of(SUM, False, 10)
        assert lib.mq_group_top(None, C.byref(o), C.byref(m), kp, *ap, None, None) == mq.MQ_EINVAL
        assert lib.mq_group_top(h, None, C.byref(m), kp, *ap, None, None) == mq.MQ_EINVAL
        assert lib.mq_group_top(h, C.byref(o), None, kp, *ap, None, None) == mq.MQ_EINVAL
        for d in outs.k + list(outs.a.values()):
            assert np.all(d.get(np.uint8, d.nbytes) == SENT_BYTE), "an error wrote something"
        # k == 0: nothing written, OK; h_info may be NULL
        o = order_of(SUM, True, 0)
        assert lib.mq_group_top(h, C.byref(o), C.byref(m), kp, *ap, None, None) == mq.MQ_OK and m.value == 0
        for d in outs.k + list(outs.a.values()):
            assert np.all(d.get(np.uint8, d.nbytes) == SENT_BYTE)
    finally:
        mq.check(lib.mq_group_free(h), "mq_group_free")


# ---------------------------------------------------------------------------
# the drop-in
# ---------------------------------------------------------------------------

def _lp(v):
    return None if v is None else C.pointer(C.c_long(int(v)))


def group_top_k(L, rpp, nres, order_by, desc, k, having_by=-1, low=None, high=None):
    """group_top_k -> (status, [(data_type, numpy array)] * nres or None)"""
    st = mq.Status(0, None)
    out = L.group_top_k(rpp, nres, order_by, desc, k, having_by, _lp(low), _lp(high), C.byref(st))
    if not out:
        return st.code, None
    res = [(out[i].contents.data_type, take(out[i])) for i in range(nres)]
    _libc.free(C.cast(out, C.c_void_p))
    return st.code, res


def peek(rpp, nres):
    """The Results as numpy copies, nothing freed."""
    return [(rpp[i].contents.data_type, take(rpp[i], free=False)) for i in range(nres)]


def check_dropin(L, rpp, nres, order_by, desc, k, having_by, low, high, tag):
    before = peek(rpp, nres)
    cols = [a for _, a in before]
    idx = tc.topk64(None if order_by < 0 else cols[order_by].astype(np.int64), None if having_by < 0 else cols[having_by].astype(np.int64),
                    (low, high), k, desc, n=len(cols[0]))
    code, out = group_top_k(L, rpp, nres, order_by, desc, k, having_by, low, high)
    assert code == mq.OK and out is not None, tag
    assert [t for t, _ in out] == [t for t, _ in before], tag
    for i, ((_, got), c) in enumerate(zip(out, cols)):
        assert got.dtype == c.dtype and np.array_equal(got, c[idx]), tag + (i,)
    after = peek(rpp, nres)
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(before, after)), tag + ("the inputs changed",)
    return len(idx)


def free_results(rpp, nres):
    for i in range(nres):
        take(rpp[i])
    _libc.free(C.cast(rpp, C.c_void_p))


def test_dropin_over_group_aggregate(lib, capfd):
    n = N
    keys = gc.keys_of("range_S_plus_1", n, 2048)
    v = gc.values_of("uniform", keys)
    ck, cv = make_column(keys), make_column(v)
    gk, gv, st = gcol(ck), gcol(cv), mq.Status(0, None)
    rpp = lib.group_aggregate(C.byref(gk), C.byref(gv), C.byref(st))
    assert st.code == mq.OK and rpp
    wk, wc_, ws, wmn, wmx = gc.group(keys, v)
    g = len(wk)
    x = int(np.sort(wmn)[g // 3])
    assert check_dropin(lib, rpp, 5, 2, True, 20, -1, None, None, ("top 20 by sum",)) == 20
    m = check_dropin(lib, rpp, 5, 1, True, 20, 3, x, None, ("by count having min >= x",))
    assert m == 20
    check_dropin(lib, rpp, 5, 1, False, g + 5, 4, None, int(np.sort(wmx)[g // 2]), ("by count asc having max < y",))
    assert check_dropin(lib, rpp, 5, -1, True, 2**64 - 1, 3, x, None, ("key order, having",)) == int((wmn >= x).sum())
    assert check_dropin(lib, rpp, 5, -1, False, 7, -1, None, None, ("key order, limit",)) == 7
    assert check_dropin(lib, rpp, 5, 0, True, 5, -1, None, None, ("by the key",)) == 5
    assert check_dropin(lib, rpp, 5, 2, True, 0, -1, None, None, ("k = 0",)) == 0
    assert check_dropin(lib, rpp, 5, 2, True, 9, 1, n + 1, None, ("nothing passes",)) == 0
    # every error case, each with its line on stderr
    capfd.readouterr()
    def refused(*args):
        code, out = group_top_k(lib, *args)
        return (code, out) == (mq.ERROR, None) and "libmq: group_top_k" in capfd.readouterr().err
    assert refused(rpp, 0, 0, True, 5)                      # nresults < 1
    assert refused(None, 5, 0, True, 5)
    assert refused(rpp, 5, 5, True, 5)                      # an index out of range
    assert refused(rpp, 5, -2, True, 5)
    assert refused(rpp, 5, 2, True, 5, 5, 0, None)
    assert refused(rpp, 5, 2, True, 5, -2, 0, None)
    fl = make_result(np.zeros(g, np.float32), mq.FLOAT)   # neither INT nor LONG
    short = make_result(np.zeros(g - 1, np.int32))          # unequal lengths
    for badr in (fl, short):
        arr = (C.POINTER(mq.Result) * 5)(*[rpp[i] for i in range(4)], C.pointer(badr))
        assert refused(arr, 5, 2, True, 5)
    arr = (C.POINTER(mq.Result) * 5)(*[rpp[i] for i in range(4)], None)
    assert refused(arr, 5, 2, True, 5)
    assert check_dropin(lib, rpp, 5, 2, False, 3, -1, None, None, ("after the errors",)) == 3
    for r in (fl, short):
        free_result_struct(r)
    free_results(rpp, 5)
    # empty inputs
    e = np.empty(0, np.int32)
    ce = make_column(e)
    ge = gcol(ce)
    rpp = lib.group_aggregate(C.byref(ge), C.byref(ge), C.byref(st))
    assert st.code == mq.OK and rpp
    assert check_dropin(lib, rpp, 5, 2, True, 20, 1, 1, None, ("no groups",)) == 0
    free_results(rpp, 5)
    for c in (ck, cv, ce):
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_over_group_aggregate_measures(lib):
    """Order by a measure's int64 sum, filter by another measure's max (both LONG Results)."""
    n = N
    terms = sc.make("km_plain_km", (4, 8, 8), n, seed=16)
    cols, ranges = sc.case("uniform_50", n, 2)
    price, qty, disc, _ = mc.columns(n, seed=16, big=True)
    cc = [make_column(c) for c in cols]
    cf = [make_column(t.col) for t in terms]
    ck = [make_column(t.dim_keys) if t.kind != "plain" else None for t in terms]
    ca = [make_column(t.dim_attrs) if t.kind == "km" else None for t in terms]
    cp, cq, cd = make_column(price), make_column(qty), make_column(disc)
    ops = [mc.OPS[o] for o in ("mul", "col", "sub")]
    keep = where_args(cc, ranges)
    (fa, k1), (ka, k2), (aa, k3) = gptrs(cf), gptrs(ck), gptrs(ca)
    (ma, k4), (mb, k5) = gptrs([cp, cq, cp]), gptrs([cd, None, cq])
    st = mq.Status(0, None)
    rpp = lib.group_aggregate_measures(keep[1], keep[2], keep[3], 2, fa, ka, aa, 3, ma, mb, (C.c_int * 3)(*ops), 3, C.byref(st))
    assert st.code == mq.OK and rpp
    nres = 3 + 1 + 9
    res = peek(rpp, nres)
    assert [t for t, _ in res] == [mq.INT] * 3 + [mq.LONG] * 10 and len(res[0][1]) > 50
    sum0, max1 = 4, 4 + 3 + 2  # measure 0's sums; measure 1's maxima
    y = int(np.sort(res[max1][1])[len(res[max1][1]) // 2])
    assert abs(res[sum0][1]).max() > 2**31  # past int32: what top_k could not order
    assert check_dropin(lib, rpp, nres, sum0, True, 10, max1, None, y, ("by sum having max < y",)) == 10
    check_dropin(lib, rpp, nres, sum0, False, 2**64 - 1, max1, y, None, ("by sum asc having max >= y",))
    check_dropin(lib, rpp, nres, 3, True, 10, -1, None, None, ("by count",))
    check_dropin(lib, rpp, nres, -1, False, 10, sum0, 0, None, ("key order having sum >= 0",))
    free_results(rpp, nres)
    for c in cc + cf + [c for c in ck + ca if c is not None] + [cp, cq, cd]:
        lib.mq_column_invalidate(C.byref(c))
