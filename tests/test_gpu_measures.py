"""group_aggregate_measures on gfx950 (k_group_measures_dense, k_measures_eval_pos,
k_measures_seg_write and mq_group_measures_plan / _write in csrc/mq_measures.hip;
group_aggregate_measures in mq_query.c), every comparison exact equality: with the numpy
restatement in measurecases.py, and through libmq itself with mq_group_star_plan and mq_sub.

Rows: a wave tile, the 1024-row tile and the unrolled iteration of every (terms, measures) pair
(1 to 4 tiles) each +-1, 70 001 rows for several blocks, 300 001 rows on one or two CUs for many
iterations a block.
"""
import ctypes as C

import numpy as np
import pytest

import measurecases as mc
import starcases as sc
import wherecases as wc
from devbuf import Dev
from refapi import make_column, mq
from test_gpu_group_by_where import results
from test_gpu_group_where import c_ptrs, c_ranges, lib, where_args  # noqa: F401
from test_gpu_star import Star, gptrs, read_raw, splan

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
TILE, PAD = 1024, 8
I32_MIN, I32_MAX = mc.I32_MIN, mc.I32_MAX
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SIZES = sorted({0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70_001} | {u * TILE + d for u in (1, 2, 3, 4) for d in (-1, 0, 1)})
# one layout per number of terms, each with a key space of at most 256: dense for every nmeas
SHAPES = {1: ("km", (200,)), 2: ("plain_km", (16, 16)), 3: ("km_plain_km", (4, 8, 8)), 4: ("ks_km_plain_km", (4, 8, 8))}


def cap(nmeas):
    return mc.SLOTS[nmeas]


class Query:
    """The device side of a query: every distinct array uploaded once (by identity, so that
    aliasing survives; the k-th one offs[k % len(offs)] dwords off a 16-byte boundary), the
    terms' maps and sets, the measures as an MqMeasure array."""

    def __init__(self, L, cols, terms, measures, offs=(0,)):
        self.devs = {}
        for a in list(cols) + [t.col for t in terms] + [x for q in measures for x in (q.a, q.b) if x is not None]:
            if id(a) not in self.devs:
                self.devs[id(a)] = Dev.of(a, offset_elems=offs[len(self.devs) % len(offs)])
        self.star = Star(L, terms, offs, self.devs)
        self.cols = [self.devs[id(c)].ptr for c in cols]
        self.meas = (mq.MqMeasure * max(len(measures), 1))()
        for i, q in enumerate(measures):
            self.meas[i] = mq.MqMeasure(self.devs[id(q.a)].ptr, self.devs[id(q.b)].ptr if q.b is not None else None, mc.OPS[q.op], 0)
        self.nmeas, self.nkeys, self.n = len(measures), self.star.nkeys, len(terms[0].col)

    def free(self):
        self.star.free()


def mplan(L, q, ranges, path, bounds=None, stream=None, **over):
    """(rc, handle, groups, path taken, joined rows)"""
    h, groups, taken, rows = C.c_void_p(77), C.c_uint64(12345), C.c_int(-1), C.c_uint64(54321)
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    a = dict(cols=c_ptrs(q.cols) if q.cols else None, ranges=c_ranges(ranges) if ranges else None, ncols=len(q.cols), terms=q.star.arr,
             nterms=len(q.star.terms), meas=q.meas, nmeas=q.nmeas, n=q.n)
    a.update(over)
    rc = L.mq_group_measures_plan(a["cols"], a["ranges"], a["ncols"], a["terms"], a["nterms"], a["meas"], a["nmeas"], a["n"], b, path,
                                  C.byref(h), C.byref(groups), C.byref(taken), C.byref(rows), stream)
    return rc, h.value, groups.value, taken.value, rows.value


def refused(L, *args, **kw):
    rc, h, g, _, rows = mplan(L, *args, **kw)
    return (rc, h, g, rows) == (mq.MQ_EINVAL, None, 0, 0) and b"mq_group_measures_plan" in L.mq_last_error()


class Outs:
    """Sentinel-filled outputs of g + PAD entries; `skip` names the ones passed as NULL:
    "keys", "count", "sum", "min", "max" (the whole array), ("key", j), ("sum", m), .."""

    def __init__(self, g, nkeys, nmeas, skip=()):
        self.g, self.skip = g, set(skip)
        mk = lambda dt, s: Dev.of(np.full(g + PAD, s, dt))  # noqa: E731
        self.keys = [None if ("key", j) in self.skip else mk(np.uint32, SENT32) for j in range(nkeys)]
        self.count = None if "count" in self.skip else mk(np.uint64, SENT64)
        self.agg = {nm: [None if (nm, m) in self.skip else mk(np.uint64, SENT64) for m in range(nmeas)] for nm in ("sum", "min", "max")}

    def write(self, L, h, stream=None):
        arr = lambda ds: (C.c_void_p * len(ds))(*[d.ptr if d else None for d in ds])  # noqa: E731
        return L.mq_group_measures_write(h, None if "keys" in self.skip else arr(self.keys), self.count.ptr if self.count else None,
                                         *[None if nm in self.skip else arr(self.agg[nm]) for nm in ("sum", "min", "max")], stream)

    def check(self, want, tag, written=True):
        g = self.g
        keys, count, aggs = want

        def one(dev, dt, w, is_null, what):
            if dev is None:
                return
            got = dev.get(dt, g + PAD)
            bits, sent = got.view(f"u{got.itemsize}"), SENT32 if got.itemsize == 4 else SENT64
            if is_null or not written:
                assert np.all(bits == sent), tag + (what, "written though not asked for")
            else:
                assert np.array_equal(got[:g], w), tag + (what, got[:4], w[:4])
                assert np.all(bits[g:] == sent), tag + (what, "wrote past the groups")

        for j, k in enumerate(self.keys):
            one(k, np.int32, keys[j], "keys" in self.skip, ("key", j))
        one(self.count, np.uint64, count, False, "count")
        for i, nm in enumerate(("sum", "min", "max")):
            for m, d in enumerate(self.agg[nm]):
                one(d, np.int64, aggs[m][i], nm in self.skip, (nm, m))

    def raw(self):
        g = self.g
        return ([k.get(np.int32, g).tobytes() for k in self.keys] + [self.count.get(np.uint64, g).tobytes()] +
                [d.get(np.int64, g).tobytes() for nm in ("sum", "min", "max") for d in self.agg[nm]])


def run(L, q, ranges, path, want, tag, bounds=None):
    rc, h, g, taken, rows = mplan(L, q, ranges, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[1]), tag + ("groups", g, len(want[1]))
    assert rows == int(want[1].sum()), tag + ("rows", rows)
    o = Outs(g, q.nkeys, q.nmeas)
    mq.check(o.write(L, h), "mq_group_measures_write")
    o.check(want, tag)
    raw = o.raw()
    mq.check(L.mq_group_measures_free(h), "mq_group_measures_free")
    return taken, raw


def run_paths(L, cols, ranges, terms, measures, tag, offs=(0,), bounds=None, dense_ok=True, want=None):
    """DENSE (where the key space allows), SORT and AUTO against the model; DENSE and SORT give
    the same bytes; AUTO takes the dense path exactly when it is allowed."""
    want = mc.model(cols, ranges, terms, measures) if want is None else want
    q = Query(L, cols, terms, measures, offs)
    try:
        raws = {}
        settled = q.n == 0 or any(t.kind != "plain" and len(t.dim_keys) == 0 for t in terms)
        for path in (DENSE, SORT, AUTO) if dense_ok else (SORT, AUTO):
            taken, raws[path] = run(L, q, ranges, path, want, tag + (path,), bounds)
            if not settled:
                assert taken == (path if path != AUTO else DENSE if dense_ok else SORT), tag + (path, taken)
        if dense_ok:
            assert raws[DENSE] == raws[SORT], tag + ("dense and sort differ",)
        elif q.n:
            assert refused(L, q, ranges, DENSE, bounds), tag + ("DENSE forced past the capacity",)
    finally:
        q.free()
    return want


# ---------------------------------------------------------------------------
# 1-4: sizes, few CUs, alignment, runs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("nmeas", [1, 2, 4])
@pytest.mark.parametrize("nterms", [1, 2, 3, 4])
def test_sizes(lib, nterms, nmeas):
    layout, cards = SHAPES[nterms]
    assert int(np.prod(cards)) <= cap(nmeas)
    for i, n in enumerate(SIZES):
        terms = sc.make(layout, cards, n, seed=2)
        cols, ranges = sc.case("uniform_50", n, (0, 2)[i % 2])
        ops = mc.columns(n, seed=i, big=bool(i % 3 == 0))
        offs = [(0,), (1,), (2, 0), (3, 1, 0)][i % 4]
        bounds = sc.bounds_of(cards) if n < 2 or i % 2 else None
        run_paths(lib, cols, ranges, terms, mc.q1_measures(ops, nmeas), (layout, nmeas, n), offs, bounds=bounds)


@pytest.mark.parametrize("limit", [1, 2])
def test_few_cus(lib, limit):
    """300 001 rows on the blocks of one or two CUs: many iterations a block."""
    n = 300_001
    layout, cards = SHAPES[3]
    terms = sc.make(layout, cards, n, seed=4)
    cols, ranges = sc.case("uniform_50", n, 1)
    meas = mc.q1_measures(mc.columns(n, seed=limit, big=True), 4)
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        run_paths(lib, cols, ranges, terms, meas, ("cu limit", limit))
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_alignment(lib, off):
    """Every column `off` dwords off a 16-byte boundary, then only every other one."""
    n = 5 * TILE + 37
    layout, cards = SHAPES[2]
    terms = sc.make(layout, cards, n, seed=6)
    cols, ranges = sc.case("uniform_50", n, 2)
    meas = mc.q1_measures(mc.columns(n, seed=off, big=True), 4)
    run_paths(lib, cols, ranges, terms, meas, ("all off", off), (off,))
    run_paths(lib, cols, ranges, terms, meas, ("some off", off), (0, off))


@pytest.mark.parametrize("nmeas", [1, 4])
def test_wave_uniform_runs(lib, nmeas):
    """Keys constant over 3 000 rows, then changing; large values: the run fold, its flush and
    its u64 sums; with and without a predicate that thins the tiles."""
    n = 40_000
    k0 = (np.arange(n) // 3000 % 5).astype(np.int32)
    k1 = (np.arange(n) // 9000 % 3 + 10).astype(np.int32)
    terms = [sc.Term("plain", k0), sc.Term("plain", k1)]
    rng = np.random.default_rng(3)
    big = [np.ascontiguousarray(rng.integers(I32_MAX - 1000, I32_MAX + 1, n), dtype=np.int32),
           np.ascontiguousarray(rng.integers(I32_MIN, I32_MIN + 1000, n), dtype=np.int32)]
    meas = [mc.Measure("mul", big[0], big[0]), mc.Measure("mul", big[0], big[1]), mc.Measure("sub", big[1], big[0]),
            mc.Measure("col", big[1])][:nmeas]
    want = run_paths(lib, [], [], terms, meas, ("runs",), bounds=[0, 4, 10, 12])
    assert np.any(want[2][0][0] < 0) or nmeas == 1  # a sum that wrapped
    cols, ranges = sc.case("uniform_50", n, 1)
    run_paths(lib, cols, ranges, terms, meas, ("thinned runs",), (1, 0), bounds=[0, 4, 10, 12])


# ---------------------------------------------------------------------------
# 5-8: extremes, dropped rows, rows out of bounds, aliasing
# ---------------------------------------------------------------------------

def test_extremes(lib):
    lo, hi = np.full(4, I32_MIN, np.int32), np.full(4, I32_MAX, np.int32)
    four, two = [sc.Term("plain", np.zeros(4, np.int32))], [sc.Term("plain", np.zeros(2, np.int32))]
    w = run_paths(lib, [], [], four, [mc.Measure("mul", lo, lo)], ("min x min, four rows",))
    assert w[2][0][0].tolist() == [0] and w[2][0][1].tolist() == [1 << 62]
    lo2, hi2 = lo[:2].copy(), hi[:2].copy()
    w = run_paths(lib, [], [], two, [mc.Measure("mul", lo2, lo2)], ("min x min, two rows",))
    assert w[2][0][0].tolist() == [mc.I64_MIN]
    w = run_paths(lib, [], [], two, [mc.Measure("mul", lo2, hi2), mc.Measure("sub", lo2, hi2), mc.Measure("add", hi2, hi2)], ("ends",))
    assert [a[1].tolist() for a in w[2]] == [[I32_MIN * I32_MAX], [-4294967295], [4294967294]]
    assert [a[2].tolist() for a in w[2]] == [[I32_MIN * I32_MAX], [-4294967295], [4294967294]]
    # the same values among 5 000 rows of several groups, every tile form
    n = 5000
    k = (np.arange(n) % 7).astype(np.int32)
    a = np.where(np.arange(n) % 2 == 0, I32_MIN, I32_MAX).astype(np.int32)
    b = np.where(np.arange(n) % 3 == 0, I32_MIN, I32_MAX).astype(np.int32)
    run_paths(lib, [], [], [sc.Term("plain", k)],
              [mc.Measure("mul", a, b), mc.Measure("sub", a, b), mc.Measure("add", a, b), mc.Measure("mul", a, a)], ("ends, many rows",))


@pytest.mark.parametrize("nmeas", [2, 4])
def test_dropped_rows_never_count(lib, nmeas):
    """Rows that fail a predicate, miss the map or miss the set carry INT32_MIN / INT32_MAX in
    every measure column and a plain key outside the bounds: same result, no error."""
    n = 6 * TILE + 11
    layout, cards = SHAPES[4]  # ks, km, plain, km
    terms = sc.make(layout, cards, n, seed=8)
    cols, ranges = sc.case("uniform_50", n, 2)
    ops = mc.columns(n, seed=8)
    m = sc.joined(cols, ranges, terms)
    assert m.any() and (~m).any()
    want = mc.model(cols, ranges, terms, mc.q1_measures(ops, nmeas))
    poison = np.where(np.arange(n) % 2 == 0, I32_MIN, I32_MAX).astype(np.int32)
    dirty = [np.where(m, c, poison).astype(np.int32) for c in ops]
    plain = np.where(m, terms[2].col, np.where(np.arange(n) % 2 == 0, I32_MIN, 10_000)).astype(np.int32)
    dterms = [terms[0], terms[1], sc.Term("plain", plain), terms[3]]
    got = run_paths(lib, cols, ranges, dterms, mc.q1_measures(dirty, nmeas), ("poisoned",), (0, 1), bounds=sc.bounds_of(cards), want=want)
    assert got is want


def test_joined_row_out_of_bounds(lib):
    n = 3 * TILE + 5
    layout, cards = SHAPES[2]  # plain, km
    terms = sc.make(layout, cards, n, seed=9)
    meas = mc.q1_measures(mc.columns(n, seed=9), 2)
    m = sc.joined([], [], terms)
    row = int(np.flatnonzero(m)[len(np.flatnonzero(m)) // 2])
    stray = terms[0].col.copy()
    stray[row] = sc.COMP_BASE[0] + cards[0]  # one past its bounds; the summed code stays inside the table
    q = Query(lib, [], [sc.Term("plain", stray), terms[1]], meas)
    good = Query(lib, [], terms, meas)
    try:
        for path in (DENSE, SORT, AUTO):
            assert refused(lib, q, [], path, sc.bounds_of(cards)), path
            run(lib, good, [], path, mc.model([], [], terms, meas), ("after a refusal", path), sc.bounds_of(cards))
    finally:
        q.free()
        good.free()


def test_aliasing(lib):
    n = 4 * TILE + 3
    layout, cards = SHAPES[2]  # plain, km
    terms = sc.make(layout, cards, n, seed=10)
    cols, ranges = sc.case("uniform_50", n, 1)
    x = mc.columns(n, seed=10, big=True)[0]
    meas = [mc.Measure("mul", x, x), mc.Measure("sub", terms[1].col, x), mc.Measure("add", cols[0], cols[0]), mc.Measure("col", terms[0].col)]
    run_paths(lib, cols, ranges, terms, meas, ("aliased",), (0, 1))


# ---------------------------------------------------------------------------
# 9: cross-checks through libmq itself
# ---------------------------------------------------------------------------

def read_m(L, q, ranges, meas_idx, path, bounds):
    """The raw outputs of a plan over the measures meas_idx of q."""
    arr = (mq.MqMeasure * len(meas_idx))(*[q.meas[i] for i in meas_idx])
    rc, h, g, _, _ = mplan(L, q, ranges, path, bounds, meas=arr, nmeas=len(meas_idx))
    assert rc == mq.MQ_OK, L.mq_last_error()
    o = Outs(g, q.nkeys, len(meas_idx))
    mq.check(o.write(L, h), "write")
    keys = [k.get(np.int32, g) for k in o.keys]
    out = (keys, o.count.get(np.uint64, g), [[o.agg[nm][m].get(np.int64, g) for nm in ("sum", "min", "max")] for m in range(len(meas_idx))])
    mq.check(L.mq_group_measures_free(h), "free")
    return out


@pytest.mark.parametrize("path", [DENSE, SORT])
def test_cross_checks(lib, path):
    n = 70_001
    layout, cards = SHAPES[3]
    terms = sc.make(layout, cards, n, seed=11)
    cols, ranges = sc.case("uniform_50", n, 2)
    price, qty, disc, tax = mc.columns(n, seed=11)
    meas = [mc.Measure("col", price), mc.Measure("sub", price, qty), mc.Measure("mul", price, disc), mc.Measure("add", tax, qty)]
    q = Query(lib, cols, terms, meas)
    diff = Dev(4 * n)
    try:
        b = sc.bounds_of(cards)
        every = read_m(lib, q, ranges, [0, 1, 2, 3], path, b)
        # the star plan on the same column: the same bytes, min / max after widening
        rc, h, g, _, _ = splan(lib, q.cols, ranges, q.star, q.devs[id(price)].ptr, n, path, b)
        assert rc == mq.MQ_OK and g == len(every[1])
        raw = read_raw(lib, h, g, q.nkeys)
        mq.check(lib.mq_group_free(h), "mq_group_free")
        one = read_m(lib, q, ranges, [0], path, b)
        assert [k.tobytes() for k in one[0]] == raw[:q.nkeys] and one[1].tobytes() == raw[q.nkeys]
        assert one[2][0][0].tobytes() == raw[q.nkeys + 1]
        assert np.array_equal(one[2][0][1], np.frombuffer(raw[q.nkeys + 2], np.int32).astype(np.int64))
        assert np.array_equal(one[2][0][2], np.frombuffer(raw[q.nkeys + 3], np.int32).astype(np.int64))
        # a 4-measure plan equals its four one-measure plans
        for m in range(4):
            single = read_m(lib, q, ranges, [m], path, b)
            assert all(np.array_equal(x, y) for x, y in zip(single[0], every[0])) and np.array_equal(single[1], every[1])
            assert all(np.array_equal(x, y) for x, y in zip(single[2][0], every[2][m])), m
        # SUB on inputs that do not wrap equals mq_sub -> mq_group_star_plan
        mq.check(lib.mq_sub(q.devs[id(price)].ptr, q.devs[id(qty)].ptr, n, diff.ptr, None), "mq_sub")
        rc, h, g, _, _ = splan(lib, q.cols, ranges, q.star, diff.ptr, n, path, b)
        assert rc == mq.MQ_OK
        raw = read_raw(lib, h, g, q.nkeys)
        mq.check(lib.mq_group_free(h), "mq_group_free")
        assert every[2][1][0].tobytes() == raw[q.nkeys + 1] and every[1].tobytes() == raw[q.nkeys]
        assert np.array_equal(every[2][1][1], np.frombuffer(raw[q.nkeys + 2], np.int32).astype(np.int64))
        assert np.array_equal(every[2][1][2], np.frombuffer(raw[q.nkeys + 3], np.int32).astype(np.int64))
    finally:
        q.free()
        diff.free()


# ---------------------------------------------------------------------------
# 10-12: the capacity edge, the write, the refusals
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("nmeas", [1, 2, 3, 4])
def test_capacity_edge(lib, nmeas):
    n = 9001
    c = cap(nmeas)
    assert lib.mq_group_measures_dense_slots(nmeas) == c
    ops = mc.columns(n, seed=nmeas, big=True)
    meas = (mc.q1_measures(ops, 4) * 2)[1:1 + nmeas]
    for space, dense_ok in ((c, True), (c + 1, False)):
        k = np.ascontiguousarray((np.arange(n) * 7919) % space - 40, dtype=np.int32)  # every value of the space occurs
        assert len(np.unique(k)) == space
        for bounds in (None, [-40, space - 41]):
            run_paths(lib, [], [], [sc.Term("plain", k)], meas, ("edge", nmeas, space, bounds), bounds=bounds, dense_ok=dense_ok)
    # two components whose product is the capacity, then one more value
    k0, k1 = (np.arange(n) % 2).astype(np.int32), (np.arange(n) // 2 % (c // 2)).astype(np.int32)
    run_paths(lib, [], [], [sc.Term("plain", k0), sc.Term("plain", k1)], meas, ("edge, two keys", nmeas), bounds=[0, 1, 0, c // 2 - 1])
    run_paths(lib, [], [], [sc.Term("plain", k0), sc.Term("plain", k1)], meas, ("edge, two keys, past", nmeas), bounds=[0, 1, 0, c // 2],
              dense_ok=False)


@pytest.mark.parametrize("path", [DENSE, SORT])
def test_write(lib, path):
    n = 20_011
    layout, cards = SHAPES[3]
    terms = sc.make(layout, cards, n, seed=12)
    meas = mc.q1_measures(mc.columns(n, seed=12, big=True), 4)
    want = mc.model([], [], terms, meas)
    q = Query(lib, [], terms, meas)
    st2 = C.c_void_p()
    mq.check(lib.mq_stream_create(C.byref(st2)), "mq_stream_create")
    try:
        rc, h, g, taken, _ = mplan(lib, q, [], path, sc.bounds_of(cards))
        assert rc == mq.MQ_OK and taken == path and g == len(want[1])
        subsets = [(), ("keys",), ("count",), ("sum", "min", "max"), ("keys", "count", "sum", "min", "max"), ("min",), ("sum", "max"),
                   (("key", 0), ("key", 2), ("sum", 0), ("min", 1), ("max", 3), ("sum", 2), ("min", 2), ("max", 2)),
                   (("key", 1), "count", ("sum", 1), ("sum", 2), ("sum", 3), ("min", 0), ("max", 0))]
        for i, skip in enumerate(subsets):
            o = Outs(g, q.nkeys, q.nmeas, skip)
            stream = st2 if i % 2 else None
            mq.check(o.write(lib, h, stream), "mq_group_measures_write")
            mq.check(lib.mq_stream_sync(stream), "sync")
            o.check(want, ("subset", skip))
        mq.check(lib.mq_group_measures_free(h), "mq_group_measures_free")
        assert lib.mq_group_measures_free(None) == mq.MQ_OK
    finally:
        mq.check(lib.mq_device_sync(), "sync")
        mq.check(lib.mq_stream_destroy(st2), "mq_stream_destroy")
        q.free()


@pytest.mark.parametrize("name", ["no_rows", "empty_map", "unsatisfiable"])
def test_settled_on_the_host(lib, name):
    n = 0 if name == "no_rows" else 4097
    terms = sc.make("plain_km", (16, 16), n, seed=13)
    if name == "empty_map":
        terms[1] = sc.Term("km", terms[1].col, np.empty(0, np.int32), np.empty(0, np.int32))
    cols, ranges = sc.case("uniform_50", n, 1)
    if name == "unsatisfiable":
        ranges = [(5, 5)]
    meas = mc.q1_measures(mc.columns(n, seed=13), 2)
    q = Query(lib, cols, terms, meas)
    try:
        for path in (AUTO, DENSE, SORT):
            rc, h, g, taken, rows = mplan(lib, q, ranges, path)
            assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h
            o = Outs(0, q.nkeys, q.nmeas)
            mq.check(o.write(lib, h), "write")
            o.check(([np.empty(0, np.int32)] * q.nkeys, np.empty(0, np.uint64), [(np.empty(0, np.int64),) * 3] * 2), (name,))
            mq.check(lib.mq_group_measures_free(h), "free")
    finally:
        q.free()


def test_refusals(lib):
    n = 2049
    layout, cards = SHAPES[2]
    terms = sc.make(layout, cards, n, seed=14)
    cols, ranges = sc.case("uniform_50", n, 1)
    ops = mc.columns(n, seed=14)
    meas = mc.q1_measures(ops, 4)
    q = Query(lib, cols, terms, meas)
    b = sc.bounds_of(cards)

    def with_meas(i, **f):
        arr = (mq.MqMeasure * 4)(*[q.meas[j] for j in range(4)])
        for k, v in f.items():
            setattr(arr[i], k, v)
        return arr

    try:
        rc, h, _, _, _ = mplan(lib, q, ranges, AUTO, b)  # the base case is fine
        assert rc == mq.MQ_OK and lib.mq_group_measures_free(h) == mq.MQ_OK
        cases = {
            "nmeas 0": dict(nmeas=0), "nmeas 5": dict(nmeas=5), "NULL h_meas": dict(meas=None),
            "op -1": dict(meas=with_meas(1, op=-1)), "op 4": dict(meas=with_meas(0, op=4)),
            "NULL d_a": dict(meas=with_meas(2, d_a=None)), "misaligned d_a": dict(meas=with_meas(2, d_a=q.meas[2].d_a + 2)),
            "binary without d_b": dict(meas=with_meas(0, d_b=None)), "COL with d_b": dict(meas=with_meas(1, d_b=q.meas[0].d_a)),
            "reserved": dict(meas=with_meas(3, reserved=1)),
            "nterms 0": dict(nterms=0), "nterms 5": dict(nterms=5), "NULL terms": dict(terms=None), "ncols 9": dict(ncols=9),
            "ncols -1": dict(ncols=-1), "NULL cols": dict(cols=None), "n 2^31": dict(n=1 << 31),
        }
        for name, over in cases.items():
            assert refused(lib, q, ranges, AUTO, b, **over), name
        assert refused(lib, q, ranges, 3, b), "path"
        assert refused(lib, q, ranges, AUTO, [0, -1, 0, 1]), "empty bounds"
        assert refused(lib, q, ranges, AUTO, [I32_MIN, I32_MAX, 0, 1]), "P > 2^32"
        assert refused(lib, q, ranges, DENSE, [0, 15, 0, 16]), "DENSE past the capacity"
        both = (mq.MqStarTerm * 2)(q.star.arr[0], mq.MqStarTerm(q.star.arr[1].d_col, q.star.arr[1].km, q.star.arr[1].km))
        assert refused(lib, q, ranges, AUTO, b, terms=both), "km and ks"
        bad_col = (mq.MqStarTerm * 2)(mq.MqStarTerm(None, None, None), q.star.arr[1])
        assert refused(lib, q, ranges, AUTO, b, terms=bad_col), "NULL term column"
        assert lib.mq_group_measures_write(None, None, None, None, None, None, None) == mq.MQ_EINVAL
        run(lib, q, ranges, AUTO, mc.model(cols, ranges, terms, meas), ("after the refusals",), b)
    finally:
        mq.check(lib.mq_device_sync(), "sync")
        q.free()


# ---------------------------------------------------------------------------
# 13: the drop-in
# ---------------------------------------------------------------------------

def fused(L, objs, ranges, fkeys, dim_keys, dim_attrs, meas_a, meas_b, ops, nkeys):
    keep = where_args(objs, ranges) if objs else (None, None, None, None)
    (fa, k1), (ka, k2), (aa, k3) = gptrs(fkeys), gptrs(dim_keys), gptrs(dim_attrs)
    (ma, k4), (mb, k5) = gptrs(meas_a), gptrs(meas_b)
    st = mq.Status(0, None)
    rpp = L.group_aggregate_measures(keep[1], keep[2], keep[3], len(objs), fa, ka, aa, len(fkeys), ma, mb, (C.c_int * len(ops))(*ops),
                                     len(ops), C.byref(st))
    return (st.code, results(rpp, nkeys + 1 + 3 * len(ops))) if rpp else (st.code, None)


def test_dropin(lib, capfd):
    n = 70_001
    layout, cards = SHAPES[3]  # km, plain, km
    terms = sc.make(layout, cards, n, seed=16)
    cols, ranges = sc.case("uniform_50", n, 2)
    price, qty, disc, _ = mc.columns(n, seed=16, big=True)
    meas = [mc.Measure("mul", price, disc), mc.Measure("col", qty), mc.Measure("sub", price, qty)]
    cc = [make_column(c) for c in cols]
    cf = [make_column(t.col) for t in terms]
    ck = [make_column(t.dim_keys) if t.kind != "plain" else None for t in terms]
    ca = [make_column(t.dim_attrs) if t.kind == "km" else None for t in terms]
    cp, cq, cd = make_column(price), make_column(qty), make_column(disc)
    ops = [mc.OPS[m.op] for m in meas]

    def check(out, want, tag):
        assert len(out) == 3 + 1 + 9 and [t for t, _ in out] == [mq.INT] * 3 + [mq.LONG] * 10, tag
        flat = list(want[0]) + [want[1]] + [x for agg in want[2] for x in agg]
        for i, ((_, got), w) in enumerate(zip(out, flat)):
            assert len(got) == len(w) and np.array_equal(np.asarray(got).astype(np.int64), w.astype(np.int64)), tag + (i,)

    want = mc.model(cols, ranges, terms, meas)
    assert len(want[1]) > 50
    code, out = fused(lib, cc, ranges, cf, ck, ca, [cp, cq, cp], [cd, None, cq], ops, 3)
    assert code == mq.OK
    check(out, want, ("columns",))
    # an empty dimension: empty Results and OK
    e = np.empty(0, np.int32)
    code, out = fused(lib, cc, ranges, cf, [make_column(e), None, ck[2]], [make_column(e), None, ca[2]], [cp, cq, cp], [cd, None, cq], ops, 3)
    assert code == mq.OK
    check(out, mc.model(cols, ranges, [sc.Term("km", terms[0].col, e, e), terms[1], terms[2]], meas), ("empty dimension",))
    # a binary op without its second operand, and a plain column with one: ERROR and NULL
    assert fused(lib, cc, ranges, cf, ck, ca, [cp, cq, cp], [None, None, cq], ops, 3) == (mq.ERROR, None)
    assert fused(lib, cc, ranges, cf, ck, ca, [cp, cq, cp], [cd, cd, cq], ops, 3) == (mq.ERROR, None)
    capfd.readouterr()
