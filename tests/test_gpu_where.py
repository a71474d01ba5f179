"""select_where on gfx950 (csrc/mq_where.hip; select_where / aggregate_where in mq_query.c),
every comparison exact equality: with the numpy restatement in wherecases.py, with
mq_select_positions / mq_select_agg for one column, and with the chain select -> fetch ->
select_result run through libmq itself.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import wherecases as wc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

PAD = 8
SENT_BYTE = 0xA5
SENT = np.frombuffer(bytes([SENT_BYTE] * 4), np.int32)[0]
SENT64 = np.frombuffer(bytes([SENT_BYTE] * 8), np.uint64)[0]


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    # the drop-in's first operator pins glibc's mmap threshold (see test_gpu_topk.py)
    one = np.arange(4, dtype=np.int32)
    col, st = make_column(one), mq.Status(0, None)
    take(L.select_column_scan(C.byref(col), C.pointer(C.c_int(0)), C.pointer(C.c_int(2)), C.byref(st)))
    assert st.code == mq.OK
    L.mq_column_invalidate(C.byref(col))
    return L


def c_ranges(ranges):
    return (mq.MqRange * len(ranges))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in ranges])


def c_ptrs(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


class Bench:
    """The device buffers of one caller for columns of up to `cap` rows: workspace, positions
    (cap + PAD), count and aggregate, the outputs refilled with a sentinel before each call."""

    def __init__(self, lib, cap, stream=None):
        self.lib, self.cap, self.stream = lib, cap, stream
        self.ws_bytes = max(lib.mq_where_workspace_bytes(cap), lib.mq_scan_workspace_bytes(cap))
        self.ws = Dev(self.ws_bytes)
        self.out = Dev(4 * (cap + PAD))
        self.cnt = Dev(16)
        self.agg = Dev(48)

    def reset(self, n):
        L = self.lib
        mq.check(L.mq_memset(self.out.ptr, SENT_BYTE, 4 * (n + PAD), self.stream), "mq_memset")
        mq.check(L.mq_memset(self.cnt.ptr, SENT_BYTE, 16, self.stream), "mq_memset")
        mq.check(L.mq_memset(self.agg.ptr, SENT_BYTE, 48, self.stream), "mq_memset")

    def positions_async(self, ptrs, ranges, pay, n):
        return self.lib.mq_where_positions(c_ptrs(ptrs), c_ranges(ranges), len(ptrs), pay, n, self.out.ptr, self.cnt.ptr,
                                           self.ws.ptr, self.ws_bytes, self.stream)

    def agg_async(self, ptrs, ranges, val, n):
        return self.lib.mq_where_agg(c_ptrs(ptrs), c_ranges(ranges), len(ptrs), val, n, self.agg.ptr, self.ws.ptr,
                                     self.ws_bytes, self.stream)

    def read_positions(self, n):
        """(K, the cap + PAD entries) once the stream has drained."""
        mq.check(self.lib.mq_stream_sync(self.stream), "sync")
        c = self.cnt.get(np.uint64, 2)
        assert c[1] == SENT64, "wrote past the count"
        return int(c[0]), self.out.get(np.int32, n + PAD)

    def read_agg(self):
        mq.check(self.lib.mq_stream_sync(self.stream), "sync")
        raw = self.agg.get(np.uint8, 48)
        assert np.all(raw[32:] == SENT_BYTE), "wrote past the aggregate"
        a = mq.MqAgg.from_buffer_copy(raw[:32].tobytes())
        return int(a.count), int(a.sum), int(a.min), int(a.max)

    def positions(self, ptrs, ranges, pay, n, want, tag):
        self.reset(n)
        rc = self.positions_async(ptrs, ranges, pay, n)
        assert rc == mq.MQ_OK, tag + (self.lib.mq_last_error(),)
        self.check_positions(n, want, tag)

    def check_positions(self, n, want, tag):
        k, got = self.read_positions(n)
        assert k == len(want), tag + ("count", k, len(want))
        assert np.array_equal(got[:k], want), tag
        assert np.all(got[k:] == SENT), tag + ("wrote past K",)

    def aggregate(self, ptrs, ranges, val, n, want, tag):
        self.reset(0)
        rc = self.agg_async(ptrs, ranges, val, n)
        assert rc == mq.MQ_OK, tag + (self.lib.mq_last_error(),)
        assert self.read_agg() == want, tag


class Columns:
    """A case's distinct columns, the payload and the value column on the device, each 0 and
    1 dword off a 16-byte boundary."""

    def __init__(self, cols, pay, val):
        self.cols = cols
        self.devs = {}
        for c in cols:
            if id(c) not in self.devs:
                self.devs[id(c)] = [Dev.of(c, offset_elems=o) for o in (0, 1)]
        self.pay = [Dev.of(pay, offset_elems=o) for o in (0, 1)]
        self.val = [Dev.of(val, offset_elems=o) for o in (0, 1)]

    def ptrs(self, offs):
        """offs: per distinct column (in order of first use) 0 or 1; the same column twice is
        the same pointer twice."""
        order = list(self.devs)
        return [self.devs[id(c)][offs[order.index(id(c)) % len(offs)]].ptr for c in self.cols]


# offsets of (columns..., payload, value): all aligned (the dwordx4 path), mixed, all off
VARIANTS = [([0], 0, 0), ([0, 1, 1, 0, 1, 0, 0, 1], 1, 0), ([1, 0], 0, 1), ([1], 1, 1)]


def run_case(lib, bench, name, n, ncols, variants=VARIANTS):
    cols, ranges = wc.case(name, n, ncols)
    pay, val = wc.payload_of(n), wc.values_of(n)
    dev = Columns(cols, pay, val)
    want_pos, want_pay = wc.positions(cols, ranges), wc.positions(cols, ranges, pay)
    want_agg = wc.aggregate(cols, ranges, val)
    for offs, po, vo in variants:
        tag = (name, n, ncols, tuple(offs), po, vo)
        ptrs = dev.ptrs(offs)
        bench.positions(ptrs, ranges, None, n, want_pos, tag + ("positions",))
        bench.positions(ptrs, ranges, dev.pay[po].ptr, n, want_pay, tag + ("payload",))
        bench.aggregate(ptrs, ranges, dev.val[vo].ptr, n, want_agg, tag + ("aggregate",))
    # the value column may be one of the predicate columns
    bench.aggregate(ptrs, ranges, ptrs[-1], n, wc.aggregate(cols, ranges, cols[-1]), (name, n, ncols, "value = column"))


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(lib):
    return Bench(lib, max(wc.SIZES))


@pytest.fixture(scope="module")
def big(lib):
    return Bench(lib, wc.BIG)


@pytest.mark.parametrize("name", wc.CASES)
def test_forms_agree_with_the_restatement(lib, small, name):
    """Every size, column set and ncols: positions with and without a payload and the
    aggregate, columns, payload and values independently 0 and 1 dword off a 16-byte
    boundary, the same exact answers and nothing written past K."""
    for n in wc.SIZES:
        for ncols in wc.NCOLS:
            run_case(lib, small, name, n, ncols)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("name", wc.CASES)
def test_many_iterations_a_block(lib, big, name, limit):
    """BIG rows on a grid of 1 or 2 CUs' blocks: each block runs many wave iterations and its
    chunk edges fall inside lines of the misaligned columns."""
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        for ncols in wc.NCOLS:
            run_case(lib, big, name, wc.BIG, ncols, variants=VARIANTS[limit - 1:limit + 1])
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


@pytest.mark.parametrize("n", [0, 1, 257, 4097, 70_001])
def test_one_column_equals_the_select(lib, n):
    """ncols == 1 is mq_select_positions and mq_select_agg on the same inputs, bit for bit."""
    bench = Bench(lib, n)
    ref_out, ref_cnt, ref_agg = Dev(4 * (n + PAD)), Dev(16), Dev(48)
    sws = lib.mq_scan_workspace_bytes(n)
    ws = Dev(sws)
    v = np.random.default_rng(n).integers(-1000, 1000, n).astype(np.int32)
    pay = wc.payload_of(n)
    for off in (0, 1):
        dv, dp = Dev.of(v, offset_elems=off), Dev.of(pay, offset_elems=1 - off)
        for lo, hi in [(-100, 250), (None, 0), (990, None), (None, None), (5, 5), (wc.I32_MIN, wc.I32_MAX), (999, 1000)]:
            b = mq.bounds(lo, hi)
            for p in (None, dp.ptr):
                for d in (ref_out, ref_cnt):
                    mq.check(lib.mq_memset(d.ptr, SENT_BYTE, d.nbytes, None), "mq_memset")
                mq.check(lib.mq_select_positions(dv.ptr, p, n, *b, ref_out.ptr, ref_cnt.ptr, ws.ptr, sws, None), "select")
                k = int(ref_cnt.get(np.uint64, 1)[0])
                want = ref_out.get(np.int32, n + PAD)[:k]
                bench.positions([dv.ptr], [(lo, hi)], p, n, want, (n, off, lo, hi, p is not None))
            mq.check(lib.mq_select_agg(dv.ptr, n, *b, ref_agg.ptr, ws.ptr, sws, None), "select_agg")
            a = mq.MqAgg.from_buffer_copy(ref_agg.get(np.uint8, 32).tobytes())
            bench.aggregate([dv.ptr], [(lo, hi)], dv.ptr, n, (int(a.count), int(a.sum), int(a.min), int(a.max)),
                            (n, off, lo, hi, "agg"))


@pytest.mark.parametrize("name", ["uniform_10", "clustered_lead", "islands_alt", "unbounded_middle", "same_twice"])
def test_predicate_order_does_not_matter(lib, name):
    n = 8193
    bench = Bench(lib, n)
    cols, ranges = wc.case(name, n, 3)
    pay, val = wc.payload_of(n), wc.values_of(n)
    dev = Columns(cols, pay, val)
    ptrs = dev.ptrs([0, 1])
    want_pay, want_agg = wc.positions(cols, ranges, pay), wc.aggregate(cols, ranges, val)
    for perm in itertools.permutations(range(3)):
        pp, rr = [ptrs[i] for i in perm], [ranges[i] for i in perm]
        bench.positions(pp, rr, dev.pay[0].ptr, n, want_pay, (name, perm))
        bench.aggregate(pp, rr, dev.val[1].ptr, n, want_agg, (name, perm))
    # eight predicates, reversed and rotated
    cols, ranges = wc.case(name, n, 8)
    dev = Columns(cols, pay, val)
    ptrs = dev.ptrs([1, 0, 0])
    want_pos, want_agg = wc.positions(cols, ranges), wc.aggregate(cols, ranges, val)
    for perm in (list(range(8))[::-1], [3, 4, 5, 6, 7, 0, 1, 2], [1, 0, 3, 2, 5, 4, 7, 6]):
        pp, rr = [ptrs[i] for i in perm], [ranges[i] for i in perm]
        bench.positions(pp, rr, None, n, want_pos, (name, tuple(perm)))
        bench.aggregate(pp, rr, dev.val[0].ptr, n, want_agg, (name, tuple(perm)))


def test_sixteen_streams(lib):
    """Mixed positions / aggregate calls on sixteen streams at once, a workspace each."""
    n = 70_001
    streams = []
    for _ in range(16):
        s = C.c_void_p()
        mq.check(lib.mq_stream_create(C.byref(s)), "mq_stream_create")
        streams.append(s)
    try:
        jobs = []
        for i, s in enumerate(streams):
            name, ncols = wc.CASES[i % len(wc.CASES)], wc.NCOLS[(i // 4) % 4]
            cols, ranges = wc.case(name, n, ncols)
            pay, val = wc.payload_of(n), wc.values_of(n)
            jobs.append((Bench(lib, n, s), Columns(cols, pay, val), cols, ranges, pay, val, (name, ncols, i)))
        mq.check(lib.mq_device_sync(), "device sync")  # the uploads (null stream) are done
        for b, *_ in jobs:
            b.reset(n)
        for rep in range(2):
            for i, (b, dev, cols, ranges, pay, val, tag) in enumerate(jobs):
                ptrs = dev.ptrs([i & 1, (i >> 1) & 1])
                if (i + rep) & 1:
                    assert b.positions_async(ptrs, ranges, dev.pay[i & 1].ptr if i & 2 else None, n) == mq.MQ_OK, tag
                else:
                    assert b.agg_async(ptrs, ranges, dev.val[i & 1].ptr, n) == mq.MQ_OK, tag
        for i, (b, dev, cols, ranges, pay, val, tag) in enumerate(jobs):
            b.check_positions(n, wc.positions(cols, ranges, pay if i & 2 else None), tag)
            assert b.read_agg() == wc.aggregate(cols, ranges, val), tag
    finally:
        mq.check(lib.mq_device_sync(), "device sync")
        for s in streams:
            lib.mq_stream_destroy(s)


def test_errors_write_nothing(lib):
    n = 1025
    bench = Bench(lib, n)
    cols, ranges = wc.case("uniform_50", n, 2)
    dev = Columns(cols, wc.payload_of(n), wc.values_of(n))
    ptrs = dev.ptrs([0, 1])
    ok_p, ok_r = c_ptrs(ptrs), c_ranges(ranges)
    bench.reset(n)
    L, ws, wsb = lib, bench.ws.ptr, lib.mq_where_workspace_bytes(n)
    out, cnt, agg = bench.out.ptr, bench.cnt.ptr, bench.agg.ptr
    pay, val = dev.pay[0].ptr, dev.val[0].ptr
    bad_pos = [
        (ok_p, ok_r, 0, None, n, out, cnt, ws, wsb),                      # ncols outside 1..8
        (c_ptrs((ptrs * 5)[:9]), c_ranges((ranges * 5)[:9]), 9, None, n, out, cnt, ws, wsb),
        (ok_p, ok_r, -1, None, n, out, cnt, ws, wsb),
        (ok_p, ok_r, 2, None, 2**31, out, cnt, ws, 2**40),                # 2^31 rows (never read)
        (c_ptrs([ptrs[0], None]), ok_r, 2, None, n, out, cnt, ws, wsb),   # a NULL column
        (c_ptrs([ptrs[0], ptrs[1] + 2]), ok_r, 2, None, n, out, cnt, ws, wsb),  # not 4-byte aligned
        (ok_p, ok_r, 2, pay + 1, n, out, cnt, ws, wsb),
        (ok_p, None, 2, None, n, out, cnt, ws, wsb),                      # no ranges
        (None, ok_r, 2, None, n, out, cnt, ws, wsb),
        (ok_p, ok_r, 2, None, n, out, cnt, ws, wsb - 1),                  # a short workspace
        (ok_p, ok_r, 2, None, n, out, cnt, None, wsb),
        (ok_p, ok_r, 2, None, n, None, cnt, ws, wsb),                     # no output
    ]
    for a in bad_pos:
        assert L.mq_where_positions(*a, None) == mq.MQ_EINVAL, a[2:5]
        assert L.mq_last_error()
    bad_agg = [
        (ok_p, ok_r, 0, val, n, agg, ws, wsb),
        (c_ptrs((ptrs * 5)[:9]), c_ranges((ranges * 5)[:9]), 9, val, n, agg, ws, wsb),
        (ok_p, ok_r, 2, val, 2**31, agg, ws, 2**40),
        (ok_p, ok_r, 2, None, n, agg, ws, wsb),                           # no value column
        (ok_p, ok_r, 2, val + 2, n, agg, ws, wsb),
        (c_ptrs([None, ptrs[1]]), ok_r, 2, val, n, agg, ws, wsb),
        (ok_p, None, 2, val, n, agg, ws, wsb),
        (ok_p, ok_r, 2, val, n, agg, ws, 1000),
        (ok_p, ok_r, 2, val, n, None, ws, wsb),
    ]
    for a in bad_agg:
        assert L.mq_where_agg(*a, None) == mq.MQ_EINVAL, a[2:5]
        assert L.mq_last_error()
    k, got = bench.read_positions(n)
    assert np.all(got == SENT) and np.all(bench.cnt.get(np.uint64, 2) == SENT64)
    assert np.all(bench.agg.get(np.uint8, 48) == SENT_BYTE)
    # no rows: K = 0 and the empty aggregate, NULL columns are fine
    none = c_ptrs([None, None])
    assert L.mq_where_positions(none, ok_r, 2, None, 0, None, cnt, ws, wsb, None) == mq.MQ_OK
    assert L.mq_where_agg(none, ok_r, 2, None, 0, agg, ws, wsb, None) == mq.MQ_OK
    assert bench.read_positions(0)[0] == 0 and bench.read_agg() == (0, 0, wc.I32_MAX, wc.I32_MIN)


# ---------------------------------------------------------------------------
# the drop-ins
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
    n = len(gs)
    gp = (C.POINTER(mq.GeneralizedColumn) * max(n, 1))(*[C.pointer(g) for g in gs])
    lows = (C.POINTER(C.c_int) * max(n, 1))(*[_b(lo) for lo, _ in ranges])
    highs = (C.POINTER(C.c_int) * max(n, 1))(*[_b(hi) for _, hi in ranges])
    return gs, gp, lows, highs


def select_where(L, objs, ranges, positions=None, ncols=None):
    """select_where -> (status, numpy positions or None)"""
    keep = where_args(objs, ranges)
    st = mq.Status(0, None)
    pos = None if positions is None else positions if isinstance(positions, C.POINTER(mq.Result)) else C.byref(positions)
    rp = L.select_where(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, pos, C.byref(st))
    if not rp:
        return st.code, None
    assert rp.contents.data_type == mq.INT
    return st.code, take(rp)


def aggregate_where(L, objs, ranges, values, ncols=None):
    """aggregate_where -> (status, (count, sum, min, max) or None)"""
    keep = where_args(objs, ranges)
    gv, st = gcol(values), mq.Status(0, None)
    rpp = L.aggregate_where(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, C.byref(gv), C.byref(st))
    if not rpp:
        return st.code, None
    assert [rpp[i].contents.data_type for i in range(4)] == [mq.LONG, mq.LONG, mq.INT, mq.INT]
    assert all(rpp[i].contents.num_tuples == 1 for i in range(4))
    out = tuple(int(take(rpp[i])[0]) for i in range(4))
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def chain(L, cols_c, ranges):
    """select_column_scan -> fetch_column -> select_result (-> ...) through libmq: the
    positions Result* (the caller takes it)."""
    st = mq.Status(0, None)
    pos = L.select_column_scan(C.byref(cols_c[0]), _b(ranges[0][0]), _b(ranges[0][1]), C.byref(st))
    assert st.code == mq.OK and pos
    for c, (lo, hi) in zip(cols_c[1:], ranges[1:]):
        f = L.fetch_column(C.byref(c), pos, C.byref(st))
        assert st.code == mq.OK and f
        nxt = L.select_result(f, pos, _b(lo), _b(hi), C.byref(st))
        assert st.code == mq.OK and nxt
        take(f)
        take(pos)
        pos = nxt
    return pos


def reduce_chain(L, val_c, pos):
    """fetch_column -> sum / min / max of a positions Result*."""
    st = mq.Status(0, None)
    f = L.fetch_column(C.byref(val_c), pos, C.byref(st))
    assert st.code == mq.OK and f
    g = gcol(f)
    s = int(take(L.sum(C.byref(g), C.byref(st)))[0])
    mn, mx = int(take(L.min(f, C.byref(st)))[0]), int(take(L.max(f, C.byref(st)))[0])
    assert st.code == mq.OK
    k = int(f.contents.num_tuples)
    take(f)
    return k, s, mn, mx


@pytest.mark.parametrize("name", ["uniform_10", "sorted_lead", "islands_alt", "last_kills"])
@pytest.mark.parametrize("ncols", [2, 3])
def test_dropin_equals_the_chain(lib, name, ncols):
    n = wc.BIG
    cols, ranges = wc.case(name, n, ncols)
    val = wc.values_of(n)
    cc, cv = [make_column(c) for c in cols], make_column(val)
    pos = chain(lib, cc, ranges)
    want = wc.positions(cols, ranges)
    assert len(want) > 0
    k, s, mn, mx = reduce_chain(lib, cv, pos)
    assert np.array_equal(take(pos), want)
    code, got = select_where(lib, cc, ranges)
    assert code == mq.OK and got.dtype == np.int32 and np.array_equal(got, want)
    code, agg = aggregate_where(lib, cc, ranges, cv)
    assert code == mq.OK and agg == (k, s, mn, mx) == wc.aggregate(cols, ranges, val)
    for c in cc + [cv]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_positions_results_and_outcomes(lib):
    n = 70_001
    cols, ranges = wc.case("uniform_50", n, 3)
    pay, val = wc.payload_of(n), wc.values_of(n)
    cc, cv = [make_column(c) for c in cols], make_column(val)
    rpay = make_result(pay)
    code, got = select_where(lib, cc, ranges, rpay)  # the positions argument is honoured
    assert code == mq.OK and np.array_equal(got, wc.positions(cols, ranges, pay))
    # INT Results as column arguments: a Result with an HBM shadow and a caller's own
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    f1 = lib.fetch_column(C.byref(cc[1]), C.byref(every), C.byref(st))
    assert st.code == mq.OK and f1
    r2 = make_result(cols[2])
    mixed = [cc[0], f1, r2]
    code, got = select_where(lib, mixed, ranges)
    assert code == mq.OK and np.array_equal(got, wc.positions(cols, ranges))
    code, agg = aggregate_where(lib, mixed, ranges, f1)
    assert code == mq.OK and agg == wc.aggregate(cols, ranges, cols[1])
    code, agg = aggregate_where(lib, mixed, ranges, r2)
    assert code == mq.OK and agg == wc.aggregate(cols, ranges, cols[2])
    # full and empty outcomes
    full = [(None, None), (0, 1000), (None, 5000)]
    code, got = select_where(lib, cc, full)
    assert code == mq.OK and np.array_equal(got, np.arange(n, dtype=np.int32))
    assert aggregate_where(lib, cc, full, cv) == (mq.OK, wc.aggregate(cols, full, val))
    for none in ([(0, 1000), (7, 7), (None, None)], [(2000, 3000), (None, None), (0, 1000)]):
        code, got = select_where(lib, cc, none, rpay)
        assert code == mq.OK and got.dtype == np.int32 and len(got) == 0
        assert aggregate_where(lib, cc, none, cv) == (mq.OK, (0, 0, wc.I32_MAX, wc.I32_MIN))
    # one column, eight columns
    assert np.array_equal(select_where(lib, cc[:1], ranges[:1])[1], wc.positions(cols[:1], ranges[:1]))
    c8, r8 = wc.case("uniform_50", n, 8)
    cc8 = [make_column(c) for c in c8]
    assert np.array_equal(select_where(lib, cc8, r8)[1], wc.positions(c8, r8))
    assert aggregate_where(lib, cc8, r8, cv) == (mq.OK, wc.aggregate(c8, r8, val))
    # no rows
    e = np.empty(0, np.int32)
    ce = [make_column(e), make_column(e)]
    code, got = select_where(lib, ce, ranges[:2])
    assert code == mq.OK and len(got) == 0
    assert aggregate_where(lib, ce, ranges[:2], ce[0]) == (mq.OK, (0, 0, wc.I32_MAX, wc.I32_MIN))
    take(f1)
    for r in (rpay, every, r2):
        free_result_struct(r)
    for c in cc + cc8 + ce + [cv]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_errors(lib, capfd):
    n = 1000
    cols, ranges = wc.case("uniform_50", n, 2)
    cc = [make_column(c) for c in cols]
    short = make_column(cols[0][:999].copy())
    lng = make_result(cols[0].astype(np.int64), mq.LONG)
    rshort = make_result(cols[0][:999])
    capfd.readouterr()

    def refused(call):
        ok = call == (mq.ERROR, None)
        return ok and "libmq" in capfd.readouterr().err

    assert refused(select_where(lib, cc, ranges, ncols=0))
    assert refused(select_where(lib, cc * 5, ranges * 5, ncols=9))
    assert refused(aggregate_where(lib, cc, ranges, cc[0], ncols=0))
    assert refused(aggregate_where(lib, cc * 5, ranges * 5, cc[0], ncols=9))
    assert refused(select_where(lib, [cc[0], short], ranges))            # different lengths
    assert refused(aggregate_where(lib, cc, ranges, short))
    assert refused(select_where(lib, cc, ranges, rshort))
    assert refused(select_where(lib, [cc[0], lng], ranges))              # a LONG Result as a column
    assert refused(select_where(lib, cc, ranges, lng))                   # ... as positions
    assert refused(aggregate_where(lib, cc, ranges, lng))                # ... as values
    g = mq.GeneralizedColumn()
    g.column_type = 7  # neither a Column nor a Result
    g.column_pointer.column = C.pointer(cc[0])
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(g))
    lows, highs = (C.POINTER(C.c_int) * 1)(None), (C.POINTER(C.c_int) * 1)(None)
    st = mq.Status(0, None)
    assert not lib.select_where(gp, lows, highs, 1, None, C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.select_where(None, lows, highs, 1, None, C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 2
    code, got = select_where(lib, cc, ranges)  # and the operator still works
    assert code == mq.OK and np.array_equal(got, wc.positions(cols, ranges))
    for r in (lng, rshort):
        free_result_struct(r)
    for c in cc + [short]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_under_row_shards(lib):
    """A column held as row shards gives the same answer (the operator runs on the calling
    device) and is split again by the next sharded operator."""
    n = wc.BIG
    cols, ranges = wc.case("clustered_lead", n, 3)
    val = wc.values_of(n)
    cc, cv = [make_column(c) for c in cols], make_column(val)
    devs = (C.c_int * 2)(0, 0)
    assert lib.mq_shard_config(2, devs, 2, 0) == 0
    try:
        st = mq.Status(0, None)
        first = lib.select_column(C.byref(cc[0]), _b(ranges[0][0]), _b(ranges[0][1]), C.byref(st))  # splits column 0
        assert st.code == mq.OK and np.array_equal(take(first), wc.positions(cols[:1], ranges[:1]))
        code, got = select_where(lib, cc, ranges)
        assert code == mq.OK and np.array_equal(got, wc.positions(cols, ranges))
        assert aggregate_where(lib, cc, ranges, cv) == (mq.OK, wc.aggregate(cols, ranges, val))
        again = lib.select_column(C.byref(cc[0]), _b(ranges[0][0]), _b(ranges[0][1]), C.byref(st))
        assert st.code == mq.OK and np.array_equal(take(again), wc.positions(cols[:1], ranges[:1]))
    finally:
        for c in cc + [cv]:
            lib.mq_column_invalidate(C.byref(c))
        assert lib.mq_shard_config(0, None, 0, 0) == 0
