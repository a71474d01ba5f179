"""select_where_in on gfx950 (csrc/mq_keyset.hip, the k_semi_* kernels of csrc/mq_where.hip;
select_where_in / aggregate_where_in in mq_query.c), every comparison exact equality: with the
numpy restatement in semicases.py, with mq_where_positions / mq_where_agg where the key
predicate drops out, and with the hash join's per-row counts.
"""
import ctypes as C

import numpy as np
import pytest

import semicases as sc
import wherecases as wc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take
from test_gpu_where import PAD, SENT, SENT64, SENT_BYTE, Bench, Columns, c_ptrs, c_ranges, gcol, lib, where_args  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = [mq.MQ_SEMI_AUTO, mq.MQ_SEMI_LDS, mq.MQ_SEMI_GLOBAL]
LDS_FORCED_MAX = 128 * 1024  # a forced MQ_SEMI_LDS takes bitmaps up to this size (mq_device.h)


class KeySet:
    """A key set built on the device from a numpy column."""

    def __init__(self, lib, keys, offset_elems=0, bounds=None, stream=None):
        self.lib = lib
        self.keys = np.ascontiguousarray(keys, dtype=np.int32)
        self.dev = Dev.of(self.keys, offset_elems=offset_elems)
        self.h, self.info = C.c_void_p(), mq.MqKeysetInfo()
        hb, lo, hi = (0, 0, 0) if bounds is None else (1, bounds[0], bounds[1])
        self.rc = lib.mq_keyset_build(self.dev.ptr if len(self.keys) else None, len(self.keys), hb, lo, hi,
                                      C.byref(self.h), C.byref(self.info), stream)

    def free(self):
        if self.h:
            mq.check(self.lib.mq_device_sync(), "device sync")
            assert self.lib.mq_keyset_free(self.h) == mq.MQ_OK
            self.h = C.c_void_p()

    def paths(self):
        return PATHS if self.info.bytes <= LDS_FORCED_MAX else [mq.MQ_SEMI_AUTO, mq.MQ_SEMI_GLOBAL]


class SemiBench(Bench):
    def semi_positions_async(self, ptrs, ranges, key, ks, anti, path, pay, n):
        return self.lib.mq_semi_positions(c_ptrs(ptrs) if ptrs else None, c_ranges(ranges) if ranges else None, len(ptrs), key,
                                          ks, anti, path, pay, n, self.out.ptr, self.cnt.ptr, self.ws.ptr, self.ws_bytes,
                                          self.stream)

    def semi_agg_async(self, ptrs, ranges, key, ks, anti, path, val, n):
        return self.lib.mq_semi_agg(c_ptrs(ptrs) if ptrs else None, c_ranges(ranges) if ranges else None, len(ptrs), key, ks,
                                    anti, path, val, n, self.agg.ptr, self.ws.ptr, self.ws_bytes, self.stream)

    def semi_positions(self, ptrs, ranges, key, ks, anti, path, pay, n, want, tag):
        self.reset(n)
        rc = self.semi_positions_async(ptrs, ranges, key, ks, anti, path, pay, n)
        assert rc == mq.MQ_OK, tag + (self.lib.mq_last_error(),)
        self.check_positions(n, want, tag)

    def semi_aggregate(self, ptrs, ranges, key, ks, anti, path, val, n, want, tag):
        self.reset(0)
        rc = self.semi_agg_async(ptrs, ranges, key, ks, anti, path, val, n)
        assert rc == mq.MQ_OK, tag + (self.lib.mq_last_error(),)
        assert self.read_agg() == want, tag

    def probe_all(self, n):
        """The n + PAD output entries and K of the last positions call."""
        return self.read_positions(n)


def run_probe(bench, cols, ranges, key, ks, n, offs=(0, 1), ko=0, po=0, vo=0, tag=()):
    """Semi and anti, positions with and without a payload and the aggregate, on every path the
    set allows, against the restatement."""
    pay, val = wc.payload_of(n), wc.values_of(n)
    dev = Columns(cols + [key], pay, val)
    ptrs = dev.ptrs(list(offs) + [ko])  # the key's alignment is the last distinct column's
    kptr, ptrs = ptrs[-1], ptrs[:-1]
    for anti in (0, 1):
        want_pos = sc.positions(cols, ranges, key, ks.keys, anti)
        want_pay = sc.positions(cols, ranges, key, ks.keys, anti, pay)
        want_agg = sc.aggregate(cols, ranges, key, ks.keys, val, anti)
        for path in ks.paths():
            t = tag + (n, len(cols), anti, path)
            bench.semi_positions(ptrs, ranges, kptr, ks.h, anti, path, None, n, want_pos, t + ("positions",))
            bench.semi_positions(ptrs, ranges, kptr, ks.h, anti, path, dev.pay[po].ptr, n, want_pay, t + ("payload",))
            bench.semi_aggregate(ptrs, ranges, kptr, ks.h, anti, path, dev.val[vo].ptr, n, want_agg, t + ("aggregate",))
    return dev, ptrs, kptr


@pytest.fixture(scope="module")
def small(lib):
    return SemiBench(lib, max(wc.SIZES))


@pytest.fixture(scope="module")
def big(lib):
    return SemiBench(lib, wc.BIG)


def lds_threshold(lib):
    """kSemiLdsBytes: the largest bitmap MQ_SEMI_AUTO copies into LDS."""
    lo, hi = 16, 512 << 20  # LDS at lo, GLOBAL at hi (test_semi_host.py)
    while hi - lo > 16:
        mid = (lo + hi) // 32 * 16
        lo, hi = (mid, hi) if lib.mq_semi_auto_path(mid) == mq.MQ_SEMI_LDS else (lo, mid)
    return lo


# ---------------------------------------------------------------------------
# the build
# ---------------------------------------------------------------------------

def check_build(lib, keys, offset_elems=0, bounds=None, tag=()):
    """distinct, lo / hi and the bitmap's size; then a full probe of [lo - 2, hi + 2] returns
    exactly the unique keys, on every path the set allows."""
    ks = KeySet(lib, keys, offset_elems, bounds)
    try:
        assert ks.rc == mq.MQ_OK, tag + (lib.mq_last_error(),)
        uniq = np.unique(ks.keys)
        assert ks.info.distinct == len(uniq), tag
        if len(uniq) == 0:
            assert ks.info.lo > ks.info.hi and ks.info.bytes == 0, tag
            lo, hi = 0, 3
        else:
            lo, hi = (int(uniq[0]), int(uniq[-1])) if bounds is None else bounds
            assert (ks.info.lo, ks.info.hi) == (lo, hi), tag
            assert ks.info.bytes == (hi - lo + 128) // 128 * 16, tag
        probe = np.arange(max(lo - 2, wc.I32_MIN), min(hi + 2, wc.I32_MAX) + 1, dtype=np.int64).astype(np.int32)
        n = len(probe)
        bench, dp = SemiBench(lib, n), Dev.of(probe)
        for path in ks.paths():
            bench.semi_positions([], [], dp.ptr, ks.h, 0, path, dp.ptr, n, uniq, tag + ("probe", path))
    finally:
        ks.free()


@pytest.mark.parametrize("n1", [0, 1, 257, 4097, 70_001])
def test_build_sizes(lib, n1):
    check_build(lib, np.random.default_rng(n1).integers(-3000, 3000, n1), tag=(n1,))


@pytest.mark.parametrize("limit", [1, 2])
def test_build_many_iterations_a_block(lib, limit):
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        keys = np.random.default_rng(limit).integers(-40_000, 40_000, 300_001)
        check_build(lib, keys, offset_elems=limit - 1, tag=(limit,))
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_build_unaligned_duplicates_and_a_hot_key(lib):
    rng = np.random.default_rng(5)
    for off in (1, 2, 3):
        check_build(lib, rng.integers(-500, 500, 8193 + off), offset_elems=off, tag=("unaligned", off))
    check_build(lib, np.repeat(rng.integers(-100, 100, 40), 300), tag=("duplicates",))
    hot = np.full(10**6, 12345)
    check_build(lib, hot, tag=("hot",))
    hot[[0, 333_333, 999_999]] = [12000, 12345 + 64, 12001]
    check_build(lib, hot, offset_elems=1, tag=("hot and three more",))


@pytest.mark.parametrize("span", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129])
def test_build_spans_around_a_word(lib, span):
    for base in (0, -70, wc.I32_MIN, wc.I32_MAX - span + 1):
        ends = np.array([base, base + span - 1])
        check_build(lib, ends, tag=(span, base, "ends"))
        check_build(lib, np.arange(base, base + span, 2), tag=(span, base, "every other"))


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_build_span_around_the_lds_threshold(lib, d):
    t = lds_threshold(lib)
    span = t * 8 + d
    ks = KeySet(lib, [-5, span - 6])
    try:
        assert ks.rc == mq.MQ_OK and ks.info.bytes == (t if d <= 0 else t + 16)
        assert lib.mq_semi_auto_path(ks.info.bytes) == (mq.MQ_SEMI_LDS if d <= 0 else mq.MQ_SEMI_GLOBAL)
    finally:
        ks.free()
    check_build(lib, np.array([-5, 0, span // 2, span - 7, span - 6]), tag=("threshold", d))


def test_build_the_full_span(lib):
    """{INT32_MIN, INT32_MAX}: a 512 MiB bitmap, bit 0 and bit 2^32 - 1."""
    ks = KeySet(lib, [wc.I32_MIN, wc.I32_MAX, wc.I32_MAX])
    try:
        assert ks.rc == mq.MQ_OK, lib.mq_last_error()
        assert (ks.info.lo, ks.info.hi, ks.info.distinct, ks.info.bytes) == (wc.I32_MIN, wc.I32_MAX, 2, 512 << 20)
        probe = np.array([wc.I32_MIN, wc.I32_MIN + 1, -1, 0, 1, wc.I32_MAX - 1, wc.I32_MAX, 31, 32, wc.I32_MIN + 32], dtype=np.int32)
        bench, dp = SemiBench(lib, len(probe)), Dev.of(probe)
        assert ks.paths() == [mq.MQ_SEMI_AUTO, mq.MQ_SEMI_GLOBAL]
        for anti, want in ((0, [0, 6]), (1, [1, 2, 3, 4, 5, 7, 8, 9])):
            for path in (mq.MQ_SEMI_AUTO, mq.MQ_SEMI_GLOBAL):
                bench.semi_positions([], [], dp.ptr, ks.h, anti, path, None, len(probe), np.array(want, np.int32), (anti, path))
    finally:
        ks.free()
        lib.mq_trim()


def test_build_given_bounds(lib):
    keys = np.random.default_rng(3).integers(-50, 50, 4097)
    check_build(lib, keys, bounds=(-50, 49), tag=("exact",))
    check_build(lib, keys, bounds=(-1000, 777), offset_elems=1, tag=("wider",))
    for bounds, bad in (((-49, 49), -50), ((-50, 48), 49), ((0, 10), None)):
        k2 = keys.copy()
        if bad is not None:
            k2[4000] = bad  # present for certain
        ks = KeySet(lib, k2, bounds=bounds)
        assert ks.rc == mq.MQ_EINVAL and not ks.h and "outside the bounds" in lib.mq_last_error().decode()
    dk = Dev.of(keys)
    h = C.c_void_p(1)
    assert lib.mq_keyset_build(dk.ptr, len(keys), 1, 5, 4, C.byref(h), None, None) == mq.MQ_EINVAL and not h  # lo > hi
    h = C.c_void_p(1)
    assert lib.mq_keyset_build(dk.ptr, 2**31, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL and not h
    assert lib.mq_keyset_build(None, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keyset_build(dk.ptr + 2, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keyset_build(dk.ptr, 5, 0, 0, 0, None, None, None) == mq.MQ_EINVAL
    assert lib.mq_keyset_free(None) == mq.MQ_OK
    h = C.c_void_p()
    assert lib.mq_keyset_build(dk.ptr, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_OK and h  # h_info may be NULL
    assert lib.mq_keyset_free(h) == mq.MQ_OK


# ---------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("ncols", sc.NCOLS)
def test_probe_agrees_with_the_restatement(lib, small, ncols):
    """Every size, the range sets and the named key sets rotated over them: semi and anti,
    positions with and without a payload and the aggregate, on every path the set allows, the
    columns, key, payload and values 0 and 1 dword off a 16-byte boundary."""
    for i, n in enumerate(wc.SIZES):
        name = wc.CASES[(3 * i + ncols) % len(wc.CASES)]
        for j in range(3):
            sname = sc.SETS[(i + 3 * j + ncols) % len(sc.SETS)]
            cols, ranges = sc.case(name, n, ncols)
            key, s = sc.keyset(sname, n)
            ks = KeySet(lib, s, offset_elems=j & 1)
            try:
                assert ks.rc == mq.MQ_OK
                run_probe(small, cols, ranges, key, ks, n, offs=[(i + j) & 1, j & 1, 1], ko=(i + j + 1) & 1, po=j & 1,
                          vo=(i + 1) & 1, tag=(name, sname))
            finally:
                ks.free()


@pytest.mark.parametrize("sname", sc.SETS)
def test_probe_every_named_set(lib, small, sname):
    """Each key set at sizes around a tile, an expand block and a full iteration, with no
    range and behind one: keys below lo, above hi, at lo and hi, and at both ends of int32."""
    for n in (1, 33, 1025, 4097, 8193):
        key, s = sc.keyset(sname, n)
        ks = KeySet(lib, s)
        try:
            assert ks.rc == mq.MQ_OK
            for ncols, name in ((0, "uniform_50"), (1, "uniform_50")):
                cols, ranges = sc.case(name, n, ncols)
                run_probe(small, cols, ranges, key, ks, n, offs=[n & 1], ko=1 - (n & 1), tag=(sname, name))
        finally:
            ks.free()


@pytest.mark.parametrize("name", ["islands_first", "islands_last", "islands_alt", "clustered_lead", "tail_only", "ends_only",
                                  "first_none", "empty_range", "extreme_bounds", "same_twice"])
def test_probe_dead_key_lines_next_to_live_ones(lib, small, name):
    n = 8193
    for ncols, sname in ((1, "dense_small"), (3, "sparse_wide"), (3, "min_edge")):
        cols, ranges = sc.case(name, n, ncols)
        key, s = sc.keyset(sname, n)
        ks = KeySet(lib, s)
        try:
            run_probe(small, cols, ranges, key, ks, n, offs=[0, 1], ko=ncols & 1, tag=(name, sname))
        finally:
            ks.free()


@pytest.mark.parametrize("limit", [1, 2])
def test_probe_many_iterations_a_block(lib, big, limit):
    """BIG rows on a grid of 1 or 2 CUs' blocks, both paths: many iterations a block, chunk
    edges inside lines of the misaligned columns, the LDS copy made once per block."""
    n = wc.BIG
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        for ncols, name, sname in ((0, "uniform_10", "dense_small"), (1, "clustered_lead", "dups"), (3, "uniform_50", "negative"),
                                   (8, "islands_alt", "sparse_wide")):
            cols, ranges = sc.case(name, n, ncols)
            key, s = sc.keyset(sname, n)
            ks = KeySet(lib, s)
            try:
                run_probe(big, cols, ranges, key, ks, n, offs=[limit - 1, 1, 0], ko=2 - limit, po=limit - 1, vo=2 - limit,
                          tag=(name, sname, limit))
            finally:
                ks.free()
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_probe_key_aliases_a_predicate_and_the_value_column(lib, small):
    n = 8193
    cols, ranges = wc.case("uniform_50", n, 3)
    s = np.random.default_rng(1).integers(200, 800, 300).astype(np.int32)
    ks = KeySet(lib, s)
    try:
        dev = Columns(cols, wc.payload_of(n), wc.values_of(n))
        for offs in ([0], [1], [0, 1]):
            ptrs = dev.ptrs(offs)
            for c in (0, 2):  # the key is predicate column c, and the value column too
                for anti in (0, 1):
                    for path in ks.paths():
                        tag = (tuple(offs), c, anti, path)
                        small.semi_positions(ptrs, ranges, ptrs[c], ks.h, anti, path, None, n,
                                             sc.positions(cols, ranges, cols[c], s, anti), tag)
                        small.semi_aggregate(ptrs, ranges, ptrs[c], ks.h, anti, path, ptrs[c], n,
                                             sc.aggregate(cols, ranges, cols[c], s, cols[c], anti), tag)
    finally:
        ks.free()


# ---------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------

def where_positions(bench, ptrs, ranges, pay, n):
    bench.reset(n)
    assert bench.positions_async(ptrs, ranges, pay, n) == mq.MQ_OK
    k, got = bench.read_positions(n)
    return got[:k].copy()


def test_semi_and_anti_partition_the_where_result(lib, small):
    n = 8193
    for ncols, name, sname in ((1, "uniform_50", "dense_small"), (3, "sorted_lead", "sparse_wide"), (8, "first_all", "dups")):
        cols, ranges = wc.case(name, n, ncols)
        key, s = sc.keyset(sname, n)
        ks = KeySet(lib, s)
        try:
            dev = Columns(cols + [key], wc.payload_of(n), wc.values_of(n))
            ptrs = dev.ptrs([0, 1])
            kptr, ptrs = ptrs[-1], ptrs[:-1]
            whole = where_positions(small, ptrs, ranges, None, n)
            for path in ks.paths():
                parts = []
                for anti in (0, 1):
                    small.reset(n)
                    assert small.semi_positions_async(ptrs, ranges, kptr, ks.h, anti, path, None, n) == mq.MQ_OK
                    k, got = small.read_positions(n)
                    parts.append(got[:k].copy())
                assert len(np.intersect1d(parts[0], parts[1])) == 0
                assert np.array_equal(np.sort(np.concatenate(parts)), whole) and len(parts[0]) and len(parts[1])
        finally:
            ks.free()


def test_semi_equals_the_join_counts(lib):
    """ncols == 0: the semi positions are the probe rows with a join partner, by the hash join's
    own per-row counts, duplicates on both sides."""
    n1, n2 = 4097, 70_001
    rng = np.random.default_rng(21)
    c1 = rng.integers(-900, 900, n1).astype(np.int32)
    c2 = rng.integers(-2000, 2000, n2).astype(np.int32)
    d1, p1, d2 = Dev.of(c1), Dev.of(np.arange(n1, dtype=np.int32)), Dev.of(c2)
    dcnt = Dev(4 * n2)
    j, m = C.c_void_p(), C.c_uint64()
    mq.check(lib.mq_join_build(d1.ptr, p1.ptr, n1, C.byref(j), None), "mq_join_build")
    try:
        mq.check(lib.mq_join_probe(j, d2.ptr, n2, C.byref(m), None), "mq_join_probe")
        mq.check(lib.mq_join_counts(j, dcnt.ptr, None), "mq_join_counts")
        counts = dcnt.get(np.uint32, n2)
    finally:
        lib.mq_join_free(j)
    assert int(counts.sum()) == m.value and 0 < np.count_nonzero(counts) < n2
    ks, bench = KeySet(lib, c1), SemiBench(lib, n2)
    try:
        for path in ks.paths():
            bench.semi_positions([], [], d2.ptr, ks.h, 0, path, None, n2, np.flatnonzero(counts > 0).astype(np.int32), (path,))
            bench.semi_positions([], [], d2.ptr, ks.h, 1, path, None, n2, np.flatnonzero(counts == 0).astype(np.int32), (path,))
    finally:
        ks.free()


def test_the_empty_set_and_the_full_set(lib, small):
    """NOT IN the empty set is mq_where_positions / mq_where_agg bit for bit (every row with no
    range), IN the empty set is nothing; a set of every key gives the where result and nothing."""
    n = 8193
    pay, val = wc.payload_of(n), wc.values_of(n)
    empty = KeySet(lib, np.empty(0, np.int32))
    try:
        for ncols, name in ((0, "uniform_10"), (1, "uniform_10"), (3, "clustered_lead"), (3, "empty_range")):
            cols, ranges = sc.case(name, n, ncols)
            key, s = sc.keyset("every_key", n)
            full = KeySet(lib, s)
            dev = Columns(cols + [key], pay, val)
            ptrs = dev.ptrs([0, 1])
            kptr, ptrs = ptrs[-1], ptrs[:-1]
            if ncols:
                want_pos = where_positions(small, ptrs, ranges, dev.pay[1].ptr, n)
                small.reset(0)
                assert small.agg_async(ptrs, ranges, dev.val[1].ptr, n) == mq.MQ_OK
                want_agg = small.read_agg()
            else:
                want_pos, want_agg = pay, wc.aggregate([val], [(None, None)], val)
            try:
                for path in PATHS:
                    tag = (name, ncols, path)
                    small.semi_positions(ptrs, ranges, kptr, empty.h, 1, path, dev.pay[1].ptr, n, want_pos, tag + ("anti empty",))
                    small.semi_aggregate(ptrs, ranges, kptr, empty.h, 1, path, dev.val[1].ptr, n, want_agg, tag + ("anti empty",))
                    small.semi_positions(ptrs, ranges, kptr, empty.h, 0, path, None, n, np.empty(0, np.int32), tag)
                    small.semi_aggregate(ptrs, ranges, kptr, empty.h, 0, path, dev.val[0].ptr, n, (0, 0, wc.I32_MAX, wc.I32_MIN), tag)
                    small.semi_positions(ptrs, ranges, kptr, full.h, 0, path, dev.pay[1].ptr, n, want_pos, tag + ("semi full",))
                    small.semi_aggregate(ptrs, ranges, kptr, full.h, 0, path, dev.val[1].ptr, n, want_agg, tag + ("semi full",))
                    small.semi_positions(ptrs, ranges, kptr, full.h, 1, path, None, n, np.empty(0, np.int32), tag + ("anti full",))
            finally:
                full.free()
    finally:
        empty.free()


def test_predicate_order_does_not_matter(lib, small):
    n = 8193
    cols, ranges = wc.case("uniform_50", n, 3)
    key, s = sc.keyset("dense_small", n)
    ks = KeySet(lib, s)
    try:
        pay, val = wc.payload_of(n), wc.values_of(n)
        dev = Columns(cols + [key], pay, val)
        ptrs = dev.ptrs([0, 1])
        kptr, ptrs = ptrs[-1], ptrs[:-1]
        for perm in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [2, 0, 1]):
            pp, rr = [ptrs[i] for i in perm], [ranges[i] for i in perm]
            for anti in (0, 1):
                for path in ks.paths():
                    small.semi_positions(pp, rr, kptr, ks.h, anti, path, dev.pay[0].ptr, n,
                                         sc.positions(cols, ranges, key, s, anti, pay), (tuple(perm), anti, path))
                    small.semi_aggregate(pp, rr, kptr, ks.h, anti, path, dev.val[1].ptr, n,
                                         sc.aggregate(cols, ranges, key, s, val, anti), (tuple(perm), anti, path))
    finally:
        ks.free()


def test_sixteen_streams_one_key_set(lib):
    """One key set probed from sixteen streams at once, different ranges, forms and paths."""
    n = 70_001
    key, s = sc.keyset("dense_small", n)
    ks = KeySet(lib, s)
    streams = []
    for _ in range(16):
        st = C.c_void_p()
        mq.check(lib.mq_stream_create(C.byref(st)), "mq_stream_create")
        streams.append(st)
    try:
        dkey = Dev.of(key)
        jobs = []
        for i, st in enumerate(streams):
            name, ncols = wc.CASES[i % len(wc.CASES)], sc.NCOLS[(i // 4) % 4]
            cols, ranges = sc.case(name, n, ncols)
            pay, val = wc.payload_of(n), wc.values_of(n)
            jobs.append((SemiBench(lib, n, st), Columns(cols + [key], pay, val), cols, ranges, pay, val, (name, ncols, i)))
        mq.check(lib.mq_device_sync(), "device sync")  # the uploads (null stream) are done
        for b, *_ in jobs:
            b.reset(n)
        for i, (b, dev, cols, ranges, pay, val, tag) in enumerate(jobs):
            ptrs = dev.ptrs([i & 1, (i >> 1) & 1])[:-1]
            anti, path = i & 1, PATHS[i % 3]
            assert b.semi_positions_async(ptrs, ranges, dkey.ptr, ks.h, anti, path, dev.pay[i & 1].ptr if i & 2 else None, n) == mq.MQ_OK, tag
            assert b.semi_agg_async(ptrs, ranges, dkey.ptr, ks.h, 1 - anti, path, dev.val[i & 1].ptr, n) == mq.MQ_OK, tag
        for i, (b, dev, cols, ranges, pay, val, tag) in enumerate(jobs):
            b.check_positions(n, sc.positions(cols, ranges, key, s, i & 1, pay if i & 2 else None), tag)
            assert b.read_agg() == sc.aggregate(cols, ranges, key, s, val, 1 - (i & 1)), tag
    finally:
        mq.check(lib.mq_device_sync(), "device sync")
        for st in streams:
            lib.mq_stream_destroy(st)
        ks.free()


def test_errors_write_nothing(lib):
    n = 1025
    bench = SemiBench(lib, n)
    cols, ranges = wc.case("uniform_50", n, 2)
    key, s = sc.keyset("dense_small", n)
    ks, wide = KeySet(lib, s), KeySet(lib, sc.keyset("sparse_wide", n)[1])
    try:
        dev = Columns(cols + [key], wc.payload_of(n), wc.values_of(n))
        ptrs = dev.ptrs([0, 1])
        kp, ptrs = ptrs[-1], ptrs[:-1]
        ok_p, ok_r = c_ptrs(ptrs), c_ranges(ranges)
        bench.reset(n)
        L, ws, wsb = lib, bench.ws.ptr, lib.mq_semi_workspace_bytes(n)
        out, cnt, agg = bench.out.ptr, bench.cnt.ptr, bench.agg.ptr
        pay, val = dev.pay[0].ptr, dev.val[0].ptr
        A = mq.MQ_SEMI_AUTO
        bad_pos = [
            (ok_p, ok_r, -1, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),       # ncols outside 0..8
            (c_ptrs((ptrs * 5)[:9]), c_ranges((ranges * 5)[:9]), 9, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, 2**31, out, cnt, ws, 2**40),  # 2^31 rows (never read)
            (ok_p, ok_r, 2, kp, None, 0, A, None, n, out, cnt, ws, wsb),        # no key set
            (ok_p, ok_r, 2, None, ks.h, 0, A, None, n, out, cnt, ws, wsb),      # no key column
            (ok_p, ok_r, 2, kp + 2, ks.h, 1, A, None, n, out, cnt, ws, wsb),    # not 4-byte aligned
            (c_ptrs([ptrs[0], None]), ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),
            (c_ptrs([ptrs[0], ptrs[1] + 2]), ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),
            (ok_p, None, 2, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),        # ranges missing with ncols > 0
            (None, ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, pay + 1, n, out, cnt, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, None, cnt, ws, wsb),       # no output
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, out + 2, cnt, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, out, None, ws, wsb),       # no count
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, ws, wsb - 1),    # a short workspace
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, ws + 4, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, out, cnt, None, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, 3, None, n, out, cnt, ws, wsb),        # a path that is none of the three
            (ok_p, ok_r, 2, kp, ks.h, 0, -1, None, n, out, cnt, ws, wsb),
            (ok_p, ok_r, 2, kp, wide.h, 0, mq.MQ_SEMI_LDS, None, n, out, cnt, ws, wsb),  # LDS forced on a set that does not fit
        ]
        for a in bad_pos:
            assert L.mq_semi_positions(*a, None) == mq.MQ_EINVAL, a[2:9]
            assert L.mq_last_error()
        bad_agg = [
            (ok_p, ok_r, -1, kp, ks.h, 0, A, val, n, agg, ws, wsb),
            (c_ptrs((ptrs * 5)[:9]), c_ranges((ranges * 5)[:9]), 9, kp, ks.h, 0, A, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, val, 2**31, agg, ws, 2**40),
            (ok_p, ok_r, 2, kp, None, 1, A, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, None, ks.h, 0, A, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, kp + 1, ks.h, 0, A, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, None, n, agg, ws, wsb),             # no value column
            (ok_p, ok_r, 2, kp, ks.h, 0, A, val + 2, n, agg, ws, wsb),
            (c_ptrs([None, ptrs[1]]), ok_r, 2, kp, ks.h, 0, A, val, n, agg, ws, wsb),
            (ok_p, None, 2, kp, ks.h, 0, A, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, val, n, None, ws, wsb),
            (ok_p, ok_r, 2, kp, ks.h, 0, A, val, n, agg, ws, 1000),
            (ok_p, ok_r, 2, kp, ks.h, 0, 3, val, n, agg, ws, wsb),
            (ok_p, ok_r, 2, kp, wide.h, 1, mq.MQ_SEMI_LDS, val, n, agg, ws, wsb),
        ]
        for a in bad_agg:
            assert L.mq_semi_agg(*a, None) == mq.MQ_EINVAL, a[2:9]
            assert L.mq_last_error()
        k, got = bench.read_positions(n)
        assert np.all(got == SENT) and np.all(bench.cnt.get(np.uint64, 2) == SENT64)
        assert np.all(bench.agg.get(np.uint8, 48) == SENT_BYTE)
        # no rows: K = 0 and the empty aggregate, NULL columns are fine
        assert L.mq_semi_positions(None, None, 0, None, ks.h, 0, A, None, 0, None, cnt, ws, wsb, None) == mq.MQ_OK
        assert L.mq_semi_agg(None, None, 0, None, ks.h, 1, A, None, 0, agg, ws, wsb, None) == mq.MQ_OK
        assert bench.read_positions(0)[0] == 0 and bench.read_agg() == (0, 0, wc.I32_MAX, wc.I32_MIN)
    finally:
        ks.free()
        wide.free()


# ---------------------------------------------------------------------------
# the drop-ins
# ---------------------------------------------------------------------------

def select_where_in(L, objs, ranges, keys, set_keys, anti, positions=None, ncols=None, null_arrays=False):
    """select_where_in -> (status, numpy positions or None)"""
    keep = where_args(objs, ranges)
    gk, gs, st = gcol(keys), gcol(set_keys), mq.Status(0, None)
    pos = None if positions is None else positions if isinstance(positions, C.POINTER(mq.Result)) else C.byref(positions)
    a = (None, None, None) if null_arrays else keep[1:4]
    rp = L.select_where_in(*a, len(objs) if ncols is None else ncols, C.byref(gk), C.byref(gs), anti, pos, C.byref(st))
    if not rp:
        return st.code, None
    assert rp.contents.data_type == mq.INT
    return st.code, take(rp)


def aggregate_where_in(L, objs, ranges, keys, set_keys, anti, values, ncols=None, null_arrays=False):
    """aggregate_where_in -> (status, (count, sum, min, max) or None)"""
    keep = where_args(objs, ranges)
    gk, gs, gv, st = gcol(keys), gcol(set_keys), gcol(values), mq.Status(0, None)
    a = (None, None, None) if null_arrays else keep[1:4]
    rpp = L.aggregate_where_in(*a, len(objs) if ncols is None else ncols, C.byref(gk), C.byref(gs), anti, C.byref(gv), C.byref(st))
    if not rpp:
        return st.code, None
    assert [rpp[i].contents.data_type for i in range(4)] == [mq.LONG, mq.LONG, mq.INT, mq.INT]
    assert all(rpp[i].contents.num_tuples == 1 for i in range(4))
    out = tuple(int(take(rpp[i])[0]) for i in range(4))
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def test_dropin_equals_the_device_calls(lib):
    n = 70_001
    cols, ranges = wc.case("uniform_50", n, 3)
    pay, val = wc.payload_of(n), wc.values_of(n)
    cc, cv = [make_column(c) for c in cols], make_column(val)
    rpay = make_result(pay)
    for sname in ("dense_small", "sparse_wide", "empty", "min_edge"):
        key, s = sc.keyset(sname, n)
        ck, cs, rs, rk = make_column(key), make_column(s), make_result(s), make_result(key)
        for anti in (False, True):
            for p in (3, 1, 0):
                want = sc.positions(cols[:p], ranges[:p], key, s, anti)
                tag = (sname, anti, p)
                code, got = select_where_in(lib, cc[:p], ranges[:p], ck, cs, anti)
                assert code == mq.OK and got.dtype == np.int32 and np.array_equal(got, want), tag
                code, got = select_where_in(lib, cc[:p], ranges[:p], rk, rs, anti, rpay)  # INT Results, positions
                assert code == mq.OK and np.array_equal(got, sc.positions(cols[:p], ranges[:p], key, s, anti, pay)), tag
                assert aggregate_where_in(lib, cc[:p], ranges[:p], ck, rs, anti, cv) == (
                    mq.OK, sc.aggregate(cols[:p], ranges[:p], key, s, val, anti)), tag
            # no range at all, the arrays NULL
            code, got = select_where_in(lib, [], [], ck, cs, anti, null_arrays=True)
            assert code == mq.OK and np.array_equal(got, sc.positions([], [], key, s, anti))
            assert aggregate_where_in(lib, [], [], ck, cs, anti, ck, null_arrays=True) == (
                mq.OK, sc.aggregate([], [], key, s, key, anti))  # the values are the keys
        for r in (rs, rk):
            free_result_struct(r)
        for c in (ck, cs):
            lib.mq_column_invalidate(C.byref(c))
    # a select_where output as the subquery: rows of column 1 in a range, as a set of row ids
    code, sub = select_where(lib, cc[1:2], [(0, 300)])
    st = mq.Status(0, None)
    keep = where_args(cc[1:2], [(0, 300)])
    subq = lib.select_where(keep[1], keep[2], keep[3], 1, None, C.byref(st))
    assert st.code == mq.OK and subq and subq.contents.num_tuples == len(sub) > 0
    rowid = np.arange(n, dtype=np.int32)
    cid = make_column(rowid)
    for anti in (False, True):
        code, got = select_where_in(lib, cc[:1], ranges[:1], cid, subq, anti)
        assert code == mq.OK and np.array_equal(got, sc.positions(cols[:1], ranges[:1], rowid, sub, anti))
    take(subq)
    free_result_struct(rpay)
    for c in cc + [cv, cid]:
        lib.mq_column_invalidate(C.byref(c))


def select_where(L, objs, ranges):
    keep = where_args(objs, ranges)
    st = mq.Status(0, None)
    rp = L.select_where(keep[1], keep[2], keep[3], len(objs), None, C.byref(st))
    return st.code, take(rp)


def test_dropin_errors(lib, capfd):
    n = 1000
    cols, ranges = wc.case("uniform_50", n, 2)
    key, s = sc.keyset("dense_small", n)
    cc, ck, cs = [make_column(c) for c in cols], make_column(key), make_column(s)
    short = make_column(cols[0][:999].copy())
    lng = make_result(cols[0].astype(np.int64), mq.LONG)
    rshort = make_result(cols[0][:999])
    capfd.readouterr()

    def refused(call):
        ok = call == (mq.ERROR, None)
        return ok and "libmq" in capfd.readouterr().err

    assert refused(select_where_in(lib, cc, ranges, ck, cs, False, ncols=-1))
    assert refused(select_where_in(lib, cc * 5, ranges * 5, ck, cs, True, ncols=9))
    assert refused(aggregate_where_in(lib, cc * 5, ranges * 5, ck, cs, False, cc[0], ncols=9))
    assert refused(select_where_in(lib, cc, ranges, short, cs, False))              # different lengths
    assert refused(select_where_in(lib, [cc[0], short], ranges, ck, cs, False))
    assert refused(aggregate_where_in(lib, cc, ranges, ck, cs, True, short))
    assert refused(select_where_in(lib, cc, ranges, ck, cs, False, rshort))
    assert refused(select_where_in(lib, cc, ranges, lng, cs, False))                # a LONG Result as the keys
    assert refused(select_where_in(lib, cc, ranges, ck, lng, True))                 # ... as the set keys
    assert refused(select_where_in(lib, cc, ranges, ck, cs, False, lng))            # ... as positions
    assert refused(aggregate_where_in(lib, cc, ranges, ck, cs, False, lng))         # ... as values
    assert refused(select_where_in(lib, [cc[0], lng], ranges, ck, cs, False))
    g = mq.GeneralizedColumn()
    g.column_type = 7  # neither a Column nor a Result
    g.column_pointer.column = C.pointer(cc[0])
    gk, gs = gcol(ck), gcol(cs)
    for a in ((C.byref(g), C.byref(gs)), (C.byref(gk), C.byref(g)), (None, C.byref(gs)), (C.byref(gk), None)):
        st = mq.Status(0, None)
        assert not lib.select_where_in(None, None, None, 0, a[0], a[1], False, None, C.byref(st)) and st.code == mq.ERROR
    st = mq.Status(0, None)
    assert not lib.select_where_in(None, None, None, 1, C.byref(gk), C.byref(gs), False, None, C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 5
    code, got = select_where_in(lib, cc, ranges, ck, cs, True)  # and the operator still works
    assert code == mq.OK and np.array_equal(got, sc.positions(cols, ranges, key, s, True))
    for r in (lng, rshort):
        free_result_struct(r)
    for c in cc + [short, ck, cs]:
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_under_row_shards(lib):
    """Columns held as row shards give the same answer (the operator runs on the calling device)
    and are split again by the next sharded operator."""
    n = wc.BIG
    cols, ranges = wc.case("clustered_lead", n, 3)
    key, s = sc.keyset("dense_small", n)
    val = wc.values_of(n)
    cc, ck, cs, cv = [make_column(c) for c in cols], make_column(key), make_column(s), make_column(val)
    devs = (C.c_int * 2)(0, 0)
    assert lib.mq_shard_config(2, devs, 2, 0) == 0
    try:
        st = mq.Status(0, None)
        lo, hi = C.pointer(C.c_int(100)), C.pointer(C.c_int(600))
        for c, a in ((cc[0], cols[0]), (ck, key)):  # splits column 0 and the key column
            first = lib.select_column(C.byref(c), lo, hi, C.byref(st))
            assert st.code == mq.OK and np.array_equal(take(first), wc.positions([a], [(100, 600)]))
        for anti in (False, True):
            code, got = select_where_in(lib, cc, ranges, ck, cs, anti)
            assert code == mq.OK and np.array_equal(got, sc.positions(cols, ranges, key, s, anti))
            assert aggregate_where_in(lib, cc, ranges, ck, cs, anti, cv) == (mq.OK, sc.aggregate(cols, ranges, key, s, val, anti))
        again = lib.select_column(C.byref(ck), lo, hi, C.byref(st))
        assert st.code == mq.OK and np.array_equal(take(again), wc.positions([key], [(100, 600)]))
    finally:
        for c in cc + [ck, cs, cv]:
            lib.mq_column_invalidate(C.byref(c))
        assert lib.mq_shard_config(0, None, 0, 0) == 0
