"""mq_topk64 on gfx950 (csrc/mq_topk64.hip): HAVING, ORDER BY and LIMIT over int64 entries, every
comparison exact equality with the numpy restatement in topk64cases.py (the reference has no such
operator).
"""
import ctypes as C

import numpy as np
import pytest

import topk64cases as tc
from devbuf import Dev
from refapi import mq

pytestmark = pytest.mark.gpu

AUTO, SELECT, SORT = mq.MQ_TOPK_AUTO, mq.MQ_TOPK_SELECT, mq.MQ_TOPK_SORT
PAD = 8
SENT_BYTE = 0xA5
SENT64 = np.frombuffer(bytes([SENT_BYTE] * 8), np.int64)[0]
SENT32 = np.frombuffer(bytes([SENT_BYTE] * 4), np.uint32)[0]
# (path, cand_cap): the select path with the default cap, with caps that force every level and the
# rank-limited tie emission, the sort path, and the rule
CONFIGS = [(SELECT, 0), (SELECT, 1), (SELECT, 64), (SORT, 0), (AUTO, 0), (AUTO, 64)]


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    return L


class Outs:
    """Values (int64) and indices (u32) of cap + PAD entries, refilled with the sentinel before each call."""

    def __init__(self, lib, cap):
        self.lib, self.cap = lib, cap
        self.v, self.i = Dev(8 * (cap + PAD)), Dev(4 * (cap + PAD))

    def reset(self, m):
        mq.check(self.lib.mq_memset(self.v.ptr, SENT_BYTE, 8 * (m + PAD), None), "mq_memset")
        mq.check(self.lib.mq_memset(self.i.ptr, SENT_BYTE, 4 * (m + PAD), None), "mq_memset")

    def check(self, m, want_v, want_i, skip, tag):
        gv, gi = self.v.get(np.int64, m + PAD), self.i.get(np.uint32, m + PAD)
        if "v" in skip:
            assert np.all(gv == SENT64), tag + ("values were not asked for",)
        else:
            assert np.array_equal(gv[:m], want_v) and np.all(gv[m:] == SENT64), tag + ("values",)
        if "i" in skip:
            assert np.all(gi == SENT32), tag + ("indices were not asked for",)
        else:
            assert np.array_equal(gi[:m], want_i) and np.all(gi[m:] == SENT32), tag + ("indices",)


class Case:
    """One value column, the second column and the device copies of both."""

    def __init__(self, vset, n, off=0):
        self.n = n
        self.vals = tc.values_of(vset, n)
        self.second = tc.second_of(n)
        self.dv, self.ds = Dev.of(self.vals, offset_elems=off), Dev.of(self.second, offset_elems=off)

        self.orders = {}

    def having(self, which):
        return {None: (None, None), "second": (self.second, self.ds.ptr), "vals": (self.vals, self.dv.ptr)}[which]

    def order(self, fname, desc, with_vals):
        """The model's order of all passing entries (computed once a filter and direction)."""
        key = (fname, desc and with_vals, with_vals)
        if key not in self.orders:
            which, rng = tc.filter_of(fname, self.vals)
            self.orders[key] = tc.topk64(self.vals if with_vals else None, self.having(which)[0], rng, tc.K_ALL, desc, n=self.n)
        return self.orders[key]


def rng64(low, high):
    return mq.MqRange64(low is not None, low or 0, high is not None, high or 0)


def run(L, outs, case, with_vals, fname, k, desc, path, cap, tag, skip=()):
    """One mq_topk64 call checked against the model, outputs and info; returns the info."""
    n = case.n
    which, (low, high) = tc.filter_of(fname, case.vals)
    hav, dh = case.having(which)
    full = case.order(fname, desc, with_vals)
    passed = len(full)
    m = min(k, passed)
    want = full[:m]
    outs.reset(m)
    info = mq.MqTopk64Info()
    r = rng64(low, high)
    rc = L.mq_topk64(case.dv.ptr if with_vals else None, dh, C.byref(r) if dh else None, n, k, int(desc), path, cap,
                     None if "v" in skip else outs.v.ptr, None if "i" in skip else outs.i.ptr, C.byref(info), None)
    assert rc == mq.MQ_OK, tag + (L.mq_last_error(),)
    outs.check(m, case.vals[want] if with_vals else want.astype(np.int64), want.astype(np.uint32), skip, tag)
    # the info, field by field
    ce = cap or L.mq_topk_default_cap()
    rule = SORT if min(k, n) + ce > n // mq.MQ_TOPK_SORT_DIV else SELECT  # as mq_device.h states it
    assert info.path == (path if path != AUTO else rule), tag
    assert info.m == m, tag
    assert info.passed == passed, tag
    if m == 0:
        assert (info.candidates, info.ties, info.levels) == (0, 0, 0), tag
        return info
    if not with_vals:  # index order: the first m passing entries are the result
        assert (info.candidates, info.ties, info.levels) == (m, 0, 1 if info.path == SELECT else 0), tag
        return info
    sv = case.vals[full]  # monotone
    assert info.ties == int(np.count_nonzero(sv[m:] == sv[m - 1])), tag
    if info.path == SORT:
        assert (info.levels, info.candidates) == (0, passed), tag
    else:
        assert 1 <= info.levels <= 6 and m <= info.candidates <= m + ce, tag
        pv = case.vals[want]
        if cap == 1 and (info.ties or (m > 1 and pv[m - 1] == pv[m - 2])):  # the threshold value repeats: no level fits the cap
            assert info.levels == 6 and info.candidates == m, tag
    return info


@pytest.mark.parametrize("n", tc.SIZES)
@pytest.mark.parametrize("vset", tc.VALUE_SETS)
def test_paths_agree_with_the_restatement(lib, vset, n):
    """Every size, value set and filter in both directions, with values and in index order, every k
    under rotating paths and caps, the columns 0 and 8 bytes off a 16-byte boundary: the same exact
    answer, nothing written past m, and the info the header promises."""
    cases = [Case(vset, n, off) for off in (0, 1)]
    outs = Outs(lib, n)
    i = 0
    for fname in tc.FILTERS:
        which, rng = tc.filter_of(fname, cases[0].vals)
        passed = int(tc.mask_of(cases[0].having(which)[0], rng, n).sum())
        for desc in (False, True):
            for k in tc.ks_of(n, passed):
                for j in range(2):
                    i += 1
                    path, cap = CONFIGS[i % len(CONFIGS)]
                    with_vals = i % 5 != 0
                    run(lib, outs, cases[(i // 3) & 1], with_vals, fname, k, desc, path, cap,
                        (vset, n, fname, desc, k, path, cap, with_vals))


def test_levels_follow_the_shared_digits(lib):
    """cand_cap = 1 over 55 shared bits with repeats walks all six digits; the whole int64 range at
    the default cap needs one read; j shared digits at a cap below the column need j + 1."""
    n = 4097
    outs = Outs(lib, n)
    c = Case("shared_55", n)
    for desc in (False, True):
        info = run(lib, outs, c, True, "none", 100, desc, SELECT, 1, ("shared_55", desc))
        assert info.levels == 6
    c = Case("full_range", n)
    for desc in (False, True):
        assert run(lib, outs, c, True, "none", 100, desc, SELECT, 0, ("full_range", desc)).levels == 1
    for j in range(1, 6):
        c = Case(f"shared_{11 * j}", n)
        info = run(lib, outs, c, True, "half", 10, j & 1 == 1, SELECT, 64, ("shared", j))
        assert info.levels == j + 1, j


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("vset", tc.VALUE_SETS)
def test_many_tiles_a_block(lib, vset, limit):
    """A few hundred thousand entries on a grid of 1 or 2 CUs' blocks: each block owns many tiles,
    and the rank of a threshold entry is carried across tiles and blocks."""
    n = tc.BIG
    case = Case(vset, n, limit & 1)
    outs = Outs(lib, n)
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        i = 0
        for fname in ("none", "half", "on_vals"):
            for desc in (False, True):
                for k in (1, 65, 40_000, n + 5):
                    i += 1
                    for path, cap in (CONFIGS[i % 3], CONFIGS[3]):
                        if k > 65 and (path, cap) == (SELECT, 0) and desc:
                            continue  # the same candidates as ascending: keep the case quick
                        run(lib, outs, case, (i + cap) % 4 != 0, fname, k, desc, path, cap, (vset, limit, fname, desc, k, path, cap))
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_no_workspace_of_n(lib):
    """All entries equal, k = 10, cap 1: exactly 10 entries are collected, whatever n is."""
    n = tc.BIG
    case = Case("all_equal", n)
    outs = Outs(lib, 10)
    for limit in (1, 2, 0):
        mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
        try:
            for desc in (False, True):
                info = run(lib, outs, case, True, "none", 10, desc, SELECT, 1, ("all equal", limit, desc))
                assert (info.candidates, info.ties, info.levels, info.path) == (10, n - 10, 6, SELECT)
        finally:
            mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


@pytest.mark.parametrize("skip", [("v",), ("i",), ("v", "i")])
def test_null_outputs(lib, skip):
    n, k = 4097, 65
    case = Case("shared_22", n)
    outs = Outs(lib, n)
    for desc in (False, True):
        for fname in ("none", "half"):
            for path, cap in CONFIGS[:4]:
                for with_vals in (True, False):
                    run(lib, outs, case, with_vals, fname, k, desc, path, cap, (skip, desc, fname, path, cap), skip=skip)


def test_errors_write_nothing(lib):
    n = 1025
    case = Case("full_range", n)
    dv, ds = case.dv.ptr, case.ds.ptr
    outs = Outs(lib, n)
    outs.reset(n)
    info = mq.MqTopk64Info()
    r = rng64(0, 50)
    R = C.byref(r)
    ov, oi = outs.v.ptr, outs.i.ptr
    bad_calls = [
        (dv, None, None, n, 5, 3, ov, oi),             # a path that is none of the three
        (dv, ds, R, n, 5, -1, ov, oi),
        (dv, None, None, 2**31, 5, AUTO, ov, oi),      # 2^31 entries (no pointer is ever read)
        (None, None, None, 2**31, 5, SELECT, ov, oi),
        (dv, ds, R, 2**31, 0, SORT, ov, oi),
        (dv + 4, None, None, n, 5, AUTO, ov, oi),      # values not 8-byte aligned
        (dv + 1, None, None, n, 5, AUTO, ov, oi),
        (dv, ds + 4, R, n, 5, AUTO, ov, oi),           # the filter column
        (dv, None, None, n, 5, AUTO, ov + 4, oi),      # the value output
        (dv, None, None, n, 5, AUTO, ov, oi + 2),      # the index output: 4-byte
        (dv, ds, None, n, 5, AUTO, ov, oi),            # a filter column without a range
    ]
    for v, h, rr, rows, k, path, o1, o2 in bad_calls:
        assert lib.mq_topk64(v, h, rr, rows, k, 0, path, 0, o1, o2, C.byref(info), None) == mq.MQ_EINVAL
        assert lib.mq_last_error()
    assert np.all(outs.v.get(np.int64, n + PAD) == SENT64) and np.all(outs.i.get(np.uint32, n + PAD) == SENT32)
    # nothing to do: NULL pointers are fine
    for v, rows, k in ((None, 0, 5), (dv, n, 0), (None, 0, 0)):
        for path in (AUTO, SELECT, SORT):
            assert lib.mq_topk64(v, None, None, rows, k, 1, path, 0, None, None, C.byref(info), None) == mq.MQ_OK
            assert (info.m, info.candidates, info.ties, info.levels) == (0, 0, 0, 0)
    # a range that no int64 satisfies, both ways of writing one: no entry passes, nothing is written
    for low, high in ((5, 5), (7, 3), (None, tc.I64_MIN)):
        r = rng64(low, high)
        assert lib.mq_topk64(dv, ds, C.byref(r), n, 5, 0, SELECT, 0, ov, oi, C.byref(info), None) == mq.MQ_OK
        assert (info.m, info.passed) == (0, 0)
    assert np.all(outs.v.get(np.int64, n + PAD) == SENT64) and np.all(outs.i.get(np.uint32, n + PAD) == SENT32)


def test_widen_and_take(lib):
    """The helpers around the call: int32 aggregates made sortable, columns gathered through the indices."""
    n = 70_001
    rng = np.random.default_rng(8)
    a = rng.integers(-2**31, 2**31 - 1, n, endpoint=True).astype(np.int32)
    a[:2] = (-2**31, 2**31 - 1)
    b = tc.values_of("full_range", n)
    idx = rng.integers(0, n, 5000).astype(np.uint32)
    da, db, di = Dev.of(a, offset_elems=1), Dev.of(b, offset_elems=1), Dev.of(idx)
    w, t4, t8 = Dev(8 * n), Dev(4 * len(idx)), Dev(8 * len(idx))
    mq.check(lib.mq_topk64_widen(da.ptr, n, w.ptr, None), "widen")
    mq.check(lib.mq_topk64_take(da.ptr, 4, di.ptr, len(idx), t4.ptr, None), "take 4")
    mq.check(lib.mq_topk64_take(db.ptr, 8, di.ptr, len(idx), t8.ptr, None), "take 8")
    assert np.array_equal(w.get(np.int64, n), a.astype(np.int64))
    assert np.array_equal(t4.get(np.int32, len(idx)), a[idx]) and np.array_equal(t8.get(np.int64, len(idx)), b[idx])
    assert lib.mq_topk64_take(da.ptr, 2, di.ptr, 5, t4.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_topk64_take(db.ptr + 4, 8, di.ptr, 5, t8.ptr, None) == mq.MQ_EINVAL
    assert lib.mq_topk64_widen(da.ptr, 0, None, None) == mq.MQ_OK
