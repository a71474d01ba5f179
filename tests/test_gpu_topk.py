"""Top k on gfx950 (csrc/mq_topk.hip; top_k in mq_query.c), every comparison exact equality
with the numpy restatement in topkcases.py (the reference has no such operator).
"""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

import groupcases as gc
import topkcases as tc
from devbuf import Dev
from refapi import _libc, make_column, make_result, free_result_struct, mq, take

pytestmark = pytest.mark.gpu

AUTO, SELECT, SORT = mq.MQ_TOPK_AUTO, mq.MQ_TOPK_SELECT, mq.MQ_TOPK_SORT
PAD = 8
SENT_BYTE = 0xA5
SENT = np.frombuffer(bytes([SENT_BYTE] * 4), np.int32)[0]
# (path, cand_cap): the select path with the default cap, with caps that force every level
# and the rank-limited tie emission, the sort path, and the rule
CONFIGS = [(SELECT, 0), (SELECT, 1), (SELECT, 7), (SORT, 0), (AUTO, 0), (AUTO, 7)]


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


class Outs:
    """Two device buffers of cap + PAD entries, refilled with the sentinel before each call."""

    def __init__(self, lib, cap):
        self.lib, self.cap = lib, cap
        self.v, self.p = Dev(4 * (cap + PAD)), Dev(4 * (cap + PAD))

    def reset(self, m):
        for d in (self.v, self.p):
            mq.check(self.lib.mq_memset(d.ptr, SENT_BYTE, 4 * (m + PAD), None), "mq_memset")


def run(L, outs, dv, dp, n, k, desc, path, cap, want, tag, skip=()):
    """One mq_topk call checked against `want`; returns its info."""
    m = min(k, n)
    outs.reset(m)
    info = mq.MqTopkInfo()
    rc = L.mq_topk(dv, dp, n, k, int(desc), path, cap, None if "v" in skip else outs.v.ptr,
                   None if "p" in skip else outs.p.ptr, C.byref(info), None)
    assert rc == mq.MQ_OK, tag + (L.mq_last_error(),)
    assert info.m == m, tag
    for nm, d, w in (("v", outs.v, want[0]), ("p", outs.p, want[1])):
        got = d.get(np.int32, m + PAD)
        if nm in skip:
            assert np.all(got == SENT), tag + (nm, "an output that was not asked for was written")
            continue
        assert np.array_equal(got[:m], w[:m]), tag + (nm,)
        assert np.all(got[m:] == SENT), tag + (nm, "wrote past m")
    return info


def check_info(L, info, vals, idx, n, k, desc, path, cap, tag):
    m = min(k, n)
    ce = cap or L.mq_topk_default_cap()
    rule = SORT if m + ce > n // mq.MQ_TOPK_SORT_DIV else SELECT  # as mq_device.h states it
    assert info.path == (path if path != AUTO else rule), tag
    if m == 0:
        return
    ties = tc.ties_left_out(vals, k, desc, idx)
    assert info.ties == ties, tag
    if info.path == SORT:
        assert info.levels == 0, tag
        return
    assert 1 <= info.levels <= 3 and m <= info.candidates <= m + ce, tag
    if cap == 1:
        if ties or (m > 1 and vals[idx[m - 1]] == vals[idx[m - 2]]):  # the threshold value repeats: no level fits the cap
            assert info.levels == 3 and info.candidates == m, tag


# ---------------------------------------------------------------------------
# device level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", tc.SIZES)
@pytest.mark.parametrize("vset", tc.VALUE_SETS)
def test_paths_agree_with_the_restatement(lib, vset, n):
    """Every value set, size, k and direction under every path and cap, values and payload
    0 and 1 dword off a 16-byte boundary independently, with and without a payload: the
    same exact answer, nothing written past m, and the info the header promises."""
    vals, pay = tc.values_of(vset, n), tc.payload_of(n)
    dvs = [Dev.of(vals, offset_elems=o) for o in (0, 1)]
    dps = [Dev.of(pay, offset_elems=o) for o in (0, 1)]
    outs = Outs(lib, n)
    i = 0
    for desc in (False, True):
        idx = tc.order(vals, desc)
        full = {None: (vals[idx], idx.astype(np.int32)), 1: (vals[idx], pay[idx])}
        for k in tc.ks_of(n):
            for path, cap in CONFIGS:
                i += 1
                with_pay = 1 if i % 3 else None
                dv, dp = dvs[i & 1], dps[(i >> 1) & 1]
                tag = (vset, n, desc, k, path, cap, with_pay)
                info = run(lib, outs, dv.ptr, dp.ptr if with_pay else None, n, k, desc, path, cap, full[with_pay], tag)
                check_info(lib, info, vals, idx, n, k, desc, path, cap, tag)


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("vset", tc.VALUE_SETS)
def test_many_tiles_a_block(lib, vset, limit):
    """A few hundred thousand rows on a grid of 1 or 2 CUs' blocks: each block owns many
    tiles, and the rank of a threshold row is carried across tiles and blocks."""
    n = tc.BIG
    vals, pay = tc.values_of(vset, n), tc.payload_of(n)
    dv, dp = Dev.of(vals, offset_elems=limit & 1), Dev.of(pay)
    outs = Outs(lib, n)
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        for desc in (False, True):
            idx = tc.order(vals, desc)
            full = {None: (vals[idx], idx.astype(np.int32)), 1: (vals[idx], pay[idx])}
            for j, k in enumerate((1, 10, 65, 40_000, n - 1, n + 5)):
                for path, cap in CONFIGS[:5]:
                    if k > 65 and path == SELECT and cap == 0 and desc:
                        continue  # the same candidates as ascending: keep the case quick
                    with_pay = 1 if (j + cap) & 1 else None
                    tag = (vset, limit, desc, k, path, cap, with_pay)
                    info = run(lib, outs, dv.ptr, dp.ptr if with_pay else None, n, k, desc, path, cap, full[with_pay], tag)
                    check_info(lib, info, vals, idx, n, k, desc, path, cap, tag)
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_no_workspace_of_n(lib):
    """All rows equal, k = 10, cap 1: exactly 10 entries are collected, whatever n is."""
    n = tc.BIG
    vals = tc.values_of("all_equal", n)
    dv = Dev.of(vals)
    outs = Outs(lib, 10)
    for limit in (1, 2, 0):
        mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
        try:
            for desc in (False, True):
                want = tc.topk(vals, None, 10, desc)
                info = run(lib, outs, dv.ptr, None, n, 10, desc, SELECT, 1, want, ("all equal", limit, desc))
                assert (info.candidates, info.ties, info.levels, info.path) == (10, n - 10, 3, SELECT)
        finally:
            mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_auto_rule_on_both_sides(lib):
    n, cap = 4097, 7
    vals = tc.values_of("full_range", n)
    dv = Dev.of(vals)
    outs = Outs(lib, n)
    edge = n // mq.MQ_TOPK_SORT_DIV - cap  # k + cap == n / DIV: the last k that selects
    for k, want_path in ((1, SELECT), (edge, SELECT), (edge + 1, SORT), (n, SORT)):
        assert lib.mq_topk_auto_path(n, k, cap) == want_path
        info = run(lib, outs, dv.ptr, None, n, k, True, AUTO, cap, tc.topk(vals, None, k, True), ("auto", k))
        assert info.path == want_path, k
    # the default cap: a column this small is sorted, whatever k is
    info = run(lib, outs, dv.ptr, None, n, 1, False, AUTO, 0, tc.topk(vals, None, 1, False), ("auto default",))
    assert info.path == SORT and lib.mq_topk_default_cap() > n


@pytest.mark.parametrize("skip", [("v",), ("p",), ("v", "p")])
def test_null_outputs(lib, skip):
    n, k = 4097, 65
    vals, pay = tc.values_of("top22_shared", n), tc.payload_of(n)
    dv, dp = Dev.of(vals), Dev.of(pay, offset_elems=1)
    outs = Outs(lib, n)
    for desc in (False, True):
        want, idx = tc.topk(vals, pay, k, desc), tc.order(vals, desc)
        for path, cap in CONFIGS[:4]:
            info = run(lib, outs, dv.ptr, dp.ptr, n, k, desc, path, cap, want, (skip, desc, path, cap), skip=skip)
            check_info(lib, info, vals, idx, n, k, desc, path, cap, (skip, desc, path, cap))


def test_errors_write_nothing(lib):
    n = 1025
    vals = tc.values_of("full_range", n)
    dv = Dev.of(vals, offset_elems=1)
    outs = Outs(lib, n)
    outs.reset(n)
    info = mq.MqTopkInfo()
    bad_calls = [
        (dv.ptr, None, n, 5, 3),             # a path that is none of the three
        (dv.ptr, None, n, 5, -1),
        (dv.ptr, None, 2**31, 5, AUTO),      # 2^31 rows (the pointer is never read)
        (dv.ptr, None, 2**31, 0, SELECT),
        (dv.ptr + 1, None, n, 5, AUTO),      # not 4-byte aligned
        (dv.ptr, dv.ptr + 2, n, 5, AUTO),
        (None, None, n, 5, AUTO),            # no column
    ]
    for v, p, rows, k, path in bad_calls:
        assert lib.mq_topk(v, p, rows, k, 0, path, 0, outs.v.ptr, outs.p.ptr, C.byref(info), None) == mq.MQ_EINVAL
        assert lib.mq_last_error()
    for d in (outs.v, outs.p):
        assert np.all(d.get(np.int32, n + PAD) == SENT)
    # no rows or k == 0: nothing to do, NULL pointers are fine
    for v, rows, k in ((None, 0, 5), (dv.ptr, n, 0), (None, 0, 0)):
        for path in (AUTO, SELECT, SORT):
            assert lib.mq_topk(v, None, rows, k, 1, path, 0, None, None, C.byref(info), None) == mq.MQ_OK
            assert (info.m, info.candidates, info.ties, info.levels) == (0, 0, 0, 0)


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


def top_k(L, values, positions, k, desc):
    """top_k -> (status, [(data_type, numpy array)] * 2 or None)"""
    gv, st = gcol(values), mq.Status(0, None)
    pos = None if positions is None else positions if isinstance(positions, C.POINTER(mq.Result)) else C.byref(positions)
    rpp = L.top_k(C.byref(gv), pos, k, desc, C.byref(st))
    if not rpp:
        return st.code, None
    out = [(rpp[i].contents.data_type, take(rpp[i])) for i in range(2)]
    _libc.free(C.cast(rpp, C.c_void_p))
    return st.code, out


def check_results(code, out, want, tag):
    assert code == mq.OK and out is not None, tag
    assert [t for t, _ in out] == [mq.INT, mq.INT], tag
    for (_, got), w, nm in zip(out, want, ("values", "positions")):
        assert got.dtype == np.int32 and np.array_equal(got, w), tag + (nm,)


@pytest.fixture(scope="module")
def column():
    n = tc.BIG
    vals = tc.values_of("full_range", n)
    vals[::7] = vals[3]  # repeats
    return n, vals


def test_dropin_column_and_result_arguments(lib, column):
    n, vals = column
    cv = make_column(vals)
    pay = tc.payload_of(n)
    rpay = make_result(pay)
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    fv = lib.fetch_column(C.byref(cv), C.byref(every), C.byref(st))  # a Result with an HBM shadow
    assert st.code == mq.OK and fv
    for desc in (False, True):
        for k in (1, 20, 1000, n + 5):
            check_results(*top_k(lib, cv, None, k, desc), tc.topk(vals, None, k, desc), ("column", desc, k))
            check_results(*top_k(lib, cv, rpay, k, desc), tc.topk(vals, pay, k, desc), ("column, positions", desc, k))
            check_results(*top_k(lib, fv, None, k, desc), tc.topk(vals, None, k, desc), ("result", desc, k))
            check_results(*top_k(lib, fv, rpay, k, desc), tc.topk(vals, pay, k, desc), ("result, positions", desc, k))
    take(fv)
    free_result_struct(every)
    free_result_struct(rpay)
    lib.mq_column_invalidate(C.byref(cv))


def test_dropin_positions_from_a_select(lib, column):
    """select_column -> fetch_column -> top_k of (values, positions): the rows' own ids."""
    n, vals = column
    cv = make_column(vals)
    st = mq.Status(0, None)
    low, high = -2**30, 2**30
    pos = lib.select_column(C.byref(cv), C.pointer(C.c_int(low)), C.pointer(C.c_int(high)), C.byref(st))
    fv = lib.fetch_column(C.byref(cv), pos, C.byref(st))
    assert st.code == mq.OK and pos and fv
    sel = np.flatnonzero((vals >= low) & (vals < high)).astype(np.int32)
    assert 1000 < len(sel) < n
    for desc in (False, True):
        for k in (10, 5000):
            check_results(*top_k(lib, fv, pos, k, desc), tc.topk(vals[sel], sel, k, desc), ("select", desc, k))
    for r in (pos, fv):
        take(r)
    lib.mq_column_invalidate(C.byref(cv))


def test_dropin_top_groups(lib):
    """group_aggregate -> top_k of the maxima with the keys as positions: the 20 groups
    with the largest maximum, and the 20 with the smallest minimum."""
    n = 70_001
    keys = gc.keys_of("range_S_plus_1", n, 2048)
    v = gc.values_of("uniform", keys)
    ck, cv = make_column(keys), make_column(v)
    gk, gv, st = gcol(ck), gcol(cv), mq.Status(0, None)
    rpp = lib.group_aggregate(C.byref(gk), C.byref(gv), C.byref(st))
    assert st.code == mq.OK and rpp
    wk, _, _, wmn, wmx = gc.group(keys, v)
    check_results(*top_k(lib, rpp[4], rpp[0], 20, True), tc.topk(wmx, wk, 20, True), ("largest max",))
    check_results(*top_k(lib, rpp[3], rpp[0], 20, False), tc.topk(wmn, wk, 20, False), ("smallest min",))
    for i in range(5):
        take(rpp[i])
    _libc.free(C.cast(rpp, C.c_void_p))
    for c in (ck, cv):
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_empty_and_errors(lib, capfd):
    empty = np.empty(0, np.int32)
    none = (empty, empty)
    ce = make_column(empty)
    re_ = make_result(empty)
    for desc in (False, True):
        check_results(*top_k(lib, ce, None, 5, desc), none, ("no rows",))
        check_results(*top_k(lib, ce, re_, 5, desc), none, ("no rows, positions",))
        check_results(*top_k(lib, re_, None, 0, desc), none, ("empty result",))
    small = np.arange(100, dtype=np.int32)[::-1].copy()
    ck = make_column(small)
    check_results(*top_k(lib, ck, None, 0, False), none, ("k = 0",))
    capfd.readouterr()
    short = make_result(small[:99])
    assert top_k(lib, ck, short, 5, False) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err  # lengths differ
    lng = make_result(small.astype(np.int64), mq.LONG)
    assert top_k(lib, lng, None, 5, False) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err  # LONG values
    assert top_k(lib, ck, lng, 5, False) == (mq.ERROR, None) and "libmq" in capfd.readouterr().err  # LONG positions
    g, st = mq.GeneralizedColumn(), mq.Status(0, None)
    g.column_type = 7  # neither a Column nor a Result
    g.column_pointer.column = C.pointer(ck)
    assert not lib.top_k(C.byref(g), None, 5, False, C.byref(st)) and st.code == mq.ERROR
    assert not lib.top_k(None, None, 5, False, C.byref(st)) and st.code == mq.ERROR
    assert capfd.readouterr().err.count("libmq") == 2
    check_results(*top_k(lib, ck, None, 3, False), tc.topk(small, None, 3, False), ("after the errors",))
    for r in (short, lng, re_):
        free_result_struct(r)
    for c in (ce, ck):
        lib.mq_column_invalidate(C.byref(c))


def test_dropin_uses_the_resident_column(lib):
    """A column in a file mapping stays resident: the second top_k uploads nothing."""
    n = 1_000_003
    vals = tc.values_of("full_range", n)
    fd = os.memfd_create("mqcol")
    os.ftruncate(fd, vals.nbytes)
    m = mmap.mmap(fd, vals.nbytes, mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE)
    os.close(fd)
    a = np.frombuffer(m, dtype=np.int32)[:n]
    a[:] = vals
    col = make_column(a)
    check_results(*top_k(lib, col, None, 10, True), tc.topk(vals, None, 10, True), ("first",))
    r0 = mq.residency(lib)
    check_results(*top_k(lib, col, None, 10, True), tc.topk(vals, None, 10, True), ("second",))
    check_results(*top_k(lib, col, None, 1000, False), tc.topk(vals, None, 1000, False), ("third",))
    r1 = mq.residency(lib)
    assert r1["column_uploads"] == r0["column_uploads"], "the resident column was uploaded again"
    lib.mq_column_invalidate(C.byref(col))
    del a, col
    try:
        m.close()
    except BufferError:
        pass
