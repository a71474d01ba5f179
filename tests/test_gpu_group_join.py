"""group_aggregate_join on gfx950 (csrc/mq_keymap.hip; mq_group_join_plan and k_group_join_dense
in csrc/mq_group.hip; group_aggregate_join in mq_query.c), every comparison exact equality: with
the numpy restatement in groupjoincases.py, with mq_group_where_plan and mq_semi_agg where the
join drops out, and with the chain mq_hash_join -> mq_fetch x 2 -> mq_group_plan run through
libmq itself.
"""
import ctypes as C

import numpy as np
import pytest

import groupcases as gc
import groupjoincases as gj
import groupwherecases as gw
import wherecases as wc
from devbuf import Dev
from refapi import make_column, make_result, free_result_struct, mq, take
from test_gpu_group_where import (DTYPE, NAMES, S, c_ptrs, c_ranges, check_outputs, check_results, filled_outputs, five,  # noqa: F401
                                  gcol, lib, upload, where_args, wplan, write)
from test_gpu_where import PAD, SENT, SENT_BYTE

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
FULL_PROBE_SPAN = 2**26  # up to this span the build test looks up every value of [lo - 2, hi + 2]


def geometry(L, span):
    b, c = C.c_uint32(), C.c_uint64()
    L.mq_keymap_geometry(span, C.byref(b), C.byref(c))
    return b.value, c.value


@pytest.fixture(scope="module")
def chunk(lib):
    return geometry(lib, gj.WORD_EDGES_SPAN)[1]


class KeyMap:
    """A key map built on the device from numpy columns, each `ko` / `ao` dwords off a 16-byte
    boundary."""

    def __init__(self, L, keys, attrs, ko=0, ao=0, bounds=None, stream=None):
        self.lib = L
        self.keys, self.attrs = np.ascontiguousarray(keys, np.int32), np.ascontiguousarray(attrs, np.int32)
        self.dk, self.da = Dev.of(self.keys, offset_elems=ko), Dev.of(self.attrs, offset_elems=ao)
        self.h, self.info = C.c_void_p(), mq.MqKeymapInfo()
        hb, lo, hi = (0, 0, 0) if bounds is None else (1, bounds[0], bounds[1])
        n1 = len(self.keys)
        self.rc = L.mq_keymap_build(self.dk.ptr if n1 else None, self.da.ptr if n1 else None, n1, hb, lo, hi, C.byref(self.h),
                                    C.byref(self.info), stream)

    def fields(self):
        i = self.info
        return i.lo, i.hi, i.attr_lo, i.attr_hi, i.entries, i.bytes

    def free(self):
        if self.h:
            mq.check(self.lib.mq_device_sync(), "device sync")
            assert self.lib.mq_keymap_free(self.h) == mq.MQ_OK
            self.h = C.c_void_p()


def device_lookup(L, km, keys_ptr, pos_ptr, k, missing, want, tag, hits=True):
    """mq_keymap_lookup into sentinel-filled outputs of k + PAD entries: exactly the
    restatement's attributes and hits, nothing written at or past entry k."""
    out, hit = Dev(4 * (k + PAD)), Dev(k + PAD)
    mq.check(L.mq_memset(out.ptr, SENT_BYTE, 4 * (k + PAD), None), "mq_memset")
    mq.check(L.mq_memset(hit.ptr, SENT_BYTE, k + PAD, None), "mq_memset")
    rc = L.mq_keymap_lookup(km, keys_ptr, pos_ptr, k, missing, out.ptr, hit.ptr if hits else None, None)
    assert rc == mq.MQ_OK, tag + (L.mq_last_error(),)
    mq.check(L.mq_stream_sync(None), "sync")
    got, gh = out.get(np.int32, k + PAD), hit.get(np.uint8, k + PAD)
    assert np.array_equal(got[:k], want[0]), tag + ("attributes",)
    assert np.all(got[k:] == SENT), tag + ("wrote past k",)
    assert np.array_equal(gh[:k], want[1]) if hits else np.all(gh[:k] == SENT_BYTE), tag + ("hits",)
    assert np.all(gh[k:] == SENT_BYTE), tag + ("wrote hits past k",)


def probe_keys(dk):
    """Every value of [lo - 2, hi + 2] for a span up to FULL_PROBE_SPAN; otherwise a sample: the
    keys, their neighbours, 70 values inside and 2 outside both ends of the span, both ends of
    int32 and 20 000 random values."""
    if len(dk) == 0:
        return np.array([0, 1, -1, wc.I32_MIN, wc.I32_MAX], dtype=np.int32)
    k64 = dk.astype(np.int64)
    lo, hi = int(k64.min()), int(k64.max())
    if hi - lo + 1 <= FULL_PROBE_SPAN:
        p = np.arange(max(lo - 2, wc.I32_MIN), min(hi + 2, wc.I32_MAX) + 1, dtype=np.int64)
    else:
        rnd = np.random.default_rng(len(dk)).integers(lo, hi, 20_000, endpoint=True)
        p = np.concatenate((k64, k64 - 1, k64 + 1, np.arange(lo - 2, lo + 71), np.arange(hi - 70, hi + 3), [wc.I32_MIN, wc.I32_MAX], rnd))
        p = p[(p >= wc.I32_MIN) & (p <= wc.I32_MAX)]
    return np.ascontiguousarray(p, dtype=np.int32)


def check_build(L, dk, da, ko=0, ao=0, bounds=None, tag=()):
    """The build's info against numpy, the key set it shares, and a lookup of the whole span
    and two values beyond at each end."""
    km = KeyMap(L, dk, da, ko, ao, bounds)
    try:
        assert km.rc == mq.MQ_OK and km.h, tag + (L.mq_last_error(),)
        want = gj.info(dk, da)
        if bounds is not None and len(dk):
            want = bounds + want[2:5] + (gj.map_bytes(bounds[1] - bounds[0] + 1, len(dk)),)
        assert km.fields() == want, tag + (km.fields(), want)
        span = want[1] - want[0] + 1
        assert km.info.bytes == (L.mq_keymap_bytes(span, len(dk)) if len(dk) else 0), tag
        assert bool(L.mq_keymap_keyset(km.h)), tag
        probe = probe_keys(km.keys)
        dp = Dev.of(probe)
        device_lookup(L, km.h, dp.ptr, None, len(probe), -7, gj.lookup(probe, dk, da, -7), tag + ("lookup",))
    finally:
        km.free()


# ---------------------------------------------------------------------------
# the build
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n1", [0, 1, 63, 64, 65, 2048, 2049, 70_001])
def test_build_sizes(lib, n1):
    dk, da = gj.dimension("dense", 7, n1=n1)
    check_build(lib, dk, da, ko=n1 % 4, ao=(n1 + 1) % 4, tag=(n1,))
    sparse = (dk.astype(np.int64) * 37 - 5).astype(np.int32)  # 36 of 37 values of the span are no key
    check_build(lib, sparse, da, ko=(n1 + 2) % 4, ao=n1 % 4, tag=(n1, "sparse"))


@pytest.mark.parametrize("name", gj.DIM_SETS)
def test_build_dimension_sets(lib, chunk, name):
    """Every named dimension, the columns 1 to 3 dwords off a 16-byte boundary; word_edges' span
    gives the prefix pass more than one block and more than one step a block."""
    dk, da = gj.dimension(name, 2048, chunk_words=chunk)
    if name == "word_edges":
        blocks, words = geometry(lib, gj.WORD_EDGES_SPAN)
        assert blocks > 1 and words > 256
    try:
        for ko, ao in ((1, 3), (2, 2), (3, 0)) if len(dk) < 10_000 and name not in ("int32_ends", "sparse_wide") else ((1, 2),):
            check_build(lib, dk, da, ko, ao, tag=(name, ko, ao))
    finally:
        lib.mq_trim()


@pytest.mark.parametrize("limit", [1, 2])
def test_build_many_iterations_a_block(lib, limit):
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        dk, da = gj.dimension("dense", 2048, n1=300_001)
        check_build(lib, dk, da, ko=limit - 1, ao=2 - limit, tag=(limit,))
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_build_refuses_a_repeated_key_and_releases_everything(lib):
    """One repeated key among 70 001: MQ_EINVAL, a NULL handle, the number of repeats in the
    message. The pool has no counter, so its state is read through its reuse rule: idle blocks
    of the bitmap's, the directory's and the attributes' sizes, planted before the call, are
    what the same requests receive again after it (a block the build kept would not be)."""
    dk, da = gj.dimension("dense", 7, n1=70_001)
    dk = dk.copy()
    dk[60_000] = dk[5]
    assert gj.repeated(dk) == 1
    span = int(dk.max()) - int(dk.min()) + 1
    words = (span + 127) // 128 * 4
    sizes = [words * 4, words * 8, len(dk) * 4]
    lib.mq_trim()

    def take_blocks():
        ps = []
        for b in sizes:
            p = C.c_void_p()
            mq.check(lib.mq_pool_malloc(C.byref(p), b), "mq_pool_malloc")
            ps.append(p.value)
        for p in ps:
            mq.check(lib.mq_pool_free(p), "mq_pool_free")
        return ps

    before = take_blocks()
    km = KeyMap(lib, dk, da)
    assert km.rc == mq.MQ_EINVAL and not km.h
    msg = lib.mq_last_error().decode()
    assert "not a primary key" in msg and "1 of 70001" in msg, msg
    assert take_blocks() == before
    check_build(lib, np.delete(dk, 60_000), np.delete(da, 60_000), tag=("after the refusal",))


def test_build_bounds_and_arguments(lib):
    dk, da = gj.dimension("negative", 7)
    lo, hi = int(dk.min()), int(dk.max())
    check_build(lib, dk, da, bounds=(lo, hi), tag=("exact",))
    check_build(lib, dk, da, ko=1, bounds=(lo - 1000, hi + 777), tag=("wider",))
    for bounds in ((lo + 1, hi), (lo, hi - 1), (0, 10)):
        km = KeyMap(lib, dk, da, bounds=bounds)
        assert km.rc == mq.MQ_EINVAL and not km.h and "outside the bounds" in lib.mq_last_error().decode()
    k, a = Dev.of(dk), Dev.of(da)
    n1 = len(dk)
    h = C.c_void_p(1)
    assert lib.mq_keymap_build(k.ptr, a.ptr, n1, 1, 5, 4, C.byref(h), None, None) == mq.MQ_EINVAL and not h  # lo > hi
    h = C.c_void_p(1)
    assert lib.mq_keymap_build(k.ptr, a.ptr, 2**31, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL and not h
    assert lib.mq_keymap_build(None, a.ptr, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keymap_build(k.ptr, None, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keymap_build(k.ptr + 2, a.ptr, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keymap_build(k.ptr, a.ptr + 1, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_EINVAL
    assert lib.mq_keymap_build(k.ptr, a.ptr, 5, 0, 0, 0, None, None, None) == mq.MQ_EINVAL
    assert lib.mq_keymap_free(None) == mq.MQ_OK
    h = C.c_void_p()
    assert lib.mq_keymap_build(k.ptr, a.ptr, 5, 0, 0, 0, C.byref(h), None, None) == mq.MQ_OK and h  # h_info may be NULL
    assert lib.mq_keymap_free(h) == mq.MQ_OK


# ---------------------------------------------------------------------------
# the lookup
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [0, 1, 1025, 300_001])
def test_lookup(lib, k):
    """With and without positions; `missing` for the misses; d_hit_out may be NULL; nothing at
    or past entry k."""
    dk, da = gj.dimension("dense", 2048)
    km = KeyMap(lib, dk, da)
    try:
        assert km.rc == mq.MQ_OK
        n = k + 500
        f = gj.fact_keys("half_present", n, dk)
        pos = np.random.default_rng(k).integers(0, n, k).astype(np.int32)
        for off in (0, 1):
            df, dp = Dev.of(f, offset_elems=off), Dev.of(pos, offset_elems=1 - off)
            for missing in (0, wc.I32_MIN):
                device_lookup(lib, km.h, df.ptr, None, k, missing, gj.lookup(f[:k], dk, da, missing), (k, off, missing, "direct"))
                device_lookup(lib, km.h, df.ptr, dp.ptr, k, missing, gj.lookup(f[pos], dk, da, missing), (k, off, missing, "positions"))
            device_lookup(lib, km.h, df.ptr, dp.ptr, k, 5, gj.lookup(f[pos], dk, da, 5), (k, off, "no hits"), hits=False)
        df = Dev.of(f)
        out = Dev(4 * (k + PAD))
        assert lib.mq_keymap_lookup(None, df.ptr, None, k, 0, out.ptr, None, None) == mq.MQ_EINVAL
        assert lib.mq_keymap_lookup(km.h, df.ptr, None, 2**31, 0, out.ptr, None, None) == mq.MQ_EINVAL
        if k:
            assert lib.mq_keymap_lookup(km.h, None, None, k, 0, out.ptr, None, None) == mq.MQ_EINVAL
            assert lib.mq_keymap_lookup(km.h, df.ptr, None, k, 0, None, None, None) == mq.MQ_EINVAL
            assert lib.mq_keymap_lookup(km.h, df.ptr + 2, None, k, 0, out.ptr, None, None) == mq.MQ_EINVAL
    finally:
        km.free()
    empty = KeyMap(lib, [], [])
    try:
        assert empty.rc == mq.MQ_OK and empty.fields() == gj.info([], [])
        f = gj.fact_keys("half_present", max(k, 1), [])
        device_lookup(lib, empty.h, Dev.of(f).ptr, None, k, -9, gj.lookup(f[:k], [], [], -9), (k, "empty map"))
    finally:
        empty.free()


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------

def jplan(L, ptrs, ranges, dfk, km, dv, n, path, bounds=None, stream=None):
    """(rc, handle, groups, path taken, joined rows)"""
    h, groups, taken, rows = C.c_void_p(), C.c_uint64(12345), C.c_int(-1), C.c_uint64(54321)
    b = None if bounds is None else (C.c_int32 * 2)(*bounds)
    rc = L.mq_group_join_plan(c_ptrs(ptrs) if ptrs else None, c_ranges(ranges) if ranges else None, len(ptrs), dfk, km, dv, n, b,
                              path, C.byref(h), C.byref(groups), C.byref(taken), C.byref(rows), stream)
    return rc, h.value, groups.value, taken.value, rows.value


def read_all(L, h, g):
    outs = filled_outputs(L, g)
    mq.check(write(L, h, outs), "mq_group_write")
    return [outs[nm].get(DTYPE[nm], g) for nm in NAMES]


def run(L, ptrs, ranges, dfk, km, dv, n, path, want, tag, bounds=None, alone=False):
    """Plan, write into 0x5A-filled outputs, compare, free. alone: each output is also asked for
    by itself. Returns the path taken."""
    rc, h, g, taken, rows = jplan(L, ptrs, ranges, dfk, km, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[0]), tag + ("groups", g, len(want[0]))
    assert rows == int(want[1].sum()), tag + ("rows", rows)
    outs = filled_outputs(L, g)
    mq.check(write(L, h, outs), "mq_group_write")
    check_outputs(outs, g, want, tag)
    if alone:
        for i, nm in enumerate(NAMES):
            one = filled_outputs(L, g)
            args = [one[x].ptr if x == nm else None for x in NAMES]
            mq.check(L.mq_group_write(h, *args, None), "mq_group_write")
            got = one[nm].get(DTYPE[nm], g + PAD)
            assert np.array_equal(got[:g], want[i]), tag + ("alone", nm)
            for x in NAMES:
                if x != nm:  # the others stay filled
                    raw = one[x].get(np.uint8, one[x].nbytes)
                    assert np.all(raw == 0x5A), tag + ("alone", nm, "wrote", x)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken


def refused(L, ptrs, ranges, dfk, km, dv, n, path, bounds=None):
    rc, h, g, _, rows = jplan(L, ptrs, ranges, dfk, km, dv, n, path, bounds)
    return (rc, h, g, rows) == (mq.MQ_EINVAL, None, 0, 0) and bool(L.mq_last_error())


def run_paths(L, S, km, cols, ranges, fkey, vals, tag, offs=(0,), alone=False):
    """Every path the map's attribute range allows, against the model; AUTO's choice and the
    refusal of DENSE on a wider range are asserted. The outputs are the same bytes on both."""
    n = len(fkey)
    want = gj.model(cols, ranges, fkey, km.keys, km.attrs, vals)
    ptrs, keep = upload(list(cols) + [fkey, vals], offs)
    dfk, dv = ptrs[len(cols)], ptrs[-1]
    arange = int(km.info.attr_hi) - int(km.info.attr_lo) + 1 if len(km.keys) else 0
    dense_ok = arange <= S
    for path in (AUTO, DENSE, SORT) if dense_ok else (AUTO, SORT):
        taken = run(L, ptrs[:len(cols)], ranges, dfk, km.h, dv, n, path, want, tag + (path,), alone=alone and path != AUTO)
        settled = n == 0 or len(km.keys) == 0 or any(lo is not None and hi is not None and lo >= hi for lo, hi in ranges) or \
            any(hi == wc.I32_MIN for _, hi in ranges)
        if not settled:
            assert taken == (path if path != AUTO else DENSE if dense_ok else SORT), tag + (path, taken)
    if not dense_ok and n:
        assert refused(L, ptrs[:len(cols)], ranges, dfk, km.h, dv, n, DENSE), tag + ("DENSE forced past S",)
    return want


@pytest.fixture(scope="module")
def maps(lib):
    """The dense dimension under the three attribute cardinalities."""
    out = {card: KeyMap(lib, *gj.dimension("dense", card)) for card in gj.CARDS}
    assert all(m.rc == mq.MQ_OK for m in out.values())
    yield out
    for m in out.values():
        m.free()


@pytest.mark.parametrize("ncols", gj.NCOLS)
@pytest.mark.parametrize("n", [0, 1, 33, 1025, 8193])
def test_plan_agrees_with_the_model(lib, S, maps, n, ncols):
    """Dense and forced sort path, attribute cardinalities 1, 7 and 2048, wherecases' predicate
    sets and the fact key sets rotating along, columns 0 and 1 dword off a 16-byte boundary in
    turn, each output asked for alone and all together."""
    q = gj.NCOLS.index(ncols) + 4 * [0, 1, 33, 1025, 8193].index(n)
    for j, card in enumerate(gj.CARDS):
        km = maps[card]
        names = [wc.CASES[(3 * q + 7 * j + i) % len(wc.CASES)] for i in range(2)] + ["uniform_50"]
        for i, name in enumerate(names):
            cols, ranges = gj.case(name, n, ncols)
            fname = gj.FACT_SETS[(q + j + i) % len(gj.FACT_SETS)] if name != "uniform_50" else "half_present"
            fkey = gj.fact_keys(fname, n, km.keys)
            vals = gc.values_of(gc.VALUE_SETS[(q + i) % 3], fkey)
            offs = [(0,), (0, 1), (1, 0, 0), (1,)][(q + j + i) % 4]
            want = run_paths(lib, S, km, cols, ranges, fkey, vals, (n, ncols, card, name, fname), offs, alone=i == 2)
            if name == "uniform_50" and n >= 1025 and ncols <= 1:
                assert len(want[0]) >= min(card, 7), (n, ncols, card)  # no pass on an empty result


def test_plan_aliased_and_misaligned_columns(lib, S, maps):
    """The foreign key column is a predicate column and the value column; column pointers 1 to
    3 dwords off a 16-byte boundary."""
    km, n = maps[7], 8193
    fkey = gj.fact_keys("half_present", n, km.keys)
    other = np.ascontiguousarray(np.random.default_rng(3).integers(0, 1000, n), dtype=np.int32)
    for cols, ranges in (([fkey, other], [(-500, 1500), (100, 900)]), ([other, fkey, fkey], [(0, 800), (None, 1200), (-900, None)])):
        want = gj.model(cols, ranges, fkey, km.keys, km.attrs, fkey)
        assert len(want[0]) == 7
        for offs in ((0,), (1, 2), (3, 1), (2,)):
            ptrs, keep = upload(cols + [fkey], offs)
            for path in (DENSE, SORT):
                run(lib, ptrs[:len(cols)], ranges, ptrs[-1], km.h, ptrs[-1], n, path, want, ("aliased", len(cols), offs, path))


@pytest.mark.parametrize("name", gw.POISON_SETS)
def test_dead_rows_are_never_looked_at(lib, S, name):
    """groupwherecases' poison sets: every row that fails a predicate, in live lines and in
    whole dead lines, carries a foreign key whose attribute lies outside the bounds given, or a
    key outside the map's span: the plan succeeds on both paths, so no dead row reached the
    lookup or the tables. The same key in one live row is refused."""
    cols, ranges, keys, vals, (lo, hi) = gw.poisoned(name, S)
    n = len(keys)
    m = wc.mask(cols, ranges)
    # the dimension: the matching rows' keys map to themselves, four poison keys to attributes
    # outside [lo, hi]; the dead rows' other keys (both int32 ends among them) are no key at all
    poison = np.array([lo - 1, hi + 1, hi + S, lo - S], dtype=np.int64)
    dk = np.concatenate((np.arange(lo, hi + 1), poison)).astype(np.int32)
    da = dk.copy()
    km = KeyMap(lib, dk, da)
    try:
        assert km.rc == mq.MQ_OK
        both, dead = gw.line_census(m)
        assert (both > 0 or dead > 0) and np.isin(keys[~m], poison).any() and not np.isin(keys[~m], dk).all()
        want = gj.model(cols, ranges, keys, dk, da, vals)
        assert np.array_equal(want[0], gc.group(keys[m], vals[m])[0]) and len(want[0]) >= 1  # ends_only: two rows
        ptrs, keep = upload(cols + [keys, vals], (0, 1))
        for path in (DENSE, SORT):
            run(lib, ptrs[:2], ranges, ptrs[2], km.h, ptrs[3], n, path, want, (name, path), bounds=(lo, hi))
        live = keys.copy()
        live[np.flatnonzero(m)[len(want[0]) // 2]] = hi + 1  # a joined row whose attribute is out of bounds
        pl, keep2 = upload([live], (1,))
        for path in (DENSE, SORT):
            assert refused(lib, ptrs[:2], ranges, pl[0], km.h, ptrs[3], n, path, bounds=(lo, hi)), (name, path)
            assert "outside the bounds" in lib.mq_last_error().decode()
    finally:
        km.free()


def test_fact_keys_outside_the_span_and_given_bounds(lib, S, maps, chunk):
    """Fact keys outside the span in dead and in live rows, for every dimension set; attribute
    bounds wider than, equal to and narrower than the joined attributes."""
    n = 8193
    try:
        for dname in gj.DIM_SETS:
            dk, da = gj.dimension(dname, 7, chunk_words=chunk)
            km = KeyMap(lib, dk, da, ko=1)
            try:
                assert km.rc == mq.MQ_OK, dname
                for fname in ("outside_ends", "half_present"):
                    fkey = gj.fact_keys(fname, n, dk)
                    for ncols in (0, 2):
                        cols, ranges = gj.case("uniform_50", n, ncols)
                        run_paths(lib, S, km, cols, ranges, fkey, wc.values_of(n), (dname, fname, ncols), (0, 1))
            finally:
                km.free()
    finally:
        lib.mq_trim()
    km = maps[7]
    fkey = gj.fact_keys("half_present", n, km.keys)
    vals = wc.values_of(n)
    cols, ranges = gj.case("uniform_50", n, 1)
    want = gj.model(cols, ranges, fkey, km.keys, km.attrs, vals)
    lo, hi = int(want[0][0]), int(want[0][-1])
    assert (lo, hi) == (gj.ATTR_BASE, gj.ATTR_BASE + 6)
    ptrs, keep = upload(cols + [fkey, vals])
    for bounds in ((lo, hi), (lo - 100, hi + S - 200), (lo - 1, hi + 1)):
        for path in (AUTO, DENSE, SORT):
            run(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, path, want, ("bounds", bounds, path), bounds=bounds)
    run(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, AUTO, want, ("wide bounds",), bounds=(wc.I32_MIN, wc.I32_MAX))
    for bounds in ((lo + 1, hi), (lo, hi - 1), (hi + 1, hi + 5)):
        for path in (AUTO, DENSE, SORT):
            assert refused(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, path, bounds=bounds), (bounds, path)
    assert refused(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, AUTO, bounds=(5, 4))
    assert refused(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, DENSE, bounds=(lo, lo + S))  # S + 1 values
    assert refused(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], n, 3)
    assert refused(lib, ptrs[:1], ranges, ptrs[1], None, ptrs[2], n, AUTO)
    assert refused(lib, ptrs[:1], ranges, None, km.h, ptrs[2], n, AUTO)
    assert refused(lib, ptrs[:1], ranges, ptrs[1] + 2, km.h, ptrs[2], n, AUTO)
    assert refused(lib, ptrs[:1], ranges, ptrs[1], km.h, ptrs[2], 2**31, AUTO)
    assert refused(lib, ptrs * 3, ranges * 9, ptrs[1], km.h, ptrs[2], n, AUTO)  # ncols == 9


@pytest.mark.parametrize("n", [8193, gc.SORT_N_TWO_TILES])
def test_plan_sort_path(lib, S, n):
    """An attribute range of S + 1 and attributes at both ends of int32 take the sort path; a
    forced MQ_GROUP_SORT on a dense-sized range gives the dense path's bytes."""
    dk, _ = gj.dimension("dense", 7)
    rng = np.random.default_rng(n)
    big = n == gc.SORT_N_TWO_TILES  # every row joins: the sort path's K is n, two tiles in its first block
    fkey = gj.fact_keys("all_present" if big else "half_present", n, dk)
    vals = wc.values_of(n)
    col = np.ascontiguousarray(rng.integers(0, 1000, n), dtype=np.int32)
    ptrs, keep = upload([col, fkey, vals], (0, 1))
    for tag, da in (("S + 1", gj.attributes(dk, S + 1, seed=1)),
                    ("int32 ends", np.where(np.arange(len(dk)) % 3 == 0, wc.I32_MIN, np.where(np.arange(len(dk)) % 3 == 1, wc.I32_MAX, 5))),
                    ("dense-sized", gj.attributes(dk, 7, seed=2))):
        km = KeyMap(lib, dk, da)
        try:
            assert km.rc == mq.MQ_OK
            for cols, ranges, p in (([], [], []), ([col], [(100, 700)], ptrs[:1]))[:1 if big else 2]:
                want = gj.model(cols, ranges, fkey, km.keys, km.attrs, vals)
                assert int(want[1].sum()) == n if big else len(want[0]) >= 3
                dense_ok = tag == "dense-sized"
                for path in (AUTO, SORT, DENSE) if dense_ok else (AUTO, SORT):
                    taken = run(lib, p, ranges, ptrs[1], km.h, ptrs[2], n, path, want, (tag, n, len(cols), path))
                    assert taken == (SORT if path == SORT or not dense_ok else DENSE)
                if not dense_ok:
                    assert refused(lib, p, ranges, ptrs[1], km.h, ptrs[2], n, DENSE)
        finally:
            km.free()


@pytest.mark.parametrize("limit", [1, 2])
def test_many_iterations_a_block(lib, S, maps, limit):
    """wherecases.BIG rows on a grid of 1 or 2 CUs' blocks, ncols 0, 1 and 8, half of the keys
    present; and a wave-uniform run: a fact table sorted by key joined to 7 attributes."""
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        n = wc.BIG
        for ncols in (0, 1, 8):
            km = maps[2048 if ncols == 1 else 7]
            cols, ranges = gj.case("uniform_50" if ncols < 8 else "first_all", n, ncols)
            fkey = gj.fact_keys("half_present", n, km.keys)
            want = run_paths(lib, S, km, cols, ranges, fkey, wc.values_of(n), ("big", limit, ncols), (limit - 1, 1))
            assert int(want[1].sum()) > 100
        km = maps[7]
        srt = np.sort(gj.fact_keys("all_present", n, km.keys))
        dk_sorted = np.sort(km.keys)
        blocky = KeyMap(lib, dk_sorted, np.repeat(np.arange(7, dtype=np.int32) * 11, len(dk_sorted) // 7 + 1)[:len(dk_sorted)])
        try:
            assert blocky.rc == mq.MQ_OK
            want = run_paths(lib, S, blocky, [], [], srt, wc.values_of(n), ("runs", limit), (2 - limit,))
            assert len(want[0]) == 7 and int(want[1].min()) > 4 * 1024  # whole tiles of one attribute
        finally:
            blocky.free()
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


# ---------------------------------------------------------------------------
# cross-checks on the device
# ---------------------------------------------------------------------------

def test_equals_group_where_plan_when_the_join_drops_out(lib, S):
    """Every fact key present and attr == key: mq_group_where_plan on the key column, bit for
    bit, on both paths."""
    n = 70_001
    for keyset in ("uniform_100", "all_distinct"):
        keys = gc.keys_of(keyset, n, S)
        dk = np.unique(keys)
        km = KeyMap(lib, dk, dk)
        try:
            assert km.rc == mq.MQ_OK
            cols, ranges = wc.case("uniform_50", n, 2)
            vals = gc.values_of("uniform", keys)
            ptrs, keep = upload(cols + [keys, vals], (0, 1))
            for path in (AUTO, SORT):
                rc, h, g, taken, rows = wplan(lib, ptrs[:2], ranges, ptrs[2], ptrs[3], n, path)
                assert rc == mq.MQ_OK and g > 50
                ref = read_all(lib, h, g)
                mq.check(lib.mq_group_free(h), "mq_group_free")
                rc, h2, g2, taken2, rows2 = jplan(lib, ptrs[:2], ranges, ptrs[2], km.h, ptrs[3], n, path)
                assert (rc, g2, taken2, rows2) == (mq.MQ_OK, g, taken, rows), lib.mq_last_error()
                got = read_all(lib, h2, g2)
                mq.check(lib.mq_group_free(h2), "mq_group_free")
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), (keyset, path)
        finally:
            km.free()


def test_one_attribute_equals_semi_agg(lib, maps):
    """One constant attribute: the single group's count, sum, min and max are mq_semi_agg's on
    the map's own key set."""
    km, n = maps[1], 70_001
    fkey = gj.fact_keys("half_present", n, km.keys)
    vals = wc.values_of(n)
    ks = lib.mq_keymap_keyset(km.h)
    assert ks
    ws_bytes = lib.mq_semi_workspace_bytes(n)
    ws, agg = Dev(ws_bytes), Dev(32)
    for ncols in (0, 3):
        cols, ranges = gj.case("uniform_50", n, ncols)
        ptrs, keep = upload(list(cols) + [fkey, vals], (0, 1))
        rc = lib.mq_semi_agg(c_ptrs(ptrs[:ncols]) if ncols else None, c_ranges(ranges) if ncols else None, ncols, ptrs[ncols], ks, 0,
                             mq.MQ_SEMI_AUTO, ptrs[-1], n, agg.ptr, ws.ptr, ws_bytes, None)
        assert rc == mq.MQ_OK, lib.mq_last_error()
        a = mq.MqAgg.from_buffer_copy(agg.get(np.uint8, 32).tobytes())
        assert a.count > 100
        for path in (DENSE, SORT):
            rc, h, g, taken, rows = jplan(lib, ptrs[:ncols], ranges, ptrs[ncols], km.h, ptrs[-1], n, path)
            assert (rc, g, rows) == (mq.MQ_OK, 1, a.count), lib.mq_last_error()
            k, c, s, mn, mx = read_all(lib, h, 1)
            mq.check(lib.mq_group_free(h), "mq_group_free")
            assert (int(k[0]), int(c[0]), int(s[0]), int(mn[0]), int(mx[0])) == (gj.ATTR_BASE, a.count, a.sum, a.min, a.max)


def test_equals_the_hash_join_chain(lib, maps):
    """mq_hash_join -> mq_fetch x 2 -> mq_group_plan at 8193 rows, bit for bit."""
    km, n = maps[2048], 8193
    n1 = len(km.keys)
    fkey = gj.fact_keys("half_present", n, km.keys)
    vals = wc.values_of(n)
    df, dv = Dev.of(fkey), Dev.of(vals)
    p1, p2 = Dev.of(np.arange(n1, dtype=np.int32)), Dev.of(np.arange(n, dtype=np.int32))
    o1, o2, m = Dev(4 * n), Dev(4 * n), C.c_uint64()
    mq.check(lib.mq_hash_join(km.dk.ptr, p1.ptr, n1, df.ptr, p2.ptr, n, o1.ptr, o2.ptr, n, C.byref(m), None), "mq_hash_join")
    m = m.value
    assert 0 < m < n and m == int(np.isin(fkey, km.keys).sum())
    ja, jv = Dev(4 * m), Dev(4 * m)
    mq.check(lib.mq_fetch(km.da.ptr, o1.ptr, m, ja.ptr, None), "mq_fetch")
    mq.check(lib.mq_fetch(dv.ptr, o2.ptr, m, jv.ptr, None), "mq_fetch")
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    mq.check(lib.mq_group_plan(ja.ptr, jv.ptr, m, None, AUTO, C.byref(h), C.byref(g), C.byref(taken), None), "mq_group_plan")
    ref = read_all(lib, h, g.value)
    mq.check(lib.mq_group_free(h), "mq_group_free")
    assert g.value > 1000
    for path in (AUTO, SORT):
        rc, h2, g2, _, rows = jplan(lib, [], [], df.ptr, km.h, dv.ptr, n, path)
        assert (rc, g2, rows) == (mq.MQ_OK, g.value, m), lib.mq_last_error()
        got = read_all(lib, h2, g2)
        mq.check(lib.mq_group_free(h2), "mq_group_free")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), path


# ---------------------------------------------------------------------------
# the drop-in
# ---------------------------------------------------------------------------

def fused(L, objs, ranges, fkeys, dim_keys, dim_attrs, values, ncols=None):
    """group_aggregate_join -> (status, the five Results as (data_type, numpy array) or None)"""
    keep = where_args(objs, ranges) if objs else (None, None, None, None)
    gs = [gcol(o) for o in (fkeys, dim_keys, dim_attrs, values)]
    st = mq.Status(0, None)
    rpp = L.group_aggregate_join(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, *[C.byref(g) for g in gs],
                                 C.byref(st))
    return (st.code, five(rpp)) if rpp else (st.code, None)


def test_dropin(lib, S, capfd):
    """Columns and INT Results as input, ncols 0 and 2, an empty and a non-unique dimension; the
    five Results' types, lengths and contents, freed through the existing helpers."""
    n = 70_001
    dk, da = gj.dimension("dense", 2048)
    fkey = gj.fact_keys("half_present", n, dk)
    vals = wc.values_of(n)
    cols, ranges = wc.case("uniform_50", n, 2)
    cc, cf, cv, cdk, cda = [make_column(c) for c in cols], make_column(fkey), make_column(vals), make_column(dk), make_column(da)
    for objs, rg, model_cols in ((cc, ranges, cols), ([], [], [])):
        want = gj.model(model_cols, rg, fkey, dk, da, vals)
        assert len(want[0]) > 1000
        code, out = fused(lib, objs, rg, cf, cdk, cda, cv)
        assert code == mq.OK
        check_results(out, want, ("columns", len(objs)))
    # INT Results: two with an HBM shadow, two of the caller's own
    st = mq.Status(0, None)
    every, every1 = make_result(np.arange(n, dtype=np.int32)), make_result(np.arange(len(dk), dtype=np.int32))
    rf = lib.fetch_column(C.byref(cf), C.byref(every), C.byref(st))
    rk = lib.fetch_column(C.byref(cdk), C.byref(every1), C.byref(st))
    assert st.code == mq.OK and rf and rk
    ra, rv = make_result(da), make_result(vals)
    code, out = fused(lib, cc, ranges, rf, rk, ra, rv)
    assert code == mq.OK
    check_results(out, gj.model(cols, ranges, fkey, dk, da, vals), ("results",))
    # a wide attribute range: the sort path behind the same call
    da_wide = da * 1000  # a Column does not own its rows: the array stays named
    wide = make_column(da_wide)
    code, out = fused(lib, [], [], cf, cdk, wide, cv)
    assert code == mq.OK
    check_results(out, gj.model([], [], fkey, dk, da_wide, vals), ("sort path",))
    # an empty dimension: five empty Results and OK
    e = np.empty(0, np.int32)
    ce = make_column(e)
    code, out = fused(lib, cc, ranges, cf, ce, ce, cv)
    assert code == mq.OK
    check_results(out, gc.group(e, e), ("empty dimension",))
    capfd.readouterr()

    def refused_dropin(call):
        return call == (mq.ERROR, None) and "libmq" in capfd.readouterr().err

    twice = dk.copy()
    twice[17] = twice[400]
    ct = make_column(twice)
    assert refused_dropin(fused(lib, cc, ranges, cf, ct, cda, cv))          # not a primary key
    da_short = da[:-1].copy()
    short = make_column(da_short)
    assert refused_dropin(fused(lib, cc, ranges, cf, cdk, short, cv))       # dim_keys and dim_attrs differ in length
    assert refused_dropin(fused(lib, cc, ranges, cf, cdk, cda, cdk))        # values as long as the dimension
    assert refused_dropin(fused(lib, cc * 5, ranges * 5, cf, cdk, cda, cv, ncols=9))
    lng = make_result(da.astype(np.int64), mq.LONG)
    assert refused_dropin(fused(lib, cc, ranges, cf, cdk, lng, cv))         # a LONG Result as attributes
    code, out = fused(lib, cc, ranges, cf, cdk, cda, cv)                    # and the operator still works
    assert code == mq.OK
    check_results(out, gj.model(cols, ranges, fkey, dk, da, vals), ("after the errors",))
    for r in (rf, rk):
        take(r)
    for r in (every, every1, ra, rv, lng):
        free_result_struct(r)
    for c in cc + [cf, cv, cdk, cda, wide, ce, ct, short]:
        lib.mq_column_invalidate(C.byref(c))
