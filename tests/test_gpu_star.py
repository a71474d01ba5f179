"""group_aggregate_star on gfx950 (k_star_mask and mq_star_positions in csrc/mq_where.hip;
k_group_star_dense, k_group_star_pack_pos and mq_group_star_plan in csrc/mq_group.hip;
group_aggregate_star in mq_query.c), every comparison exact equality: with the numpy restatement
in starcases.py, and through libmq itself with mq_group_join_plan, mq_group_by_where_plan,
mq_semi_agg, mq_semi_positions and the chain mq_keymap_lookup -> mq_group_by_where_plan that the
operator replaces.

Rows: a 32-row line, a 256-row wave tile, the 1024-row tile and the unrolled iteration of every
number of terms (4, 4, 3 and 2 tiles) each +-1, 70 001 rows for several blocks, 300 001 rows on
one or two CUs for many iterations a block.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import groupbycases as gb
import groupjoincases as gj
import starcases as sc
import wherecases as wc
from devbuf import Dev
from refapi import make_column, make_result, free_result_struct, mq, take
from test_gpu_group_by_where import AGGS, DTYPE, check_outputs, check_results, out_buffers, results
from test_gpu_group_by_where import write as by_write
from test_gpu_group_join import KeyMap, jplan
from test_gpu_group_where import NAMES, S, c_ptrs, c_ranges, filled_outputs, gcol, lib, upload, where_args  # noqa: F401
from test_gpu_group_where import DTYPE as DTYPE1
from test_gpu_where import PAD, SENT

pytestmark = pytest.mark.gpu

AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
TILE = 1024
IN_FLIGHT = {1: 4, 2: 4, 3: 3, 4: 2}  # tiles of an unrolled iteration by number of terms
SIZES = sorted({0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70_001} |
               {u * TILE + d for u in IN_FLIGHT.values() for d in (-1, 0, 1)})
PATHS = {"dense": DENSE, "sort": SORT}


class Star:
    """The device side of a list of starcases.Term: every distinct column uploaded once (the
    k-th one offs[k % len(offs)] dwords off a 16-byte boundary), a key map per "km" and a key
    set per "ks" term built here unless the term brings a handle in extra["h"]."""

    def __init__(self, L, terms, offs=(0,), devs=None):
        self.lib, self.terms, self.maps, self.sets = L, terms, [], []
        self.devs = {} if devs is None else devs
        self.arr = (mq.MqStarTerm * max(len(terms), 1))()
        for j, t in enumerate(terms):
            if id(t.col) not in self.devs:
                self.devs[id(t.col)] = Dev.of(t.col, offset_elems=offs[len(self.devs) % len(offs)])
            km = ks = None
            if "h" in t.extra:
                km, ks = (t.extra["h"], None) if t.kind == "km" else (None, t.extra["h"])
            elif t.kind == "km":
                m = KeyMap(L, t.dim_keys, t.dim_attrs, ko=j % 4, ao=(j + 1) % 4)
                assert m.rc == mq.MQ_OK, L.mq_last_error()
                self.maps.append(m)
                km = m.h.value
            elif t.kind == "ks":
                keys = np.ascontiguousarray(t.dim_keys, np.int32)
                dk, h = Dev.of(keys), C.c_void_p()
                mq.check(L.mq_keyset_build(dk.ptr if len(keys) else None, len(keys), 0, 0, 0, C.byref(h), None, None), "mq_keyset_build")
                self.sets.append(h)
                ks = h.value
            self.arr[j] = mq.MqStarTerm(self.devs[id(t.col)].ptr, km, ks)
        self.nkeys = sc.nkeys_of([t.kind for t in terms])

    def ptr(self, arr):
        return self.devs[id(arr)].ptr

    def free(self):
        mq.check(self.lib.mq_device_sync(), "device sync")
        for m in self.maps:
            m.free()
        for h in self.sets:
            assert self.lib.mq_keyset_free(h) == mq.MQ_OK
        self.maps, self.sets = [], []


def splan(L, ptrs, ranges, star, dv, n, path, bounds=None, nterms=None, stream=None):
    """(rc, handle, groups, path taken, joined rows)"""
    h, groups, taken, rows = C.c_void_p(77), C.c_uint64(12345), C.c_int(-1), C.c_uint64(54321)
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    rc = L.mq_group_star_plan(c_ptrs(ptrs) if ptrs else None, c_ranges(ranges) if ranges else None, len(ptrs), star.arr,
                              len(star.terms) if nterms is None else nterms, dv, n, b, path, C.byref(h), C.byref(groups),
                              C.byref(taken), C.byref(rows), stream)
    return rc, h.value, groups.value, taken.value, rows.value


def refused(L, *args, **kw):
    rc, h, g, _, rows = splan(L, *args, **kw)
    return (rc, h, g, rows) == (mq.MQ_EINVAL, None, 0, 0) and b"mq_group_star_plan" in L.mq_last_error()


def read_raw(L, h, g, nkeys):
    """The outputs of mq_group_by_write as bytes (it serves a one-key handle too)."""
    keys, aggs = out_buffers(g, nkeys)
    mq.check(by_write(L, h, keys, aggs), "mq_group_by_write")
    return [k.get(np.int32, g).tobytes() for k in keys] + [aggs[nm].get(DTYPE[nm], g).tobytes() for nm in AGGS]


def run(L, ptrs, ranges, star, dv, n, path, want, tag, bounds=None):
    """Plan, write into sentinel-filled outputs of g + PAD entries, compare, free. Returns
    (path taken, the outputs' bytes)."""
    rc, h, g, taken, rows = splan(L, ptrs, ranges, star, dv, n, path, bounds)
    assert rc == mq.MQ_OK and h, tag + (L.mq_last_error(),)
    assert g == len(want[1]), tag + ("groups", g, len(want[1]))
    assert rows == int(want[1].sum()), tag + ("rows", rows)
    keys, aggs = out_buffers(g, star.nkeys)
    mq.check(by_write(L, h, keys, aggs), "mq_group_by_write")
    check_outputs(keys, aggs, g, want, tag)
    raw = read_raw(L, h, g, star.nkeys)
    mq.check(L.mq_group_free(h), "mq_group_free")
    return taken, raw


def run_paths(L, cols, ranges, terms, vals, tag, offs=(0,), bounds=None, dense_ok=True, star=None, want=None):
    """DENSE (where the key space allows), SORT and AUTO against the model; DENSE and SORT give
    the same bytes; AUTO takes the dense path exactly when it is allowed."""
    n = len(vals)
    want = sc.model(cols, ranges, terms, vals) if want is None else want
    devs = {}
    ptrs, keep = upload(list(cols) + [vals], offs) if star is None else (None, None)
    own = star is None
    if own:
        for a, p in zip(list(cols) + [vals], ptrs):
            devs[id(a)] = type("P", (), {"ptr": p})()
        star = Star(L, terms, offs, devs)
    try:
        pc, dv = [star.ptr(c) for c in cols], star.ptr(vals)
        raws = {}
        for path in (DENSE, SORT, AUTO) if dense_ok else (SORT, AUTO):
            taken, raws[path] = run(L, pc, ranges, star, dv, n, path, want, tag + (path,), bounds)
            settled = n == 0 or any(t.kind != "plain" and len(t.dim_keys) == 0 for t in terms)
            if not settled:
                assert taken == (path if path != AUTO else DENSE if dense_ok else SORT), tag + (path, taken)
        if dense_ok:
            assert raws[DENSE] == raws[SORT], tag + ("dense and sort differ",)
        elif n:
            assert refused(L, pc, ranges, star, dv, n, DENSE, bounds), tag + ("DENSE forced past the slots",)
    finally:
        if own:
            star.free()
    return want


def all_spaces():
    return [(layout, cards, path) for layout, kinds in sc.LAYOUTS.items() for cards, path in sc.SPACES[sc.nkeys_of(kinds)]]


# ---------------------------------------------------------------------------
# the plan against the model
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_sizes_and_alignment(lib, S, layout):
    """Every size of SIZES, the columns 0 to 3 dwords off a 16-byte boundary in turn (both VEC
    forms), the layout's first (dense) attribute space, no range and two."""
    kinds = sc.LAYOUTS[layout]
    cards, _ = sc.SPACES[sc.nkeys_of(kinds)][0]
    assert IN_FLIGHT[len(kinds)] * TILE + 1 in SIZES
    for i, n in enumerate(SIZES):
        terms = sc.make(layout, cards, n, seed=2)
        ncols = (0, 2)[i % 2]
        cols, ranges = sc.case("uniform_50", n, ncols)
        offs = [(0,), (1,), (2, 0), (3, 1, 0)][i % 4]
        bounds = sc.bounds_of(cards) if n < 2 else None  # too few rows to span a plain component's bounds
        run_paths(lib, cols, ranges, terms, wc.values_of(n), (layout, n, offs), offs, bounds=bounds)


@pytest.mark.parametrize("ncols", gj.NCOLS)
@pytest.mark.parametrize("layout,cards,path", all_spaces())
def test_layouts_agree_with_the_model(lib, S, layout, cards, path, ncols):
    """Every term layout x attribute space (P on both sides of the switch) x number of ranges
    at 70 001 rows, on every path the space allows."""
    n = 70_001
    q = gj.NCOLS.index(ncols)
    terms = sc.make(layout, cards, n, seed=1)
    cols, ranges = sc.case(["uniform_50", "uniform_10", "sorted_lead", "uniform_50"][q], n, ncols)
    space = int(np.prod(cards))
    assert (space <= S) == (path == "dense")
    want = run_paths(lib, cols, ranges, terms, wc.values_of(n), (layout, cards, ncols), [(0,), (0, 1), (1,), (2, 3)][q],
                     dense_ok=path == "dense")
    assert len(want[1]) >= 1 and int(want[1].sum()) < n  # a joined row and a dropped row (test_star_host.py checks the cases)


def test_term_interplay(lib, S):
    """Rows that hit term 0 and miss term 1 and the reverse; whole 32-row lines that miss term 0
    while term 1's column there holds both ends of int32 and keys just outside its span; the
    same column in two terms with different maps; d_vals equal to a term's column."""
    n = 3 * TILE + 100
    cards = (32, 64)
    terms = sc.make("km_km", cards, n, seed=3, miss=0.3)
    t0, t1 = terms
    h0, h1 = np.isin(t0.col, t0.dim_keys), np.isin(t1.col, t1.dim_keys)
    assert (h0 & ~h1).any() and (~h0 & h1).any() and (h0 & h1).any()
    vals = wc.values_of(n)
    want = run_paths(lib, [], [], terms, vals, ("interplay",), (0, 1))
    # whole lines that miss term 0; term 1's column is poisoned there
    c0, c1 = t0.col.copy(), t1.col.copy()
    lo1, hi1 = int(t1.dim_keys.min()), int(t1.dim_keys.max())
    poison = np.array([wc.I32_MIN, wc.I32_MAX, lo1 - 1, hi1 + 1, lo1 - 2, hi1 + 2], dtype=np.int64)
    absent0 = gj.absent_keys(t0.dim_keys)
    for line in (0, 5, 31, 32, 64, 95, (n - 1) // 32):
        rows = slice(32 * line, min(32 * line + 32, n))
        c0[rows] = absent0[line % len(absent0)]
        c1[rows] = poison[np.arange(rows.stop - rows.start) % len(poison)]
    dead = ~np.isin(c0, t0.dim_keys)
    p0 = sc.Term("km", c0, t0.dim_keys, t0.dim_attrs)
    clean = [p0, sc.Term("km", np.where(dead, t1.dim_keys[0], c1).astype(np.int32), t1.dim_keys, t1.dim_attrs)]
    dirty = [p0, sc.Term("km", np.ascontiguousarray(c1, np.int32), t1.dim_keys, t1.dim_attrs)]
    ref = sc.model([], [], clean, vals)
    got = run_paths(lib, [], [], dirty, vals, ("poisoned lines",), (1, 0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0] + list(got[1:]), ref[0] + list(ref[1:])))
    # the same column under two different maps, and as the values
    d2k, d2a = sc.dimension(77, 64, sc.COMP_BASE[1])
    d2k = (d2k.astype(np.int64) - int(d2k.min()) + int(t0.dim_keys.min())).astype(np.int32)  # over term 0's span
    twice = [t0, sc.Term("km", t0.col, d2k, d2a)]
    assert (np.isin(t0.col, t0.dim_keys) & np.isin(t0.col, d2k)).any()
    run_paths(lib, [], [], twice, vals, ("one column, two maps",), (2,))
    run_paths(lib, [], [], terms, t1.col, ("values are a term's column",), (0, 3))
    run_paths(lib, [t0.col], [(int(t0.dim_keys.min()), 0)], [sc.Term("plain", terms[0].col % 7), t1], t0.col, ("aliased",), (1,),
              bounds=[-6, 6, sc.COMP_BASE[1], sc.COMP_BASE[1] + 63])
    assert len(want[1]) > 100


@pytest.fixture(scope="module")
def chunk(lib):
    b, c = C.c_uint32(), C.c_uint64()
    lib.mq_keymap_geometry(gj.WORD_EDGES_SPAN, C.byref(b), C.byref(c))
    return c.value


@pytest.mark.parametrize("dname", gj.DIM_SETS)
def test_dimension_sets(lib, S, chunk, dname):
    """One term takes each named dimension of groupjoincases (both ends of int32, a span past
    2^31, keys around word and chunk edges, the empty one) beside a dense second dimension; as a
    map and, except for the 1.5 GiB one, as a filtering set; fact sets half_present and
    outside_ends."""
    n = 8193
    dk, da = gj.dimension(dname, 7, chunk_words=chunk)
    dk2, da2 = gj.dimension("dense", 64)
    vals = wc.values_of(n)
    try:
        for fname in ("half_present", "outside_ends"):
            f1, f2 = gj.fact_keys(fname, n, dk), gj.fact_keys("half_present", n + 1, dk2)[:n].copy()
            second = sc.Term("km", f2, dk2, da2)
            kinds = ("km",) if dname == "int32_ends" and fname == "outside_ends" else ("km", "ks")
            if dname == "int32_ends" and fname == "half_present":
                kinds = ("ks",)  # the map of the full span is built once
            for kind in kinds:
                first = sc.Term(kind, f1, dk, da if kind == "km" else None)
                star = Star(lib, [first, second, sc.Term("plain", vals)], (0, 1))
                try:
                    h = [star.arr[0].km or star.arr[0].ks, star.arr[1].km]
                    turned = [sc.Term("km", f2, dk2, da2, {"h": h[1]}), sc.Term(kind, f1, dk, first.dim_attrs, {"h": h[0]})]
                    back = Star(lib, turned, devs=star.devs)
                    for st, terms in ((star, [first, second]), (back, turned)):
                        st.terms, st.nkeys = terms, sc.nkeys_of([t.kind for t in terms])
                        want = run_paths(lib, [], [], terms, vals, (dname, fname, kind), star=st)
                        assert len(want[1]) == 0 if dname == "empty" else not gj.promises(fname, dname)[0] or len(want[1]) >= 1
                finally:
                    star.free()
    finally:
        lib.mq_trim()


@pytest.mark.parametrize("drop", [False, True])
def test_the_run_fold(lib, S, drop):
    """Foreign keys constant over stretches of 3 tiles + 100 rows: whole waves share a tuple and
    the tuple changes inside a block; with one dropped row inside a stretch."""
    stretch, reps = 3 * TILE + 100, 9
    n = stretch * reps
    t = sc.make("km_plain_km", (8, 16, 16), reps, seed=4, miss=0.0)
    terms = [sc.Term(x.kind, np.repeat(x.col, stretch), x.dim_keys, x.dim_attrs) for x in t]
    if drop:
        terms[2].col[4 * stretch + 1500] = gj.absent_keys(terms[2].dim_keys)[0]
        terms[0].col[stretch + 7] = wc.I32_MAX
    vals = wc.values_of(n)
    want = run_paths(lib, [], [], terms, vals, ("runs", drop), (0, 1), bounds=sc.bounds_of((8, 16, 16)))
    assert int(want[1].sum()) == n - 2 * drop and int(want[1].max()) >= stretch - 1 and len(want[1]) <= reps


@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("layout", ["km_km", "ks_km_plain_km"])
def test_many_iterations_a_block(lib, S, layout, limit):
    """300 001 rows on a grid of 1 or 2 CUs' blocks: the unrolled loop of 2 and of 4 terms runs
    many times a block."""
    n = wc.BIG
    cards, _ = sc.SPACES[sc.nkeys_of(sc.LAYOUTS[layout])][0]
    terms = sc.make(layout, cards, n, seed=6)
    cols, ranges = sc.case("uniform_50", n, limit - 1)
    mq.check(lib.mq_test_set_cu_limit(limit), "mq_test_set_cu_limit")
    try:
        want = run_paths(lib, cols, ranges, terms, wc.values_of(n), ("big", layout, limit), (limit - 1, 1))
        assert int(want[1].sum()) > 1000
    finally:
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


# ---------------------------------------------------------------------------
# bounds, order, arguments
# ---------------------------------------------------------------------------

def pool_blocks(L, sizes):
    """The idle blocks the pool hands out for `sizes`, returned to it at once: its state as its
    reuse rule shows it (test_build_refuses_a_repeated_key_and_releases_everything). The plan
    frees some blocks in its stream's order: a block whose free is still in flight is passed
    over, so the device is synchronised first."""
    mq.check(L.mq_device_sync(), "device sync")
    ps = []
    for b in sizes:
        p = C.c_void_p()
        mq.check(L.mq_pool_malloc(C.byref(p), b), "mq_pool_malloc")
        ps.append(p.value)
    for p in ps:
        mq.check(L.mq_pool_free(p), "mq_pool_free")
    return ps


def test_bounds(lib, S):
    n = 8193
    cards = (32, 64)
    terms = sc.make("plain_km", cards, n, seed=7)
    vals = wc.values_of(n)
    want = sc.model([], [], terms, vals)
    exact = [int(want[0][0].min()), int(want[0][0].max()), int(want[0][1].min()), int(want[0][1].max())]
    assert exact == sc.bounds_of(cards)
    star = Star(lib, terms + [sc.Term("plain", vals)], (0, 1))
    star.terms, star.nkeys = terms, 2  # the values ride along as an uploaded column
    try:
        dv = star.ptr(vals)
        for b in (exact, [exact[0] - 3, exact[1], exact[2], exact[3] + 1], [exact[0] - 20, exact[1] + 10, exact[2] - 1, exact[3]]):
            space = gb.space_of(b)
            run_paths(lib, [], [], terms, vals, ("bounds", tuple(b)), bounds=b, dense_ok=space <= S, star=star, want=want)
        # a joined row's component outside its bounds: refused, everything released
        sizes = [16 + 2048 * 28, 4 * n, lib.mq_semi_workspace_bytes(n), 8]
        lib.mq_trim()
        before = pool_blocks(lib, sizes)
        for b in ([exact[0] + 1] + exact[1:], exact[:3] + [exact[3] - 1], [exact[0], exact[0], exact[2], exact[3]]):
            for path in (AUTO, DENSE, SORT):
                assert refused(lib, [], [], star, dv, n, path, b), (b, path)
                assert b"outside its bounds" in lib.mq_last_error()
        assert pool_blocks(lib, sizes) == before
        assert refused(lib, [], [], star, dv, n, AUTO, [5, 4] + exact[2:])                            # lo > hi
        assert refused(lib, [], [], star, dv, n, AUTO, [wc.I32_MIN, wc.I32_MAX, exact[2], exact[3]])  # P > 2^32
        assert refused(lib, [], [], star, dv, n, DENSE, [exact[0], exact[1], exact[2], exact[2] + 64])  # 32 x 65 > 2048
        run_paths(lib, [], [], terms, vals, ("after the refusals",), bounds=exact, star=star, want=want)
    finally:
        star.free()
    # the same stray value on a row that is not joined is fine; on a joined row it is refused
    pcol, kcol = terms[0].col.copy(), terms[1].col
    miss = np.flatnonzero(~np.isin(kcol, terms[1].dim_keys))
    hit = np.flatnonzero(np.isin(kcol, terms[1].dim_keys))
    pcol[miss[:5]] = [exact[1] + 1, exact[0] - 1, wc.I32_MIN, wc.I32_MAX, exact[1] + 1000]
    stray = [sc.Term("plain", pcol), terms[1]]
    assert sc.model([], [], stray, vals)[1].tobytes() == want[1].tobytes()
    run_paths(lib, [], [], stray, vals, ("stray in a dropped row",), (1,), bounds=exact)
    pcol2 = terms[0].col.copy()
    pcol2[hit[len(hit) // 2]] = exact[1] + 1
    star2 = Star(lib, [sc.Term("plain", pcol2), terms[1], sc.Term("plain", vals)])
    star2.terms, star2.nkeys = star2.terms[:2], 2
    try:
        for path in (DENSE, SORT):
            assert refused(lib, [], [], star2, star2.ptr(vals), n, path, exact), path
    finally:
        star2.free()


def test_row_code_checks_every_component(lib, S):
    """(3, 12) under ranges (10, 10) sums to code 42, inside the table: refused all the same."""
    n = 5 * TILE + 5
    a = (np.arange(n) % 10).astype(np.int32)
    b = ((np.arange(n) // 10) % 10).astype(np.int32)
    vals = wc.values_of(n)
    terms = [sc.Term("plain", a), sc.Term("plain", b)]
    bounds = [0, 9, 0, 9]
    run_paths(lib, [], [], terms, vals, ("in bounds",), bounds=bounds)
    for row in (7, 4 * TILE + 3, n - 1):  # a tile of the unrolled loop, a single tile, the ragged tile
        a2, b2 = a.copy(), b.copy()
        a2[row], b2[row] = 3, 12
        star = Star(lib, [sc.Term("plain", a2), sc.Term("plain", b2), sc.Term("plain", vals)])
        star.terms, star.nkeys = star.terms[:2], 2
        try:
            for path in (DENSE, SORT):
                assert refused(lib, [], [], star, star.ptr(vals), n, path, bounds), (row, path)
        finally:
            star.free()


def test_order_of_the_terms(lib, S):
    """A ks term anywhere among the others leaves every output unchanged; permuting the
    component terms permutes the key outputs and reorders the rows as the model says."""
    n = 8193
    base = sc.make("ks_km_plain_km", (2, 4, 16, 16)[:3], n, seed=8)
    ks, comps = base[0], base[1:]
    vals = wc.values_of(n)
    cols, ranges = sc.case("uniform_50", n, 2)
    ref = None
    for at in range(4):
        terms = comps[:at] + [ks] + comps[at:]
        want = run_paths(lib, cols, ranges, terms, vals, ("ks at", at), (0, 1))
        raw = [k.tobytes() for k in want[0]] + [w.tobytes() for w in want[1:]]
        assert ref is None or raw == ref
        ref = raw
    assert len(want[1]) > 50
    seen = set()
    for perm in itertools.permutations(range(3)):
        terms = [ks] + [comps[j] for j in perm]
        want = run_paths(lib, cols[::-1], ranges[::-1], terms, vals, ("perm", perm), (1,))
        seen.add(tuple(k.tobytes() for k in want[0]))
        m = sc.joined(cols, ranges, terms)
        assert int(want[1].sum()) == int(m.sum())
    assert len(seen) == 6


def test_arguments(lib, S):
    """Every MQ_EINVAL of the header, with *out == NULL and *h_groups == 0, and what is settled
    on the host."""
    n = 1025
    terms = sc.make("ks_km", (64,), n, seed=9)
    vals = wc.values_of(n)
    cols, ranges = sc.case("uniform_50", n, 1)
    ptrs, keep = upload(list(cols) + [vals])
    star = Star(lib, terms)
    try:
        pc, dv = ptrs[:1], ptrs[1]
        assert splan(lib, pc, ranges, star, dv, n, AUTO)[0] == mq.MQ_OK
        for nt in (0, -1, 5):
            assert refused(lib, pc, ranges, star, dv, n, AUTO, nterms=nt)
        assert refused(lib, pc, ranges, star, dv, n, 3)
        assert refused(lib, pc, ranges, star, dv, 2**31, AUTO)
        assert refused(lib, pc, ranges, star, None, n, AUTO)
        assert refused(lib, pc, ranges, star, dv + 2, n, AUTO)
        assert refused(lib, [pc[0] + 1], ranges, star, dv, n, AUTO)
        assert refused(lib, pc * 9, ranges * 9, star, dv, n, AUTO)
        h, g = C.c_void_p(5), C.c_uint64(5)
        assert lib.mq_group_star_plan(None, None, 0, None, 2, dv, n, None, AUTO, C.byref(h), C.byref(g), None, None, None) == mq.MQ_EINVAL
        assert not h and g.value == 0
        assert lib.mq_group_star_plan(None, None, 0, star.arr, 2, dv, n, None, AUTO, None, C.byref(g), None, None, None) == mq.MQ_EINVAL
        assert lib.mq_group_star_plan(c_ptrs(pc), None, 1, star.arr, 2, dv, n, None, AUTO, C.byref(h), C.byref(g), None, None, None) == mq.MQ_EINVAL
        keep_arr = [mq.MqStarTerm(t.d_col, t.km, t.ks) for t in star.arr]
        try:
            star.arr[1] = mq.MqStarTerm(keep_arr[1].d_col, keep_arr[1].km, keep_arr[0].ks)  # both a map and a set
            assert refused(lib, pc, ranges, star, dv, n, AUTO)
            star.arr[1] = mq.MqStarTerm(keep_arr[1].d_col, None, keep_arr[0].ks)            # terms that are all ks
            assert refused(lib, pc, ranges, star, dv, n, AUTO)
            star.arr[1] = mq.MqStarTerm(None, keep_arr[1].km, None)                         # a NULL column
            assert refused(lib, pc, ranges, star, dv, n, AUTO)
            star.arr[1] = mq.MqStarTerm(keep_arr[1].d_col + 2, keep_arr[1].km, None)        # misaligned
            assert refused(lib, pc, ranges, star, dv, n, AUTO)
        finally:
            star.arr[1] = keep_arr[1]
        # settled on the host: no rows, an unsatisfiable range, an empty set: zero groups and a handle to free
        empty = Star(lib, [sc.Term("ks", terms[0].col, np.empty(0, np.int32)), sc.Term("km", terms[1].col, extra={"h": star.arr[1].km})],
                     devs=star.devs)
        try:
            for args, path in (((pc, ranges, star, dv, 0), AUTO), ((pc, [(5, 5)], star, dv, n), SORT), (([], [], empty, dv, n), DENSE)):
                rc, h, g, taken, rows = splan(lib, *args, path)
                assert (rc, g, rows) == (mq.MQ_OK, 0, 0) and h and taken == (SORT if path == SORT else DENSE)
                assert lib.mq_group_write(h, None, None, None, None, None, None) == mq.MQ_OK
                mq.check(lib.mq_group_free(h), "mq_group_free")
        finally:
            empty.free()
    finally:
        star.free()


def test_handle(lib, S):
    """Write twice; any output NULL; one component through mq_group_write, several through
    mq_group_by_write (mq_group_write refuses their keys); free."""
    n = 8193
    for layout, cards in (("ks_km", (64,)), ("km_plain_km", (8, 16, 16))):
        terms = sc.make(layout, cards, n, seed=10)
        vals = wc.values_of(n)
        want = sc.model([], [], terms, vals)
        star = Star(lib, terms + [sc.Term("plain", vals)])
        star.terms, star.nkeys = terms, len(cards)
        try:
            for path in (DENSE, SORT):
                rc, h, g, taken, rows = splan(lib, [], [], star, star.ptr(vals), n, path)
                assert rc == mq.MQ_OK and g == len(want[1]) and taken == path
                for _ in range(2):
                    keys, aggs = out_buffers(g, star.nkeys)
                    mq.check(by_write(lib, h, keys, aggs), "mq_group_by_write")
                    check_outputs(keys, aggs, g, want, (layout, path))
                for skip in AGGS:
                    keys, aggs = out_buffers(g, star.nkeys, skip_keys=(0,), skip=(skip,))
                    mq.check(by_write(lib, h, keys, aggs), "mq_group_by_write")
                    check_outputs(keys, aggs, g, want, (layout, path, "without", skip))
                keys, aggs = out_buffers(g, star.nkeys)
                mq.check(by_write(lib, h, keys, aggs, keys_null=True), "mq_group_by_write")
                check_outputs(keys, aggs, g, want, (layout, path, "no keys"), keys_written=False)
                outs = filled_outputs(lib, g)
                if star.nkeys == 1:
                    mq.check(lib.mq_group_write(h, *[outs[nm].ptr for nm in NAMES], None), "mq_group_write")
                    for nm, w in zip(NAMES, [want[0][0]] + list(want[1:])):
                        got = outs[nm].get(DTYPE1[nm], g + PAD)
                        assert np.array_equal(got[:g], w) and np.all(got[g:].view(np.uint8) == 0x5A), (layout, path, nm)
                else:
                    assert lib.mq_group_write(h, *[outs[nm].ptr for nm in NAMES], None) == mq.MQ_EINVAL
                    mq.check(lib.mq_group_write(h, None, *[outs[nm].ptr for nm in NAMES[1:]], None), "mq_group_write")
                    assert np.array_equal(outs["count"].get(np.uint64, g), want[1])
                mq.check(lib.mq_group_free(h), "mq_group_free")
        finally:
            star.free()


# ---------------------------------------------------------------------------
# cross-checks through libmq itself
# ---------------------------------------------------------------------------

def test_one_map_equals_group_join_plan(lib, S):
    n = 70_001
    for cards, path in sc.SPACES[1]:
        terms = sc.make("km", cards, n, seed=11)
        vals = wc.values_of(n)
        cols, ranges = sc.case("uniform_50", n, 2)
        ptrs, keep = upload(list(cols) + [vals], (0, 1))
        star = Star(lib, terms, (1,))
        try:
            for p in (AUTO, SORT):
                rc, h, g, taken, rows = jplan(lib, ptrs[:2], ranges, star.arr[0].d_col, star.arr[0].km, ptrs[2], n, p)
                assert rc == mq.MQ_OK and g > 50
                ref = read_raw(lib, h, g, 1)
                mq.check(lib.mq_group_free(h), "mq_group_free")
                rc, h2, g2, taken2, rows2 = splan(lib, ptrs[:2], ranges, star, ptrs[2], n, p)
                assert (rc, g2, taken2, rows2) == (mq.MQ_OK, g, taken, rows), lib.mq_last_error()
                assert read_raw(lib, h2, g2, 1) == ref, (cards, p)
                mq.check(lib.mq_group_free(h2), "mq_group_free")
        finally:
            star.free()


def by_where_plan(L, ptrs, ranges, dks, dv, n, path, bounds=None):
    h, groups, taken, rows = C.c_void_p(), C.c_uint64(), C.c_int(-1), C.c_uint64()
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    rc = L.mq_group_by_where_plan(c_ptrs(ptrs), c_ranges(ranges), len(ptrs), c_ptrs(dks), len(dks), dv, n, b, path, C.byref(h),
                                  C.byref(groups), C.byref(taken), C.byref(rows), None)
    return rc, h.value, groups.value, taken.value, rows.value


def test_plain_terms_equal_group_by_where_plan(lib, S):
    n = 70_001
    for nk, cards in ((1, (2048,)), (2, (32, 64)), (2, (7, 293)), (4, (2, 4, 16, 16))):
        rng = np.random.default_rng(nk)
        keys = [np.ascontiguousarray(rng.integers(0, c, n) + sc.COMP_BASE[j], np.int32) for j, c in enumerate(cards)]
        terms = [sc.Term("plain", k) for k in keys]
        vals = wc.values_of(n)
        cols, ranges = sc.case("uniform_10", n, 3)
        ptrs, keep = upload(list(cols) + [vals], (0, 1))
        star = Star(lib, terms, (1, 0))
        try:
            dks = [star.arr[j].d_col for j in range(nk)]
            for p in (AUTO, SORT):
                for bounds in (None, sc.bounds_of(cards)):
                    rc, h, g, taken, rows = by_where_plan(lib, ptrs[:3], ranges, dks, ptrs[3], n, p, bounds)
                    assert rc == mq.MQ_OK and g > 50, lib.mq_last_error()
                    ref = read_raw(lib, h, g, nk)
                    mq.check(lib.mq_group_free(h), "mq_group_free")
                    rc, h2, g2, taken2, rows2 = splan(lib, ptrs[:3], ranges, star, ptrs[3], n, p, bounds)
                    assert (rc, g2, rows2) == (mq.MQ_OK, g, rows), lib.mq_last_error()
                    assert bounds is None or taken2 == taken
                    assert read_raw(lib, h2, g2, nk) == ref, (cards, p, bounds)
                    mq.check(lib.mq_group_free(h2), "mq_group_free")
        finally:
            star.free()


def test_a_set_and_a_constant_equal_semi_agg(lib, S):
    """[ks, plain]: the total count and sum over the groups are mq_semi_agg's."""
    n = 70_001
    t = sc.make("ks_km", (64,), n, seed=12)[0]
    plain = sc.Term("plain", (np.arange(n) % 5).astype(np.int32))
    vals = wc.values_of(n)
    star = Star(lib, [t, plain])
    ws_bytes = lib.mq_semi_workspace_bytes(n)
    ws, agg = Dev(ws_bytes), Dev(32)
    try:
        for ncols in (0, 3):
            cols, ranges = sc.case("uniform_50", n, ncols)
            ptrs, keep = upload(list(cols) + [vals], (0, 1))
            rc = lib.mq_semi_agg(c_ptrs(ptrs[:ncols]) if ncols else None, c_ranges(ranges) if ncols else None, ncols, star.arr[0].d_col,
                                 star.arr[0].ks, 0, mq.MQ_SEMI_AUTO, ptrs[-1], n, agg.ptr, ws.ptr, ws_bytes, None)
            assert rc == mq.MQ_OK, lib.mq_last_error()
            mq.check(lib.mq_stream_sync(None), "sync")
            a = mq.MqAgg.from_buffer_copy(agg.get(np.uint8, 32).tobytes())
            assert a.count > 100
            for path in (DENSE, SORT):
                rc, h, g, taken, rows = splan(lib, ptrs[:ncols], ranges, star, ptrs[-1], n, path)
                assert (rc, g, rows) == (mq.MQ_OK, 5, a.count), lib.mq_last_error()
                keys, aggs = out_buffers(g, 1)
                mq.check(by_write(lib, h, keys, aggs), "mq_group_by_write")
                mq.check(lib.mq_group_free(h), "mq_group_free")
                cnt, sm = aggs["count"].get(np.uint64, g), aggs["sum"].get(np.int64, g)
                mn, mx = aggs["min"].get(np.int32, g), aggs["max"].get(np.int32, g)
                assert (int(cnt.sum()), int(sm.sum()), int(mn.min()), int(mx.max())) == (a.count, a.sum, a.min, a.max)
    finally:
        star.free()


@pytest.mark.parametrize("layout", [k for k in sc.LAYOUTS])
def test_equals_the_chain_it_replaces(lib, S, layout):
    """One mq_keymap_lookup per dimension into an n-row attribute column, `missing` below the
    map's attr_lo, then mq_group_by_where_plan with one added range per attribute column (a
    filtering dimension is looked up through a map of zeros and only adds its range)."""
    n = 70_001
    kinds = sc.LAYOUTS[layout]
    cards, path = sc.SPACES[sc.nkeys_of(kinds)][0]
    terms = sc.make(layout, cards, n, seed=13)
    vals = wc.values_of(n)
    cols, ranges = sc.case("uniform_50", n, 1)
    ptrs, keep = upload(list(cols) + [vals], (0, 1))
    star = Star(lib, terms, (1, 0))
    zero_maps, attr_cols = [], []
    try:
        cptrs, cranges, dks = list(ptrs[:1]), list(ranges), []
        for j, t in enumerate(terms):
            if t.kind == "plain":
                dks.append(star.arr[j].d_col)
                continue
            if t.kind == "km":
                km, attr_lo = star.arr[j].km, int(t.dim_attrs.min())
            else:
                zm = KeyMap(lib, t.dim_keys, np.zeros(len(t.dim_keys), np.int32))
                assert zm.rc == mq.MQ_OK
                zero_maps.append(zm)
                km, attr_lo = zm.h, 0
            out = Dev(4 * n)
            mq.check(lib.mq_keymap_lookup(km, star.arr[j].d_col, None, n, attr_lo - 1, out.ptr, None, None), "mq_keymap_lookup")
            attr_cols.append(out)
            cptrs.append(out.ptr)
            cranges.append((attr_lo, None))
            if t.kind == "km":
                dks.append(out.ptr)
        for p in (AUTO, SORT):
            rc, h, g, taken, rows = by_where_plan(lib, cptrs, cranges, dks, ptrs[1], n, p)
            assert rc == mq.MQ_OK and g >= 1, lib.mq_last_error()
            ref = read_raw(lib, h, g, len(dks))
            mq.check(lib.mq_group_free(h), "mq_group_free")
            rc, h2, g2, taken2, rows2 = splan(lib, ptrs[:1], ranges, star, ptrs[1], n, p)
            assert (rc, g2, rows2) == (mq.MQ_OK, g, rows), lib.mq_last_error()
            assert read_raw(lib, h2, g2, len(dks)) == ref, (layout, p)
            mq.check(lib.mq_group_free(h2), "mq_group_free")
    finally:
        for zm in zero_maps:
            zm.free()
        star.free()


# ---------------------------------------------------------------------------
# mq_star_positions
# ---------------------------------------------------------------------------

def star_positions(L, ptrs, ranges, star, pay, n, k_want, tag, nterms=None):
    """The positions into a sentinel-filled output of K + PAD entries."""
    out, cnt = Dev.of(np.full(k_want + PAD, SENT, np.int32)), Dev.of(np.full(1, 2**63 + 5, np.uint64))
    ws_bytes = L.mq_semi_workspace_bytes(n)
    ws = Dev(ws_bytes)
    rc = L.mq_star_positions(c_ptrs(ptrs) if ptrs else None, c_ranges(ranges) if ranges else None, len(ptrs), star.arr,
                             len(star.terms) if nterms is None else nterms, pay, n, out.ptr, cnt.ptr, ws.ptr, ws_bytes, None)
    assert rc == mq.MQ_OK, tag + (L.mq_last_error(),)
    mq.check(L.mq_stream_sync(None), "sync")
    return int(cnt.get(np.uint64, 1)[0]), out.get(np.int32, k_want + PAD)


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_star_positions(lib, layout):
    """Against numpy for every layout, with and without payload, aligned and not; nothing is
    written at or past K."""
    kinds = sc.LAYOUTS[layout]
    cards, _ = sc.SPACES[sc.nkeys_of(kinds)][0]
    for i, n in enumerate((0, 1, 257, 8 * TILE - 1, 8 * TILE + 1, 70_001)):  # k_star_mask keeps 8 tiles in flight
        terms = sc.make(layout, cards, n, seed=14)
        pay = wc.payload_of(n)
        cols, ranges = sc.case("uniform_50", n, (0, 2)[i % 2])
        ptrs, keep = upload(list(cols) + [pay], [(0,), (1, 0), (0, 3)][i % 3])
        star = Star(lib, terms, [(0,), (2,), (1, 0)][i % 3])
        try:
            for payload in (None, pay):
                want = sc.positions(cols, ranges, terms, payload)
                k, got = star_positions(lib, ptrs[:-1], ranges, star, None if payload is None else ptrs[-1], n, len(want), (layout, n))
                assert k == len(want), (layout, n, k, len(want))
                assert np.array_equal(got[:k], want) and np.all(got[k:] == SENT), (layout, n)
        finally:
            star.free()


def test_star_positions_equal_semi_positions_and_arguments(lib):
    n = 70_001
    terms = sc.make("ks_km", (64,), n, seed=15)
    cols, ranges = sc.case("uniform_50", n, 2)
    ptrs, keep = upload(list(cols))
    star = Star(lib, terms)
    ws_bytes = lib.mq_semi_workspace_bytes(n)
    ws = Dev(ws_bytes)
    try:
        want = sc.positions(cols, ranges, terms[:1])
        k, got = star_positions(lib, ptrs, ranges, star, None, n, len(want), ("one ks",), nterms=1)
        out, cnt = Dev.of(np.full(len(want) + PAD, SENT, np.int32)), Dev(8)
        for path in (mq.MQ_SEMI_GLOBAL, mq.MQ_SEMI_AUTO):
            mq.check(lib.mq_semi_positions(c_ptrs(ptrs), c_ranges(ranges), 2, star.arr[0].d_col, star.arr[0].ks, 0, path, None, n,
                                           out.ptr, cnt.ptr, ws.ptr, ws_bytes, None), "mq_semi_positions")
            mq.check(lib.mq_stream_sync(None), "sync")
            assert int(cnt.get(np.uint64, 1)[0]) == k == len(want) > 100
            assert out.get(np.int32, k + PAD).tobytes() == got.tobytes()
        # the map's own key set gives what the map gives
        ksm = lib.mq_keymap_keyset(star.arr[1].km)
        both = Star(lib, [terms[0], sc.Term("ks", terms[1].col, terms[1].dim_keys, extra={"h": ksm})], devs=star.devs)
        try:
            k2, got2 = star_positions(lib, ptrs, ranges, both, None, n, len(sc.positions(cols, ranges, terms)), ("km as ks",))
        finally:
            both.free()
        k3, got3 = star_positions(lib, ptrs, ranges, star, None, n, k2, ("km",))
        assert k2 == k3 == len(sc.positions(cols, ranges, terms)) and got2.tobytes() == got3.tobytes()
        args = (c_ptrs(ptrs), c_ranges(ranges), 2, star.arr)
        tail = (None, n, out.ptr, cnt.ptr, ws.ptr, ws_bytes, None)
        for nt in (0, 5):
            assert lib.mq_star_positions(*args, nt, *tail) == mq.MQ_EINVAL
        assert lib.mq_star_positions(c_ptrs(ptrs), c_ranges(ranges), 2, None, 1, *tail) == mq.MQ_EINVAL
        assert lib.mq_star_positions(*args, 2, None, n, out.ptr, None, ws.ptr, ws_bytes, None) == mq.MQ_EINVAL
        assert lib.mq_star_positions(*args, 2, None, n, None, cnt.ptr, ws.ptr, ws_bytes, None) == mq.MQ_EINVAL
        assert lib.mq_star_positions(*args, 2, None, n, out.ptr, cnt.ptr, ws.ptr, ws_bytes - 16, None) == mq.MQ_EINVAL
        assert lib.mq_star_positions(*args, 2, None, 2**31, out.ptr, cnt.ptr, ws.ptr, ws_bytes, None) == mq.MQ_EINVAL
        # settled on the host: K = 0
        empty = Star(lib, [sc.Term("ks", terms[0].col, np.empty(0, np.int32))], devs=star.devs)
        try:
            for a in ((c_ptrs(ptrs), c_ranges(ranges), 2, empty.arr, 1, None, n), (c_ptrs(ptrs), c_ranges([(3, 3), (None, None)]), 2, star.arr, 2, None, n),
                      (None, None, 0, star.arr, 2, None, 0)):
                mq.check(lib.mq_memset(cnt.ptr, 0x5A, 8, None), "mq_memset")
                assert lib.mq_star_positions(*a, out.ptr, cnt.ptr, ws.ptr, ws_bytes, None) == mq.MQ_OK
                mq.check(lib.mq_stream_sync(None), "sync")
                assert int(cnt.get(np.uint64, 1)[0]) == 0
        finally:
            empty.free()
    finally:
        star.free()


# ---------------------------------------------------------------------------
# the drop-in
# ---------------------------------------------------------------------------

def gptrs(objs):
    gs = [gcol(o) if o is not None else None for o in objs]
    arr = (C.POINTER(mq.GeneralizedColumn) * len(objs))(*[C.pointer(g) if g is not None else None for g in gs])
    return arr, gs


def fused(L, objs, ranges, fkeys, dim_keys, dim_attrs, values, nkeys, ncols=None, nterms=None):
    """group_aggregate_star -> (status, the nkeys + 4 Results as numpy arrays or None)"""
    keep = where_args(objs, ranges) if objs else (None, None, None, None)
    (fa, k1), (ka, k2), (aa, k3) = gptrs(fkeys), gptrs(dim_keys), gptrs(dim_attrs)
    gv = gcol(values)
    st = mq.Status(0, None)
    rpp = L.group_aggregate_star(keep[1], keep[2], keep[3], len(objs) if ncols is None else ncols, fa, ka, aa,
                                 len(fkeys) if nterms is None else nterms, C.byref(gv), C.byref(st))
    return (st.code, results(rpp, nkeys + 4)) if rpp else (st.code, None)


def test_dropin(lib, S, capfd):
    """Columns and INT Results mixed, a filtering and a plain term; a repeated dimension key
    (ERROR, NULL); an empty dimension (empty Results, OK)."""
    n = 70_001
    terms = sc.make("ks_km_plain_km", (2, 4, 16), n, seed=16)
    vals = wc.values_of(n)
    cols, ranges = sc.case("uniform_50", n, 2)
    cc, cv = [make_column(c) for c in cols], make_column(vals)
    cf = [make_column(t.col) for t in terms]
    ck = [make_column(t.dim_keys) if t.kind != "plain" else None for t in terms]
    ca = [make_column(t.dim_attrs) if t.kind == "km" else None for t in terms]
    for objs, rg, mc in ((cc, ranges, cols), ([], [], [])):
        want = sc.model(mc, rg, terms, vals)
        assert len(want[1]) > 50
        code, out = fused(lib, objs, rg, cf, ck, ca, cv, 3)
        assert code == mq.OK
        check_results(out, want, ("columns", len(objs)))
    # INT Results among the Columns: a shadowed one and two of the caller's own
    st = mq.Status(0, None)
    every = make_result(np.arange(n, dtype=np.int32))
    rf = lib.fetch_column(C.byref(cf[1]), C.byref(every), C.byref(st))
    assert st.code == mq.OK and rf
    ra, rv = make_result(terms[3].dim_attrs), make_result(vals)
    code, out = fused(lib, cc, ranges, [cf[0], rf, cf[2], cf[3]], ck, [None, ca[1], None, ra], rv, 3)
    assert code == mq.OK
    check_results(out, sc.model(cols, ranges, terms, vals), ("results",))
    # one component: group_aggregate's five
    one = sc.model([], [], terms[:2], vals)
    code, out = fused(lib, [], [], cf[:2], ck[:2], ca[:2], cv, 1)
    assert code == mq.OK
    check_results(out, one, ("one component",))
    # an empty dimension: empty Results and OK
    e = np.empty(0, np.int32)
    ce = make_column(e)
    code, out = fused(lib, cc, ranges, cf, [ce] + ck[1:], ca, cv, 3)
    assert code == mq.OK
    check_results(out, gb.group_by([e, e, e], e), ("empty filter dimension",))
    code, out = fused(lib, cc, ranges, cf, [ck[0], ce] + ck[2:], [None, ce] + ca[2:], cv, 3)
    assert code == mq.OK
    check_results(out, gb.group_by([e, e, e], e), ("empty mapped dimension",))
    capfd.readouterr()

    def refused_dropin(call):
        return call == (mq.ERROR, None) and "libmq" in capfd.readouterr().err

    twice = terms[1].dim_keys.copy()
    twice[17] = twice[400]
    ct = make_column(twice)
    assert refused_dropin(fused(lib, cc, ranges, cf, [ck[0], ct] + ck[2:], ca, cv, 3))          # not a primary key
    assert refused_dropin(fused(lib, cc, ranges, cf, ck, [None, ca[1], ca[3], ca[3]], cv, 3))   # dim_attrs without dim_keys
    assert refused_dropin(fused(lib, cc, ranges, cf[:1], ck[:1], ca[:1], cv, 0))                # no group key
    assert refused_dropin(fused(lib, cc, ranges, cf, ck, ca, cv, 3, nterms=5))
    assert refused_dropin(fused(lib, cc * 5, ranges * 5, cf, ck, ca, cv, 3, ncols=9))
    assert refused_dropin(fused(lib, cc, ranges, cf, ck, ca, ck[0], 3))                         # values as long as a dimension
    code, out = fused(lib, cc, ranges, cf, ck, ca, cv, 3)                                       # and the operator still works
    assert code == mq.OK
    check_results(out, sc.model(cols, ranges, terms, vals), ("after the errors",))
    take(rf)
    for r in (every, ra, rv):
        free_result_struct(r)
    for c in cc + cf + [cv, ce, ct] + [c for c in ck + ca if c is not None]:
        lib.mq_column_invalidate(C.byref(c))
