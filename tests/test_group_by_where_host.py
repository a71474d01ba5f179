"""group_aggregate_by_where and mq_group_by_where_plan behind it: what holds on any machine.
The names are declared in the headers, exported by libmq.so and bound by mq.py; the composed
model the GPU tests compare against (groupbycases.group_by over wherecases.mask) agrees with a
plain Python loop; the named sets of groupbywherecases.py are what they claim; and without a
device every call answers MQ_ENODEV / ERROR (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import groupbycases as gb
import groupbywherecases as gbw
import groupcases as gc
import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_group_by_where_plan"]
DROPIN_API = ["group_aggregate_by_where"]


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    qry_h = open(f"{mq.INCLUDE_DIR}/mq_query.h").read()
    assert "int mq_group_by_where_plan(const int32_t* const* d_cols" in dev_h
    assert "Result** group_aggregate_by_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols," in qry_h
    assert "GeneralizedColumn** keys, int nkeys, GeneralizedColumn* values," in qry_h
    # the plan takes the predicates as mq_group_where_plan does, then what mq_group_by_plan takes, with h_rows
    # before the stream as in mq_group_where_plan
    where, by, fused = (mq._SIGS[n][1] for n in ("mq_group_where_plan", "mq_group_by_plan", "mq_group_by_where_plan"))
    assert fused[:3] == where[:3] and fused[3:12] == by[:9] and fused[12] == where[11] and fused[13] == by[9]
    assert len(fused) == 14 and mq._SIGS["mq_group_by_where_plan"][0] == C.c_int
    wsig, bsig, fsig = (mq._SIGS[n] for n in ("group_aggregate_where", "group_aggregate_by", "group_aggregate_by_where"))
    assert fsig[0] == bsig[0] and fsig[1] == wsig[1][:4] + bsig[1]


def test_composed_model_against_a_dict_loop():
    """300 rows x 3 predicate columns x 1 to 4 key columns: both int32 ends among keys, values
    and predicate columns, every kind of bound, and a mask that matches nothing."""
    rng = np.random.default_rng(29)
    n = 300
    cols = [rng.integers(-20, 20, n).astype(np.int32) for _ in range(3)]
    cols[1][5], cols[1][6] = wc.I32_MIN, wc.I32_MAX
    keys = [rng.integers(-3, 3, n).astype(np.int32), rng.integers(-2, 2, n).astype(np.int32),
            rng.integers(-1, 2, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)]
    keys[0][5], keys[0][6], keys[1][7] = gc.I32_MIN, gc.I32_MAX, gc.I32_MAX
    vals = wc.values_of(n)
    seen_empty = False
    for nkeys in (1, 2, 3, 4):
        for ranges in ([(-5, 12), (None, 9), (-15, None)], [(None, None), (wc.I32_MIN, None), (None, None)],
                       [(-20, 20), (None, wc.I32_MIN + 1), (None, None)], [(3, 3), (None, None), (None, None)],
                       [(0, 5), (100, 200), (None, None)]):
            table = {}
            for i in range(n):
                if all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi) for c, (lo, hi) in zip(cols, ranges)):
                    t, v = tuple(int(k[i]) for k in keys[:nkeys]), int(vals[i])
                    c, s, mn, mx = table.get(t, (0, 0, v, v))
                    table[t] = (c + 1, s + v, min(mn, v), max(mx, v))
            order = sorted(table)
            ks, cnt, sm, mn, mx = gbw.model(cols, ranges, keys[:nkeys], vals)
            assert list(zip(*[k.tolist() for k in ks])) == order
            assert cnt.tolist() == [table[t][0] for t in order]
            assert sm.tolist() == [table[t][1] for t in order]
            assert mn.tolist() == [table[t][2] for t in order]
            assert mx.tolist() == [table[t][3] for t in order]
            assert [k.dtype for k in ks] == [np.int32] * nkeys
            assert (cnt.dtype, sm.dtype, mn.dtype, mx.dtype) == (np.uint64, np.int64, np.int32, np.int32)
            assert int(cnt.sum()) == int(wc.mask(cols, ranges).sum())
            seen_empty |= len(order) == 0
    assert seen_empty
    full = gbw.model(cols, [(None, None)] * 3, keys[:3], vals)
    want = gb.group_by(keys[:3], vals)
    assert all(np.array_equal(a, b) for a, b in zip(full[0] + list(full[1:]), want[0] + list(want[1:])))


def test_matrix_covers_what_it_claims():
    seen = set()
    for ci, name in enumerate(wc.CASES):
        combos = gbw.matrix(ci)
        assert {(c[0], c[1]) for c in combos} == {(a, b) for a in wc.NCOLS for b in gbw.NKEYS}, name
        assert {c[2] for c in combos} >= {0, 1025, 8193}, name
        seen |= {c[2] for c in combos}
        assert all(c[3] in gbw.TUPLE_SETS and c[4] in gbw.VALUE_SETS for c in combos)
    assert seen == set(wc.SIZES)
    used = [c for ci in range(len(wc.CASES)) for c in gbw.matrix(ci)]
    assert {c[3] for c in used} == set(gbw.TUPLE_SETS) and {c[4] for c in used} == set(gbw.VALUE_SETS)
    assert {(c[1], c[3]) for c in used} >= {(k, t) for k in gbw.NKEYS for t in ("space_S", "space_S_plus_1", "seven_sorted")}


def test_named_sets_are_what_they_claim():
    lib = mq.load()
    S = lib.mq_group_dense_slots()
    # the filter narrows the key space: exactly S matching tuples in a space of S, then one tuple more
    for nkeys in gbw.NKEYS:
        for extra in (0, 1):
            cols, ranges, keys, vals = gbw.narrow(S, extra, nkeys)
            m = wc.mask(cols, ranges)
            assert gb.space_of(gb.bounds_of(keys)) > 4 * S
            groups = len(gbw.model(cols, ranges, keys, vals)[1])
            assert groups == S + extra == int(m.sum())
            space = gb.space_of(gbw.matching_bounds(cols, ranges, keys))
            assert (space == S) if extra == 0 else (S < space <= 2**32)
    # the poisoned sets
    for name in gbw.POISON_SETS:
        for nkeys in gbw.NKEYS:
            cols, ranges, keys, vals, bounds = gbw.poisoned(name, nkeys)
            m = wc.mask(cols, ranges)
            assert m.sum() >= 2 and gbw.matching_bounds(cols, ranges, keys) == bounds, (name, nkeys)
            assert gb.space_of(bounds) <= S
            out = np.zeros(len(m), dtype=bool)
            for j, k in enumerate(keys):
                out |= (k.astype(np.int64) < bounds[2 * j]) | (k.astype(np.int64) > bounds[2 * j + 1])
            assert np.array_equal(out, ~m), (name, nkeys)  # exactly the failing rows are out of bounds
            starts = np.arange(0, len(m), wc.LINE)
            live = np.add.reduceat(m.astype(np.int64), starts)
            rows = np.diff(np.concatenate([starts, [len(m)]]))
            assert np.sum((live > 0) & (live < rows)) >= 1 and np.sum(live == 0) >= 1, (name, nkeys)
            dead = np.flatnonzero(~m)
            for j, k in enumerate(keys):
                stray = set(k[dead].astype(np.int64).tolist())
                if len(dead) >= nkeys * gbw.POISON_KINDS:
                    assert {gc.I32_MIN, gc.I32_MAX, bounds[2 * j] - 1, bounds[2 * j + 1] + 1} <= stray, (name, nkeys, j)
            code = gbw.code_of(keys, bounds, dead)
            inside = np.array([0 <= c < gb.space_of(bounds) for c in code])
            assert inside.any() and not inside.all(), (name, nkeys)  # some strays sum to a slot of the table


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    rng = (mq.MqRange * 2)(mq.MqRange(1, 0, 1, 5), mq.MqRange(0, 0, 0, 0))
    ptrs = (C.c_void_p * 2)(None, None)
    h, groups, path, rows = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    for n in (0, 10):
        assert lib.mq_group_by_where_plan(ptrs, rng, 2, ptrs, 2, None, n, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups),
                                          C.byref(path), C.byref(rows), None) == mq.MQ_ENODEV
    assert lib.mq_group_by_where_plan(None, None, 0, None, 0, None, 0, None, 7, None, None, None, None, None) == mq.MQ_ENODEV
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 2)(C.pointer(g), C.pointer(g))
    lows = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(2)))
    highs = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(6)))
    st = mq.Status(0, None)
    assert not lib.group_aggregate_by_where(gp, lows, highs, 1, gp, 2, C.byref(g), C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
