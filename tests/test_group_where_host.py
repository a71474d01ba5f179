"""group_aggregate_where and mq_group_where_plan behind it: what holds on any machine. The
names are declared in the headers, exported by libmq.so and bound by mq.py; the composed
model the GPU tests compare against (groupcases.group over wherecases.mask) agrees with a
plain Python loop; the named sets of groupwherecases.py are what they claim; and without a
device every call answers MQ_ENODEV / ERROR (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import groupcases as gc
import groupwherecases as gw
import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_group_where_plan"]
DROPIN_API = ["group_aggregate_where"]


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    qry_h = open(f"{mq.INCLUDE_DIR}/mq_query.h").read()
    assert "int mq_group_where_plan(const int32_t* const* d_cols" in dev_h
    assert "Result** group_aggregate_where(GeneralizedColumn** columns, int** lows, int** highs, int ncols," in qry_h
    assert "GeneralizedColumn* keys, GeneralizedColumn* values, Status* ret_status);" in qry_h
    # the plan takes what mq_where_positions takes, then what mq_group_plan takes, then h_rows
    where, group, fused = (mq._SIGS[n][1] for n in ("mq_where_positions", "mq_group_plan", "mq_group_where_plan"))
    assert fused[:3] == where[:3] and fused[3:11] == group[:8] and fused[12] == group[8]
    assert fused[11] == C.POINTER(C.c_uint64) and len(fused) == 13
    assert mq._SIGS["mq_group_where_plan"][0] == C.c_int
    wsig, gsig, fsig = (mq._SIGS[n] for n in ("aggregate_where", "group_aggregate", "group_aggregate_where"))
    assert fsig[0] == gsig[0] and fsig[1] == wsig[1][:4] + gsig[1]


def test_composed_model_against_a_dict_loop():
    """300 rows x 3 predicate columns: both int32 ends among keys, values and predicate
    columns, every kind of bound, and a mask that matches nothing."""
    rng = np.random.default_rng(23)
    cols = [rng.integers(-20, 20, 300).astype(np.int32) for _ in range(3)]
    cols[1][5], cols[1][6] = wc.I32_MIN, wc.I32_MAX
    keys = rng.integers(-9, 9, 300).astype(np.int32)
    keys[5], keys[6], keys[7] = gc.I32_MIN, gc.I32_MAX, gc.I32_MAX
    vals = wc.values_of(300)
    seen_empty = False
    for ranges in ([(-5, 12), (None, 9), (-15, None)], [(None, None), (wc.I32_MIN, None), (None, None)],
                   [(-20, 20), (None, wc.I32_MIN + 1), (None, None)], [(None, None), (wc.I32_MAX, None), (-20, 20)],
                   [(3, 3), (None, None), (None, None)], [(0, 5), (100, 200), (None, None)]):
        table = {}
        for i in range(300):
            if all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi) for c, (lo, hi) in zip(cols, ranges)):
                k, v = int(keys[i]), int(vals[i])
                c, s, mn, mx = table.get(k, (0, 0, v, v))
                table[k] = (c + 1, s + v, min(mn, v), max(mx, v))
        order = sorted(table)
        gk, gn, gs, gmn, gmx = gw.model(cols, ranges, keys, vals)
        assert gk.tolist() == order
        assert gn.tolist() == [table[k][0] for k in order]
        assert gs.tolist() == [table[k][1] for k in order]
        assert gmn.tolist() == [table[k][2] for k in order]
        assert gmx.tolist() == [table[k][3] for k in order]
        assert (gk.dtype, gn.dtype, gs.dtype, gmn.dtype, gmx.dtype) == (np.int32, np.uint64, np.int64, np.int32, np.int32)
        assert int(gn.sum()) == int(wc.mask(cols, ranges).sum())
        seen_empty |= len(order) == 0
    assert seen_empty
    full = gw.model(cols, [(None, None)] * 3, keys, vals)
    assert all(np.array_equal(a, b) for a, b in zip(full, gc.group(keys, vals)))
    assert full[0][0] == gc.I32_MIN and full[0][-1] == gc.I32_MAX


def test_matrix_covers_what_it_claims():
    sizes_by_case, seen = {}, set()
    for ci, name in enumerate(wc.CASES):
        combos = gw.matrix(ci)
        assert {c[0] for c in combos} == set(wc.NCOLS), name
        sizes_by_case[name] = {c[1] for c in combos}
        assert sizes_by_case[name] >= {0, 1025, 8193} and len(sizes_by_case[name]) >= 3, name
        seen |= {(c[0], c[1]) for c in combos}
        assert all(c[2] in gw.KEY_SETS and c[3] in gw.VALUE_SETS for c in combos)
    assert {n for _, n in seen} == set(wc.SIZES)
    used = [c for ci in range(len(wc.CASES)) for c in gw.matrix(ci)]
    assert {c[2] for c in used} == set(gw.KEY_SETS) and {c[3] for c in used} == set(gw.VALUE_SETS)
    assert set(gw.KEY_SETS) == {"one_key", "seven_sorted", "seven_shuffled", "uniform_100", "range_S", "int32_ends",
                                "skewed", "all_distinct"}


def test_named_sets_are_what_they_claim():
    lib = mq.load()
    S = lib.mq_group_dense_slots()
    # the filter narrows the range: exactly S matching key values, then exactly one more
    for extra in (0, 1):
        cols, ranges, keys, vals = gw.narrow(S, extra)
        m = wc.mask(cols, ranges)
        assert cols[0] is keys and gc.key_range(keys) == gw.NARROW_N > S
        assert gc.key_range(keys[m]) == S + extra == int(m.sum())
    # the poisoned sets
    for name in gw.POISON_SETS:
        cols, ranges, keys, vals, (lo, hi) = gw.poisoned(name, S)
        m = wc.mask(cols, ranges)
        assert m.sum() >= 1 and (int(keys[m].min()), int(keys[m].max())) == (lo, hi), name
        assert hi - lo + 1 <= S, name  # DENSE is asserted for it
        k64 = keys.astype(np.int64)
        assert np.all((k64[~m] < lo) | (k64[~m] > hi)), name  # every failing row is out of bounds
        mixed, dead = gw.line_census(m)
        assert mixed >= 1 and dead >= 1, (name, mixed, dead)  # ... in live lines and in whole dead lines
        assert {gc.I32_MIN, gc.I32_MAX, lo - 1, hi + 1} <= set(k64[~m].tolist()), name
    # the run-fold and many-iterations key sets fit the dense path whatever the filter keeps
    for ks in ("seven_sorted", "one_key", "uniform_100"):
        for n in (8193, 70_001, wc.BIG):
            assert gc.key_range(gc.keys_of(ks, n, S)) <= S
    # the large sort case
    col, m = gw.sort_big_mask()
    k = int(m.sum())
    assert len(col) == gw.SORT_BIG_N and k > 2_097_152 and 0.58 < k / gw.SORT_BIG_N < 0.62
    blocks, chunk = C.c_uint32(), C.c_uint64()
    lib.mq_group_sort_geometry(k, C.byref(blocks), C.byref(chunk))
    assert chunk.value >= 2 * gc.SEG_TILE and blocks.value >= 2  # the two-tile regime
    cols, ranges, keys, vals, runs = gw.sort_big(chunk.value)
    assert runs.sum() == k and np.array_equal(gc.group(keys[m], vals[m])[1], runs.astype(np.uint64))
    assert gc.key_range(keys[m]) == 2**32


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    rng = (mq.MqRange * 2)(mq.MqRange(1, 0, 1, 5), mq.MqRange(0, 0, 0, 0))
    ptrs = (C.c_void_p * 2)(None, None)
    h, groups, path, rows = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    for n in (0, 10):
        assert lib.mq_group_where_plan(ptrs, rng, 2, None, None, n, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups),
                                       C.byref(path), C.byref(rows), None) == mq.MQ_ENODEV
    assert lib.mq_group_where_plan(None, None, 0, None, None, 0, None, 7, None, None, None, None, None) == mq.MQ_ENODEV
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(g))
    lows = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(2)))
    highs = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(6)))
    st = mq.Status(0, None)
    assert not lib.group_aggregate_where(gp, lows, highs, 1, C.byref(g), C.byref(g), C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
