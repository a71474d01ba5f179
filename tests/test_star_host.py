"""group_aggregate_star and the device entry points behind it: what holds on any machine. The
names are declared in the headers, exported by libmq.so and bound by mq.py; mq_star_term is the
24 bytes the header says; the numpy restatement the GPU tests compare against agrees with a
plain Python loop for every term layout; every generated case that the GPU tests rely on has a
joined row and a dropped row; the attribute-space layouts lie on the side of the dense path's
slots they are meant for; and without a device every call answers MQ_ENODEV / ERROR.
"""
import ctypes as C

import numpy as np
import pytest

import groupjoincases as gj
import starcases as sc
import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_star_positions", "mq_group_star_plan"]
DROPIN_API = ["group_aggregate_star"]


def test_names_declared_exported_and_bound():
    declared = mq.header_functions()
    lib = mq.load()
    for name in DEVICE_API + DROPIN_API:
        assert name in declared, name
        assert name in mq._SIGS, name
        assert list(getattr(lib, name).argtypes) == mq._SIGS[name][1], name
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    qry_h = open(f"{mq.INCLUDE_DIR}/mq_query.h").read()
    assert all(f" {n}(" in dev_h for n in DEVICE_API)
    assert all(f" {n}(" in qry_h for n in DROPIN_API)
    assert "enum { MQ_STAR_MAX_TERMS = 4 };" in dev_h and mq.MQ_STAR_MAX_TERMS == 4 == sc.MAX_TERMS
    assert "enum { MQ_GROUP_MAX_KEYS = 4 };" in dev_h and mq.MQ_GROUP_MAX_KEYS == 4
    assert [n for n, _ in mq.MqStarTerm._fields_] == ["d_col", "km", "ks"]
    assert C.sizeof(mq.MqStarTerm) == 24
    assert [getattr(mq.MqStarTerm, n).offset for n, _ in mq.MqStarTerm._fields_] == [0, 8, 16]
    assert (mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT) == (0, 1, 2)
    for note in ("WHOLE column", "Bounds from the caller avoid that pass", "most selective filter first", "no LDS form"):
        assert note in dev_h, note  # what the issue asks the header to say


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_model_agrees_with_a_plain_loop(layout):
    """300 rows, 0 to 3 ranges, every attribute space of the layout's number of components."""
    n = 300
    nk = sc.nkeys_of(sc.LAYOUTS[layout])
    for cards, _ in sc.SPACES[nk] + [((3,) * nk, "dense")]:
        terms = sc.make(layout, cards, n, seed=5)
        vals = wc.values_of(n)
        for ncols in (0, 1, 3):
            cols, ranges = sc.case("uniform_50", n, ncols)
            got, want = sc.model(cols, ranges, terms, vals), sc.brute(cols, ranges, terms, vals)
            assert len(got[0]) == nk == len(want[0])
            for a, b in zip(got[0], want[0]):
                assert a.dtype == np.int32 and a.tolist() == b.tolist(), (layout, cards, ncols)
            for a, b in zip(got[1:], want[1:]):
                assert a.dtype == b.dtype and a.tolist() == b.tolist(), (layout, cards, ncols)
            m = sc.joined(cols, ranges, terms)
            assert int(got[1].sum()) == int(m.sum())
            assert sc.positions(cols, ranges, terms).tolist() == np.flatnonzero(m).tolist()
            pay = wc.payload_of(n)
            assert sc.positions(cols, ranges, terms, pay).tolist() == pay[m].tolist()
        if nk == 1:
            t = [t for t in terms if t.kind != "ks"][0]
            if t.kind == "km":  # one mapped component and no filter: groupjoincases' model
                only = [x for x in terms if x.kind == "ks"]
                if not only:
                    ref = gj.model([], [], t.col, t.dim_keys, t.dim_attrs, vals)
                    got = sc.model([], [], terms, vals)
                    assert got[0][0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist()


@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_generated_cases_have_a_joined_and_a_dropped_row(layout):
    """The sizes and predicate sets the GPU tests use: no one of them passes vacuously."""
    nk = sc.nkeys_of(sc.LAYOUTS[layout])
    has_filter = any(k != "plain" for k in sc.LAYOUTS[layout])
    for cards, _ in sc.SPACES[nk]:
        for n in (1025, 70_001):
            terms = sc.make(layout, cards, n, seed=1)
            for t in terms:
                assert t.col.dtype == np.int32 and len(t.col) == n
                if t.kind != "plain":
                    assert gj.is_primary_key(t.dim_keys)
                    hit = np.isin(t.col, t.dim_keys)
                    assert hit.any() and (~hit).any(), (layout, t.kind)
                    assert {wc.I32_MIN, wc.I32_MAX} & set(t.col.tolist()) or n < 5000
            for ncols in gj.NCOLS:
                cols, ranges = sc.case("uniform_50", n, ncols)
                some, dropped = sc.promises(cols, ranges, terms)
                assert some and (dropped or not (has_filter or ncols)), (layout, cards, n, ncols)
            want = sc.model([], [], terms, wc.values_of(n))
            if n == 70_001:  # the components reach both ends of their bounds: P is the product of the cardinalities
                b = sc.bounds_of(cards)
                for j, k in enumerate(want[0]):
                    assert (int(k.min()), int(k.max())) == (b[2 * j], b[2 * j + 1]), (layout, cards, j)
                assert len(want[1]) > min(int(np.prod(cards)), 1000) // 2


def test_attribute_spaces_take_the_intended_path():
    """mq_group_by_auto_path needs no device: P on both sides of the switch, and past 2^32."""
    lib = mq.load()
    paths = {"dense": mq.MQ_GROUP_DENSE, "sort": mq.MQ_GROUP_SORT}
    seen = set()
    for nk, spaces in sc.SPACES.items():
        for cards, path in spaces:
            assert len(cards) == nk
            b = sc.bounds_of(cards)
            space = C.c_uint64()
            assert lib.mq_group_by_auto_path((C.c_int32 * len(b))(*b), nk, C.byref(space)) == paths[path], cards
            assert space.value == int(np.prod(cards)) and (space.value <= sc.SLOTS) == (path == "dense")
            seen.add(space.value)
    assert {2048, 2049, 2051} <= seen
    wide = [wc.I32_MIN, wc.I32_MAX, 0, 1]
    assert lib.mq_group_by_auto_path((C.c_int32 * 4)(*wide), 2, None) == mq.MQ_EINVAL  # P = 2^33


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    terms = (mq.MqStarTerm * 1)(mq.MqStarTerm(None, None, None))
    h, g, p, r = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    assert lib.mq_group_star_plan(None, None, 0, terms, 1, None, 0, None, 0, C.byref(h), C.byref(g), C.byref(p), C.byref(r),
                                  None) == mq.MQ_ENODEV
    assert lib.mq_group_star_plan(None, None, 0, None, 9, None, 10, None, 7, None, None, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_star_positions(None, None, 0, terms, 1, None, 0, None, None, None, 0, None) == mq.MQ_ENODEV
    col = make_column(np.arange(8, dtype=np.int32))
    gcol = mq.GeneralizedColumn()
    gcol.column_type = mq.COLUMN
    gcol.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(gcol))
    none = (C.POINTER(mq.GeneralizedColumn) * 1)()
    st = mq.Status(0, None)
    assert not lib.group_aggregate_star(None, None, None, 0, gp, gp, gp, 1, C.byref(gcol), C.byref(st))
    assert st.code == mq.ERROR and "libmq" in capfd.readouterr().err
    st = mq.Status(0, None)
    assert not lib.group_aggregate_star(None, None, None, 0, gp, none, none, 1, C.byref(gcol), C.byref(st))
    assert st.code == mq.ERROR and "libmq" in capfd.readouterr().err
