"""group_aggregate_join and the device entry points behind it: what holds on any machine. The
names are declared in the headers, exported by libmq.so and bound by mq.py; the key map's size
and the geometry of its prefix pass need no device; the numpy restatement the GPU tests compare
against agrees with a plain Python loop, and the named sets are what they claim; and without a
device every call answers MQ_ENODEV / ERROR (no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import groupjoincases as gj
import wherecases as wc
from refapi import make_column, mq

DEVICE_API = ["mq_keymap_bytes", "mq_keymap_geometry", "mq_keymap_build", "mq_keymap_keyset", "mq_keymap_lookup",
              "mq_keymap_free", "mq_group_join_plan"]
DROPIN_API = ["group_aggregate_join"]


def geometry(lib, span):
    b, c = C.c_uint32(), C.c_uint64()
    lib.mq_keymap_geometry(span, C.byref(b), C.byref(c))
    return b.value, c.value


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
    assert "typedef struct mq_keymap mq_keymap;" in dev_h
    assert [(n, t) for n, t in mq.MqKeymapInfo._fields_] == [
        ("lo", C.c_int32), ("hi", C.c_int32), ("attr_lo", C.c_int32), ("attr_hi", C.c_int32),
        ("entries", C.c_uint64), ("bytes", C.c_uint64)]
    assert C.sizeof(mq.MqKeymapInfo) == 32
    assert [getattr(mq.MqKeymapInfo, n).offset for n, _ in mq.MqKeymapInfo._fields_] == [0, 4, 8, 12, 16, 24]
    assert "GeneralizedColumn* fkeys, GeneralizedColumn* dim_keys," in qry_h


def test_size_and_geometry_need_no_device():
    lib = mq.load()
    assert lib.mq_keymap_bytes(2**32, 0) == (512 << 20) + (1 << 30)
    for n1 in (1, 1000, 2**31 - 1):
        assert lib.mq_keymap_bytes(2**32, n1) == (512 << 20) + (1 << 30) + 4 * n1
    last = 0
    for span in [0, 1, 31, 32, 33, 127, 128, 129, 4096, 10**6, 2**25, 2**31, 2**31 + 1, 2**32]:
        b = lib.mq_keymap_bytes(span, 5)
        assert b >= last and b == gj.map_bytes(span, 5), span
        assert lib.mq_keymap_bytes(span, 6) == b + 4
        last = b
        blocks, chunk = geometry(lib, span)
        words = (span + 127) // 128 * 4
        assert blocks >= 1 and chunk >= 256 and chunk % 256 == 0, span   # whole 256-word steps
        assert blocks * chunk >= words > (blocks - 1) * chunk - (words == 0), span
    lib.mq_keymap_geometry(100, None, None)  # either pointer may be NULL
    assert geometry(lib, 256 * 32) == (1, 256)
    assert geometry(lib, 256 * 32 + 1)[0] == 2
    blocks, chunk = geometry(lib, gj.WORD_EDGES_SPAN)
    assert blocks > 1 and chunk > 256  # several blocks and several steps a block
    blocks, chunk = geometry(lib, 2**32)
    assert blocks * chunk >= 2**27 and blocks <= 2**16


def test_model_is_consistent():
    """The restatement against a plain Python loop: 300 rows, both ends of int32 as fact keys
    and as dimension keys, 0 to 3 ranges."""
    rng = np.random.default_rng(13)
    cols = [rng.integers(-20, 20, 300).astype(np.int32) for _ in range(3)]
    fkey = rng.integers(-8, 8, 300).astype(np.int32)
    fkey[3], fkey[4], fkey[290], fkey[291] = wc.I32_MIN, wc.I32_MAX, wc.I32_MIN, wc.I32_MAX
    val = wc.values_of(300)
    dims = [([-3, 0, 5, 7], [10, 20, 10, -1]), ([wc.I32_MIN, 2], [wc.I32_MAX, wc.I32_MIN]), ([wc.I32_MAX], [0]),
            ([wc.I32_MAX, wc.I32_MIN, 1], [4, 4, 4]), ([], []), (list(range(7, -9, -1)), [k % 3 for k in range(16)])]
    for ranges in ([], [(-5, 12)], [(-5, 12), (None, 9), (-15, None)], [(None, None), (3, 3), (0, 5)]):
        p = len(ranges)
        for dk, da in dims:
            table = dict(zip(dk, da))
            groups = {}
            rows = 0
            for i in range(300):
                ok = all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi) for c, (lo, hi) in zip(cols[:p], ranges))
                if ok and int(fkey[i]) in table:
                    rows += 1
                    groups.setdefault(table[int(fkey[i])], []).append(int(val[i]))
            want = sorted(groups)
            got = gj.model(cols[:p], ranges, fkey, np.array(dk, np.int32), np.array(da, np.int32), val)
            assert got[0].tolist() == want, (ranges, dk)
            assert got[1].tolist() == [len(groups[a]) for a in want] and int(got[1].sum()) == rows
            assert got[2].tolist() == [sum(groups[a]) for a in want]
            assert got[3].tolist() == [min(groups[a]) for a in want] and got[4].tolist() == [max(groups[a]) for a in want]
            attrs, hits = gj.lookup(fkey, dk, da, missing=-77)
            assert attrs.tolist() == [table.get(int(k), -77) for k in fkey]
            assert hits.dtype == np.uint8 and hits.tolist() == [int(int(k) in table) for k in fkey]
    assert gj.is_primary_key([1, 2, 3]) and not gj.is_primary_key([1, 2, 1]) and gj.is_primary_key([])
    assert gj.repeated([1, 2, 1, 1]) == 2
    with pytest.raises(AssertionError):
        gj.lookup(fkey, [1, 1], [2, 3])
    assert gj.info([], []) == (0, -1, wc.I32_MAX, wc.I32_MIN, 0, 0)
    assert gj.info([5, -2], [9, 9]) == (-2, 5, 9, 9, 2, 16 + 32 + 8)
    assert gj.info([wc.I32_MIN, wc.I32_MAX], [1, -1])[5] == (512 << 20) + (1 << 30) + 8


def test_named_sets_are_what_they_claim():
    lib = mq.load()
    _, chunk = geometry(lib, gj.WORD_EDGES_SPAN)
    n = 8193
    for dname in gj.DIM_SETS:
        for card in gj.CARDS:
            dk, da = gj.dimension(dname, card, chunk_words=chunk)
            assert dk.dtype == da.dtype == np.int32 and len(dk) == len(da) and gj.is_primary_key(dk), dname
            if len(dk) >= 2 * card:
                assert (int(da.min()), int(da.max())) == (gj.ATTR_BASE, gj.ATTR_BASE + card - 1), (dname, card)
            if len(dk) >= 50 * card:
                assert len(np.unique(da)) == card, (dname, card)
        dk, da = gj.dimension(dname, 7, chunk_words=chunk)
        for fname in gj.FACT_SETS:
            for rows in (16, 33, n):
                f = gj.fact_keys(fname, rows, dk)
                assert f.dtype == np.int32 and len(f) == rows
                hit = np.isin(f, dk)
                joined, dropped = gj.promises(fname, dname)
                assert (not joined or hit.any()) and (not dropped or (~hit).any()), (dname, fname, rows)
                if fname == "all_present" and len(dk):
                    assert hit.all()
                if fname == "none_present":
                    assert not hit.any()
            assert len(gj.fact_keys(fname, 0, dk)) == 0
        if len(dk) > 1:
            g = gj.model([], [], gj.fact_keys("half_present", n, dk), dk, da, wc.values_of(n))
            assert 0 < int(g[1].sum()) < n and len(g[0]) >= 2, dname  # no GPU test passes on an empty result
    dk, _ = gj.dimension("dense", n1=3000)
    assert sorted(dk.tolist()) == list(range(-1000, 2000)) and dk.tolist() != sorted(dk.tolist())
    dk, _ = gj.dimension("sparse_wide")
    assert int(dk.max()) - int(dk.min()) + 1 > 2**31
    dk, _ = gj.dimension("int32_ends")
    assert {wc.I32_MIN, wc.I32_MAX} <= set(dk.tolist())
    f = gj.fact_keys("outside_ends", n, gj.dimension("negative")[0])
    lo, hi = -5000, -4001
    assert {wc.I32_MIN, wc.I32_MAX} <= set(f.tolist()) and f.min() < lo and f.max() > hi
    dk, _ = gj.dimension("word_edges", chunk_words=chunk)
    offs = set((dk.astype(np.int64) - gj.WORD_EDGES_LO).tolist())
    edge = chunk * 32
    assert set(gj.WORD_OFFSETS) <= offs and {edge - 1, edge, 2 * edge - 1, 2 * edge, gj.WORD_EDGES_SPAN - 1} <= offs
    assert min(offs) == 0 and max(offs) == gj.WORD_EDGES_SPAN - 1
    assert gj.case("uniform_10", n, 0) == ([], []) and len(gj.case("uniform_10", n, 3)[0]) == 3


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    rng = (mq.MqRange * 1)(mq.MqRange(1, 0, 1, 5))
    ptrs = (C.c_void_p * 1)(None)
    km, info = C.c_void_p(), mq.MqKeymapInfo()
    assert lib.mq_keymap_build(None, None, 0, 0, 0, 0, C.byref(km), C.byref(info), None) == mq.MQ_ENODEV
    assert lib.mq_keymap_build(None, None, 10, 1, 0, 5, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_keymap_free(None) == mq.MQ_ENODEV
    assert lib.mq_keymap_lookup(None, None, None, 0, 0, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_keymap_lookup(None, None, None, 10, -1, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_keymap_keyset(None) is None
    h, g, p, r = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    assert lib.mq_group_join_plan(ptrs, rng, 1, None, None, None, 0, None, 0, C.byref(h), C.byref(g), C.byref(p), C.byref(r),
                                  None) == mq.MQ_ENODEV
    assert lib.mq_group_join_plan(None, None, 0, None, None, None, 10, None, 7, None, None, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_keymap_bytes(10, 1) > 0
    col = make_column(np.arange(8, dtype=np.int32))
    gcol = mq.GeneralizedColumn()
    gcol.column_type = mq.COLUMN
    gcol.column_pointer.column = C.pointer(col)
    gp = (C.POINTER(mq.GeneralizedColumn) * 1)(C.pointer(gcol))
    lows = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(2)))
    highs = (C.POINTER(C.c_int) * 1)(C.pointer(C.c_int(6)))
    for args in ((gp, lows, highs, 1), (None, None, None, 0)):
        st = mq.Status(0, None)
        assert not lib.group_aggregate_join(*args, C.byref(gcol), C.byref(gcol), C.byref(gcol), C.byref(gcol), C.byref(st))
        assert st.code == mq.ERROR
        assert "libmq" in capfd.readouterr().err
