"""top_k and the device entry point behind it: what holds on any machine. The names are
declared in the headers, exported by libmq.so and bound by mq.py; the default candidate
cap and the AUTO rule need no device; the numpy restatement the GPU tests compare against
agrees with a plain Python sort; and without a device every call answers MQ_ENODEV / ERROR
(no CPU fall-back).
"""
import ctypes as C

import numpy as np
import pytest

import topkcases as tc
from refapi import make_column, mq

DEVICE_API = ["mq_topk_default_cap", "mq_topk_auto_path", "mq_topk"]
DROPIN_API = ["top_k"]


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
    assert ("Result** top_k(GeneralizedColumn* values, Result* positions, size_t k, bool descending, "
            "Status* ret_status);") in qry_h
    assert "enum { MQ_TOPK_AUTO = 0, MQ_TOPK_SELECT = 1, MQ_TOPK_SORT = 2 };" in dev_h
    assert (mq.MQ_TOPK_AUTO, mq.MQ_TOPK_SELECT, mq.MQ_TOPK_SORT) == (0, 1, 2)
    assert f"enum {{ MQ_TOPK_SORT_DIV = {mq.MQ_TOPK_SORT_DIV} }};" in dev_h
    assert "min(k, n) + cand_cap > n / MQ_TOPK_SORT_DIV" in dev_h  # the rule is stated where the constant is
    # the info struct as the header lays it out
    assert [(n, t) for n, t in mq.MqTopkInfo._fields_] == [
        ("m", C.c_uint64), ("candidates", C.c_uint64), ("ties", C.c_uint64), ("path", C.c_int32), ("levels", C.c_int32)]
    assert C.sizeof(mq.MqTopkInfo) == 32


def test_default_cap_and_auto_rule_need_no_device():
    lib = mq.load()
    cap = lib.mq_topk_default_cap()
    assert cap > 0 and lib.mq_topk_default_cap() == cap
    div = mq.MQ_TOPK_SORT_DIV
    for n, k, c in [(0, 0, 0), (1, 1, 0), (10**9, 10, 0), (10**9, 1 << 20, 0), (8 * cap, cap, 0), (8 * cap, cap + 1, 0),
                    (4000, 10, 1), (4000, 999, 1), (4000, 1000, 1), (4000, 5000, 7), (40, 3, 7), (40, 4, 7)]:
        ce = c or cap
        want = mq.MQ_TOPK_SORT if min(k, n) + ce > n // div else mq.MQ_TOPK_SELECT
        assert lib.mq_topk_auto_path(n, k, c) == want, (n, k, c)
    assert lib.mq_topk_auto_path(10**9, 10, 0) == mq.MQ_TOPK_SELECT
    assert lib.mq_topk_auto_path(10**9, 10**9, 0) == mq.MQ_TOPK_SORT


def test_model_is_consistent():
    """The restatement against a plain sorted(range(n), key=(v[i], i)) loop: 300 rows,
    negatives, repeats, both directions, with and without a payload."""
    rng = np.random.default_rng(5)
    v = rng.integers(-20, 9, 300).astype(np.int32)
    v[17], v[200] = tc.I32_MIN, tc.I32_MAX
    pay = tc.payload_of(300)
    vl = v.tolist()
    assert len(set(vl)) < 300 and min(vl) < 0
    for desc in (False, True):
        idx = sorted(range(300), key=lambda i: ((-vl[i] if desc else vl[i]), i))
        for k in (0, 1, 7, 299, 300, 305):
            m = min(k, 300)
            gv, gp = tc.topk(v, None, k, desc)
            assert gv.tolist() == [vl[i] for i in idx[:m]] and gp.tolist() == idx[:m], (desc, k)
            gv, gp = tc.topk(v, pay, k, desc)
            assert gp.tolist() == [int(pay[i]) for i in idx[:m]], (desc, k)
            assert (gv.dtype, gp.dtype) == (np.int32, np.int32)
            t = vl[idx[m - 1]] if m else None
            assert tc.ties_left_out(v, k, desc) == (sum(vl[i] == t for i in idx[m:]) if m else 0)
    assert all(len(a) == 0 for a in tc.topk(v[:0], None, 5, False))
    # the named sets are what they say
    n = 4097
    key = lambda a: a.astype(np.int64) + 2**31
    assert len(np.unique(tc.values_of("all_equal", n))) == 1 and len(np.unique(tc.values_of("two_values", n))) == 2
    f = tc.values_of("full_range", n)
    assert f.min() == tc.I32_MIN and f.max() == tc.I32_MAX
    assert len(np.unique(key(tc.values_of("uniform_100", n)) >> 10)) == 1
    a = key(tc.values_of("top11_shared", n))
    assert len(np.unique(a >> 21)) == 1 and len(np.unique((a >> 10) & 2047)) > 1000
    b = key(tc.values_of("top22_shared", n))
    assert len(np.unique(b >> 10)) == 1 and 500 < len(np.unique(b)) < n
    assert np.all(np.diff(tc.values_of("sorted_asc", n)) >= 0) and np.all(np.diff(tc.values_of("sorted_desc", n)) <= 0)
    s = tc.values_of("straddle", tc.BIG)
    assert np.all(s[tc.BIG // 8:tc.BIG - tc.BIG // 8] == 0) and s.min() < 0 < s.max()
    assert len(np.unique(tc.payload_of(n))) == n


def _has_gpu():
    return mq.load().mq_device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present; the no-device path is not reachable")
def test_without_a_device(capfd):
    lib = mq.load()
    info = mq.MqTopkInfo()
    assert lib.mq_topk(None, None, 0, 0, 0, mq.MQ_TOPK_AUTO, 0, None, None, C.byref(info), None) == mq.MQ_ENODEV
    assert lib.mq_topk(None, None, 10, 3, 1, mq.MQ_TOPK_SELECT, 1, None, None, None, None) == mq.MQ_ENODEV
    assert lib.mq_topk_default_cap() > 0
    data = np.arange(8, dtype=np.int32)
    col = make_column(data)
    g = mq.GeneralizedColumn()
    g.column_type = mq.COLUMN
    g.column_pointer.column = C.pointer(col)
    st = mq.Status(0, None)
    assert not lib.top_k(C.byref(g), None, 3, False, C.byref(st))
    assert st.code == mq.ERROR
    assert "libmq" in capfd.readouterr().err
