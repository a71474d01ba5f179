"""mq_topk64, mq_group_top and group_top_k: what holds on any machine. The names are declared in
the headers, exported by libmq.so and bound by mq.py; the key mapping and the AUTO rule need no
device; the structs in mq.py have the header's layout; and the numpy restatement the GPU tests
compare against agrees with a plain Python sort.
"""
import ctypes as C

import numpy as np

import topk64cases as tc
from refapi import mq

DEVICE_API = ["mq_topk64_key", "mq_topk64_auto_path", "mq_topk64", "mq_topk64_widen", "mq_topk64_take", "mq_group_top"]
DROPIN_API = ["group_top_k"]


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
    assert "Result** group_top_k(Result** groups, int nresults, int order_by" in qry_h
    assert "enum { MQ_AGG_KEY = 0, MQ_AGG_COUNT = 1, MQ_AGG_SUM = 2, MQ_AGG_MIN = 3, MQ_AGG_MAX = 4 };" in dev_h
    assert (mq.MQ_AGG_KEY, mq.MQ_AGG_COUNT, mq.MQ_AGG_SUM, mq.MQ_AGG_MIN, mq.MQ_AGG_MAX) == (0, 1, 2, 3, 4)
    # the rule is mq_topk's, and the header says that its constants were not swept for 64-bit entries
    assert "min(k, n) + cand_cap > n / MQ_TOPK_SORT_DIV" in dev_h and "NOT been swept" in dev_h


def test_struct_layouts_match_the_header():
    dev_h = open(f"{mq.INCLUDE_DIR}/mq_device.h").read()
    assert "typedef struct mq_range64 { int has_low; int64_t low; int has_high; int64_t high; } mq_range64;" in dev_h
    # x86-64: an int64 member is 8-byte aligned, so every int before one is padded to 8
    r = mq.MqRange64
    assert C.sizeof(r) == 32 and [getattr(r, f).offset for f, _ in r._fields_] == [0, 8, 16, 24]
    i = mq.MqTopk64Info
    assert [f for f, _ in i._fields_] == ["m", "passed", "candidates", "ties", "path", "levels"]
    assert C.sizeof(i) == 40 and [getattr(i, f).offset for f, _ in i._fields_] == [0, 8, 16, 24, 32, 36]
    for f in ("uint64_t m;", "uint64_t passed;", "uint64_t candidates;", "uint64_t ties;", "int32_t  path;", "int32_t  levels;"):
        assert f in dev_h.split("typedef struct mq_topk64_info {")[1].split("}")[0], f
    o = mq.MqGroupOrder
    assert [f for f, _ in o._fields_] == ["order_by", "descending", "k", "having_by", "having", "path", "cand_cap"]
    assert C.sizeof(o) == 72 and [getattr(o, f).offset for f, _ in o._fields_] == [0, 4, 8, 16, 24, 56, 64]
    body = dev_h.split("typedef struct mq_group_order {")[1].split("} mq_group_order;")[0]
    order = [body.index(s) for s in ("int order_by;", "int descending;", "uint64_t k;", "int having_by;", "mq_range64 having;",
                                     "int path;", "uint64_t cand_cap;")]
    assert order == sorted(order)


def test_key_orders_as_the_values_do():
    lib = mq.load()
    key = lib.mq_topk64_key
    edges = [tc.I64_MIN, tc.I64_MIN + 1, -2**32 - 1, -2**32, -2**31 - 1, -2**31, -2, -1, 0, 1, 2, 2**31 - 1, 2**31, 2**32,
             2**53, tc.I64_MAX - 1, tc.I64_MAX]
    assert key(tc.I64_MIN, 0) == 0 and key(tc.I64_MAX, 0) == 2**64 - 1
    assert key(tc.I64_MIN, 1) == 2**64 - 1 and key(tc.I64_MAX, 1) == 0 and key(0, 0) == 2**63
    for a in edges:
        for b in edges:
            assert (key(a, 0) < key(b, 0)) == (a < b), (a, b)
            assert (key(a, 1) < key(b, 1)) == (a > b), (a, b)
            assert (key(a, 0) == key(b, 0)) == (a == b) and (key(a, 7) == key(b, 7)) == (a == b)
    rng = np.random.default_rng(64)
    pairs = rng.integers(tc.I64_MIN, tc.I64_MAX, (2000, 2), endpoint=True, dtype=np.int64)
    pairs[::5, 1] = pairs[::5, 0] + rng.integers(-2, 3, len(pairs[::5]))  # near pairs (wrap-around is still a pair)
    for a, b in pairs.tolist():
        assert (key(a, 0) < key(b, 0)) == (a < b) and (key(a, 1) < key(b, 1)) == (a > b), (a, b)
    # the key is what the model sorts by: ascending key order is the model's order
    v = tc.values_of("full_range", 65)
    for desc in (0, 1):
        ks = np.array([key(int(x), desc) for x in v], dtype=np.uint64)
        assert np.array_equal(np.argsort(ks, kind="stable"), tc.topk64(v, None, None, 65, bool(desc)))


def test_auto_rule_needs_no_device():
    lib = mq.load()
    cap = lib.mq_topk_default_cap()
    div = mq.MQ_TOPK_SORT_DIV
    for n, k, c in [(0, 0, 0), (1, 1, 0), (2**26, 10, 0), (2**26, 1 << 20, 0), (8 * cap, cap, 0), (8 * cap, cap + 1, 0),
                    (4000, 10, 1), (4000, 999, 1), (4000, 1000, 1), (4000, 5000, 7), (40, 3, 7), (40, 4, 7),
                    (2**26, tc.K_ALL, 0), (4097, tc.K_ALL, 1)]:
        ce = c or cap
        want = mq.MQ_TOPK_SORT if min(k, n) + ce > n // div else mq.MQ_TOPK_SELECT
        assert lib.mq_topk64_auto_path(n, k, c) == want, (n, k, c)
        assert lib.mq_topk64_auto_path(n, k, c) == lib.mq_topk_auto_path(n, k, c)  # one rule
    n, c = 4097, 7
    edge = n // div - c  # k + cap == n / DIV: the last k that selects
    assert lib.mq_topk64_auto_path(n, edge, c) == mq.MQ_TOPK_SELECT and lib.mq_topk64_auto_path(n, edge + 1, c) == mq.MQ_TOPK_SORT


def test_model_is_consistent():
    """The restatement against a plain sorted(passing, key=(v[i], i)): repeats, both ends of int64, both
    directions, every kind of filter, and index order without values."""
    n = 300
    rng = np.random.default_rng(6)
    v = rng.integers(-20, 9, n).astype(np.int64) * (1 << 40)
    v[17], v[200], v[201] = tc.I64_MIN, tc.I64_MAX, tc.I64_MAX
    second = tc.second_of(n)
    vl, sl = v.tolist(), second.tolist()
    for having, hl, (low, high) in [(None, None, (None, None)), (second, sl, (25, 75)), (second, sl, (50, None)),
                                    (second, sl, (None, 30)), (second, sl, (200, 300)), (v, vl, (0, None)),
                                    (v, vl, (None, tc.I64_MAX)), (v, vl, (5, 5))]:
        passing = [i for i in range(n) if hl is None or ((low is None or hl[i] >= low) and (high is None or hl[i] < high))]
        assert tc.mask_of(having, (low, high), n).sum() == len(passing)
        if having is v and high == tc.I64_MAX:
            assert 200 not in passing and 17 in passing
        for desc in (False, True):
            idx = sorted(passing, key=lambda i: ((-vl[i] if desc else vl[i]), i))
            for k in (0, 1, 7, len(passing) - 1, len(passing), len(passing) + 5, tc.K_ALL):
                if k < 0:
                    continue
                m = min(k, len(passing))
                assert tc.topk64(v, having, (low, high), k, desc).tolist() == idx[:m], (desc, k)
                assert tc.topk64(None, having, (low, high), k, desc, n=n).tolist() == passing[:m]
                t = vl[idx[m - 1]] if m else None
                assert tc.ties_left_out(v, having, (low, high), k, desc) == (sum(vl[i] == t for i in idx[m:]) if m else 0)
    # the named sets are what they say
    n = 4097
    key = lambda a: a.view(np.uint64) ^ np.uint64(1 << 63)
    assert len(np.unique(tc.values_of("all_equal", n))) == 1 and len(np.unique(tc.values_of("two_values", n))) == 2
    f = tc.values_of("full_range", n)
    assert f.min() == tc.I64_MIN and f.max() == tc.I64_MAX
    c = tc.values_of("counts", n)
    assert c.min() >= 0 and len(np.unique(key(c) >> np.uint64(20))) == 1
    w = tc.values_of("int32_widened", n)
    assert w.min() == -2**31 and w.max() == 2**31 - 1
    for j in range(1, 6):
        a = key(tc.values_of(f"shared_{11 * j}", n))
        assert len(np.unique(a >> np.uint64(64 - 11 * j))) == 1
        nxt = (a >> np.uint64(max(64 - 11 * (j + 1), 0))) & np.uint64(2047 if j < 5 else 511)
        assert len(np.unique(nxt)) > 400, j
    assert len(np.unique(tc.values_of("shared_55", n))) < n  # repeats
    assert np.all(np.diff(tc.values_of("sorted_asc", n)) >= 0) and np.all(np.diff(tc.values_of("sorted_desc", n)) <= 0)
    s = tc.values_of("straddle", tc.BIG)
    assert np.all(s[tc.BIG // 8:tc.BIG - tc.BIG // 8] == 0) and s.min() < 0 < s.max()
    for name in tc.FILTERS:
        having, _ = tc.filter_of(name, f)
        assert having in (None, "second", "vals")
