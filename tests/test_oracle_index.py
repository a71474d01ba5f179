"""Pin the index-build restatement (oracle/refcpu.c rc_index_build_lomuto /
rc_histogram, composed as build_index in tests/indexcases.py model()) against the
reference's own build_index (tests/golden/index_goldens.json, from
oracle/_ref/libdbm.so) and its own quicksort symbol: exact, equal values included.
And the sorted-index select restatement (rc_index_select) against a closed form on
every small case and against the reference's own select_column_sorted_index.
CPU only.
"""
import bisect
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from indexcases import cases, csv_text, model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "index_goldens.json")))
CASES = {name: (cols, spec) for name, cols, spec in cases()}


def digest(refcpu, c, spec):
    f = lambda x: f"{refcpu.fnv1a64(np.ascontiguousarray(x)):016x}"  # noqa: E731
    d = {"cols": [f(col.astype(np.int32)) for col in c["cols"]]}
    for j, clustered in spec:
        d[f"ix{j}_values"] = f(np.asarray(c[f"ix{j}_values"], dtype=np.int32))
        d[f"ix{j}_positions"] = f(np.asarray(c[f"ix{j}_positions"], dtype=np.uint64))
        if not clustered:
            d[f"hist{j}_bin_size"] = int(c[f"hist{j}_bin_size"])
            d[f"hist{j}_values"] = [int(v) for v in c[f"hist{j}_values"]]
            d[f"hist{j}_counts"] = [int(v) for v in c[f"hist{j}_counts"]]
    return d


def check_index_result(refcpu, name, result):
    """result: a build_index outcome (cols + ix*/hist* arrays) for case `name`."""
    g = GOLD[name]
    spec = [tuple(x) for x in g["spec"]]
    got = digest(refcpu, result, spec)
    for k, v in got.items():
        assert v == g[k], (name, k)


def test_index_inputs_match_goldens(refcpu):
    assert set(CASES) == set(GOLD)
    for name, (cols, spec) in CASES.items():
        assert f"{refcpu.fnv1a64_bytes(csv_text(cols)):016x}" == GOLD[name]["in_fnv"], name
        assert [tuple(x) for x in GOLD[name]["spec"]] == [tuple(x) for x in spec]


@pytest.mark.parametrize("name", sorted(CASES))
def test_index_restatement_vs_reference_goldens(refcpu, name):
    cols, spec = CASES[name]
    check_index_result(refcpu, name, model(refcpu, cols, spec))


def test_index_restatement_is_stable(refcpu):
    rng = np.random.default_rng(3)
    col = rng.integers(-5, 5, 10_000).astype(np.int32)
    v, p = refcpu.index_build(col)
    assert np.array_equal(v, np.sort(col, kind="stable"))
    assert np.array_equal(p, np.argsort(col, kind="stable").astype(np.uint64))


def _lomuto_inputs():
    rng = np.random.default_rng(11)
    yield "empty", np.zeros(0, np.int32)
    yield "one", np.array([5], np.int32)
    yield "all_equal", np.full(700, 3, np.int32)
    yield "sorted", np.arange(900, dtype=np.int32)
    yield "reverse", np.arange(900, 0, -1).astype(np.int32)
    yield "two_values", rng.integers(0, 2, 1500).astype(np.int32)
    yield "few_values", rng.integers(-3, 4, 2000).astype(np.int32)
    yield "dups", rng.integers(0, 200, 3000).astype(np.int32)
    yield "distinct", rng.permutation(3000).astype(np.int32)
    yield "extremes", rng.choice(np.array([-2**31, 2**31 - 1, 0, -1, 1], np.int32), 1200)
    yield "sorted_dups", np.sort(rng.integers(0, 50, 1000)).astype(np.int32)
    yield "organ_pipe", np.concatenate([np.arange(500), np.arange(500, 0, -1)]).astype(np.int32)


@pytest.mark.parametrize("name,col", list(_lomuto_inputs()))
def test_lomuto_restatement_equals_reference_quicksort(refcpu, name, col):
    """rc_index_build_lomuto against the reference's own quicksort symbol (libdbm.so):
    values AND positions identical, equal values included."""
    import refload
    if not refload.have():
        pytest.skip("oracle/_ref/libdbm.so not built (no /root/reference)")
    rv, rp = refload.quicksort(col)
    v, p = refcpu.index_build_lomuto(col)
    assert np.array_equal(v, rv), name
    assert np.array_equal(p, rp), name


def _qs_goldens():
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quicksort_goldens.json")
    return [c for c in json.load(open(path)) if c["log2n"] == 22]


@pytest.mark.parametrize("case", _qs_goldens(), ids=lambda c: f"s{c['seed']}_m{c['modulus']}")
def test_lomuto_restatement_2e22_vs_reference_quicksort(refcpu, case):
    """rc_index_build_lomuto (the iterative restatement the GPU
    tests compare with) against the reference's own quicksort at 2^22 rows: the
    goldens that symbol produced (make_quicksort_goldens.py) and, where libdbm.so is
    built, a fresh run of the symbol itself on the seed-42 column."""
    n = case["n"]
    col = refcpu.gen_uniform(n, case["seed"], case["modulus"])
    assert f"{refcpu.fnv1a64(col):016x}" == case["col_fnv"]
    v, p = refcpu.index_build_lomuto(col)
    assert f"{refcpu.fnv1a64(v):016x}" == case["values_fnv"]
    assert f"{refcpu.fnv1a64(p):016x}" == case["positions_fnv"]
    assert int(np.count_nonzero(v[1:] == v[:-1])) == case["ties"]
    import refload
    if case["seed"] == 42 and refload.have():
        rv, rp = refload.quicksort(col)
        assert np.array_equal(v, rv) and np.array_equal(p, rp)


# ---------------------------------------------------------------------------
# sorted-index select: rc_index_select
# ---------------------------------------------------------------------------
I32MAX = 2 ** 31 - 1


def closed_form_run(values, low, high):
    """(first row, K) of the sorted-index select over the ascending list `values`.
    With lb(x) the first row whose value is >= x: the run is [lb(low), lb(high) - 1],
    except that a `high` present in the column with low <= high never leaves the run
    empty (the reference's walk down the run of `high` stops at `left`): one row then."""
    left = bisect.bisect_left(values, low)
    right = bisect.bisect_left(values, high) - 1
    if low <= high and right + 1 < len(values) and values[right + 1] == high:
        right = max(right, left)
    return left, max(0, right - left + 1)


def test_index_select_restatement_vs_closed_form(refcpu):
    """Every non-decreasing column of 1..7 rows over {0..4} and every low, high in
    -1..5, bounds below the first value (the two defined extensions) included."""
    ncases = 0
    for n in range(1, 8):
        positions = (np.arange(n, dtype=np.uint64) * 7 + 3)[::-1].copy()
        want_pos = positions.astype(np.int32)
        for vals in itertools.combinations_with_replacement(range(5), n):
            v = np.array(vals, dtype=np.int32)
            for low in range(-1, 6):
                for high in range(-1, 6):
                    left, k = closed_form_run(vals, low, high)
                    got = refcpu.index_select(v, positions, low, high)
                    assert np.array_equal(got, want_pos[left:left + k]), (vals, low, high)
                    ncases += 1
    assert ncases == 38_759


def _ref_select_columns():
    """name, unsorted column: distinct values, short runs (both with gaps, so a value's
    neighbours are absent), all-equal, and values up to INT32_MAX, at 1, 2, 65 and 4097 rows."""
    rng = np.random.default_rng(21)
    for n in (1, 2, 65, 4097):
        yield f"distinct_{n}", (rng.permutation(n) * 3 + 10).astype(np.int32)
        yield f"runs_{n}", (rng.integers(0, n // 3 + 1, n) * 3 - 6).astype(np.int32)
        yield f"equal_{n}", np.full(n, 7, dtype=np.int32)
        top = rng.integers(I32MAX - 8, I32MAX, n, endpoint=True).astype(np.int32)
        top[0] = I32MAX
        yield f"int32max_{n}", top


def _ref_select_bounds(values):
    """(low, high) pairs the reference defines: both >= values[0] (below that its unsigned
    binary_search reads out of bounds). The first, a middle and the last value, each -1,
    +0 and +1, a bound well above the last value and INT32_MAX, in every pair: low > high,
    low == high, and high present with nothing in [low, high) are among them."""
    u = np.unique(values)
    picks = {int(u[0]), int(u[len(u) // 2]), int(u[-1])}
    cand = {p + d for p in picks for d in (-1, 0, 1)} | {int(u[-1]) + 1000, I32MAX}
    cand = sorted(c for c in cand if int(values[0]) <= c <= I32MAX)
    for low in cand:
        for high in cand:
            assert low >= values[0] and high >= values[0], (low, high)  # never call the reference below
            yield low, high


def test_index_select_restatement_vs_reference(refcpu):
    """rc_index_select against the reference's own select_column_sorted_index
    (oracle/_ref/libref.so), the indexed column built as the drop-in test builds it."""
    if not refcpu.have_reference():
        pytest.skip("oracle/_ref/libref.so not built (no reference sources)")
    from refapi import make_column, mq, take
    ref = refcpu.reference()
    seen = {"low == high present": 0, "high present, [low, high) empty": 0, "low > high": 0,
            "both above the last value": 0, "INT32_MAX bound": 0, "INT32_MAX value": 0}
    for name, d in _ref_select_columns():
        order = np.argsort(d, kind="stable")
        values = np.ascontiguousarray(d[order])
        positions = np.ascontiguousarray(order.astype(np.uint64))
        ix = mq.ColumnIndex()
        ix.values = values.ctypes.data_as(C.POINTER(C.c_int))
        ix.positions = positions.ctypes.data_as(C.POINTER(C.c_size_t))
        col = make_column(d)
        col.has_index = True
        col.index = C.pointer(ix)
        vlist = values.tolist()
        for low, high in _ref_select_bounds(values):
            st = mq.Status(0, None)
            want = take(ref.select_column_sorted_index(C.byref(col), low, high, C.byref(st)))
            assert st.code == mq.OK
            got = refcpu.index_select(values, positions, low, high)
            assert np.array_equal(got, want), (name, low, high)
            left, k = closed_form_run(vlist, low, high)
            assert np.array_equal(got, positions[left:left + k].astype(np.int32)), (name, low, high)
            present = bisect.bisect_left(vlist, high) < bisect.bisect_right(vlist, high)
            seen["low == high present"] += low == high and present
            seen["high present, [low, high) empty"] += (low < high and present and
                                                      bisect.bisect_left(vlist, low) == bisect.bisect_left(vlist, high))
            seen["low > high"] += low > high
            seen["both above the last value"] += low > vlist[-1] and high > vlist[-1]
            seen["INT32_MAX bound"] += I32MAX in (low, high)
            seen["INT32_MAX value"] += vlist[-1] == I32MAX
    assert all(seen.values()), seen
