"""top k over int64 entries with a filter (HAVING, ORDER BY, LIMIT): the cases and a numpy
restatement, shared by the host and GPU tests of mq_topk64, mq_group_top and group_top_k.

The reference has no such operator, so the model is the definition itself: of the entries that
pass the filter, the first min(k, passed) of a stable sort by value, ascending, or by ~value for
descending, equal values in ascending index order in both directions; index order without values.
"""
from __future__ import annotations

import numpy as np

I64_MIN, I64_MAX = -2**63, 2**63 - 1
K_ALL = 2**64 - 1

# empty; one lane; one wave +- 1; one tile +- 1; several tiles and a ragged one
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
BIG = 300_001  # under a CU limit of 1 or 2: many tiles a block, a real cross-block tie rank
VALUE_SETS = ["all_equal", "two_values", "full_range", "counts", "int32_widened", "shared_11", "shared_22", "shared_33",
              "shared_44", "shared_55", "sorted_asc", "sorted_desc", "straddle"]
FILTERS = ["none", "all_pass", "none_pass", "half", "low_only", "high_only", "on_vals", "high_is_max"]


def mask_of(having, rng, n: int) -> np.ndarray:
    """The passing entries: low <= having < high, either bound None; everything without a filter."""
    if having is None:
        return np.ones(n, dtype=bool)
    low, high = rng
    m = np.ones(n, dtype=bool)
    if low is not None:
        m &= having >= low
    if high is not None:
        m &= having < high
    return m


def topk64(vals, having, rng, k: int, desc: bool, n: int | None = None) -> np.ndarray:
    """The indices of the result, in output order."""
    n = len(vals) if vals is not None else len(having) if having is not None else n
    idx = np.flatnonzero(mask_of(having, rng, n))
    if vals is None:
        return idx[:k]
    v = np.asarray(vals, dtype=np.int64)
    return idx[np.argsort(~v[idx] if desc else v[idx], kind="stable")][:k]


def ties_left_out(vals, having, rng, k: int, desc: bool) -> int:
    """Passing entries equal to the last value taken that were not taken (tests/topkcases.py's,
    widened to int64 and restricted to the passing entries)."""
    v = np.asarray(vals, dtype=np.int64)[mask_of(having, rng, len(vals))]
    m = min(k, len(v))
    if m == 0:
        return 0
    s = v[np.argsort(~v if desc else v, kind="stable")]  # monotone
    t = s[m - 1]
    if desc:
        return int(len(s) - np.searchsorted(s[::-1], t, side="left")) - m
    return int(np.searchsorted(s, t, side="right")) - m


def _u2i(u: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(u.astype(np.uint64)).view(np.int64)


def values_of(name: str, n: int) -> np.ndarray:
    """The value column of a named set, n int64 entries."""
    rng = np.random.default_rng(37 * n + VALUE_SETS.index(name))
    if name == "all_equal":
        v = np.full(n, -12345678901234)
    elif name == "two_values":
        v = np.where(rng.integers(0, 2, n) == 1, 7 << 40, -3)
    elif name == "full_range":  # both ends present from two entries on: the sign flip and the complement
        v = rng.integers(I64_MIN, I64_MAX, n, endpoint=True, dtype=np.int64)
        if n >= 2:
            v[n // 2], v[n // 3] = I64_MIN, I64_MAX
    elif name == "counts":  # a widened u64 count: small, never negative; five digits are one bin
        v = rng.integers(0, 1000, n)
    elif name == "int32_widened":  # a widened int32 min or max: the sign extension
        v = rng.integers(-2**31, 2**31 - 1, n, endpoint=True)
        if n >= 2:
            v[n // 2], v[n // 3] = -2**31, 2**31 - 1
    elif name.startswith("shared_"):  # the top 11 j bits are one value: digit j + 1 decides (j = 5: repeats)
        bits = int(name[7:])
        free = 64 - bits
        top = np.uint64((0xB5A69C3D2E1F4788 >> free) << free)
        v = _u2i(top | rng.integers(0, 1 << free, n, dtype=np.uint64))
    elif name == "sorted_asc":
        v = np.sort(rng.integers(-1000, 1000, n)) * (1 << 33)
    elif name == "sorted_desc":
        v = np.sort(rng.integers(-1000, 1000, n))[::-1] * (1 << 33)
    elif name == "straddle":  # one value in a long middle run (it crosses every block edge a
        v = rng.integers(-50, 50, n)  # CU limit of 1 or 2 puts there), noise around it
        v[n // 8:n - n // 8] = 0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, dtype=np.int64)


def second_of(n: int) -> np.ndarray:
    """The filter column of the filters that do not look at the values: 0 .. 99."""
    return np.ascontiguousarray(np.random.default_rng(n + 11).integers(0, 100, n), dtype=np.int64)


def filter_of(name: str, vals: np.ndarray):
    """(having, (low, high)) of a named filter: having is None, "second" or "vals"."""
    if name == "none":
        return None, (None, None)
    if name == "all_pass":
        return "second", (0, 100)
    if name == "none_pass":
        return "second", (200, 300)
    if name == "half":
        return "second", (25, 75)
    if name == "low_only":
        return "second", (50, None)
    if name == "high_only":
        return "second", (None, 30)
    if name == "on_vals":  # from the median up
        return "vals", (int(np.sort(vals)[len(vals) // 2]) if len(vals) else 0, None)
    if name == "high_is_max":  # `<` excludes INT64_MAX itself
        return "vals", (None, I64_MAX)
    raise KeyError(name)


def ks_of(n: int, passed: int) -> list[int]:
    return sorted({k for k in (0, 1, 2, 63, 64, 65, passed - 1, passed, passed + 5, n + 5, K_ALL) if k >= 0})
