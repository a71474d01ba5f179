"""top k: the cases and a numpy restatement, shared by the host and GPU tests of top_k and
of the device entry point behind it (mq_topk).

The reference has no such operator, so the model is the definition itself: the first
m = min(k, n) entries of a stable sort of the rows, ascending by value or descending by
value, equal values in ascending input order in both directions.
"""
from __future__ import annotations

import numpy as np

I32_MIN, I32_MAX = -2**31, 2**31 - 1

# empty; one lane; one wave +- 1; one tile +- 1; several tiles and a ragged one
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
BIG = 300_001  # under a CU limit of 1 or 2: many tiles a block, a real cross-block tie rank
VALUE_SETS = ["all_equal", "two_values", "full_range", "uniform_100", "top11_shared", "top22_shared",
              "sorted_asc", "sorted_desc", "straddle"]


def order(vals: np.ndarray, descending: bool) -> np.ndarray:
    """Row ids in output order: a stable sort by v, or by ~v (signed order reversed, no overflow)."""
    vals = np.asarray(vals, dtype=np.int32)
    return np.argsort(~vals if descending else vals, kind="stable")


def topk(vals: np.ndarray, payload, k: int, descending: bool):
    """(values i32, payload i32) of the first min(k, n) rows in output order."""
    vals = np.asarray(vals, dtype=np.int32)
    idx = order(vals, descending)[:min(k, len(vals))]
    pay = idx.astype(np.int32) if payload is None else np.asarray(payload, dtype=np.int32)[idx]
    return vals[idx], pay


def ties_left_out(vals: np.ndarray, k: int, descending: bool, idx=None) -> int:
    """Rows equal to the last value taken that were not taken (idx: order(vals, descending),
    when the caller has it already)."""
    m = min(k, len(vals))
    if m == 0:
        return 0
    s = vals[order(vals, descending) if idx is None else idx]  # monotone
    t = s[m - 1]
    if descending:
        return int(len(s) - np.searchsorted(s[::-1], t, side="left")) - m
    return int(np.searchsorted(s, t, side="right")) - m


def values_of(name: str, n: int) -> np.ndarray:
    """The value column of a named set, n rows."""
    rng = np.random.default_rng(31 * n + VALUE_SETS.index(name))
    if name == "all_equal":
        v = np.full(n, -12345)
    elif name == "two_values":
        v = np.where(rng.integers(0, 2, n) == 1, 7, -3)
    elif name == "full_range":  # both ends present from two rows on: the sign flip and the complement
        v = rng.integers(I32_MIN, I32_MAX, n, endpoint=True)
        if n >= 2:
            v[n // 2], v[n // 3] = I32_MIN, I32_MAX
    elif name == "uniform_100":  # the first two digits are one bin
        v = rng.integers(0, 100, n)
    elif name == "top11_shared":  # the second digit decides
        v = (0x5A5 << 21) - 2**31 + rng.integers(0, 1 << 21, n)
    elif name == "top22_shared":  # the third digit decides, with repeats
        v = (0x2B3C4D << 10) - 2**31 + rng.integers(0, 1 << 10, n)
    elif name == "sorted_asc":
        v = np.sort(rng.integers(-1000, 1000, n))
    elif name == "sorted_desc":
        v = np.sort(rng.integers(-1000, 1000, n))[::-1]
    elif name == "straddle":  # one value in a long middle run (it crosses every block edge a
        v = rng.integers(-50, 50, n)  # CU limit of 1 or 2 puts there), noise around it
        v[n // 8:n - n // 8] = 0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, dtype=np.int32)


def payload_of(n: int) -> np.ndarray:
    """A positions vector that is no function of the row's rank: ties must follow i, not it."""
    return np.ascontiguousarray(np.random.default_rng(n + 3).permutation(n)[::-1] * 3 - n, dtype=np.int32)


def ks_of(n: int) -> list[int]:
    return sorted({k for k in (0, 1, 2, 63, 64, 65, n - 1, n, n + 5) if k >= 0})
