"""Grouped aggregates: the cases and a numpy restatement, shared by the host and GPU tests
of group_aggregate and of the device entry points behind it (mq_group_plan / _write).

The reference has no such operator, so the model is the definition itself: one entry per
distinct key, in ascending signed key order, with the rows' count, exact int64 sum, min
and max.
"""
from __future__ import annotations

import numpy as np

I32_MIN, I32_MAX = -2**31, 2**31 - 1

# empty; one lane; one wave +- 1; one tile +- 1; several blocks; several tiles a wave in flight
SIZES = [0, 1, 63, 64, 65, 1023, 1025, 4097, 70_001, 300_001]
KEY_SETS = ["one_key", "seven_shuffled", "seven_sorted", "uniform_100", "range_S", "range_S_plus_1",
            "int32_ends", "all_distinct", "skewed"]
VALUE_SETS = ["uniform", "all_max", "all_min", "keys"]


def group(keys: np.ndarray, vals: np.ndarray):
    """(keys, count u64, sum i64, min i32, max i32), one entry per distinct key, ascending."""
    keys = np.asarray(keys, dtype=np.int32)
    vals = np.asarray(vals, dtype=np.int32)
    assert keys.shape == vals.shape
    if len(keys) == 0:
        return (np.empty(0, np.int32), np.empty(0, np.uint64), np.empty(0, np.int64), np.empty(0, np.int32),
                np.empty(0, np.int32))
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], vals[order]
    heads = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    count = np.diff(np.concatenate([heads, [len(k)]])).astype(np.uint64)
    return (k[heads], count, np.add.reduceat(v.astype(np.int64), heads), np.minimum.reduceat(v, heads),
            np.maximum.reduceat(v, heads))


def keys_of(name: str, n: int, slots: int) -> np.ndarray:
    """The key column of a named set: n rows; slots = mq_group_dense_slots()."""
    rng = np.random.default_rng(17 * n + KEY_SETS.index(name))
    seven = np.array([-900, -3, 0, 1, 2, 500, 1000])
    if name == "one_key":
        k = np.full(n, -12345)
    elif name == "seven_shuffled":
        k = seven[rng.integers(0, 7, n)]
    elif name == "seven_sorted":  # wave-uniform keys; on the sort path, runs that span tiles
        k = np.sort(seven[rng.integers(0, 7, n)])
    elif name == "uniform_100":
        k = rng.integers(-50, 50, n)
    elif name in ("range_S", "range_S_plus_1"):  # both end keys present from two rows on
        width = slots if name == "range_S" else slots + 1
        k = rng.integers(0, width, n) - 1000
        if n >= 2:
            k[0], k[-1] = -1000, width - 1001
    elif name == "int32_ends":
        k = np.where(rng.integers(0, 2, n) == 1, I32_MAX, I32_MIN)
        if n >= 2:
            k[0], k[-1] = I32_MAX, I32_MIN
    elif name == "all_distinct":
        k = rng.permutation(n) - n // 2
    elif name == "skewed":  # 90 % of the rows one key, the rest spread over `slots` keys
        k = np.where(rng.random(n) < 0.9, 77, rng.integers(0, slots, n))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(k, dtype=np.int32)


def values_of(name: str, keys: np.ndarray) -> np.ndarray:
    n = len(keys)
    if name == "uniform":
        v = np.random.default_rng(n + 5).integers(I32_MIN, I32_MAX, n, endpoint=True)
    elif name == "all_max":  # at n = 70_001 one key's sum passes 2^47
        v = np.full(n, I32_MAX)
    elif name == "all_min":
        v = np.full(n, I32_MIN)
    elif name == "keys":
        return keys
    else:
        raise KeyError(name)
    return np.ascontiguousarray(v, dtype=np.int32)


def key_range(keys: np.ndarray) -> int:
    """hi - lo + 1 in Python integers (up to 2^32); 0 for no rows."""
    return int(keys.max()) - int(keys.min()) + 1 if len(keys) else 0
