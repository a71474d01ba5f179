"""select_where_in: the cases and a numpy restatement, shared by the host and GPU tests of
select_where_in / aggregate_where_in and of the device entry points behind them
(mq_keyset_build, mq_semi_positions, mq_semi_agg).

The reference has no such operator, so the model is the definition itself: row i matches when
every range holds for it (wherecases.mask) and key[i] is among the set keys (np.isin), or, for
the anti form, is not. With no range every row passes the ranges.

A named set is (key column of n rows, set keys): the sets are chosen for where a bitmap over
[min, max] of the set keys with the bit index (uint32)(key - lo) can go wrong: both ends of
int32, keys just outside the span, spans around a word, duplicates, and the empty set.
"""
from __future__ import annotations

import numpy as np

import wherecases as wc

I32_MIN, I32_MAX = wc.I32_MIN, wc.I32_MAX
NCOLS = [0, 1, 3, 8]
SETS = ["dense_small", "sparse_wide", "single", "negative", "min_edge", "max_edge", "every_key", "empty", "dups"]


def hit(key, set_keys) -> np.ndarray:
    return np.isin(np.asarray(key, dtype=np.int32), np.asarray(set_keys, dtype=np.int32))


def mask(cols, ranges, key, set_keys, anti=False) -> np.ndarray:
    m = wc.mask(cols, ranges) if len(cols) else np.ones(len(key), dtype=bool)
    h = hit(key, set_keys)
    return m & (~h if anti else h)


def positions(cols, ranges, key, set_keys, anti=False, payload=None) -> np.ndarray:
    idx = np.flatnonzero(mask(cols, ranges, key, set_keys, anti))
    return idx.astype(np.int32) if payload is None else np.asarray(payload, dtype=np.int32)[idx]


def aggregate(cols, ranges, key, set_keys, val, anti=False):
    """(count, sum, min, max) of val over the matching rows, as mq_agg holds them."""
    v = np.asarray(val, dtype=np.int32)[mask(cols, ranges, key, set_keys, anti)].astype(np.int64)
    if len(v) == 0:
        return 0, 0, I32_MAX, I32_MIN
    return len(v), int(v.sum()), int(v.min()), int(v.max())


def span_bytes(set_keys) -> int:
    """Size of the bitmap over [min, max]: one bit a value, rounded up to 16 bytes."""
    s = np.asarray(set_keys, dtype=np.int64)
    return 0 if len(s) == 0 else (int(s.max() - s.min()) + 128) // 128 * 16


def keyset(name: str, n: int):
    """(key column of n rows, set keys) of a named set, both int32."""
    rng = np.random.default_rng(7000 * SETS.index(name) + n)
    pick = lambda pool: rng.choice(np.asarray(pool, dtype=np.int64), n)  # noqa: E731
    if name == "dense_small":  # half of 1000 values; keys a little wider than the span
        s, key = rng.choice(np.arange(100, 1100), 500, replace=False), rng.integers(0, 1200, n)
    elif name == "sparse_wide":  # 2^22 values of span: a bitmap no block holds in LDS
        s = np.concatenate((rng.integers(-2**21, 2**21, 3000), [-2**21, 2**21 - 1]))
        key = np.where(rng.integers(0, 2, n) == 0, pick(s), rng.integers(-2**21 - 50, 2**21 + 50, n))
        if n >= 2:  # one key just below the span and one just above it
            key[n // 3], key[n - 1] = -2**21 - 1, 2**21
    elif name == "single":
        s, key = np.array([7]), rng.integers(5, 10, n)
    elif name == "negative":
        s, key = rng.integers(-5000, -4000, 300), rng.integers(-5100, -3900, n)
    elif name == "min_edge":  # lo = INT32_MIN + 1: key INT32_MIN wraps to the largest offset
        s = np.array([I32_MIN + 1, I32_MIN + 2, I32_MIN + 40, I32_MIN + 1000])
        key = pick([I32_MIN, I32_MIN + 1, I32_MIN + 2, I32_MIN + 3, I32_MIN + 40, I32_MIN + 1000, I32_MIN + 1001, I32_MAX, 0, -1])
    elif name == "max_edge":
        s = np.array([I32_MAX, I32_MAX - 33, I32_MAX - 64])
        key = pick([I32_MAX, I32_MAX - 1, I32_MAX - 33, I32_MAX - 64, I32_MAX - 65, I32_MIN, 0])
    elif name == "every_key":  # the set holds every value of the key column
        key = rng.integers(-300, 300, n)
        s = np.unique(key)
    elif name == "empty":
        s, key = np.empty(0, dtype=np.int64), rng.integers(0, 10, n)
    elif name == "dups":  # 4097 set keys over 50 values
        s, key = rng.integers(0, 50, 4097), rng.integers(-10, 70, n)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(key, dtype=np.int32), np.ascontiguousarray(s, dtype=np.int32)


def case(name: str, n: int, ncols: int):
    """wherecases.case with ncols == 0 allowed: no column, no range."""
    return wc.case(name, n, ncols) if ncols else ([], [])
