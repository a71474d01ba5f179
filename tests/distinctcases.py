"""group_count_distinct: the numpy model and the case generators shared by the host and GPU tests
of mq_group_distinct_plan and of group_count_distinct behind it.

The model: the rows that every range keeps (wherecases.mask; no range keeps every row), np.unique
over the stacked (keys.., v) rows, then np.unique over the key part with counts.
"""
from __future__ import annotations

import numpy as np

import wherecases as wc

I32_MIN, I32_MAX = -2**31, 2**31 - 1
AUTO, LDS, BITMAP, SORT = 0, 1, 2, 3
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 70_001]
SPANS = [1, 31, 32, 33, 64, 65]
LONG_N = 300_007


def mask(cols, ranges, n):
    return wc.mask(cols, ranges) if len(cols) else np.ones(n, dtype=bool)


def model(cols, ranges, keys_list, vals):
    """(key columns int32, distinct counts u64, matching rows, distinct pairs) in ascending
    lexicographic signed order of the key tuples."""
    vals = np.asarray(vals, np.int32)
    m = mask(cols, ranges, len(vals))
    rows = np.stack([np.asarray(k, np.int32)[m].astype(np.int64) for k in keys_list] + [vals[m].astype(np.int64)], axis=1)
    pairs = np.unique(rows, axis=0)
    nk = len(keys_list)
    if len(pairs) == 0:
        return [np.empty(0, np.int32) for _ in range(nk)], np.empty(0, np.uint64), 0, 0
    tuples, counts = np.unique(pairs[:, :nk], axis=0, return_counts=True)
    return [tuples[:, j].astype(np.int32) for j in range(nk)], counts.astype(np.uint64), int(m.sum()), len(pairs)


def brute(cols, ranges, keys_list, vals):
    """The same from a set of Python tuples."""
    seen = set()
    for i in range(len(vals)):
        if all((lo is None or int(c[i]) >= lo) and (hi is None or int(c[i]) < hi) for c, (lo, hi) in zip(cols, ranges)):
            seen.add(tuple(int(k[i]) for k in keys_list) + (int(vals[i]),))
    table = {}
    for t in seen:
        table[t[:-1]] = table.get(t[:-1], 0) + 1
    order = sorted(table)
    return order, [table[t] for t in order]


def matching_bounds(cols, ranges, keys_list, vals):
    """(key bounds {lo0, hi0, ..}, value bounds {lo, hi}) over the matching rows; None without one."""
    m = mask(cols, ranges, len(vals))
    if not m.any():
        return None
    kb = [int(b) for k in keys_list for b in (np.asarray(k)[m].min(), np.asarray(k)[m].max())]
    v = np.asarray(vals)[m]
    return kb, [int(v.min()), int(v.max())]


def shape(kb, vb):
    """(P, W, R, 4 P R) in Python integers."""
    p = 1
    for lo, hi in zip(kb[::2], kb[1::2]):
        p *= hi - lo + 1
    w = vb[1] - vb[0] + 1
    r = (w + 31) // 32
    return p, w, r, 4 * p * r


def paths_of(kb, vb, lds_bytes, bitmap_bytes):
    """(the path AUTO takes, every path whose size rule holds)."""
    p, _, _, b = shape(kb, vb)
    assert p <= 2**32
    ok = ([LDS] if b <= lds_bytes else []) + ([BITMAP] if b <= bitmap_bytes else []) + [SORT]
    return ok[0], ok


def predicates(n, ncols, seed=0):
    """ncols predicate columns uniform in [0, 1000) and ranges that each keep about 80 %."""
    rng = np.random.default_rng(1000 + seed)
    cols = [np.ascontiguousarray(rng.integers(0, 1000, n), dtype=np.int32) for _ in range(ncols)]
    ranges = [((100, None), (None, 900), (50, 950))[c % 3] for c in range(ncols)]
    return cols, ranges


def table(n, key_ranges, vlo, span, seed=0, key_lo=None):
    """Key columns uniform over the given ranges (from key_lo[j], default -2 * j) and values
    uniform over [vlo, vlo + span); the first key tuple holds every value of the span where n
    allows, so that its count is the span, with vlo and vlo + span - 1 among them."""
    rng = np.random.default_rng(seed)
    key_lo = key_lo or [-2 * j for j in range(len(key_ranges))]
    keys = [np.ascontiguousarray(rng.integers(0, r, n) + lo, dtype=np.int32) for r, lo in zip(key_ranges, key_lo)]
    vals = rng.integers(0, span, n) + vlo
    full = min(n, span)
    if full:
        at = rng.permutation(n)[:full]
        for k, lo in zip(keys, key_lo):
            k[at] = lo
        vals[at] = vlo + (np.arange(full) if full == span else np.r_[0, span - 1, rng.integers(0, span, full)][:full])
    return keys, np.ascontiguousarray(vals, dtype=np.int32)
