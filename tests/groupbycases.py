"""GROUP BY over several int32 key columns: the cases and a numpy restatement, shared by the
host and GPU tests of group_aggregate_by and of mq_group_by_plan / _write behind it.

The reference has no such operator, so the model is the definition itself: one entry per
distinct tuple (K_0[i], .., K_{nkeys-1}[i]), in ascending lexicographic order with K_0 the most
significant and every component compared as signed int32, with the rows' count, exact int64
sum, min and max.
"""
from __future__ import annotations

import numpy as np

import groupcases as gc

I32_MIN, I32_MAX = gc.I32_MIN, gc.I32_MAX
MAX_KEYS = 4
TUPLE_SETS = ["one_tuple", "seven_shuffled", "seven_sorted", "space_S", "space_S_plus_1", "ends_x_one", "all_distinct",
              "skewed", "last_differs", "first_differs", "first_two_last_many"]


def group_by(keys_list, vals):
    """(list of nkeys key columns, count u64, sum i64, min i32, max i32), one entry per
    distinct tuple, ascending lexicographically (keys_list[0] the most significant)."""
    keys_list = [np.asarray(k, dtype=np.int32) for k in keys_list]
    vals = np.asarray(vals, dtype=np.int32)
    assert keys_list and all(k.shape == vals.shape for k in keys_list)
    if len(vals) == 0:
        return ([np.empty(0, np.int32) for _ in keys_list], np.empty(0, np.uint64), np.empty(0, np.int64),
                np.empty(0, np.int32), np.empty(0, np.int32))
    order = np.lexsort(keys_list[::-1])  # lexsort's last key is the primary one
    ks, v = [k[order] for k in keys_list], vals[order]
    differs = np.zeros(len(v) - 1, dtype=bool)
    for k in ks:
        differs |= k[1:] != k[:-1]
    heads = np.flatnonzero(np.concatenate([[True], differs]))
    count = np.diff(np.concatenate([heads, [len(v)]])).astype(np.uint64)
    return ([k[heads] for k in ks], count, np.add.reduceat(v.astype(np.int64), heads), np.minimum.reduceat(v, heads),
            np.maximum.reduceat(v, heads))


def _split(width: int, parts: int):
    """`parts` ranges >= 1 whose product is exactly `width`: the prime factors of width dealt
    round-robin (a prime width gives (width, 1, ..))."""
    f, w, p = [], width, 2
    while w > 1:
        while w % p == 0:
            f.append(p)
            w //= p
        p += 1
    r = [1] * parts
    for i, q in enumerate(sorted(f, reverse=True)):
        r[i % parts] *= q
    assert int(np.prod(r)) == width
    return r


def tuples_of(name: str, n: int, nkeys: int, slots: int):
    """The nkeys key columns of a named set: n rows each; slots = mq_group_dense_slots()."""
    rng = np.random.default_rng(31 * n + 7 * nkeys + TUPLE_SETS.index(name))
    lo = [-5, 100, -1000, 7][:nkeys]  # every column has its own lower bound, one of them negative
    if name == "one_tuple":
        cols = [np.full(n, lo[j] - 12345) for j in range(nkeys)]
    elif name in ("seven_shuffled", "seven_sorted"):
        # seven tuples spread over 3 x 4 (x 2 x 2) values; sorted: wave-uniform tiles, runs that span tiles
        base = np.array([[0, 0, 0, 0], [0, 3, 1, 0], [1, 0, 0, 1], [1, 1, 1, 1], [2, 0, 1, 0], [2, 2, 0, 0], [2, 3, 1, 1]])
        pick = rng.integers(0, 7, n)
        if name == "seven_sorted":
            pick = np.sort(pick)
        cols = [base[pick, j] + lo[j] for j in range(nkeys)]
    elif name in ("space_S", "space_S_plus_1"):
        # ranges whose product is exactly the width; both ends of every column present from two rows on
        ranges = _split(slots if name == "space_S" else slots + 1, nkeys)
        cols = [rng.integers(0, r, n) + lo[j] for j, r in enumerate(ranges)]
        if n >= 2:
            for j, r in enumerate(ranges):
                cols[j][0], cols[j][-1] = lo[j], lo[j] + r - 1
    elif name == "ends_x_one":  # (int32_ends, one_key, ..): a key space of exactly 2^32
        cols = [gc.keys_of("int32_ends", n, slots)] + [np.full(n, 77 + j) for j in range(1, nkeys)]
    elif name == "all_distinct":  # all-distinct tuples from columns that each repeat
        side = int(np.ceil(np.sqrt(max(n, 1))))
        code = rng.permutation(n)
        cols = [code // side - side // 2, code % side] + [np.full(n, j) for j in range(2, nkeys)]
    elif name == "skewed":  # 90 % of the rows in one tuple, the rest spread over `slots` tuples
        ranges = _split(slots, nkeys)
        hot = rng.random(n) < 0.9
        cols = [np.where(hot, lo[j] + r // 2, rng.integers(0, r, n) + lo[j]) for j, r in enumerate(ranges)]
    elif name in ("last_differs", "first_differs"):  # one component varies, the others are constant
        cols = [np.full(n, lo[j]) for j in range(nkeys)]
        cols[nkeys - 1 if name == "last_differs" else 0] = rng.integers(-40, 41, n)
    elif name == "first_two_last_many":  # a swapped significance order changes the output order
        cols = [np.full(n, lo[j]) for j in range(nkeys)]
        cols[0] = np.where(rng.integers(0, 2, n) == 1, 9, -9)
        cols[nkeys - 1] = rng.integers(-40, 41, n)
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(c, dtype=np.int32) for c in cols]


def bounds_of(keys_list):
    """{lo0, hi0, lo1, hi1, ..} of the columns as a flat list of Python ints; [] for no rows."""
    if len(keys_list[0]) == 0:
        return []
    return [int(f(k)) for k in keys_list for f in (np.min, np.max)]


def space_of(bounds) -> int:
    """prod(hi_j - lo_j + 1) in Python integers (unbounded; the library saturates at 2^63)."""
    p = 1
    for lo, hi in zip(bounds[::2], bounds[1::2]):
        p *= hi - lo + 1
    return p
