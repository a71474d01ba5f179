"""group_aggregate_by_where: the named combinations shared by the host and GPU tests of
group_aggregate_by_where and of mq_group_by_where_plan behind it.

The model needs no restatement of its own: it is groupbycases.group_by over the rows that
wherecases.mask keeps.
"""
from __future__ import annotations

import numpy as np

import groupbycases as gb
import groupcases as gc
import wherecases as wc

NKEYS = [2, 3, 4]
TUPLE_SETS = gb.TUPLE_SETS
VALUE_SETS = ["uniform", "all_max", "all_min"]
MANDATORY = [0, 1025, 8193]

POISON_SETS = ["islands_first", "islands_alt", "every_257", "tail_only", "clustered_lead"]
POISON_N = 8215      # 256 whole lines and a last line of 23 rows
POISON_NCOLS = 2     # the second predicate kills some survivors of the first: whole dead lines in the island sets too
POISON_RANGES = [5, 4, 3, 2]
POISON_KINDS = 5     # below, above, INT32_MIN, INT32_MAX, and a stray whose summed code stays inside the table

NARROW_N = 8193      # all-distinct tuples (code // 64, code % 64, 0, ..) over the codes 0 .. 8192
NARROW_SIDE = 64
NARROW_LOW = 1024


def model(cols, ranges, keys_list, vals):
    """(key columns, count u64, sum i64, min i32, max i32) of the rows for which every range holds."""
    m = wc.mask(cols, ranges)
    return gb.group_by([np.asarray(k, np.int32)[m] for k in keys_list], np.asarray(vals, np.int32)[m])


def matching_bounds(cols, ranges, keys_list):
    """{lo0, hi0, ..} of the key columns over the matching rows; [] without one."""
    m = wc.mask(cols, ranges)
    return gb.bounds_of([np.asarray(k, np.int32)[m] for k in keys_list])


def matrix(case_index: int):
    """The (ncols, nkeys, n, tuple set, value set) combinations one predicate set runs at:
    every ncols with every nkeys; with two key columns at one of 0 / 1025 / 8193 rows, with
    three and four at rotating sizes, so that the 20 sets together meet every size of
    wherecases.SIZES; tuple and value sets rotate along."""
    out = []
    for j, ncols in enumerate(wc.NCOLS):
        for q, nkeys in enumerate(NKEYS):
            n = MANDATORY[j % 3] if q == 0 else wc.SIZES[(5 * case_index + 4 * j + 3 * q + 2) % len(wc.SIZES)]
            out.append((ncols, nkeys, n, TUPLE_SETS[(case_index + 3 * j + q) % len(TUPLE_SETS)],
                        VALUE_SETS[(case_index + j + 2 * q) % len(VALUE_SETS)]))
    return out


def poisoned(name: str, nkeys: int):
    """(cols, ranges, keys_list, vals, bounds): a predicate set whose failing rows all carry, in
    at least one key component, a value outside that column's entry of `bounds`, the exact
    min and max of every key column over the matching rows. The stray components take every
    side: just below, just above, both int32 ends, and (last component one above, the others
    at their lower bounds) a tuple whose summed code still lies inside the table."""
    cols, ranges = wc.case(name, POISON_N, POISON_NCOLS)
    ranges[1] = (100, None)  # nine rows in ten pass the second predicate
    m = wc.mask(cols, ranges)
    rng = np.random.default_rng(77 + nkeys)
    lo = [-5, 100, -1000, 7][:nkeys]
    keys = [rng.integers(0, POISON_RANGES[j], POISON_N) + lo[j] for j in range(nkeys)]
    live = np.flatnonzero(m)
    for j in range(nkeys):  # both ends of every column among the matching rows
        keys[j][live[0]], keys[j][live[-1]] = lo[j], lo[j] + POISON_RANGES[j] - 1
    hi = [lo[j] + POISON_RANGES[j] - 1 for j in range(nkeys)]
    for i, row in enumerate(np.flatnonzero(~m)):
        j, kind = i % nkeys, (i // nkeys) % POISON_KINDS
        if kind == 4:
            for c in range(nkeys - 1):
                keys[c][row] = lo[c]
            keys[nkeys - 1][row] = hi[nkeys - 1] + 1
        else:
            keys[j][row] = [lo[j] - 1, hi[j] + 1, gc.I32_MIN, gc.I32_MAX][kind]
    keys = [np.ascontiguousarray(k, dtype=np.int32) for k in keys]
    bounds = [b for j in range(nkeys) for b in (lo[j], hi[j])]
    return cols, ranges, keys, wc.values_of(POISON_N), bounds


def code_of(keys_list, bounds, rows):
    """The summed tuple code of `rows` under `bounds`, in Python integers (no wrap)."""
    los, his = bounds[::2], bounds[1::2]
    code = np.zeros(len(rows), dtype=object)
    stride = 1
    for j in range(len(keys_list) - 1, -1, -1):
        code = code + (keys_list[j][rows].astype(np.int64).astype(object) - los[j]) * stride
        stride *= his[j] - los[j] + 1
    return code


def narrow(slots: int, extra: int, nkeys: int):
    """(cols, ranges, keys_list, vals): 8193 all-distinct tuples (code // 64, code % 64, 0, ..)
    in shuffled order, whose columns span 129 x 64 tuples; predicate column 0 holds the code
    under [NARROW_LOW, NARROW_LOW + slots + extra): exactly slots + extra tuples match, and
    with extra == 0 their key space is exactly `slots` (a multiple of 64)."""
    assert slots % NARROW_SIDE == 0 and NARROW_LOW % NARROW_SIDE == 0
    code = np.random.default_rng(41).permutation(NARROW_N)
    keys = [code // NARROW_SIDE, code % NARROW_SIDE] + [np.full(NARROW_N, 3 * j) for j in range(2, nkeys)]
    keys = [np.ascontiguousarray(k, dtype=np.int32) for k in keys]
    lead = np.ascontiguousarray(code, dtype=np.int32)
    other = np.ascontiguousarray(np.random.default_rng(5).integers(0, 1000, NARROW_N), dtype=np.int32)
    return [lead, other], [(NARROW_LOW, NARROW_LOW + slots + extra), (None, None)], keys, gc.values_of("uniform", lead)
