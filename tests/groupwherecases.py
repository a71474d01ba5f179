"""group_aggregate_where: the named combinations shared by the host and GPU tests of
group_aggregate_where and of mq_group_where_plan behind it.

The model needs no restatement of its own: it is groupcases.group over the rows that
wherecases.mask keeps.
"""
from __future__ import annotations

import numpy as np

import groupcases as gc
import wherecases as wc

KEY_SETS = ["one_key", "seven_sorted", "seven_shuffled", "uniform_100", "range_S", "int32_ends", "skewed",
            "all_distinct"]
VALUE_SETS = gc.VALUE_SETS
MANDATORY = [0, 1025, 8193]

POISON_SETS = ["islands_first", "islands_last", "islands_alt", "every_257", "tail_only", "ends_only", "clustered_lead"]
POISON_N = 8215      # 256 whole lines and a last line of 23 rows
POISON_NCOLS = 2     # the second predicate kills some survivors of the first: whole dead lines in the island sets too

NARROW_N = 8193      # all_distinct keys -4096 .. 4096, every integer once
NARROW_LOW = -1000

SORT_BIG_N = gc.SORT_N   # 4 195 333 rows, about 60 % of which match
SORT_BIG_RANGE = (0, 600)


def model(cols, ranges, keys, vals):
    """(keys, count u64, sum i64, min i32, max i32) of the rows for which every range holds."""
    m = wc.mask(cols, ranges)
    return gc.group(np.asarray(keys, np.int32)[m], np.asarray(vals, np.int32)[m])


def matrix(case_index: int):
    """The (ncols, n, key set, value set) combinations one predicate set runs at: every ncols
    at one of the sizes 0 / 1025 / 8193 (ncols 8: a rotating one) and at a second, rotating
    size, so that the 20 sets together meet every size with every ncols; key and value sets
    rotate along."""
    out = []
    for j, ncols in enumerate(wc.NCOLS):
        first = MANDATORY[j] if j < 3 else wc.SIZES[(3 * case_index + 1) % len(wc.SIZES)]
        second = wc.SIZES[(5 * case_index + 4 * j + 2) % len(wc.SIZES)]
        for r, n in enumerate((first, second)):
            out.append((ncols, n, KEY_SETS[(case_index + 2 * j + r) % len(KEY_SETS)],
                        VALUE_SETS[(case_index + j + 2 * r) % len(VALUE_SETS)]))
    return out


def poisoned(name: str, slots: int):
    """(cols, ranges, keys, vals, bounds): a predicate set whose failing rows all carry a key
    outside `bounds`, the exact min and max of the matching rows' keys. The failing rows'
    keys take every side: just below, just above and both int32 ends."""
    cols, ranges = wc.case(name, POISON_N, POISON_NCOLS)
    ranges[1] = (100, None)  # nine rows in ten pass the second predicate
    m = wc.mask(cols, ranges)
    keys = gc.keys_of("uniform_100", POISON_N, slots).copy()
    lo, hi = int(keys[m].min()), int(keys[m].max())
    bad = np.array([lo - 1, hi + 1, gc.I32_MIN, gc.I32_MAX, hi + slots, lo - slots], dtype=np.int64)
    dead = np.flatnonzero(~m)
    keys[dead] = bad[dead % len(bad)].astype(np.int32)
    return cols, ranges, keys, wc.values_of(POISON_N), (lo, hi)


def line_census(m: np.ndarray):
    """(lines with a matching and a failing row, lines without a matching row)."""
    n, L = len(m), wc.LINE
    starts = np.arange(0, n, L)
    live = np.add.reduceat(m.astype(np.int64), starts)
    rows = np.diff(np.concatenate([starts, [n]]))
    return int(np.sum((live > 0) & (live < rows))), int(np.sum(live == 0))


def narrow(slots: int, extra: int):
    """(cols, ranges, keys, vals): all_distinct keys that are predicate column 0 too, under
    the range [NARROW_LOW, NARROW_LOW + slots + extra): the matching keys span exactly
    slots + extra values while the column spans 8193."""
    keys = gc.keys_of("all_distinct", NARROW_N, slots)
    other = np.ascontiguousarray(np.random.default_rng(5).integers(0, 1000, NARROW_N), dtype=np.int32)
    cols, ranges = [keys, other], [(NARROW_LOW, NARROW_LOW + slots + extra), (None, None)]
    return cols, ranges, keys, gc.values_of("uniform", keys)


def sort_big_mask():
    """(predicate column, matching mask) of the large sort case."""
    col = np.ascontiguousarray(np.random.default_rng(99).integers(0, 1000, SORT_BIG_N), dtype=np.int32)
    return col, wc.in_range(col, *SORT_BIG_RANGE)


def sort_big(chunk: int):
    """(cols, ranges, keys, vals, runs): the K matching rows carry keys whose sorted sequence
    has the mixed run lengths of groupcases (chunk: mq_group_sort_geometry(K)'s), with values
    planted around the tile edges of that sequence; the other rows carry noise."""
    col, m = sort_big_mask()
    k = int(m.sum())
    runs = gc.runs_of("mixed", k, chunk)
    mk, order = gc.keys_from_runs(runs, seed=k)
    rng = np.random.default_rng(k)
    keys = rng.integers(gc.I32_MIN, gc.I32_MAX, SORT_BIG_N, endpoint=True).astype(np.int32)
    vals = rng.integers(gc.I32_MIN, gc.I32_MAX, SORT_BIG_N, endpoint=True).astype(np.int32)
    keys[m] = mk
    vals[m] = gc.planted_values(runs, order, seed=9)
    return [col], [SORT_BIG_RANGE], keys, vals, runs
