"""select_where: the cases and a numpy restatement, shared by the host and GPU tests of
select_where / aggregate_where and of the device entry points behind them
(mq_where_positions, mq_where_agg).

The reference has no such operator (its DSL spells a conjunction as the chain select ->
fetch -> select_result -> ...), so the model is the definition itself: row i matches when
low_c <= col_c[i] < high_c holds for every predicate c, either bound optional.

A case is (columns, ranges): `ncols` int32 arrays of n rows (the same array object twice
means the same column twice) and `ncols` (low, high) pairs, None for a missing bound. The
sets are chosen for where a kernel that skips dead 128-byte lines (32 rows) of the later
columns, and reads ragged ends row by row, can go wrong.
"""
from __future__ import annotations

import numpy as np

I32_MIN, I32_MAX = -2**31, 2**31 - 1
MAX_COLS = 8
LINE = 32  # rows of one 128-byte line

# empty; one row; a line +- 1; two lines +- 1; a wave tile +- 1; a block tile +- 1; one
# expand block + 1; one full iteration of 8 tiles + 1
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8193]
BIG = 300_001  # under a CU limit of 1 or 2: many iterations a block, chunk edges inside lines
NCOLS = [1, 2, 3, 8]
CASES = ["uniform_0p1", "uniform_1", "uniform_10", "uniform_50", "sorted_lead", "clustered_lead",
         "islands_first", "islands_last", "islands_alt", "every_257", "tail_only", "ends_only",
         "first_all", "first_none", "last_kills", "unbounded_middle", "empty_range", "empty_high_min",
         "extreme_bounds", "same_twice"]


def in_range(v: np.ndarray, low, high) -> np.ndarray:
    v = np.asarray(v, dtype=np.int32).astype(np.int64)
    m = np.ones(len(v), dtype=bool)
    if low is not None:
        m &= v >= int(low)
    if high is not None:
        m &= v < int(high)
    return m


def mask(cols, ranges) -> np.ndarray:
    assert len(cols) == len(ranges) and 1 <= len(cols) <= MAX_COLS
    m = np.ones(len(cols[0]), dtype=bool)
    for v, (low, high) in zip(cols, ranges):
        m &= in_range(v, low, high)
    return m


def positions(cols, ranges, payload=None) -> np.ndarray:
    idx = np.flatnonzero(mask(cols, ranges))
    return idx.astype(np.int32) if payload is None else np.asarray(payload, dtype=np.int32)[idx]


def aggregate(cols, ranges, val):
    """(count, sum, min, max) of val over the matching rows, as mq_agg holds them."""
    v = np.asarray(val, dtype=np.int32)[mask(cols, ranges)].astype(np.int64)
    if len(v) == 0:
        return 0, 0, I32_MAX, I32_MIN
    return len(v), int(v.sum()), int(v.min()), int(v.max())


def _uniform(rng, n):
    return rng.integers(0, 1000, n)


def _lead_marks(n, rows):
    """A leading column that is 1 at `rows` and 0 elsewhere, with the range [1, 2)."""
    v = np.zeros(n, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    v[rows[(rows >= 0) & (rows < n)]] = 1
    return v


def case(name: str, n: int, ncols: int):
    """(columns, ranges) of a named set: n rows, ncols predicates."""
    assert 1 <= ncols <= MAX_COLS
    rng = np.random.default_rng(1000 * CASES.index(name) + 17 * n + ncols)
    # the later columns: uniform in [0, 1000), half of the rows pass each
    cols = [_uniform(rng, n) for _ in range(ncols)]
    ranges = [(250 + c, 750 + c) for c in range(ncols)]
    if name.startswith("uniform_"):
        width = {"0p1": 1, "1": 10, "10": 100, "50": 500}[name[len("uniform_"):]]
        ranges = [(37 * c, 37 * c + width) for c in range(ncols)]
    elif name == "sorted_lead":  # one long live stretch
        cols[0] = np.sort(rng.integers(-5000, 5000, n))
        ranges[0] = (-1234, 2345)
    elif name == "clustered_lead":  # live and dead stretches of 1..4097 rows at odd offsets
        v, i, live = np.empty(n, dtype=np.int64), 0, False
        lengths = [1, 3, 31, 33, 257, 4097, 7, 63, 65, 1025, 129, 2, 511]
        j = 0
        while i < n:
            run = lengths[j % len(lengths)]
            v[i:i + run] = 5 if live else -5
            i, j, live = i + run, j + 1, not live
        cols[0], ranges[0] = v, (0, 10)
    elif name == "islands_first":  # one survivor of predicate 0 per line, at its row 0
        cols[0], ranges[0] = _lead_marks(n, np.arange(0, n, LINE)), (1, 2)
    elif name == "islands_last":  # ... at its row 31
        cols[0], ranges[0] = _lead_marks(n, np.arange(LINE - 1, n, LINE)), (1, 2)
    elif name == "islands_alt":  # ... alternating between row 0 and row 31
        first = np.arange(0, n, LINE)
        cols[0], ranges[0] = _lead_marks(n, first + (LINE - 1) * ((first // LINE) & 1)), (1, 2)
    elif name == "every_257":
        cols[0], ranges[0] = _lead_marks(n, np.arange(0, n, 257)), (1, 2)
    elif name == "tail_only":  # survivors only in the last n % 32 rows
        cols[0], ranges[0] = _lead_marks(n, np.arange(n - n % LINE, n)), (1, 2)
    elif name == "ends_only":  # rows 0 and n - 1
        cols[0], ranges[0] = _lead_marks(n, [0, n - 1]), (1, 2)
    elif name == "first_all":  # a bounded range that every row of its column satisfies
        ranges[0] = (0, 1000)
    elif name == "first_none":  # a satisfiable range that no row of its column is in
        ranges[0] = (1000, 2000)
    elif name == "last_kills":
        ranges = [(0, 1000)] * (ncols - 1) + [(100, 200)]
    elif name == "unbounded_middle":  # ncols == 1: the only range is unbounded
        ranges[min(1, ncols - 1)] = (None, None)
    elif name == "empty_range":  # low >= high
        ranges[ncols - 1] = (500, 500) if n & 1 else (501, 500)
    elif name == "empty_high_min":  # nothing is below INT32_MIN
        ranges[ncols // 2] = (None, I32_MIN)
    elif name == "extreme_bounds":
        for c in range(ncols):
            v = rng.integers(I32_MIN, I32_MAX, n, endpoint=True)
            v[rng.integers(0, 8, n) == 0] = I32_MIN
            v[rng.integers(0, 8, n) == 0] = I32_MAX
            cols[c] = v
        pool = [(I32_MIN, None), (None, I32_MAX), (I32_MIN + 1, None), (I32_MIN, I32_MAX), (None, I32_MAX),
                (I32_MIN + 1, I32_MAX), (I32_MIN, None), (None, I32_MAX)]
        ranges = pool[:ncols]
    elif name == "same_twice":  # one column under two ranges (ncols == 1: one of them)
        ranges[0] = (100, None)
        if ncols > 1:
            cols[1], ranges[1] = cols[0], (None, 600)
    else:
        raise KeyError(name)
    out, seen = [], {}
    for v in cols:  # one int32 array per distinct column, identity kept
        if id(v) not in seen:
            seen[id(v)] = np.ascontiguousarray(v, dtype=np.int32)
        out.append(seen[id(v)])
    return out, list(ranges)


def values_of(n: int) -> np.ndarray:
    """A value column for the aggregate: the whole int32 range, both ends present."""
    v = np.random.default_rng(n + 11).integers(I32_MIN, I32_MAX, n, endpoint=True)
    if n >= 2:
        v[n // 2], v[n // 3] = I32_MIN, I32_MAX
    return np.ascontiguousarray(v, dtype=np.int32)


def payload_of(n: int) -> np.ndarray:
    """A positions vector that is no function of the row's index."""
    return np.ascontiguousarray(np.random.default_rng(n + 3).permutation(n)[::-1] * 3 - n, dtype=np.int32)
