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


# ---------------------------------------------------------------------------
# The sort path past one tile a block. k_group_seg_write walks a chunk in SEG_TILE-row
# tiles and carries the open run from tile to tile; a chunk is longer than one tile only
# past 2 097 152 rows (mq_group_sort_geometry). The cases below are built from the run
# lengths of the SORTED key sequence, so that runs meet tile and chunk edges as named.
# ---------------------------------------------------------------------------
SEG_TILE = 1024              # rows per tile of k_group_seg_write
SORT_N = 4_195_333           # three tiles a block; the last chunk ends in a ragged 5-row tile
SORT_N_TWO_TILES = 2_097_153  # the first size with two tiles a block; the last chunk holds one row
MIXED_RUNS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 3071, 3072, 3073, 7000, 10_000]
RUN_SETS = ["one_key", "all_distinct", "tile_runs", "tile_runs_plus_1", "tile_runs_minus_1", "chunk_runs",
            "chunk_runs_plus_1", "chunk_runs_minus_1", "mixed", "skewed"]


def _fixed_runs(n: int, length: int, first: int) -> np.ndarray:
    """Runs of exactly `length` rows after a first run of `first` rows (0: none); the last
    run takes what is left."""
    full, rest = divmod(n - first, length)
    return np.array([first] * (first > 0) + [length] * full + [rest] * (rest > 0), dtype=np.int64)


def runs_of(name: str, n: int, chunk: int) -> np.ndarray:
    """Run lengths (sum n) of the sorted keys of a named set; chunk = the rows in a block's
    chunk (mq_group_sort_geometry), a multiple of SEG_TILE."""
    rng = np.random.default_rng(29 * n + RUN_SETS.index(name))
    if name == "one_key":  # every chunk after the first has no head
        return np.array([n], dtype=np.int64)
    if name == "all_distinct":  # every tile has SEG_TILE heads
        return np.ones(n, dtype=np.int64)
    if name.startswith("tile_runs"):  # a run starts on, one row after, one row before every tile edge
        return _fixed_runs(n, SEG_TILE, {"tile_runs": 0, "tile_runs_plus_1": 1, "tile_runs_minus_1": SEG_TILE - 1}[name])
    if name.startswith("chunk_runs"):  # the same against chunk edges: the middle tiles have no head
        return _fixed_runs(n, chunk, {"chunk_runs": 0, "chunk_runs_plus_1": 1, "chunk_runs_minus_1": chunk - 1}[name])
    if name == "mixed":
        r = rng.choice(MIXED_RUNS, size=n // min(MIXED_RUNS) // 100 + 16)
        r = r[:np.searchsorted(np.cumsum(r), n) + 1]
        r[-1] -= r.sum() - n
        assert r.sum() == n and r.min() >= 1
        return r.astype(np.int64)
    if name == "skewed":  # one run of about 90 % of the rows between short runs
        short = lambda total: _fixed_runs(total, 3, 0)
        head = n // 20
        big = n * 9 // 10
        return np.concatenate([short(head), [big], short(n - head - big)])
    raise KeyError(name)


def keys_from_runs(runs: np.ndarray, seed: int):
    """(keys, order): a key column whose sorted sequence has these run lengths. The groups
    get ascending keys from I32_MIN to I32_MAX (both present from two groups on), and the
    rows are shuffled by a seeded permutation. order = the stable sort of the keys: row
    order[i] is the i-th of the sorted sequence."""
    g, n = len(runs), int(runs.sum())
    gk = I32_MIN + np.arange(g, dtype=np.int64) * ((2**32 - 1) // max(g - 1, 1))
    gk[-1] = I32_MAX if g > 1 else I32_MIN
    perm = np.random.default_rng(seed).permutation(n)
    keys = np.empty(n, dtype=np.int32)
    keys[perm] = np.repeat(gk, runs).astype(np.int32)
    return keys, np.argsort(keys, kind="stable")


def planted_values(runs: np.ndarray, order: np.ndarray, seed: int) -> np.ndarray:
    """Full-range uniform int32 values by row, with I32_MIN and I32_MAX planted in the sorted
    sequence on both sides of every tile edge (chunk edges are among them) and at the last
    row of up to 4096 runs. The pattern varies with the edge, so that a run rarely holds
    both extremes: a piece that is dropped or counted twice shows in min or max too."""
    n = len(order)
    rng = np.random.default_rng(seed)
    sv = rng.integers(I32_MIN, I32_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
    tails = np.cumsum(runs) - 1
    tails = tails[::max(len(tails) // 4096, 1)]
    sv[tails] = np.where(np.arange(len(tails)) % 2 == 0, I32_MAX, I32_MIN)
    edges = np.arange(SEG_TILE, n, SEG_TILE)
    j = np.arange(len(edges))
    sv[edges - 1] = np.where(j % 2 == 0, I32_MAX, I32_MIN)
    sv[edges] = np.where(j % 4 < 2, I32_MIN, I32_MAX)
    vals = np.empty(n, dtype=np.int32)
    vals[order] = sv
    return vals


def key_range(keys: np.ndarray) -> int:
    """hi - lo + 1 in Python integers (up to 2^32); 0 for no rows."""
    return int(keys.max()) - int(keys.min()) + 1 if len(keys) else 0
