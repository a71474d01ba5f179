"""Batched row inserts: the cases and a numpy restatement, shared by the host and GPU
tests of relational_insert and of the device entry points behind it (mq_insert_points /
_plan / _columns / _index / _slots / _positions).

The model is the reference's insert_row (db_manager.c:164-199) issued once per row, plus
what the workload generator expects of it (milestone5.py:40-78: the clustered order and
the secondary index "should be maintained when we insert new data"): an append is a
concatenation, a sorted insert is the stable sort by key of the old rows followed by
the new ones, an index merge is the stable merge with the old entries first among equals.
"""
from __future__ import annotations

import numpy as np

import dmlcases as dc

TILE = 4096  # output slots per expansion block (csrc/mq_dml.hip kDelTile)

SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 3 * 8192 + 17, 2**20 + 5]
NCOLS = [1, 4, 7]


def insertion_points(n: int) -> dict:
    """name -> ascending insertion points (uint32, each in [0, n]) into a table of n old
    rows: the j-th new row goes in front of old row points[j]. Patterns that need old rows
    are left out where there are none."""
    rng = np.random.default_rng(2000 + n)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    out = {"none": u32([]), "front": u32(np.zeros(101)), "append": u32(np.full(101, n)),
           "more_new_than_old": u32(np.sort(rng.integers(0, n + 1, 3 * n + 5)))}
    if n >= 2:  # a run of new slots that spans whole tiles, at one interior point
        out["one_point"] = u32(np.full(2 * TILE + 37, n // 2))
    if n >= 1:
        out["every_row"] = u32(np.arange(n))
        out["random_1pct"] = u32(np.sort(rng.integers(0, n + 1, max(n // 100, 3))))  # repeated points
        out["random_50pct"] = u32(np.sort(rng.integers(0, n + 1, max(n // 2, 2))))
    return out


BIG_HALF_K = dc.BIG_N // 3  # k = n / 2 new rows where n + k = dmlcases.BIG_N


def big_points(name: str, n: int, k: int) -> np.ndarray:
    """k ascending insertion points into n old rows for the sizes past one prefix step: all
    at the front, all appended, or sorted random points (repeats among them)."""
    if name == "front":
        p = np.zeros(k)
    elif name == "append":
        p = np.full(k, n)
    else:
        p = np.sort(np.random.default_rng(2000 + n + k).integers(0, n + 1, k))
    return np.ascontiguousarray(p, dtype=np.uint32)


def expand(old: np.ndarray, points: np.ndarray, new: np.ndarray) -> np.ndarray:
    """One column: new[j] in front of old[points[j]], equal points in their order."""
    return np.insert(old, points.astype(np.int64), new)


def insert_rows(cols: np.ndarray, v_old, new: np.ndarray, key_col: int = 0) -> np.ndarray:
    """The table's columns (ncols, n) after the batch `new` (ncols, k, batch order).
    v_old None: append. Else v_old[r] is old row r's key (ascending: the clustered index's
    values), a new row's key is its value for key_col, and every column is reordered by
    the stable sort of (old keys, then new keys)."""
    both = np.concatenate([cols, new], axis=1)
    if v_old is None:
        return both
    order = np.argsort(np.concatenate([v_old, new[key_col]]), kind="stable")
    return both[:, order]


def new_slots(v_old: np.ndarray, new_keys: np.ndarray):
    """(ascending insertion points of the key-sorted batch, the slot of every new row by
    batch index) of a sorted insert."""
    order = np.argsort(new_keys, kind="stable")
    points = np.searchsorted(v_old, new_keys[order], side="right")
    slots = np.empty(len(new_keys), dtype=np.uint64)
    slots[order] = points + np.arange(len(new_keys))
    return points.astype(np.uint32), slots


def insert_index(values, positions, new_values, new_positions, renumber=None):
    """Stable merge of the new (value, row) entries (batch order) into a sorted index, old
    entries first among equals. renumber: the table's ascending insertion points; every
    old position p moves to p + #{j : renumber[j] <= p}."""
    p = positions.astype(np.uint64)
    if renumber is not None:
        p = p + np.searchsorted(renumber, p, side="right").astype(np.uint64)
    o = np.argsort(new_values, kind="stable")
    v = np.concatenate([values, new_values[o]])
    p = np.concatenate([p, np.asarray(new_positions, dtype=np.uint64)[o]])
    order = np.argsort(v, kind="stable")
    return v[order].astype(np.int32), p[order]


def make_db(bufs, n: int, index_col=None, clustered=False):
    """dmlcases.make_db over buffers with spare capacity: the first n rows of each are the
    table, table_length is the buffers' length."""
    db, t, cs = dc.make_db(bufs, index_col, clustered)
    for j, b in enumerate(bufs):
        cs[j].row_count = n
        cs[j].max, cs[j].min = (int(b[:n].max()), int(b[:n].min())) if n else (0, 0)
    t.row_count, t.table_length = n, len(bufs[0])
    return db, t, cs


MILESTONE5_ROWS = np.array([[-1, -11, -111, -1111], [-2, -22, -222, -2222], [-3, -33, -333, -2222],
                            [-4, -44, -444, -2222], [-5, -55, -555, -2222]], dtype=np.int32)  # milestone5.py:67-71


def random_batch(k: int, seed: int = 9) -> np.ndarray:
    """k rows (k, 4) for dmlcases.tbl5 with repeated keys in every column, some beyond the
    old min / max."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-50, 10_050, k) // 7 * 7, rng.integers(-20, 1020, k) // 5 * 5,
                     rng.integers(-600, 600, k), rng.integers(0, 2**30, k)], axis=1).astype(np.int32)
