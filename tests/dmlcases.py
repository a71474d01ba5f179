"""Row deletes and updates: the cases and a numpy restatement, shared by the host and
GPU tests of relational_delete / relational_update and of the device entry points
behind them (mq_delete_plan / _columns / _index, mq_update_rows).

The reference has no such operator (parse.c:876-960 lacks both commands), so the model
is the workload generator's own pandas statements (milestone5.py:127-142, 186-202):
a delete is np.delete per column plus a stable filter and renumbering of an index, an
update is plain assignment.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from refapi import mq

TILE = 4096  # rows per compaction block (csrc/mq_dml.hip kDelTile)

SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 17, 2**20 + 5]
NCOLS = [1, 4, 7]
ORDERS = ["ascending", "reversed", "shuffled"]


def delete_sets(n: int) -> dict:
    """name -> sorted distinct row ids to delete from a table of n rows."""
    rng = np.random.default_rng(1000 + n)
    ar = np.arange(n, dtype=np.int64)
    out = {"none": ar[:0], "all": ar, "first": ar[:1], "last": ar[n - 1:] if n else ar[:0], "every_second": ar[::2]}
    # one whole tile (the second where there is one), and a run across a tile boundary
    t0 = TILE if n >= 2 * TILE else 0
    out["whole_tile"] = ar[t0:t0 + TILE]
    b = TILE if n > TILE else n // 2
    out["run_across_boundary"] = ar[max(b - 37, 0):min(b + 91, n)]
    out["random_1pct"] = np.flatnonzero(rng.random(n) < 0.01)
    out["random_50pct"] = np.flatnonzero(rng.random(n) < 0.5)
    return out


# ---------------------------------------------------------------------------
# Past one step a block. The word prefix (k_dml_word_sums / _prefix) walks a chunk of bitmap
# words in PREFIX_STEP-word steps, the index pass (k_dml_index_count / _write) a chunk of
# entries in INDEX_STEP-entry steps; both carry a running base from step to step. The
# chunks come from mq_dml_geometry: one step long up to 16 773 120 rows (prefix) and
# 2 097 152 rows (index).
# ---------------------------------------------------------------------------
PREFIX_STEP = 256          # bitmap words per step of k_dml_word_prefix
INDEX_STEP = 1024          # index entries per step of k_dml_index_write
BIG_N = 2**24 + 5          # two prefix steps and nine index steps a block
INDEX_N = [2_097_153, 4_195_333]  # the first sizes with 2 and 3 index steps a block
BIG_SETS = ["random_50pct", "random_1pct", "first_steps", "second_steps"]
INDEX_MULT = 1_000_003     # positions (i * INDEX_MULT) mod n: a permutation where gcd = 1


def big_delete_set(name: str, n: int, chunk_words: int) -> np.ndarray:
    """Sorted distinct row ids (int64) of a named delete set for the many-step sizes.
    first_steps: in six prefix chunks every row of the first PREFIX_STEP words and none of
    the second PREFIX_STEP words (one step's total full, the next zero), elsewhere a random
    30 %; second_steps is its complement."""
    rng = np.random.default_rng(3000 + n + BIG_SETS.index(name))
    if name == "random_50pct":
        return np.flatnonzero(rng.random(n) < 0.5)
    if name == "random_1pct":
        return np.flatnonzero(rng.random(n) < 0.01)
    gone = np.random.default_rng(3000 + n).random(n) < 0.3
    nchunks = n // (64 * chunk_words)  # whole chunks of rows
    assert nchunks >= 6 and chunk_words >= 2 * PREFIX_STEP
    for c in (0, 1, 7, nchunks // 2, nchunks - 2, nchunks - 1):
        r0 = c * chunk_words * 64
        gone[r0:r0 + PREFIX_STEP * 64] = True
        gone[r0 + PREFIX_STEP * 64:r0 + 2 * PREFIX_STEP * 64] = False
    if name == "first_steps":
        return np.flatnonzero(gone)
    if name == "second_steps":
        return np.flatnonzero(~gone)
    raise KeyError(name)


def big_index(n: int, clustered: bool):
    """A sorted index over n rows without an n-row argsort: values ascending with ties (a
    thousand distinct), positions the permutation (i * INDEX_MULT) mod n, or the identity
    for the clustered form."""
    assert np.gcd(INDEX_MULT, n) == 1
    v = np.sort(np.random.default_rng(n).integers(0, 1000, n).astype(np.int32))
    i = np.arange(n, dtype=np.uint64)
    return v, i if clustered else (i * np.uint64(INDEX_MULT)) % np.uint64(n)


def position_list(ids: np.ndarray, order: str, seed: int = 0) -> np.ndarray:
    """The ids as a position list: every id twice, in the given order."""
    p = np.repeat(ids, 2)
    if order == "reversed":
        p = p[::-1]
    elif order == "shuffled":
        p = np.random.default_rng(seed).permutation(p)
    return np.ascontiguousarray(p, dtype=np.int32)


def table(n: int, ncols: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed * 7919 + n * 31 + ncols)
    return rng.integers(-2**31, 2**31 - 1, (ncols, n), dtype=np.int64).astype(np.int32)


def delete_rows(cols: np.ndarray, ids: np.ndarray) -> np.ndarray:
    return np.stack([np.delete(c, np.unique(ids)) for c in cols]) if len(cols) else cols


def delete_index(values: np.ndarray, positions: np.ndarray, ids: np.ndarray, n: int):
    """The entries whose row survives, in their order; p -> p - (deleted rows before p)."""
    gone = np.zeros(n, dtype=bool)
    gone[np.unique(ids).astype(np.int64)] = True
    before = np.concatenate([[0], np.cumsum(gone)])[:n]  # deleted rows before each row
    p = positions.astype(np.int64)
    keep = ~gone[p]
    return values[keep], (p[keep] - before[p[keep]]).astype(np.uint64)


def update_rows(col: np.ndarray, ids: np.ndarray, value: int) -> np.ndarray:
    out = col.copy()
    ids = np.asarray(ids, dtype=np.int64)
    out[ids[(ids >= 0) & (ids < len(col))]] = value
    return out


def index_of(col: np.ndarray, clustered: bool = False):
    """A sorted index over col: values ascending, positions a (stable) permutation;
    the clustered form has the identity for positions."""
    p = np.argsort(col, kind="stable")
    return col[p], (np.arange(len(col)) if clustered else p).astype(np.uint64)


class Histogram(C.Structure):  # cs165_api.h:71-75
    _fields_ = [("bin_size", C.c_int), ("values", C.c_int * 100), ("counts", C.c_size_t * 100)]


def make_db(bufs, index_col=None, clustered=False):
    """A one-table Db over the int32 arrays in bufs (kept alive by the caller), as the
    server holds it after load_db, with create(idx, ...) applied to index_col."""
    ncols, n = len(bufs), len(bufs[0])
    cs = (mq.Column * ncols)()
    for j in range(ncols):
        c = cs[j]
        c.name = f"col{j + 1}".encode()
        c.data = bufs[j].ctypes.data_as(C.POINTER(C.c_int))
        c.fd = -1
        c.row_count = n
        c.max, c.min = (int(bufs[j].max()), int(bufs[j].min())) if n else (0, 0)
    if index_col is not None:
        cs[index_col].has_index, cs[index_col].clustered, cs[index_col].sorted = True, clustered, True
    t = mq.Table()
    t.name = b"tbl5"
    t.columns = cs
    t.col_count, t.row_count, t.table_length = ncols, n, n
    db = mq.Db()
    db.name = b"db1"
    db.tables = C.pointer(t)
    db.tables_size = db.tables_capacity = 1
    return db, t, cs


def tbl5(n: int = 10_000, seed: int = 5) -> np.ndarray:
    """Four columns of the reference suite's tbl5 size: col1 distinct (99 bins fill
    exactly: max - min = n - 1), the others with repeats."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n), rng.integers(0, 1000, n), rng.integers(-500, 500, n),
                     rng.integers(0, 2**30, n)]).astype(np.int32)
