"""group_aggregate_measures: the cases and a numpy restatement, shared by the host and GPU tests
of group_aggregate_measures and of mq_group_measures_plan / _write behind it.

The reference has no such operator, so the model is the definition itself on top of parts the
suite already pins: the joined rows are starcases.joined's, the tuples and their order are
starcases.model's (groupbycases.group_by over starcases.components). A measure is a Measure: an
op ("col", "add", "sub", "mul") and one or two int32 columns; its value for a row is computed in
int64 from the widened operands, which is exact for all four ops. Per group: the shared count, and
per measure the sum modulo 2^64 (added up through a uint64 view, so the wrap is explicit), the
int64 min and the int64 max.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import groupbycases as gb
import starcases as sc

I32_MIN, I32_MAX = sc.I32_MIN, sc.I32_MAX
I64_MIN = -(1 << 63)
MAX_MEASURES = 4
OPS = {"col": 0, "add": 1, "sub": 2, "mul": 3}  # MQ_MEAS_COL, _ADD, _SUB, _MUL
SLOTS = {1: 1024, 2: 512, 3: 512, 4: 256}       # mq_group_measures_dense_slots(nmeas)
LDS_BYTES = 40 * 1024                            # the table of every dense grouping kernel


def slot_bytes(nmeas: int) -> int:
    return 4 + 24 * nmeas


@dataclass
class Measure:
    op: str
    a: np.ndarray
    b: np.ndarray | None = None


def value(m: Measure) -> np.ndarray:
    a = np.asarray(m.a, dtype=np.int32).astype(np.int64)
    if m.op == "col":
        assert m.b is None
        return a
    b = np.asarray(m.b, dtype=np.int32).astype(np.int64)
    return a + b if m.op == "add" else a - b if m.op == "sub" else a * b


def fold(keys_list, values):
    """(list of key columns, count u64, [(sum i64, min i64, max i64) per int64 column of
    `values`]), one entry per distinct tuple, ascending lexicographically."""
    keys_list = [np.asarray(k, dtype=np.int32) for k in keys_list]
    n = len(keys_list[0])
    if n == 0:
        e = np.empty(0, np.int64)
        return [np.empty(0, np.int32) for _ in keys_list], np.empty(0, np.uint64), [(e, e, e) for _ in values]
    order = np.lexsort(keys_list[::-1])
    ks = [k[order] for k in keys_list]
    differs = np.zeros(n - 1, dtype=bool)
    for k in ks:
        differs |= k[1:] != k[:-1]
    heads = np.flatnonzero(np.concatenate([[True], differs]))
    count = np.diff(np.concatenate([heads, [n]])).astype(np.uint64)
    aggs = []
    for v in values:
        v = np.ascontiguousarray(np.asarray(v, dtype=np.int64)[order])
        aggs.append((np.add.reduceat(v.view(np.uint64), heads).view(np.int64),  # modulo 2^64
                     np.minimum.reduceat(v, heads), np.maximum.reduceat(v, heads)))
    return [k[heads] for k in ks], count, aggs


def model(cols, ranges, terms, measures):
    m = sc.joined(cols, ranges, terms)
    comps = [c[m] for c in sc.components(terms)]
    keys, count, aggs = fold(comps, [value(q)[m] for q in measures])
    ref = gb.group_by(comps, np.zeros(int(m.sum()), np.int32))  # starcases.model's tuples and order
    assert all(np.array_equal(a, b) for a, b in zip(keys, ref[0])) and np.array_equal(count, ref[1])
    return keys, count, aggs


def brute(cols, ranges, terms, measures):
    """The same from Python integers and a dictionary."""
    m = sc.joined(cols, ranges, terms)
    comps = sc.components(terms)
    groups = {}
    for i in np.flatnonzero(m):
        tup = tuple(int(c[i]) for c in comps)
        vs = []
        for q in measures:
            a, b = int(q.a[i]), int(q.b[i]) if q.b is not None else 0
            vs.append(a if q.op == "col" else a + b if q.op == "add" else a - b if q.op == "sub" else a * b)
        c, acc = groups.get(tup, (0, [(0, v, v) for v in vs]))
        groups[tup] = (c + 1, [(s + v, min(mn, v), max(mx, v)) for (s, mn, mx), v in zip(acc, vs)])
    order = sorted(groups)
    wrap = lambda s: ((s + (1 << 63)) % (1 << 64)) - (1 << 63)  # noqa: E731
    keys = [np.array([g[j] for g in order], dtype=np.int32) for j in range(len(comps))]
    count = np.array([groups[g][0] for g in order], dtype=np.uint64)
    aggs = [(np.array([wrap(groups[g][1][q][0]) for g in order], dtype=np.int64),
             np.array([groups[g][1][q][1] for g in order], dtype=np.int64),
             np.array([groups[g][1][q][2] for g in order], dtype=np.int64)) for q in range(len(measures))]
    return keys, count, aggs


def columns(n: int, seed: int = 0, big: bool = False):
    """Four int32 operand columns (price, qty, disc, tax in spirit): `big` draws over the whole of
    int32, both ends among the rows; otherwise values small enough that no sum of n terms wraps."""
    rng = np.random.default_rng(9000 + 17 * seed + n)
    if big:
        cols = [rng.integers(I32_MIN, I32_MAX + 1, n) for _ in range(4)]
        for j, c in enumerate(cols):
            if n >= 2:
                c[[(j + 1) * n // 7, (j + 2) * n // 7]] = I32_MIN, I32_MAX
    else:
        cols = [rng.integers(-50_000, 100_000, n), rng.integers(1, 51, n), rng.integers(0, 11, n), rng.integers(-8, 9, n)]
    return [np.ascontiguousarray(c, dtype=np.int32) for c in cols]


def q1_measures(cols, nmeas: int):
    """TPC-H Q1's shape over (price, qty, disc, tax): price * disc, qty, price - tax and
    price + qty: every op once, seven operands that are four distinct columns; fewer measures
    take a prefix."""
    price, qty, disc, tax = cols
    every = [Measure("mul", price, disc), Measure("col", qty), Measure("sub", price, tax), Measure("add", price, qty)]
    return every[:nmeas]
