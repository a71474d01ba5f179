"""group_aggregate_star: the cases and a numpy restatement, shared by the host and GPU tests of
group_aggregate_star and of the device entry points behind it (mq_star_positions,
mq_group_star_plan).

The reference has no such operator, so the model is the definition itself, put together from
parts the suite already pins: a fact row is joined when every range holds for it
(wherecases.mask) and every mapped or filtering term finds its key (groupjoincases.mask); the
component of a mapped term is groupjoincases.lookup's attribute, of a plain term the value
itself; the joined rows' tuples then go through groupbycases.group_by.

A term is a Term: its kind ("km": a dimension whose attribute is a group key, "ks": a dimension
joined only as a filter, "plain": a fact column that is a group key), its fact column and, for a
dimension, the dimension's keys (and attributes). A term layout names the kinds in order; an
attribute-space layout gives every component its number of values, so that their product P lies
on a chosen side of the dense path's 2048 slots.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import groupbycases as gb
import groupjoincases as gj
import wherecases as wc

I32_MIN, I32_MAX = wc.I32_MIN, wc.I32_MAX
MAX_TERMS = 4
SLOTS = 2048  # mq_group_dense_slots(), asserted by the host test through mq_group_by_auto_path

LAYOUTS = {
    "km": ["km"],
    "km_km": ["km", "km"],
    "ks_km": ["ks", "km"],
    "km_ks": ["km", "ks"],
    "plain_km": ["plain", "km"],
    "km_plain_km": ["km", "plain", "km"],
    "ks_km_plain_km": ["ks", "km", "plain", "km"],
    "km_km_km_km": ["km", "km", "km", "km"],
}
# attribute spaces by number of components: (cardinalities, the path AUTO must take)
SPACES = {
    1: [((2048,), "dense"), ((2049,), "sort")],
    2: [((32, 64), "dense"), ((7, 293), "sort")],
    3: [((8, 16, 16), "dense")],
    4: [((2, 4, 16, 16), "dense")],
}
COMP_BASE = [-3, 100, -1000, 7]  # component j takes the values COMP_BASE[j] .. COMP_BASE[j] + card - 1
DIM_KEYS = 3000                  # keys of a generated dimension, out of a span of 2 * DIM_KEYS values


@dataclass
class Term:
    kind: str
    col: np.ndarray
    dim_keys: np.ndarray | None = None
    dim_attrs: np.ndarray | None = None
    extra: dict = field(default_factory=dict)


def nkeys_of(kinds) -> int:
    return sum(k != "ks" for k in kinds)


def term_mask(t: Term) -> np.ndarray:
    if t.kind == "plain":
        return np.ones(len(t.col), dtype=bool)
    return gj.mask([], [], t.col, t.dim_keys)


def joined(cols, ranges, terms) -> np.ndarray:
    n = len(terms[0].col)
    m = wc.mask(cols, ranges) if len(cols) else np.ones(n, dtype=bool)
    for t in terms:
        m = m & term_mask(t)
    return m


def components(terms):
    """One int32 column per non-ks term: the attribute found for the row's key (0 where there is
    none: such a row is not joined) or the plain column itself."""
    out = []
    for t in terms:
        if t.kind == "km":
            out.append(gj.lookup(t.col, t.dim_keys, t.dim_attrs)[0])
        elif t.kind == "plain":
            out.append(np.asarray(t.col, dtype=np.int32))
    return out


def model(cols, ranges, terms, vals):
    """(list of nkeys key columns, count u64, sum i64, min i32, max i32), one entry per distinct
    tuple with a joined row, ascending lexicographically."""
    m = joined(cols, ranges, terms)
    return gb.group_by([c[m] for c in components(terms)], np.asarray(vals, dtype=np.int32)[m])


def positions(cols, ranges, terms, payload=None) -> np.ndarray:
    p = np.flatnonzero(joined(cols, ranges, terms)).astype(np.int32)
    return p if payload is None else np.asarray(payload, dtype=np.int32)[p]


def brute(cols, ranges, terms, vals):
    """The same result from a plain Python loop over the rows and dictionaries."""
    groups = {}
    maps = [dict(zip(map(int, t.dim_keys), map(int, t.dim_attrs))) if t.kind == "km" else
            set(map(int, t.dim_keys)) if t.kind == "ks" else None for t in terms]
    for i in range(len(vals)):
        if not all(wc.in_range(np.array([c[i]], dtype=np.int32), lo, hi)[0] for c, (lo, hi) in zip(cols, ranges)):
            continue
        tup, ok = [], True
        for t, mp in zip(terms, maps):
            k = int(t.col[i])
            if t.kind == "plain":
                tup.append(k)
            elif k not in mp:
                ok = False
                break
            elif t.kind == "km":
                tup.append(mp[k])
        if not ok:
            continue
        v = int(vals[i])
        c, s, mn, mx = groups.get(tuple(tup), (0, 0, v, v))
        groups[tuple(tup)] = (c + 1, s + v, min(mn, v), max(mx, v))
    order = sorted(groups)
    nk = nkeys_of([t.kind for t in terms])
    return ([np.array([g[j] for g in order], dtype=np.int32) for j in range(nk)],
            np.array([groups[g][0] for g in order], dtype=np.uint64), np.array([groups[g][1] for g in order], dtype=np.int64),
            np.array([groups[g][2] for g in order], dtype=np.int32), np.array([groups[g][3] for g in order], dtype=np.int32))


def bounds_of(cards):
    """{lo_0, hi_0, ..}: the exact bounds of components drawn by `make`."""
    out = []
    for j, c in enumerate(cards):
        out += [COMP_BASE[j], COMP_BASE[j] + c - 1]
    return out


def dimension(seed: int, card: int, base: int, n1: int = DIM_KEYS):
    """(keys, attributes): n1 distinct keys in no order out of a span twice as wide that starts
    at -n1 - 100 * seed; the attributes take every value of base .. base + card - 1 when
    there are keys enough."""
    rng = np.random.default_rng(7000 + seed)
    lo = -n1 - 100 * seed
    k = rng.permutation(lo + rng.choice(2 * n1, n1, replace=False))
    a = rng.integers(0, card, n1) + base
    if n1 >= card:
        a[rng.choice(n1, card, replace=False)] = base + np.arange(card)
    return np.ascontiguousarray(k, dtype=np.int32), np.ascontiguousarray(a, dtype=np.int32)


def make(layout: str, cards, n: int, seed: int = 0, miss: float = 0.15):
    """The terms of a named layout over n fact rows: every dimension is its own (seeded by its
    place), a share `miss` of every foreign key column has no partner (its neighbours in the
    span, both ends of int32 and values just outside the span among them), a filtering
    dimension passes about half of the rows, and component j has cards[j] values."""
    kinds = LAYOUTS[layout]
    assert len(cards) == nkeys_of(kinds)
    rng = np.random.default_rng(100 * seed + n + len(kinds))
    terms, c = [], 0
    for j, kind in enumerate(kinds):
        if kind == "plain":
            col = rng.integers(0, cards[c], n) + COMP_BASE[c]
            if n >= 2:
                col[[n // 5, (4 * n) // 5]] = COMP_BASE[c], COMP_BASE[c] + cards[c] - 1
            terms.append(Term(kind, np.ascontiguousarray(col, dtype=np.int32)))
            c += 1
            continue
        dk, da = dimension(10 * seed + j, cards[c] if kind == "km" else 1, COMP_BASE[c] if kind == "km" else 0)
        absent = gj.absent_keys(dk)
        absent = np.concatenate((absent, [I32_MIN, I32_MAX]))
        share = 0.5 if kind == "ks" else miss
        col = np.where(rng.random(n) < share, rng.choice(absent, n), rng.choice(dk.astype(np.int64), n))
        terms.append(Term(kind, np.ascontiguousarray(col, dtype=np.int32), dk, da if kind == "km" else None))
        c += kind == "km"
    return terms


def promises(cols, ranges, terms):
    """(some row is joined, some row is dropped)"""
    m = joined(cols, ranges, terms)
    return bool(m.any()), bool((~m).any())


def case(name: str, n: int, ncols: int):
    return gj.case(name, n, ncols)
