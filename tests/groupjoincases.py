"""group_aggregate_join: the cases and a numpy restatement, shared by the host and GPU tests of
group_aggregate_join and of the device entry points behind it (mq_keymap_build,
mq_keymap_lookup, mq_group_join_plan).

The reference has no such operator, so the model is the definition itself: the dimension's keys
are a primary key (the unique check); fact row i is kept when every range holds for it
(wherecases.mask) and fkey[i] is among the dimension's keys (np.isin); its group key is the
attribute found by searchsorted on the sorted keys; the kept rows then go through groupcases'
grouped model.

A named dimension set is (keys, attributes); a named fact key set is a foreign key column of n
rows for a given dimension. The dimensions are chosen for where a bitmap over [min, max] of
the keys with a rank directory (one entry per 32 keys, a prefix pass in chunks of whole 256-word
steps) can go wrong: both ends of int32, the full span, offsets around a word, a run of keys
across a prefix chunk's edge, one key, no key.
"""
from __future__ import annotations

import numpy as np

import groupcases as gc
import wherecases as wc

I32_MIN, I32_MAX = wc.I32_MIN, wc.I32_MAX
NCOLS = [0, 1, 3, 8]
DIM_SETS = ["dense", "sparse_wide", "single", "negative", "int32_ends", "word_edges", "empty"]
FACT_SETS = ["all_present", "none_present", "half_present", "outside_ends"]
CARDS = [1, 7, 2048]
ATTR_BASE = -3                      # the attributes of a dimension are ATTR_BASE .. ATTR_BASE + card - 1
WORD_EDGES_LO = -1000
WORD_EDGES_SPAN = 2**25 + 77        # 2^20 bitmap words and a few: several blocks, several steps a block
WORD_OFFSETS = [0, 31, 32, 33, 63, 64]


def is_primary_key(dim_keys) -> bool:
    k = np.asarray(dim_keys, dtype=np.int32)
    return len(np.unique(k)) == len(k)


def repeated(dim_keys) -> int:
    """The keys that repeat an earlier one: n1 - COUNT(DISTINCT)."""
    k = np.asarray(dim_keys, dtype=np.int32)
    return len(k) - len(np.unique(k))


def lookup(fkey, dim_keys, dim_attrs, missing=0):
    """(attributes int32, hits uint8) of the N:1 join: the attribute of every fact key, or
    `missing` where the dimension has no such key."""
    fkey = np.asarray(fkey, dtype=np.int32)
    dk, da = np.asarray(dim_keys, dtype=np.int32), np.asarray(dim_attrs, dtype=np.int32)
    assert is_primary_key(dk) and len(dk) == len(da)
    if len(dk) == 0:
        return np.full(len(fkey), missing, dtype=np.int32), np.zeros(len(fkey), dtype=np.uint8)
    order = np.argsort(dk, kind="stable")
    sk, sa = dk[order], da[order]
    idx = np.minimum(np.searchsorted(sk, fkey), len(sk) - 1)
    hit = sk[idx] == fkey
    assert np.array_equal(hit, np.isin(fkey, dk))
    return np.where(hit, sa[idx], np.int32(missing)).astype(np.int32), hit.astype(np.uint8)


def mask(cols, ranges, fkey, dim_keys) -> np.ndarray:
    m = wc.mask(cols, ranges) if len(cols) else np.ones(len(fkey), dtype=bool)
    return m & np.isin(np.asarray(fkey, dtype=np.int32), np.asarray(dim_keys, dtype=np.int32))


def model(cols, ranges, fkey, dim_keys, dim_attrs, vals):
    """(attributes, count u64, sum i64, min i32, max i32), one entry per attribute with a joined
    row, ascending."""
    m = mask(cols, ranges, fkey, dim_keys)
    attr, hit = lookup(fkey, dim_keys, dim_attrs)
    assert np.all(hit[m] == 1)
    return gc.group(attr[m], np.asarray(vals, dtype=np.int32)[m])


def map_bytes(span: int, n1: int) -> int:
    """Bitmap (one bit a key of the span, rounded up to 16 bytes), directory (8 bytes per 32-bit
    bitmap word) and attributes."""
    words = (span + 127) // 128 * 4
    return words * 4 + words * 8 + 4 * n1


def info(dim_keys, dim_attrs):
    """(lo, hi, attr_lo, attr_hi, entries, bytes) as mq_keymap_info holds them."""
    dk, da = np.asarray(dim_keys, dtype=np.int64), np.asarray(dim_attrs, dtype=np.int64)
    if len(dk) == 0:
        return 0, -1, I32_MAX, I32_MIN, 0, 0
    lo, hi = int(dk.min()), int(dk.max())
    return lo, hi, int(da.min()), int(da.max()), len(dk), map_bytes(hi - lo + 1, len(dk))


def attributes(keys: np.ndarray, card: int, seed: int) -> np.ndarray:
    """One attribute per key out of `card` values from ATTR_BASE up; both ends present when there
    are keys enough; no function of the key's order."""
    n1 = len(keys)
    a = np.random.default_rng(seed).integers(0, card, n1) + ATTR_BASE
    if n1 >= 2 and card >= 2:
        a[n1 // 3], a[(2 * n1) // 3] = ATTR_BASE, ATTR_BASE + card - 1
    return np.ascontiguousarray(a, dtype=np.int32)


def word_edges_keys(chunk_words: int) -> np.ndarray:
    """Keys at offsets 0, 31, 32, 33, 63, 64 of the span, a run of 81 keys across the edge of
    the prefix pass's first chunk (chunk_words bitmap words of 32 keys: mq_keymap_geometry of
    WORD_EDGES_SPAN), single keys on both sides of the second chunk's edge, and the span's
    last key."""
    edge = chunk_words * 32
    assert 200 < edge and 2 * edge + 64 < WORD_EDGES_SPAN
    offs = np.concatenate([WORD_OFFSETS, np.arange(edge - 40, edge + 41), [2 * edge - 1, 2 * edge], [WORD_EDGES_SPAN - 1]])
    return (np.unique(offs) + WORD_EDGES_LO).astype(np.int64)


def dimension(name: str, card: int = 7, n1: int = 3000, chunk_words: int | None = None):
    """(keys, attributes) of a named dimension set, both int32; the keys are distinct and in no
    order."""
    rng = np.random.default_rng(9000 * DIM_SETS.index(name) + n1 + card)
    if name == "dense":  # every value of the span is a key
        k = np.arange(n1, dtype=np.int64) - 1000
    elif name == "sparse_wide":  # a span over 2^31: offsets that do not fit a signed int
        k = np.unique(np.concatenate((rng.integers(-2**30, 2**30 + 2**29, n1), [-2**30 - 5, 2**30 + 2**29])))
    elif name == "single":
        k = np.array([7], dtype=np.int64)
    elif name == "negative":
        k = rng.choice(np.arange(-5000, -4000), 300, replace=False)
    elif name == "int32_ends":  # the full span: offset 0 and offset 2^32 - 1
        k = np.unique(np.concatenate((rng.integers(I32_MIN, I32_MAX, 500), [I32_MIN, I32_MAX, I32_MIN + 31, I32_MAX - 32, -1, 0])))
    elif name == "word_edges":
        assert chunk_words, "word_edges needs mq_keymap_geometry(WORD_EDGES_SPAN)'s chunk"
        k = word_edges_keys(chunk_words)
    elif name == "empty":
        k = np.empty(0, dtype=np.int64)
    else:
        raise KeyError(name)
    k = rng.permutation(k)
    return np.ascontiguousarray(k, dtype=np.int32), attributes(k, card, seed=len(k) + card)


def absent_keys(dim_keys) -> np.ndarray:
    """int32 values that are no key of the dimension: the neighbours of every key and the values
    just outside both ends of the span, where int32 has them."""
    dk = np.asarray(dim_keys, dtype=np.int64)
    lo, hi = int(dk.min()), int(dk.max())
    cand = np.unique(np.concatenate((dk - 1, dk + 1, [lo - 2, lo - 1, hi + 1, hi + 2])))
    cand = cand[(cand >= I32_MIN) & (cand <= I32_MAX)]
    return cand[~np.isin(cand, dk)]


def fact_keys(name: str, n: int, dim_keys) -> np.ndarray:
    """The foreign key column of n rows of a named fact key set, for a dimension's keys."""
    rng = np.random.default_rng(400 * FACT_SETS.index(name) + n + len(dim_keys))
    dk = np.asarray(dim_keys, dtype=np.int64)
    if len(dk) == 0:  # no key is present whatever the name says
        return np.ascontiguousarray(rng.integers(0, 10, n), dtype=np.int32)
    absent = absent_keys(dk)
    assert len(absent), "the dimension leaves no int32 out"
    lo, hi = int(dk.min()), int(dk.max())
    if name == "all_present":
        f = rng.choice(dk, n)
    elif name == "none_present":
        f = rng.choice(absent, n)
    elif name == "half_present":
        f = np.where(rng.integers(0, 2, n) == 0, rng.choice(dk, n), rng.choice(absent, n))
    elif name == "outside_ends":  # both ends of the span and what lies just outside them
        pool = np.array([lo - 2, lo - 1, lo, hi, hi + 1, hi + 2, I32_MIN, I32_MAX], dtype=np.int64)
        pool = pool[(pool >= I32_MIN) & (pool <= I32_MAX)]
        f = pool[np.arange(n) % len(pool)] if n else pool[:0]
        f = rng.permutation(f)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(f, dtype=np.int32)


def promises(fact_name: str, dim_name: str):
    """(a joined row is promised, a dropped row is promised) for n >= 16 rows and no range."""
    if dim_name == "empty":
        return False, True
    return {"all_present": (True, False), "none_present": (False, True), "half_present": (True, True),
            "outside_ends": (True, dim_name != "int32_ends")}[fact_name]


def case(name: str, n: int, ncols: int):
    """wherecases.case with ncols == 0 allowed: no column, no range."""
    return wc.case(name, n, ncols) if ncols else ([], [])
