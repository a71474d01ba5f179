"""Operator chains on live results and rewritten columns: a host-only model of a server
session, the hazards a caller can put between two operator calls, and a generator of
random programs. No GPU and no libmq here.

A Session holds a table of int32 columns and named handles (the INT / LONG arrays the
operators return, and the DOUBLE of average). Every drop-in operator has one model, and the
models are the ones the suite already pins: refcpu (select, fetch, add, sub, shared_select,
the joins, index_select), wherecases, semicases, groupcases, groupbycases, groupwherecases,
groupbywherecases, topkcases, dmlcases and insertcases. Where libmq documents a deviation
from the reference the model follows libmq and cites the comment.

A step is a tuple (kind, ins, params):
  an operator   (op, refs of its inputs, parameters); its outputs are named "t<idx>" or
                "t<idx>_<i>" after the step's index in the program;
  a hazard      (hazard, refs of its targets, parameters): a host-side action between two
                operator calls (HAZARDS);
  ("drop", names, None): the caller frees these handles (bookkeeping, neither of the above).
A ref is ("c", j) for table column j or ("h", name) for a handle. A range is ("pm", a, b):
permille of the table's first row count (column 0 holds values in [0, rows)), or ("abs", lo,
hi); None is a missing bound. So a program does not depend on the table's size: the host
tests replay it on a small table, a device replay takes the full one (ROWS).
"""
from __future__ import annotations

import numpy as np

import dmlcases as dc
import groupbycases as gb
import groupbywherecases as gbw
import groupcases as gc
import groupwherecases as gw
import insertcases as ic
import semicases as sc
import topkcases as tk
import wherecases as wc

I32_MIN, I32_MAX = -2**31, 2**31 - 1

ROWS = 600_000        # a near-full select gives a 2.4 MB payload: mmapped, guarded, shadowed
NCOLS = 4
INDEX_COL = 1         # the column that carries the unclustered index in the random programs
INSERT_ROWS = 100
HASHSET_SIZE = 16411  # prime, above twice the widest few-keys domain
SEEDS = list(range(20))
STEPS = 40

OPS = ["select_scan", "select_index", "select_result", "fetch_column", "sum_column", "sum_result", "average", "min",
       "max", "add", "sub", "shared_select", "hash_join", "nested_loop_join", "group_aggregate",
       "group_aggregate_where", "group_aggregate_by", "group_aggregate_by_where", "top_k", "select_where",
       "aggregate_where", "select_where_in", "aggregate_where_in", "hashset_insert", "print"]
REFERENCE_OPS = ["select_scan", "select_result", "fetch_column", "sum_column", "sum_result", "average", "min", "max",
                 "add", "sub", "shared_select", "hash_join", "nested_loop_join"]
HAZARDS = ["rewrite_all", "edit_one", "free_and_reuse", "shrink_budget", "update", "delete", "insert", "invalidate"]
DML = ["update", "delete", "insert"]
CLASSES = ["rewrite_all", "edit_one", "free_and_reuse", "dml"]  # what every operator must directly follow
EDIT_SPOTS = ["first", "head", "mid", "tail", "last"]
PAIRS = [(c, op) for op in OPS for c in CLASSES]
PAIRS_PER_PROGRAM = 8

# column j's value domain (make_table) and the ranges predicates on it draw from
COL_RANGES = [
    [("pm", 100, 105), ("pm", 102, 107), ("pm", 0, 500), ("pm", 250, None), ("pm", None, 900), ("pm", 400, 400)],
    [("abs", 1000, 4000), ("abs", 0, 2500), ("abs", 4990, None), ("abs", 17, 18)],
    [("abs", -25, 25), ("abs", None, 0), ("abs", -50, 50), ("abs", 49, None)],
    [("abs", None, 0), ("abs", -2**30, 2**30), ("abs", 0, None), ("abs", I32_MIN, I32_MAX)],
]
UPDATE_VALUES = [None, 4321, 7, -10]  # in-domain values per column (column 0 is never updated: the join key)


def make_table(rows: int = ROWS, seed: int = 0) -> np.ndarray:
    """(NCOLS, rows): column 0 uniform in [0, rows) (select and join key, a key span past the
    semi join's LDS bitmap at full size), column 1 in [0, 5000) (indexed; group keys past the
    dense table's slots), column 2 in [-50, 50) (dense group keys), column 3 the whole int32
    range (values)."""
    rng = np.random.default_rng(9000 + seed)
    return np.stack([rng.integers(0, rows, rows), rng.integers(0, 5000, rows), rng.integers(-50, 50, rows),
                     rng.integers(I32_MIN, I32_MAX, rows, endpoint=True)]).astype(np.int32)


def insert_batch(seed: int, k: int, rows0: int) -> np.ndarray:
    """(k, NCOLS) new rows inside the columns' domains."""
    rng = np.random.default_rng(31_000 + seed)
    return np.stack([rng.integers(0, rows0, k), rng.integers(0, 5000, k), rng.integers(-50, 50, k),
                     rng.integers(I32_MIN, I32_MAX, k, endpoint=True)], axis=1).astype(np.int32)


def spot_index(spot, n: int) -> int:
    """The element an edit_one touches: a name of EDIT_SPOTS or an index. "head" and "tail"
    lie inside the first and the last partial page of a payload that starts 16 bytes into a
    page (an mmapped malloc chunk): the bytes a guard copies aside instead of protecting."""
    i = {"first": 0, "head": 5, "mid": n // 2, "tail": n - 3, "last": n - 1}.get(spot, spot)
    return int(min(max(int(i), 0), n - 1))


def edited(old: int) -> int:
    """What edit_one stores: another value that is still a valid row id and key."""
    return 0 if int(old) != 0 else 1


def reused(old: np.ndarray) -> np.ndarray:
    """The content that takes a freed payload's place: same length and kind, other bytes."""
    new = old[::-1].copy()
    if len(new) and np.array_equal(new, old):
        new[0] = edited(new[0])
    return new


def fmt(arrays) -> str:
    """print (query.c:245-304) of INT / LONG results: "%d" per tuple, newline between tuples,
    "," between results."""
    return ",".join("\n".join("%d" % v for v in a.tolist()) for a in arrays)


def hashset_slots(keys: np.ndarray, size: int) -> np.ndarray:
    """refcpu.hashset_table of the keys in order. Inserting a key a second time changes
    nothing (hashset.c:25-32), so only first occurrences are replayed."""
    import refcpu
    keys = np.asarray(keys, dtype=np.int32)
    _, first = np.unique(keys, return_index=True)
    return refcpu.hashset_table(keys[np.sort(first)].tolist(), size)


class Session:
    """The model: table columns (live rows only), one optional sorted index, handles."""

    def __init__(self, cols, index_col=None, clustered=False):
        self.cols = [np.array(c, dtype=np.int32) for c in cols]
        self.rows0 = len(self.cols[0])
        self.h = {}
        self.index_col, self.clustered = index_col, clustered
        self.index = None
        if index_col is not None:
            self.build_index()

    def build_index(self):
        """build_index (index.c:152-178) on index_col; the clustered form reorders every
        other column by the sort and leaves the column's own rows as loaded."""
        j = self.index_col
        v, p = self.sorted_index(self.cols[j])
        if self.clustered:
            self.cols = [c if i == j else c[p.astype(np.int64)] for i, c in enumerate(self.cols)]
            p = np.arange(len(v), dtype=np.uint64)
        self.index = (v, p)

    @staticmethod
    def sorted_index(col):
        """What libmq's index_one builds: dmlcases.index_of's sorted values, with equal values
        in the reference quicksort's own order (mq_index_build_ref is exact up to
        MQ_INDEX_EXACT_MAX rows), which refcpu.index_build_lomuto restates."""
        import refcpu
        v, p = refcpu.index_build_lomuto(col)
        assert np.array_equal(v, dc.index_of(col)[0])
        return v, p

    # ---- references ----
    @property
    def rows(self) -> int:
        return len(self.cols[0])

    def val(self, ref) -> np.ndarray:
        """The bytes behind a ref; ("ix", 0 | 1) is the index's values / positions array (a
        hazard may edit it as it edits a column)."""
        if ref[0] == "ix":
            return self.index[ref[1]]
        return self.cols[ref[1]] if ref[0] == "c" else self.h[ref[1]]

    def bounds(self, spec):
        kind, lo, hi = spec
        if kind == "pm":
            return (None if lo is None else self.rows0 * lo // 1000, None if hi is None else self.rows0 * hi // 1000)
        return lo, hi

    def topk_k(self, tag, n: int) -> int:
        """k of 1, 100, or n / 4 + 1 (past n / MQ_TOPK_SORT_DIV: the sort path)."""
        return {"one": 1, "hundred": 100, "quarter": n // 4 + 1}[tag]

    # ---- operators ----
    def op(self, step, idx: int) -> dict:
        """Run an operator step; returns {output name: expected array} (for hashset_insert
        and print, {"value": ...}) and registers the array outputs as handles."""
        import refcpu
        kind, ins, p = step
        v = [self.val(r) for r in ins]
        R = lambda key="range": self.bounds(p[key])  # noqa: E731
        one = lambda x, dt: [np.array([x], dtype=dt)]  # noqa: E731
        value = None
        if kind == "select_scan":
            out = [refcpu.select_scan(v[0], *R())]
        elif kind == "select_index":
            assert ins[0] == ("c", self.index_col)
            out = [refcpu.index_select(self.index[0], self.index[1], *R())]
        elif kind == "select_result":
            out = [refcpu.select_result(v[0], v[1], *R())]
        elif kind == "fetch_column":
            out = [refcpu.fetch(v[0], v[1])]
        elif kind in ("sum_column", "sum_result"):
            out = one(v[0].astype(np.int64).sum(), np.int64)
        elif kind == "average":  # query.c:306-323: (double)int64 sum / (double)n, NaN for n == 0
            n = len(v[0])
            out = one(np.float64(v[0].astype(np.int64).sum()) / np.float64(n) if n else np.nan, np.float64)
        elif kind == "min":  # mq_query.c min(): INT_MAX for an empty input (the reference reads garbage)
            out = one(v[0].min() if len(v[0]) else I32_MAX, np.int32)
        elif kind == "max":  # mq_query.c max(): INT_MIN for an empty input
            out = one(v[0].max() if len(v[0]) else I32_MIN, np.int32)
        elif kind == "add":
            out = [refcpu.add(v[0], v[1])]
        elif kind == "sub":
            out = [refcpu.sub(v[0], v[1])]
        elif kind == "shared_select":
            bs = [self.bounds(s) for s in p["ranges"]]
            out = refcpu.shared_select(v[0], [b[0] for b in bs], [b[1] for b in bs])
        elif kind in ("hash_join", "nested_loop_join"):
            out = list(refcpu.hash_join(v[0], v[1], v[2], v[3], nested=kind == "nested_loop_join"))
        elif kind == "group_aggregate":
            out = self._group(gc.group(v[0], v[1]))
        elif kind == "group_aggregate_where":
            nc = p["ncols"]
            out = self._group(gw.model(v[:nc], self._ranges(p), v[nc], v[nc + 1]))
        elif kind == "group_aggregate_by":
            out = self._group(gb.group_by(v[:-1], v[-1]))
        elif kind == "group_aggregate_by_where":
            nc = p["ncols"]
            out = self._group(gbw.model(v[:nc], self._ranges(p), v[nc:-1], v[-1]))
        elif kind == "top_k":
            pay = v[1] if len(v) > 1 else None
            out = list(tk.topk(v[0], pay, self.topk_k(p["k"], len(v[0])), p["desc"]))
        elif kind == "select_where":
            nc = p["ncols"]
            out = [wc.positions(v[:nc], self._ranges(p), v[nc] if len(v) > nc else None)]
        elif kind == "aggregate_where":
            nc = p["ncols"]
            out = self._agg(wc.aggregate(v[:nc], self._ranges(p), v[nc]))
        elif kind == "select_where_in":
            nc = p["ncols"]
            out = [sc.positions(v[:nc], self._ranges(p), v[nc], v[nc + 1], p["anti"], v[nc + 2] if len(v) > nc + 2 else None)]
        elif kind == "aggregate_where_in":
            nc = p["ncols"]
            out = self._agg(sc.aggregate(v[:nc], self._ranges(p), v[nc], v[nc + 1], v[nc + 2], p["anti"]))
        elif kind == "hashset_insert":
            out, value = [], hashset_slots(v[0], p["size"])
        elif kind == "print":
            out, value = [], fmt(v)
        else:
            raise KeyError(kind)
        if value is not None:
            return {"value": value}
        names = out_names(idx, len(out))
        got = {}
        for nm, a in zip(names, out):
            got[nm] = self.h[nm] = np.ascontiguousarray(a)
        return got

    def _ranges(self, p):
        return [self.bounds(s) for s in p["ranges"]]

    @staticmethod
    def _group(g):
        """group_aggregate's Results: the key columns (INT), counts and sums (LONG), min, max (INT)."""
        keys, count, sm, mn, mx = g
        keys = keys if isinstance(keys, list) else [keys]
        return [k.astype(np.int32) for k in keys] + [count.astype(np.int64), sm.astype(np.int64), mn.astype(np.int32),
                                                      mx.astype(np.int32)]

    @staticmethod
    def _agg(a):
        """aggregate_where's Results: count, sum (LONG), min, max (INT; INT32_MAX / INT32_MIN
        without a match, include/mq_query.h)."""
        return [np.array([a[0]], np.int64), np.array([a[1]], np.int64), np.array([a[2]], np.int32),
                np.array([a[3]], np.int32)]

    # ---- hazards ----
    def hazard(self, step) -> None:
        kind, ins, p = step
        if kind == "rewrite_all":  # an in-place reorder of the rows, same pointer and length
            a = self.val(ins[0])
            a[:] = a[np.random.default_rng(p["seed"]).permutation(len(a))]
        elif kind == "edit_one":
            a = self.val(ins[0])
            if len(a):
                i = spot_index(p["spot"], len(a))
                a[i] = edited(a[i])
        elif kind == "free_and_reuse":
            self.h[ins[0][1]] = reused(self.h[ins[0][1]])
        elif kind == "update":
            self.update(ins[0][1], self.val(ins[1]), p["value"])
        elif kind == "delete":
            self.delete(self.val(ins[0]))
        elif kind == "insert":
            self.insert(insert_batch(p["seed"], p["k"], self.rows0))
        elif kind in ("shrink_budget", "invalidate"):
            pass  # no effect on what any operator returns
        else:
            raise KeyError(kind)

    def update(self, j: int, ids, value: int) -> None:
        assert not (self.clustered and j == self.index_col), "relational_update answers ERROR on a clustered column"
        self.cols[j] = dc.update_rows(self.cols[j], ids, value)
        if j == self.index_col:  # the unclustered index is built again (include/mq_query.h)
            self.index = self.sorted_index(self.cols[j])

    def delete(self, ids) -> None:
        n = self.rows
        if self.index is not None:
            self.index = dc.delete_index(self.index[0], self.index[1], np.asarray(ids), n)
        self.cols = list(dc.delete_rows(np.stack(self.cols), np.asarray(ids)))

    def insert(self, batch: np.ndarray) -> None:
        """batch: (k, ncols) in batch order."""
        n, k, new = self.rows, len(batch), np.ascontiguousarray(batch.T)
        if self.clustered:
            v_old, j = self.index[0], self.index_col
            self.cols = list(ic.insert_rows(np.stack(self.cols), v_old, new, j))
            v = np.sort(np.concatenate([v_old, new[j]]), kind="stable").astype(np.int32)
            self.index = (v, np.arange(n + k, dtype=np.uint64))
            return
        if self.index is not None:
            self.index = ic.insert_index(self.index[0], self.index[1], new[self.index_col], n + np.arange(k))
        self.cols = list(ic.insert_rows(np.stack(self.cols), None, new))

    def drop(self, names) -> None:
        for nm in names:
            del self.h[nm]

    def apply(self, step, idx: int):
        """Any step; an operator's expected outputs, else None."""
        if step[0] in OPS:
            return self.op(step, idx)
        if step[0] == "drop":
            return self.drop(step[1])
        return self.hazard(step)


def out_names(idx: int, count: int):
    return [f"t{idx}"] if count == 1 else [f"t{idx}_{i}" for i in range(count)]


OUT_COUNT = {"shared_select": None, "hash_join": 2, "nested_loop_join": 2, "group_aggregate": 5, "group_aggregate_where": 5,
             "group_aggregate_by": None, "group_aggregate_by_where": None, "top_k": 2, "aggregate_where": 4,
             "aggregate_where_in": 4, "hashset_insert": 0, "print": 0}


def out_count(step) -> int:
    kind, ins, p = step
    if kind == "shared_select":
        return len(p["ranges"])
    if kind in ("group_aggregate_by", "group_aggregate_by_where"):
        return p["nkeys"] + 4
    return OUT_COUNT.get(kind, 1)


# ---------------------------------------------------------------------------
# the program generator
# ---------------------------------------------------------------------------
class _Gen:
    """Symbolic state of a program under construction: which handles exist, how long each is
    (a length class: equal classes are equally long), and which hold valid row ids. It never
    looks at a value, so the same program is legal on a table of any size."""

    LIFE = 5  # operator steps an output stays alive

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(77_000 + seed)
        self.seed = seed
        self.steps = []
        self.tags = {}       # handle -> dict(cls, pos, epoch, like)
        self.roles = {}
        self.temps = []      # (names) per operator step, oldest first
        self.ver = 0         # table length version: bumps on insert and delete
        self.epoch = 0       # bumps on delete: row ids from before may lie outside the table
        self.drawn = self.replaced = self.updates = 0
        self.ncls = 0

    # ---- bookkeeping ----
    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def newcls(self):
        self.ncls += 1
        return ("r", self.ncls)

    def tcls(self):
        return ("T", self.ver)

    def emit_op(self, step, outs, keep_as=None):
        idx = len(self.steps)
        self.steps.append(step)
        names = out_names(idx, len(outs))
        for nm, t in zip(names, outs):
            self.tags[nm] = t
        if keep_as:
            self.roles[keep_as] = names[0]
        elif names:
            self.temps.append(names)
        if len(self.temps) > self.LIFE:
            gone = self.temps.pop(0)
            for nm in gone:
                del self.tags[nm]
            self.steps.append(("drop", tuple(gone), None))
        return names

    def tag(self, cls, pos=False, like=None, dtype="int", join=False, few=False):
        return dict(cls=cls, pos=pos, epoch=self.epoch, like=like, dtype=dtype, join=join, few=few)

    def ints(self, **want):
        """Live INT handles whose tags match; role handles and temps alike."""
        out = []
        for nm, t in self.tags.items():
            if t["dtype"] != "int":
                continue
            if want.get("pos") and not (t["pos"] and t["epoch"] == self.epoch):
                continue
            if "cls" in want and t["cls"] != want["cls"]:
                continue
            if want.get("join") and not t["join"]:
                continue
            if want.get("few") and not t["few"]:
                continue
            out.append(nm)
        return out

    def prefer_temp(self, names):
        """Half of the time one of the newest outputs: the previous operator's result, in place."""
        fresh = [n for n in names if n not in self.roles.values()]
        return self.pick(fresh) if fresh and self.rng.random() < 0.5 else self.pick(names)

    def href(self, name):
        return ("h", name)

    def role(self, r):
        return self.roles[r]

    # ---- table-long inputs ----
    def table_side(self):
        """"cols": the table's columns; "res": the table-long Results of the prologue (which
        stay equally long among themselves when the table grows or shrinks)."""
        return "cols" if self.rng.random() < 0.6 else "res"

    def tl(self, side, like):
        """A table-long input that looks like column `like`, and the column whose ranges fit it."""
        if side == "cols":
            return ("c", like), like
        name = {0: "P_all", 1: "K_all", 2: "K_all", 3: "V_all"}[like]
        return self.href(self.role(name)), {0: 0, 1: 2, 2: 2, 3: 3}[like]

    def preds(self, side, lo=1, hi=3):
        n = int(self.rng.integers(lo, hi + 1))
        cols, ranges = [], []
        for like in self.rng.permutation(4)[:n]:
            ref, dom = self.tl(side, int(like))
            cols.append(ref)
            ranges.append(self.pick(COL_RANGES[dom]))
        return cols, ranges

    def tl_pos(self, side):
        """A positions Result as long as the chosen side, or None."""
        if self.rng.random() < 0.5:
            return None
        if side == "res":
            return self.href(self.role("P_all"))
        return self.href(self.role("P_all")) if self.ver == 0 else None

    # ---- one operator step ----
    def build(self, op):
        """(step, output tags) of operator `op` on inputs that exist and are legal now, or None."""
        g, P, T = self, self.pick, self.tag
        if op == "select_scan":
            j = P([0, 2, 3])
            return (op, (("c", j),), {"range": P(COL_RANGES[j])}), [T(g.newcls(), pos=True)]
        if op == "select_index":
            r = P([s for s in COL_RANGES[INDEX_COL] if None not in s])
            return (op, (("c", INDEX_COL),), {"range": r}), [T(g.newcls(), pos=True)]
        if op == "select_result":
            pairs = [(a, b) for a in g.ints() for b in g.ints(cls=g.tags[a]["cls"]) if a != b]
            if not pairs:
                return None
            a, b = P(pairs)
            like = g.tags[a]["like"]
            r = P(COL_RANGES[like]) if like is not None else ("abs", None, 0)
            tb = g.tags[b]
            return (op, (g.href(a), g.href(b)), {"range": r}), [T(g.newcls(), pos=tb["pos"] and tb["epoch"] == g.epoch,
                                                                   like=tb["like"])]
        if op == "fetch_column":
            pos = g.ints(pos=True)
            if not pos:
                return None
            b, j = g.prefer_temp(pos), P([0, 1, 2, 3])
            narrow = g.tags[b].get("narrow", False)
            t = T(g.tags[b]["cls"], like=j, join=j == 0 and narrow, few=j in (1, 2) or (j == 0 and narrow))
            return (op, (("c", j), g.href(b)), {}), [t]
        if op == "sum_column":
            return (op, (("c", P([0, 1, 2, 3])),), {}), [T(g.newcls(), dtype="long")]
        if op in ("sum_result", "average", "min", "max"):
            a = g.prefer_temp(g.ints())
            dt = {"sum_result": "long", "average": "double"}.get(op, "int")
            return (op, (g.href(a),), {}), [T(g.newcls(), dtype=dt)]
        if op in ("add", "sub"):
            pairs = [(a, b) for a in g.ints() for b in g.ints(cls=g.tags[a]["cls"]) if a != b]
            if not pairs:
                return None
            a, b = P(pairs)
            return (op, (g.href(a), g.href(b)), {}), [T(g.tags[a]["cls"])]
        if op == "shared_select":
            j, q = P([0, 1, 2, 3]), P([2, 16])
            lo, hi = (0, 1000) if j == 0 else (I32_MIN, I32_MAX)  # shared_select reads both bounds of every query
            rs = [COL_RANGES[j][i % len(COL_RANGES[j])] for i in range(q)]
            rs = [(s[0], lo if s[1] is None else s[1], hi if s[2] is None else s[2]) for s in rs]
            return (op, (("c", j),), {"ranges": tuple(rs)}), [T(g.newcls(), pos=True) for _ in range(q)]
        if op in ("hash_join", "nested_loop_join"):
            a = (g.role("V_n1"), g.role("P_n1"))
            b = (g.role("V_n2"), g.role("P_n2"))
            if g.rng.random() < 0.5:
                a, b = b, a
            c = g.newcls()
            ok = lambda n: g.tags[n]["pos"] and g.tags[n]["epoch"] == g.epoch  # noqa: E731
            return (op, tuple(g.href(x) for x in a + b), {}), [T(c, pos=ok(a[1])), T(c, pos=ok(b[1]))]
        if op in ("group_aggregate", "group_aggregate_where", "group_aggregate_by", "group_aggregate_by_where"):
            side = g.table_side()
            where, by = op.endswith("where"), "_by" in op
            cols, ranges = g.preds(side, 1, 2) if where else ([], [])
            keys = [g.tl(side, k)[0] for k in ([2, 1] if by else [P([1, 2])])]
            vals = g.tl(side, 3)[0]
            c = g.newcls()
            p = {"ncols": len(cols), "ranges": tuple(ranges), "nkeys": len(keys)}
            outs = [T(c, few=True) for _ in keys] + [T(c, dtype="long"), T(c, dtype="long"), T(c), T(c)]
            return (op, tuple(cols) + tuple(keys) + (vals,), p), outs
        if op == "top_k":
            side = g.table_side()
            vals = g.tl(side, P([0, 3]))[0]
            pos = g.tl_pos(side)
            ins = (vals,) if pos is None else (vals, pos)
            c = g.newcls()
            posok = pos is None and side == "cols" or (pos is not None and g.tags[pos[1]]["pos"] and
                                                       g.tags[pos[1]]["epoch"] == g.epoch)
            return (op, ins, {"k": P(["one", "hundred", "quarter"]), "desc": bool(g.rng.integers(0, 2))}), \
                [T(c), T(c, pos=bool(posok))]
        if op in ("select_where", "aggregate_where", "select_where_in", "aggregate_where_in"):
            side = g.table_side()
            semi, agg = op.endswith("_in"), op.startswith("aggregate")
            cols, ranges = g.preds(side, 0 if semi else 1, 3)
            ins, p = list(cols), {"ncols": len(cols), "ranges": tuple(ranges)}
            if semi:
                wide = g.rng.random() < 0.5  # the set's key span picks the LDS or the global bitmap
                ins.append(g.tl(side, 0 if wide else 1)[0])
                few = g.ints(few=True)
                ins.append(("c", 0) if wide else (g.href(g.prefer_temp(few)) if few and g.rng.random() < 0.7 else ("c", 1)))
                p["anti"] = bool(g.rng.integers(0, 2))
            if agg:
                ins.append(g.tl(side, 3)[0])
                c = g.newcls()
                return (op, tuple(ins), p), [T(c, dtype="long"), T(c, dtype="long"), T(c), T(c)]
            pos = g.tl_pos(side)
            if pos is not None:
                ins.append(pos)
            posok = pos is None and side == "cols" or (pos is not None and g.tags[pos[1]]["pos"] and
                                                       g.tags[pos[1]]["epoch"] == g.epoch)
            return (op, tuple(ins), p), [T(g.newcls(), pos=bool(posok))]
        if op == "hashset_insert":
            few = g.ints(few=True)
            if not few:
                return None
            return (op, (g.href(g.prefer_temp(few)),), {"size": HASHSET_SIZE}), []
        if op == "print":
            sets = [("P_n1",), ("V_n1", "P_n2"), ("K_all",)]
            return (op, tuple(g.href(g.role(r)) for r in P(sets)), {}), []
        raise KeyError(op)

    def op_step(self, op=None, keep_as=None, forced=None):
        """Emit one operator step: `forced`, or `op`, or a random legal one. A draw whose inputs
        do not exist is replaced by the next legal operator and counted."""
        self.drawn += 1
        if forced is not None:
            return self.emit_op(forced[0], forced[1], keep_as)
        order = [op] if op else []
        order += [OPS[i] for i in self.rng.permutation(len(OPS))]
        for n, o in enumerate(order):
            built = self.build(o)
            if built is not None:
                self.replaced += n > 0
                return self.emit_op(built[0], built[1], keep_as)
        raise AssertionError("no legal operator")

    # ---- hazards ----
    def hazard(self, cls, targets=(), bumped=False):
        """Emit a hazard of class `cls` (a name of HAZARDS) against one of `targets` (the refs
        the next operator reads) where the hazard can take one. bumped: the caller has counted
        an insert's new table length already."""
        g, P = self, self.pick
        self.drawn += 1
        hs = [r for r in targets if r[0] == "h"]
        cs = [r for r in targets if r[0] == "c"]
        if cls in ("rewrite_all", "edit_one"):
            t = P(list(targets)) if targets else P([("c", P([0, 1, 2, 3])), g.href(P(g.ints()))])
            p = {"seed": int(g.rng.integers(1, 1 << 30))} if cls == "rewrite_all" else {"spot": P(EDIT_SPOTS)}
            step = (cls, (t,), p)
        elif cls == "free_and_reuse":
            step = (cls, (P(hs) if hs else g.href(P(g.ints())),), {})
        elif cls == "update":
            pos = g.role("P_n1")
            ok = [r[1] for r in cs if r[1] != 0]
            if not (g.tags[pos]["pos"] and g.tags[pos]["epoch"] == g.epoch):
                return self.hazard("insert", targets)
            j = P(ok) if ok else P([1, 2, 3])
            g.updates += 1  # a value of its own each time: a repeated update still changes rows
            step = (cls, (("c", j), g.href(pos)), {"value": UPDATE_VALUES[j] + g.updates})
        elif cls == "insert":
            step = (cls, (), {"seed": int(g.rng.integers(1, 1 << 30)), "k": INSERT_ROWS})
            g.ver += not bumped
        elif cls == "delete":
            pos = [n for n in g.ints(pos=True) if g.tags[n].get("narrow")]
            if not pos:
                return self.hazard("insert", targets)
            step = (cls, (g.href(P(pos)),), {})
            g.ver += 1
            g.epoch += 1
        elif cls == "shrink_budget":
            step = (cls, (), {"steps": int(g.rng.integers(2, 5))})
        elif cls == "invalidate":
            step = (cls, (P(cs) if cs else ("c", P([0, 1, 2, 3])),), {})
        else:
            raise KeyError(cls)
        self.steps.append(step)
        return step

    # ---- the program ----
    def prologue(self):
        """The handles every operator can draw on: all row ids and two table-long fetches (2.4 MB
        payloads at full size), and two narrow, overlapping selects on the join key with their
        fetched keys (small payloads; the joins' operands)."""
        def sel(role, spec, narrow):
            t = self.tag(self.newcls(), pos=True, like=0)
            t["narrow"] = narrow
            return self.op_step(forced=(("select_scan", (("c", 0),), {"range": spec}), [t]), keep_as=role)

        def fet(role, j, pos_role, **kw):
            pn = self.role(pos_role)
            t = self.tag(self.tags[pn]["cls"], like=j, **kw)
            return self.op_step(forced=(("fetch_column", (("c", j), self.href(pn)), {}), [t]), keep_as=role)

        sel("P_all", ("pm", None, None), False)
        fet("V_all", 3, "P_all")
        fet("K_all", 2, "P_all", few=True)
        sel("P_n1", ("pm", 100, 105), True)
        fet("V_n1", 0, "P_n1", join=True, few=True)
        sel("P_n2", ("pm", 102, 107), True)
        fet("V_n2", 0, "P_n2", join=True, few=True)

    def run(self, steps: int):
        self.prologue()
        pairs = [PAIRS[(self.seed * PAIRS_PER_PROGRAM + j) % len(PAIRS)] for j in range(PAIRS_PER_PROGRAM)]
        tail = 5
        free = steps - 7 - 2 * len(pairs) - tail
        tokens = ["pair"] * len(pairs) + ["shrink_budget", "invalidate"] + ["free"] * (free - 2)
        tokens = [tokens[i] for i in self.rng.permutation(len(tokens))]
        tokens += (["delete"] if self.seed % 3 == 0 else ["free"]) + ["free"] * (tail - 1)
        after_hazard = False
        for tok in tokens:
            if tok == "pair":
                cls, op = pairs.pop(0)
                if cls == "dml":
                    cls = self.pick(["update", "insert"])
                self.ver += cls == "insert"  # the operator is built for the table the hazard leaves
                built = self.build(op)
                assert built is not None, (self.seed, cls, op)  # every operator is legal before a delete
                self.hazard(cls, built[0][1], bumped=True)
                self.op_step(forced=built)
                after_hazard = False
            elif tok in ("shrink_budget", "invalidate", "delete"):
                self.hazard(tok)
                after_hazard = True
            elif after_hazard or self.rng.random() < 0.75:
                self.op_step()
                after_hazard = False
            else:
                self.hazard(self.pick(["rewrite_all", "edit_one", "free_and_reuse", "update", "insert", "invalidate"]))
                after_hazard = True
        return self.steps


def program(seed: int, steps: int = STEPS):
    """The program of a seed: `steps` operator and hazard steps (drops come on top). The same
    seed gives the same list."""
    return _Gen(seed).run(steps)


def census(seeds=SEEDS, steps: int = STEPS):
    """(drawn, replaced, {kind: count}, {(hazard class, operator)}) over the seeds' programs."""
    drawn = replaced = 0
    counts, follows = {}, set()
    for s in seeds:
        g = _Gen(s)
        prog = [st for st in g.run(steps) if st[0] != "drop"]
        drawn += g.drawn
        replaced += g.replaced
        for i, st in enumerate(prog):
            counts[st[0]] = counts.get(st[0], 0) + 1
            if i and st[0] in OPS and prog[i - 1][0] in HAZARDS:
                h = prog[i - 1][0]
                follows.add(("dml" if h in DML else h, st[0]))
    return drawn, replaced, counts, follows
