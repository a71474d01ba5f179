"""The chain model and its program generator (tests/chaincases.py), on the host alone.

A device replay compares libmq with this model after every step of the committed programs
("Residency under operator chains"), so three things must hold before such a
comparison means anything: the programs are
what the seeds say and reach every operator behind every kind of hazard; the model agrees
with the reference's own compiled operators wherever the reference has the operator; and
every hazard changes what the model's next call returns (a hazard that did nothing would
make the device comparison vacuous).
"""
import numpy as np
import pytest

import chaincases as cc
from refapi import Api, make_column

SMALL = 6000  # rows of the replay table: column 1's values stay inside [0, rows)


def test_programs_are_deterministic():
    progs = [cc.program(s) for s in cc.SEEDS]
    assert progs == [cc.program(s) for s in cc.SEEDS]
    assert len({repr(p) for p in progs}) == len(cc.SEEDS)
    for p in progs:
        assert sum(st[0] != "drop" for st in p) == cc.STEPS
        assert all(st[0] in cc.OPS or st[0] in cc.HAZARDS or st[0] == "drop" for st in p)


def test_committed_seeds_cover_every_operator_behind_every_hazard():
    """Preconditions on the inputs, not measurements: at most one drawn step in ten was
    replaced, every operator and hazard kind occurs three times or more, and every operator
    directly follows a rewrite_all, an edit_one, a free_and_reuse and a row edit somewhere."""
    drawn, replaced, counts, follows = cc.census()
    assert drawn >= len(cc.SEEDS) * cc.STEPS
    assert replaced * 10 <= drawn, (replaced, drawn)
    rare = {k: counts.get(k, 0) for k in cc.OPS + cc.HAZARDS if counts.get(k, 0) < 3}
    assert not rare, rare
    missing = [p for p in cc.PAIRS if p not in follows]
    assert not missing, missing


def test_programs_replay_on_any_table_size():
    """A program never looks at a value, so it is legal on the small table too: every step
    runs, equal-length operands are equally long, and every row id a fetch or a row edit
    takes lies inside the table."""
    for seed in cc.SEEDS:
        s = cc.Session(cc.make_table(SMALL), index_col=cc.INDEX_COL)
        for idx, step in enumerate(cc.program(seed)):
            if step[0] in ("fetch_column", "update", "delete"):
                ids = s.val(step[1][-1])
                assert len(ids) == 0 or (ids.min() >= 0 and ids.max() < s.rows), (seed, idx, step)
            if step[0] in ("add", "sub", "select_result"):
                assert len(s.val(step[1][0])) == len(s.val(step[1][1])), (seed, idx, step)
            s.apply(step, idx)


@pytest.fixture(scope="module")
def api(refcpu):
    if not refcpu.have_reference():
        pytest.skip("reference library not built (oracle/_ref)")
    return Api(refcpu.reference())


def _reference(api, s, step):
    """The reference's own answer to an operator step on the session's current bytes, as a
    list of arrays; None where the reference has no defined answer."""
    kind, ins, p = step
    v = [s.val(r) for r in ins]
    col = lambda a: make_column(np.ascontiguousarray(a))  # noqa: E731
    if kind == "select_scan":
        return [api.select_column(col(v[0]), *s.bounds(p["range"]))]
    if kind == "select_result":
        return [api.select_result(v[0], v[1], *s.bounds(p["range"]))]
    if kind == "fetch_column":
        return [api.fetch_column(col(v[0]), v[1])]
    if kind == "sum_column":
        return [np.array([api.sum_column(col(v[0]))])]
    if kind == "sum_result":
        return [np.array([api.sum_result(v[0])])]
    if kind == "average":
        return [np.array([api.average(v[0])])]
    if kind in ("min", "max"):
        if len(v[0]) == 0:  # the reference reads payload[0] of an empty result (query.c:392-437)
            return None
        return [np.array([getattr(api, kind)(v[0])])]
    if kind in ("add", "sub"):
        return [getattr(api, kind)(v[0], v[1])]
    if kind == "shared_select":
        # the reference splits the work by value range and reads past the column unless the
        # values lie in [0, rows) (test_oracle.py::test_shared_select_vs_reference)
        if len(v[0]) == 0 or v[0].min() < 0 or v[0].max() >= len(v[0]):
            return None
        bs = [s.bounds(r) for r in p["ranges"]]
        return api.shared_select(col(v[0]), [b[0] for b in bs], [b[1] for b in bs])
    if kind in ("hash_join", "nested_loop_join"):
        return list(api.join(v[0], v[1], v[2], v[3], kind="hash" if kind == "hash_join" else "nested"))
    raise KeyError(kind)


@pytest.mark.parametrize("seed", cc.SEEDS)
def test_model_agrees_with_the_reference(api, seed):
    s = cc.Session(cc.make_table(SMALL), index_col=cc.INDEX_COL)
    compared = 0
    for idx, step in enumerate(cc.program(seed)):
        want = _reference(api, s, step) if step[0] in cc.REFERENCE_OPS else None
        got = s.apply(step, idx)
        if want is None:
            continue
        compared += 1
        assert len(want) == len(got), (seed, idx, step)
        for w, (name, g) in zip(want, got.items()):
            assert np.array_equal(np.asarray(w, dtype=g.dtype), g, equal_nan=g.dtype == np.float64), (seed, idx, step, name)
    assert compared >= 7  # the prologue alone


def _fingerprint(s):
    """What the next operators would see: every column and every handle."""
    return [c.copy() for c in s.cols] + [s.h[k].copy() for k in sorted(s.h)]


def _differs(a, b):
    return len(a) != len(b) or any(not np.array_equal(x, y, equal_nan=x.dtype == np.float64) for x, y in zip(a, b))


@pytest.mark.parametrize("rows", [SMALL])
def test_every_hazard_changes_the_model(rows):
    """Each hazard of the committed programs that touches bytes, applied to the model alone,
    changes the bytes the following operators read (the next test shows a reader's answer
    changing with them). shrink_budget and invalidate change no bytes by definition; they
    must leave the model alone."""
    seen = {}
    for seed in cc.SEEDS:
        s = cc.Session(cc.make_table(rows), index_col=cc.INDEX_COL)
        prog = cc.program(seed)
        for idx, step in enumerate(prog):
            if step[0] in cc.HAZARDS:
                before = _fingerprint(s)
                target = s.val(step[1][0]) if step[1] else None
                s.apply(step, idx)
                changed = _differs(before, _fingerprint(s))
                if step[0] in ("shrink_budget", "invalidate"):
                    assert not changed, (seed, idx, step)
                elif target is None or len(target) > 1 or step[0] in cc.DML:
                    if step[0] in ("update", "delete") and len(s.val(step[1][-1])) == 0:
                        continue  # no row id listed: nothing to edit
                    assert changed, (seed, idx, step)
                    seen[step[0]] = seen.get(step[0], 0) + 1
            else:
                s.apply(step, idx)
    assert all(seen.get(k, 0) >= 3 for k in ("rewrite_all", "edit_one", "free_and_reuse", "update", "delete", "insert")), seen


def test_a_hazard_on_an_input_changes_the_next_result():
    """A directed cell in miniature: reader, hazard on its input, reader
    again; the second answer differs from the first for every hazard that edits bytes."""
    def fresh():
        s = cc.Session(cc.make_table(SMALL), index_col=cc.INDEX_COL)
        s.apply(("select_scan", (("c", 0),), {"range": ("pm", None, None)}), 0)
        s.apply(("fetch_column", (("c", 3), ("h", "t0")), {}), 1)
        return s
    reader = ("sum_result", (("h", "t1"),), {})
    colreader = ("select_scan", (("c", 0),), {"range": ("pm", 100, 300)})
    for hz in [("rewrite_all", (("c", 0),), {"seed": 5})] + [("edit_one", (("c", 0),), {"spot": sp}) for sp in cc.EDIT_SPOTS]:
        s = fresh()
        s.cols[0][:] = np.arange(SMALL)[::-1]  # every row distinct, ends and middle inside or outside the range
        s.cols[0][[0, 5, SMALL // 2, SMALL - 3, SMALL - 1]] = 1000
        a = s.apply(colreader, 2)["t2"].copy()
        s.apply(hz, 3)
        assert not np.array_equal(a, s.apply(colreader, 4)["t4"]), hz
    for hz in [("edit_one", (("h", "t1"),), {"spot": sp}) for sp in cc.EDIT_SPOTS] + [("free_and_reuse", (("h", "t1"),), {})]:
        s = fresh()
        a = s.apply(reader, 2)["t2"].copy()
        s.apply(hz, 3)
        b = s.apply(("fetch_column", (("c", 0), ("h", "t0")), {}), 4)  # noqa: F841
        changed = not np.array_equal(a, s.apply(reader, 5)["t5"])
        assert changed or hz[0] == "free_and_reuse", hz  # a reversal keeps a sum: checked on the bytes below
    s = fresh()
    old = s.h["t1"].copy()
    s.apply(("free_and_reuse", (("h", "t1"),), {}), 2)
    assert len(s.h["t1"]) == len(old) and not np.array_equal(s.h["t1"], old)
    for dml, reader2 in [(("update", (("c", 2), ("h", "t0")), {"value": 7}), ("sum_column", (("c", 2),), {})),
                         (("delete", (("h", "t9"),), {}), ("sum_column", (("c", 3),), {})),
                         (("insert", (), {"seed": 3, "k": 100}), ("sum_column", (("c", 3),), {}))]:
        s = fresh()
        s.apply(("select_scan", (("c", 0),), {"range": ("pm", 100, 300)}), 9)
        a = s.apply(reader2, 10)["t10"].copy()
        s.apply(dml, 11)
        assert not np.array_equal(a, s.apply(reader2, 12)["t12"]), dml
