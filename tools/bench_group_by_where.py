"""group_aggregate_by_where at full size (not product code, run by no test):
mq_group_by_where_plan + mq_group_by_write + mq_group_free with nkeys = 2 and 4 against
  (a) the device-level chain it replaces: mq_where_positions -> the count read back ->
      mq_fetch x (nkeys + 1) -> mq_group_by_plan + write + free, with the same bounds;
  (b) mq_group_by_plan + write + free when every range is unbounded (no predicate column is
      read),
at --rows resident rows per column. The leading predicate passes 0.1, 1, 10, 50 and 100 % of
a uniform column, then of a clustered one (ascending: one live stretch); a second predicate
passes half of a uniform column, so that 0.05 to 50 % of the rows match. Keys: uniform over
45 x 45 tuples (9 x 5 x 9 x 5 with four key columns), the dense path, with the key bounds given
and with NULL bounds; and with 10 % of the rows matching uniform over 100 000 x 1000 tuples
(1000 x 100 x 100 x 10), the sort path, bounds given. The legs of one
comparison alternate in one process; host clock around device-synchronised work, median of
--reps after one warm-up round; the outputs of the two legs are compared before they are
timed. Result: one JSON object, to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "tests")]
import torch  # noqa: E402
from refapi import mq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_by_where_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
S = L.mq_group_dense_slots()
AUTO, DENSE, SORT = mq.MQ_GROUP_AUTO, mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PATH_NAME = {DENSE: "dense", SORT: "sort"}
STEP = 1 << 26  # rows per piece of the torch-side work: no large temporary
LEADS = [("0.1%", 1), ("1%", 10), ("10%", 100), ("50%", 500), ("100%", 1000)]  # [0, width) of [0, 1000)
LATER = (0, 500)
LO = (-5, 100, -1000, 7)  # every key column's lower bound
DENSE_RANGES = {2: (45, 45), 4: (9, 5, 9, 5)}
SORT_RANGES = {2: (100_000, 1000), 4: (1000, 100, 100, 10)}
MAX_GROUPS = 1 << 27  # room for the sort configuration's groups (at most the 1e8 tuples)


def dev(count, dtype=torch.int32):
    return torch.empty(max(count, 1), dtype=dtype, device="cuda")


def sync():
    mq.check(L.mq_device_sync())


def timed_legs(legs, reps=args.reps):
    """{name: {ms, min_ms, max_ms}} of the legs run in turn, one warm-up round first."""
    ms = {k: [] for k in legs}
    for r in range(reps + 1):
        for k, fn in legs.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if r:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}
    return out


lead_uniform, lead_clustered, second, val, code = dev(n), dev(n), dev(n), dev(n), dev(n)
cols = [dev(n) for _ in range(4)]
pos, fv = dev(n), dev(n)
fk = [dev(n) for _ in range(4)]
cnt = dev(2, torch.int64)
groups_cap = min(n, MAX_GROUPS)
o_keys = [dev(groups_cap) for _ in range(4)]
o_aggs = [dev(groups_cap, torch.int64), dev(groups_cap, torch.int64), dev(groups_cap), dev(groups_cap)]  # count, sum, min, max
wsb = L.mq_where_workspace_bytes(n)
ws = dev(wsb, torch.uint8)

mq.check(L.mq_gen_uniform(lead_uniform.data_ptr(), n, 42, 1000, 0))
mq.check(L.mq_gen_uniform(second.data_ptr(), n, 43, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
for a in range(0, n, STEP):  # ascending, uniform over [0, 1000)
    i = torch.arange(a, min(a + STEP, n), dtype=torch.int64, device="cuda")
    lead_clustered[a:a + len(i)] = (i * 1000 // n).to(torch.int32)
torch.cuda.synchronize()


def fill_cols(ranges, seed):
    """cols[j] = LO[j] + component j of a uniform code under `ranges` (the last the least significant)."""
    space = 1
    for r in ranges:
        space *= r
    mq.check(L.mq_gen_uniform(code.data_ptr(), n, seed, space, 0))
    sync()
    for a in range(0, n, STEP):
        rest = code[a:a + STEP].clone()
        for j in range(len(ranges) - 1, -1, -1):
            cols[j][a:a + len(rest)] = rest % ranges[j] + LO[j]
            rest = rest // ranges[j]
    torch.cuda.synchronize()
    return [v for j, w in enumerate(ranges) for v in (LO[j], LO[j] + w - 1)]


def ptrs(cs):
    return (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs])


def ranges_of(rs):
    return (mq.MqRange * len(rs))(*[mq.MqRange(lo is not None, lo or 0, hi is not None, hi or 0) for lo, hi in rs])


def c_bounds(b):
    return None if b is None else (C.c_int32 * len(b))(*b)


def write_free(h, nkeys):
    mq.check(L.mq_group_by_write(h, ptrs(o_keys[:nkeys]), *[o.data_ptr() for o in o_aggs], 0))
    mq.check(L.mq_group_free(h))


def fused(cs, rs, nkeys, bounds, path=AUTO):
    h, g, rows, taken = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int()
    mq.check(L.mq_group_by_where_plan(ptrs(cs), ranges_of(rs), len(cs), ptrs(cols[:nkeys]), nkeys, val.data_ptr(), n,
                                      c_bounds(bounds), path, C.byref(h), C.byref(g), C.byref(taken), C.byref(rows), 0))
    write_free(h, nkeys)
    return g.value, rows.value, taken.value


def chain(cs, rs, nkeys, bounds, path=AUTO):
    mq.check(L.mq_where_positions(ptrs(cs), ranges_of(rs), len(cs), None, n, pos.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, 0))
    k = int(cnt[0].item())
    for j in range(nkeys):
        mq.check(L.mq_fetch(cols[j].data_ptr(), pos.data_ptr(), k, fk[j].data_ptr(), 0))
    mq.check(L.mq_fetch(val.data_ptr(), pos.data_ptr(), k, fv.data_ptr(), 0))
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    mq.check(L.mq_group_by_plan(ptrs(fk[:nkeys]), nkeys, fv.data_ptr(), k, c_bounds(bounds), path, C.byref(h), C.byref(g),
                                C.byref(taken), 0))
    write_free(h, nkeys)
    return g.value, k, taken.value


def plain(nkeys, bounds):
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    mq.check(L.mq_group_by_plan(ptrs(cols[:nkeys]), nkeys, val.data_ptr(), n, c_bounds(bounds), AUTO, C.byref(h), C.byref(g),
                                C.byref(taken), 0))
    write_free(h, nkeys)
    return g.value, n, taken.value


def snapshot(nkeys, g):
    sync()
    return [o[:g].clone() for o in o_keys[:nkeys] + o_aggs]


def compare(name, a_fn, b_fn, nkeys, b_name):
    """Run both legs once and compare every output, then time them in turn."""
    ga, rows_a, path_a = a_fn()
    a = snapshot(nkeys, ga)
    gb_, rows_b, path_b = b_fn()
    b = snapshot(nkeys, gb_)
    assert (ga, rows_a) == (gb_, rows_b) and all(torch.equal(x, y) for x, y in zip(a, b)), f"{name}: the legs differ"
    del a, b
    t = timed_legs({"fused": a_fn, b_name: b_fn})
    r = {"K": rows_a, "groups": ga, "path": PATH_NAME[path_a], **t}
    r[f"fused_over_{b_name}"] = r["fused"]["ms"] / r[b_name]["ms"]
    print(name, json.dumps(r), flush=True)
    return r


res = {"rows": n, "reps": args.reps, "dense_slots": S, "second_predicate": "half of a uniform column", "dense": {},
       "sort_10%": {}, "pass_everything": {}}
for nkeys in (2, 4):
    bounds = fill_cols(DENSE_RANGES[nkeys], 60 + nkeys)
    for lead_name, lead in (("uniform", lead_uniform), ("clustered", lead_clustered)):
        cs = [lead, second]
        for sel, width in LEADS:
            rs = [(0, width), LATER]
            for b in (bounds, None):
                name = f"nkeys{nkeys}_{lead_name}_{sel}_{'bounds' if b else 'nobounds'}"
                res["dense"][name] = compare(name, lambda: fused(cs, rs, nkeys, b), lambda: chain(cs, rs, nkeys, b), nkeys, "chain")
                assert res["dense"][name]["path"] == "dense"
    # every row passes and no predicate column is read: the fused kernel against k_group_by_dense
    for b in (bounds, None):
        name = f"nkeys{nkeys}_{'bounds' if b else 'nobounds'}"
        res["pass_everything"][name] = compare("pass_everything " + name, lambda: fused([lead_uniform], [(None, None)], nkeys, b),
                                               lambda: plain(nkeys, b), nkeys, "plain")
for nkeys in (2, 4):
    bounds = fill_cols(SORT_RANGES[nkeys], 70 + nkeys)
    cs, rs = [lead_uniform, second], [(0, 200), LATER]  # 20 % x 50 %: 10 % of the rows match
    name = f"nkeys{nkeys}_uniform_10%_bounds"
    res["sort_10%"][name] = compare("sort " + name, lambda: fused(cs, rs, nkeys, bounds), lambda: chain(cs, rs, nkeys, bounds),
                                    nkeys, "chain")
    assert res["sort_10%"][name]["path"] == "sort"

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
