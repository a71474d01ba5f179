"""GROUP BY over several key columns at full size (not product code, run by no test):
mq_group_by_plan + mq_group_by_write at --rows rows with nkeys = 2 and 4, on the dense path
and on the packed sort path (forced), each with the key bounds given and with NULL bounds
(one mq_reduce per key column more), HIP events, median of --reps after one warm-up, all
inputs resident. The composite key distributions: uniform over 4 x 3 and over 45 x 45 tuples,
the same sorted by tuple, one tuple, and for the packed path uniform over 100 000 x 1000. With
four key columns each of the two components is split in two (4 x 3 = 2 x 2 x 3 x 1, 45 x 45 =
9 x 5 x 9 x 5, 100 000 x 1000 = 1000 x 100 x 100 x 10), so the tuples and their order are the
same. Yardsticks in the same run: mq_stream_read over nkeys + 1 columns (the ceiling for the
dense path's 4 (nkeys + 1) n bytes) and mq_group_plan + mq_group_write on one prepacked key
column holding the tuple's code (what the grouping costs when the key already is one column;
same path, same bounds mode). Result: one JSON object, to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "tests")]
import torch  # noqa: E402
from refapi import mq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_by_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
S = L.mq_group_dense_slots()
DENSE, SORT = mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT
PATH_NAME = {DENSE: "dense", SORT: "sort"}

# name -> (the ranges with two key columns, with four, sorted by tuple?)
DISTS = {
    "uniform_4x3": ((4, 3), (2, 2, 3, 1), False),
    "uniform_45x45": ((45, 45), (9, 5, 9, 5), False),
    "sorted_4x3": ((4, 3), (2, 2, 3, 1), True),
    "sorted_45x45": ((45, 45), (9, 5, 9, 5), True),
    "one_tuple": ((1, 1), (1, 1, 1, 1), False),
    "uniform_100000x1000": ((100_000, 1000), (1000, 100, 100, 10), False),
}
LO = (-5, 100, -1000, 7)  # every column's lower bound


def dev(count, dtype=torch.int32):
    return torch.empty(max(count, 1), dtype=dtype, device="cuda")


def timed(fn, reps=args.reps):
    """ms of fn() between two events on the null stream, after one warm-up: median, min, max."""
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


code, vals = dev(n), dev(n)
cols = [dev(n) for _ in range(4)]
mq.check(L.mq_gen_uniform(vals.data_ptr(), n, 7, 1 << 31, 0))
o_keys = [dev(n) for _ in range(4)]
o_cnt, o_sum, o_min, o_max = dev(n, torch.int64), dev(n, torch.int64), dev(n), dev(n)
swb = L.mq_scan_workspace_bytes(n)
sws = dev(swb, torch.uint8)


def fill_code(space, is_sorted, seed):
    """code[i] = the tuple's code in [0, space): uniform, or ascending with equal shares."""
    if is_sorted:
        step = 1 << 26
        for a in range(0, n, step):  # in pieces: no 8n-byte temporary
            i = torch.arange(a, min(a + step, n), dtype=torch.int64, device="cuda")
            code[a:a + len(i)] = (i * space // n).to(torch.int32)
    elif space == 1:
        code.fill_(0)
    else:
        mq.check(L.mq_gen_uniform(code.data_ptr(), n, seed, space, 0))
    torch.cuda.synchronize()


def fill_cols(ranges):
    """cols[j] = LO[j] + component j of code under `ranges` (the last the least significant)."""
    step = 1 << 26
    for a in range(0, n, step):
        rest = code[a:a + step].clone()
        for j in range(len(ranges) - 1, -1, -1):
            cols[j][a:a + len(rest)] = rest % ranges[j] + LO[j]
            rest = rest // ranges[j]
    torch.cuda.synchronize()


def group_by(nkeys, path, bounds, info):
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    keys = (C.c_void_p * nkeys)(*[c.data_ptr() for c in cols[:nkeys]])
    outs = (C.c_void_p * nkeys)(*[o.data_ptr() for o in o_keys[:nkeys]])
    b = None if bounds is None else (C.c_int32 * len(bounds))(*bounds)
    mq.check(L.mq_group_by_plan(keys, nkeys, vals.data_ptr(), n, b, path, C.byref(h), C.byref(g), C.byref(taken), 0))
    mq.check(L.mq_group_by_write(h, outs, o_cnt.data_ptr(), o_sum.data_ptr(), o_min.data_ptr(), o_max.data_ptr(), 0))
    mq.check(L.mq_group_free(h))
    info["groups"], info["path"] = g.value, PATH_NAME[taken.value]


def group_one(path, bounds, info):
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    b = None if bounds is None else (C.c_int32 * 2)(*bounds)
    mq.check(L.mq_group_plan(code.data_ptr(), vals.data_ptr(), n, b, path, C.byref(h), C.byref(g), C.byref(taken), 0))
    mq.check(L.mq_group_write(h, o_keys[0].data_ptr(), o_cnt.data_ptr(), o_sum.data_ptr(), o_min.data_ptr(),
                              o_max.data_ptr(), 0))
    mq.check(L.mq_group_free(h))
    info["groups"], info["path"] = g.value, PATH_NAME[taken.value]


def stream(ncols):
    rd = C.c_uint64()
    for t in (cols + [vals])[:ncols]:
        mq.check(L.mq_stream_read(t.data_ptr(), n, sws.data_ptr(), swb, C.byref(rd), 0))


res = {"rows": n, "reps": args.reps, "dense_slots": S, "stream_read": {}, "distributions": {}}
for nkeys in (2, 4):
    t = timed(lambda: stream(nkeys + 1))
    t["gbs"] = 4 * (nkeys + 1) * n / t["ms"] / 1e6
    res["stream_read"][f"{nkeys + 1}_columns"] = t
print("stream_read", json.dumps(res["stream_read"]), flush=True)

for seed, (name, (r2, r4, is_sorted)) in enumerate(DISTS.items()):
    space = r2[0] * r2[1]
    fill_code(space, is_sorted, 50 + seed)
    r = {"key_space": space, "single_key": {}, "by": {}}
    paths = ([DENSE] if space <= S else []) + [SORT]
    for path in paths:
        for mode, b in (("bounds_given", (0, space - 1)), ("bounds_null", None)):
            info = {}
            t = timed(lambda: group_one(path, b, info))
            t.update(info)
            r["single_key"][f"{PATH_NAME[path]}_{mode}"] = t
    for nkeys, ranges in ((2, r2), (4, r4)):
        fill_cols(ranges)
        ceiling = res["stream_read"][f"{nkeys + 1}_columns"]["ms"]
        bounds = [v for j, w in enumerate(ranges) for v in (LO[j], LO[j] + w - 1)]
        for path in paths:
            for mode, b in (("bounds_given", bounds), ("bounds_null", None)):
                info = {}
                t = timed(lambda: group_by(nkeys, path, b, info))
                t.update(info)
                assert t["path"] == PATH_NAME[path] and t["groups"] == r["single_key"][f"{PATH_NAME[path]}_{mode}"]["groups"]
                t["over_stream_read"] = t["ms"] / ceiling
                t["over_single_key"] = t["ms"] / r["single_key"][f"{PATH_NAME[path]}_{mode}"]["ms"]
                if path == DENSE:
                    t["gbs_of_%dn" % (4 * (nkeys + 1))] = 4 * (nkeys + 1) * n / t["ms"] / 1e6
                r["by"][f"nkeys{nkeys}_{PATH_NAME[path]}_{mode}"] = t
    res["distributions"][name] = r
    print(name, json.dumps(r), flush=True)

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
