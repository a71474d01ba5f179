"""Grouped aggregates at full size (not product code, run by no test): mq_group_plan +
mq_group_write at --rows rows over five key columns (uniform in [0, 100), uniform in
[0, S), sorted with 100 keys, one key, uniform in [0, rows)), the dense path and the sort
path forced on every column both accept, and the dense path again with the key bounds
given (no extra read of the keys), HIP events, median of --reps after one warm-up,
all inputs resident. Yardsticks in the same run: mq_stream_read over both columns (the
streaming ceiling for the dense path's 8n bytes), mq_index_build of the keys alone (what
the sort path pays before it folds), and the route without the operator: both columns to
the host and a numpy group-by, timed once at --host-rows rows. Result: one JSON object,
to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import groupcases as gc  # noqa: E402
from refapi import mq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=None, help="rows of the host-route yardstick (default: --rows; 0 skips it)")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
S = L.mq_group_dense_slots()
host_rows = n if args.host_rows is None else min(args.host_rows, n)


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


keys, vals = dev(n), dev(n)
mq.check(L.mq_gen_uniform(vals.data_ptr(), n, 7, 1 << 31, 0))
o_keys, o_cnt, o_sum, o_min, o_max = dev(n), dev(n, torch.int64), dev(n, torch.int64), dev(n), dev(n)
iv, ip = dev(n), dev(n, torch.int64)
swb = L.mq_scan_workspace_bytes(n)
sws = dev(swb, torch.uint8)


def fill(name):
    if name == "uniform_100":
        mq.check(L.mq_gen_uniform(keys.data_ptr(), n, 42, 100, 0))
    elif name == "uniform_S":
        mq.check(L.mq_gen_uniform(keys.data_ptr(), n, 43, S, 0))
    elif name == "sorted_100":
        step = 1 << 26
        for a in range(0, n, step):  # in pieces: no 8n-byte temporary
            i = torch.arange(a, min(a + step, n), dtype=torch.int64, device="cuda")
            keys[a:a + len(i)] = (i * 100 // n).to(torch.int32)
    elif name == "one_key":
        keys.fill_(12345)
    elif name == "uniform_n":
        mq.check(L.mq_gen_uniform(keys.data_ptr(), n, 44, n, 0))
    torch.cuda.synchronize()


BOUNDS = {"uniform_100": (0, 99), "uniform_S": (0, S - 1), "sorted_100": (0, 99), "one_key": (12345, 12345)}


def group(path, info, bounds=None):
    h, g, taken = C.c_void_p(), C.c_uint64(), C.c_int()
    b = None if bounds is None else (C.c_int32 * 2)(*bounds)
    mq.check(L.mq_group_plan(keys.data_ptr(), vals.data_ptr(), n, b, path, C.byref(h), C.byref(g), C.byref(taken), 0))
    mq.check(L.mq_group_write(h, o_keys.data_ptr(), o_cnt.data_ptr(), o_sum.data_ptr(), o_min.data_ptr(),
                              o_max.data_ptr(), 0))
    mq.check(L.mq_group_free(h))
    info["groups"], info["path"] = g.value, {mq.MQ_GROUP_DENSE: "dense", mq.MQ_GROUP_SORT: "sort"}[taken.value]


def stream_both():
    rd = C.c_uint64()
    for t in (keys, vals):
        mq.check(L.mq_stream_read(t.data_ptr(), n, sws.data_ptr(), swb, C.byref(rd), 0))


res = {"rows": n, "reps": args.reps, "dense_slots": S, "columns": {}}
res["stream_read_both_columns"] = timed(stream_both)
res["stream_read_both_columns"]["gbs"] = 8 * n / res["stream_read_both_columns"]["ms"] / 1e6
for name in ("uniform_100", "uniform_S", "sorted_100", "one_key", "uniform_n"):
    fill(name)
    r = {}
    for label, path in (("auto", mq.MQ_GROUP_AUTO), ("sort_forced", mq.MQ_GROUP_SORT)):
        if label == "sort_forced" and r["auto"]["path"] == "sort":
            continue
        info = {}
        t = timed(lambda: group(path, info))
        t.update(info)
        if t["path"] == "dense":
            t["gbs_of_8n"] = 8 * n / t["ms"] / 1e6
            t["fraction_of_stream_read"] = res["stream_read_both_columns"]["ms"] / t["ms"]
        r[label] = t
    if name in BOUNDS:  # the caller knows the bounds: no extra read of the keys
        info = {}
        t = timed(lambda: group(mq.MQ_GROUP_AUTO, info, BOUNDS[name]))
        t.update(info)
        t["gbs_of_8n"] = 8 * n / t["ms"] / 1e6
        t["fraction_of_stream_read"] = res["stream_read_both_columns"]["ms"] / t["ms"]
        r["auto_bounds_given"] = t
    r["index_build_keys"] = timed(lambda: mq.check(L.mq_index_build(keys.data_ptr(), n, iv.data_ptr(), ip.data_ptr(), 0)))
    if "sort_forced" in r:
        r["dense_faster_than_sort"] = r["auto"]["ms"] < r["sort_forced"]["ms"]
    res["columns"][name] = r
    print(name, json.dumps(r), flush=True)

u = res["columns"]["uniform_100"]["auto"]
for name in ("sorted_100", "one_key"):
    c = res["columns"][name]["auto"]
    # no slower than the uniform column by more than the run-to-run spread of the repetitions
    res["columns"][name]["within_spread_of_uniform_100"] = c["ms"] <= u["ms"] + (u["max_ms"] - u["min_ms"])

if host_rows:
    # the route without the operator: both columns over PCIe, a numpy group-by (timed once)
    fill("uniform_100")
    hk, hv = np.empty(host_rows, np.int32), np.empty(host_rows, np.int32)
    hk[:] = 0
    hv[:] = 0  # pages touched before the clock starts
    print("host route ...", flush=True)
    t0 = time.perf_counter()
    mq.check(L.mq_memcpy_d2h(hk.ctypes.data, keys.data_ptr(), 4 * host_rows, 0))
    mq.check(L.mq_memcpy_d2h(hv.ctypes.data, vals.data_ptr(), 4 * host_rows, 0))
    mq.check(L.mq_stream_sync(0))
    t1 = time.perf_counter()
    want = gc.group(hk, hv)
    t2 = time.perf_counter()
    res["host_route_uniform_100"] = {"rows": host_rows, "download_ms": 1e3 * (t1 - t0), "numpy_ms": 1e3 * (t2 - t1),
                                     "total_ms": 1e3 * (t2 - t0)}
    if host_rows == n:  # and the device's answer is the host's
        info = {}
        group(mq.MQ_GROUP_AUTO, info)
        torch.cuda.synchronize()
        g = info["groups"]
        got = (o_keys[:g].cpu().numpy(), o_cnt[:g].cpu().numpy().astype(np.uint64), o_sum[:g].cpu().numpy(),
               o_min[:g].cpu().numpy(), o_max[:g].cpu().numpy())
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "device groups differ from the host's"
        res["host_route_over_device"] = res["host_route_uniform_100"]["total_ms"] / u["ms"]

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
