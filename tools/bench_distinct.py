"""group_count_distinct at full size (not product code, run by no test): mq_group_distinct_plan on
each of its paths against the chain it replaces and against the read floor. The chain, where it
exists (nkeys <= 3 and key space x value span <= 2^32): mq_group_by_where_plan over the key columns
plus v as one more key, a write of the key tuples, mq_group_by_plan over those tuples. The floor:
mq_stream_read over every column the operator touches. Points: --rows rows (the sweep is meant for
1e9), one predicate that passes --pass percent, P tuples of nkeys key columns and W values, bounds
given and NULL. The legs of one comparison alternate; host clock around device-synchronised work,
median of --reps after one warm-up. Result: one JSON object, to --out.
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
ap.add_argument("--pass", dest="passing", type=int, nargs="*", default=[1, 10, 50, 100])
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "distinct_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows


def dev(count, dtype=torch.int32):
    return torch.empty(max(count, 1), dtype=dtype, device="cuda")


def sync():
    mq.check(L.mq_device_sync())


def timed(legs, reps=args.reps):
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


def column(seed, span):
    t = dev(n)
    mq.check(L.mq_gen_uniform(t.data_ptr(), n, seed, span, None))
    return t


def ptrs(ts):
    return (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


# (name, key ranges, value span): the LDS path, the bitmap path from a few KiB to its cap, the sort path
SHAPES = [("lds 25 x 64", [5, 5], 64), ("lds 2048 x 32", [2048], 32), ("bitmap 2^10 x 2^10", [32, 32], 1 << 10),
          ("bitmap 2^16 x 2^10", [256, 256], 1 << 10), ("bitmap 2^20 x 2^12", [1024, 1024], 1 << 12),
          ("bitmap 1 x 2^31", [1], 1 << 31), ("bitmap 300 x 2^20 (Q16-like)", [25, 12], 1 << 20),
          ("sort 2^30 x 2^20", [1 << 15, 1 << 15], 1 << 20), ("sort 2^12 x 2^31", [64, 64], 1 << 31)]

ws_bytes = L.mq_scan_workspace_bytes(n)
ws = dev(ws_bytes // 4 + 4)
pred = column(1, 100)
points = []
for name, kr, span in SHAPES:
    keys = [column(10 + j, r) for j, r in enumerate(kr)]
    vals = column(20, span)
    nk = len(kr)
    kb = (C.c_int32 * (2 * nk))(*[b for r in kr for b in (0, r - 1)])
    vb = (C.c_int32 * 2)(0, span - 1)
    space = 1
    for r in kr:
        space *= r
    for pct in args.passing:
        rng = (mq.MqRange * 1)(mq.MqRange(0, 0, 1, pct))  # pred < pct
        info = mq.MqGdistinctInfo()
        res = {}

        def fused(bounds):
            h, g = C.c_void_p(), C.c_uint64()
            mq.check(L.mq_group_distinct_plan(ptrs([pred]), rng, 1, ptrs(keys), nk, vals.data_ptr(), n, kb if bounds else None,
                                              vb if bounds else None, mq.MQ_GDISTINCT_AUTO, C.byref(h), C.byref(g), C.byref(info), None))
            res["groups"] = g.value
            mq.check(L.mq_group_distinct_free(h))

        def chain():
            h, g = C.c_void_p(), C.c_uint64()
            b = (C.c_int32 * (2 * nk + 2))(*(list(kb) + list(vb)))
            mq.check(L.mq_group_by_where_plan(ptrs([pred]), rng, 1, ptrs(keys + [vals]), nk + 1, vals.data_ptr(), n, b, mq.MQ_GROUP_AUTO,
                                              C.byref(h), C.byref(g), None, None, None))
            tuples = [dev(g.value) for _ in range(nk + 1)]
            mq.check(L.mq_group_by_write(h, ptrs(tuples), None, None, None, None, None))
            mq.check(L.mq_group_free(h))
            h2, g2 = C.c_void_p(), C.c_uint64()
            mq.check(L.mq_group_by_plan(ptrs(tuples[:nk]), nk, tuples[0].data_ptr(), g.value, kb, mq.MQ_GROUP_AUTO, C.byref(h2),
                                        C.byref(g2), None, None))
            mq.check(L.mq_group_free(h2))

        def floor():
            got = C.c_uint64()
            for t in [pred] + keys + [vals]:
                mq.check(L.mq_stream_read(t.data_ptr(), n, ws.data_ptr(), ws_bytes, C.byref(got), None))

        legs = {"bounds": lambda: fused(True), "null_bounds": lambda: fused(False), "stream_read": floor}
        if nk <= 3 and space * span <= 1 << 32:
            legs["chain"] = chain
        t = timed(legs)
        points.append({"shape": name, "rows": n, "pass_pct": pct, "path": info.path, "space": info.space, "span": info.span,
                       "bitmap_bytes": info.bitmap_bytes, "matching": info.rows, "pairs": info.pairs, "groups": res.get("groups"), **t})
    del keys, vals

out = {"tool": "tools/bench_distinct.py", "reps": args.reps, "points": points}
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
