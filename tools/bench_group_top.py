"""group_top_k at full size (not product code, run by no test): HAVING, ORDER BY an aggregate and
LIMIT on the device against the chain it replaces, every group written, downloaded and ordered on
the host. g = 2^11: the groups of a dense mq_group_plan at --rows rows (the sweep is meant for
1e8), mq_group_top (order by sum descending, HAVING count above the median) against
mq_group_write of everything -> D2H -> numpy argsort. g = 2^20 and 2^26: mq_topk64 on synthetic
int64 columns (a uniform sum and a filter column that passes half) against D2H of both columns ->
numpy mask and argsort. k in {10, 1000, g}. The legs of one comparison alternate; host clock around
device-synchronised work, median of --reps after one warm-up. Result: one JSON object, to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "tests")]
import torch  # noqa: E402
from refapi import mq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 1 << 26])
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_top_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))


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


def d2h(t, dtype):
    out = np.empty(t.numel(), dtype)
    mq.check(L.mq_memcpy_d2h(out.ctypes.data, t.data_ptr(), out.nbytes, None))
    return out


points = []

# g = 2^11: a dense plan's groups
n, G = args.rows, 1 << 11
keys, vals = dev(n), dev(n)
mq.check(L.mq_gen_uniform(keys.data_ptr(), n, 7, G, None))
mq.check(L.mq_gen_uniform(vals.data_ptr(), n, 8, 1_000_000, None))
h, g, path = C.c_void_p(), C.c_uint64(), C.c_int()
bounds = (C.c_int32 * 2)(0, G - 1)
mq.check(L.mq_group_plan(keys.data_ptr(), vals.data_ptr(), n, bounds, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g), C.byref(path), None))
g = g.value
ok, oc, osum = dev(g), dev(g, torch.int64), dev(g, torch.int64)
med = n // G
for k in (10, 1000, g):
    o = mq.MqGroupOrder(mq.MQ_AGG_SUM, 1, k, mq.MQ_AGG_COUNT, mq.MqRange64(1, med, 0, 0), mq.MQ_TOPK_AUTO, 0)
    m = C.c_uint64()
    kp = (C.c_void_p * 1)(ok.data_ptr())

    def top():
        mq.check(L.mq_group_top(h, C.byref(o), C.byref(m), kp, oc.data_ptr(), osum.data_ptr(), None, None, None, None))

    def chain():
        mq.check(L.mq_group_write(h, ok.data_ptr(), oc.data_ptr(), osum.data_ptr(), None, None, None))
        hk, hc, hs = d2h(ok, np.int32), d2h(oc, np.int64), d2h(osum, np.int64)
        idx = np.flatnonzero(hc >= med)
        idx = idx[np.argsort(~hs[idx], kind="stable")][:k]
        return hk[idx], hc[idx], hs[idx]

    points.append({"source": "mq_group_plan dense", "rows": n, "groups": g, "k": k, **timed({"mq_group_top": top, "chain": chain})})
mq.check(L.mq_group_free(h))
del keys, vals

# synthetic int64 columns
for g in args.sizes:
    v32, f32 = dev(g), dev(g)
    mq.check(L.mq_gen_uniform(v32.data_ptr(), g, 11, 1 << 31, None))
    mq.check(L.mq_gen_uniform(f32.data_ptr(), g, 12, 100, None))
    v, f = dev(g, torch.int64), dev(g, torch.int64)
    mq.check(L.mq_topk64_widen(v32.data_ptr(), g, v.data_ptr(), None))
    mq.check(L.mq_topk64_widen(f32.data_ptr(), g, f.data_ptr(), None))
    v.mul_(1 << 20)  # past int32: a sum
    ov, oi = dev(g, torch.int64), dev(g)
    r = mq.MqRange64(1, 50, 0, 0)
    for k in (10, 1000, g):
        info = mq.MqTopk64Info()

        def top():
            mq.check(L.mq_topk64(v.data_ptr(), f.data_ptr(), C.byref(r), g, k, 1, mq.MQ_TOPK_AUTO, 0, ov.data_ptr(), oi.data_ptr(),
                                 C.byref(info), None))

        def chain():
            hv, hf = d2h(v, np.int64), d2h(f, np.int64)
            idx = np.flatnonzero(hf >= 50)
            return idx[np.argsort(~hv[idx], kind="stable")][:k]

        t = timed({"mq_topk64": top, "chain": chain})
        points.append({"source": "synthetic int64", "groups": g, "k": k, "path": info.path, "levels": info.levels,
                       "candidates": info.candidates, **t})

res = {"tool": "tools/bench_group_top.py", "reps": args.reps, "points": points}
with open(args.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
