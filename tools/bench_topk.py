"""Top k at full size (not product code, run by no test): mq_topk at --rows resident rows
over four value columns (uniform over the whole int32 range, uniform in [0, 100), all
equal, sorted ascending), k in 1, 10, 1000, 2^20, both directions, the path MQ_TOPK_AUTO
takes (the select path at these k) with the default candidate cap; HIP events, median of
--reps after one warm-up, the column resident. Yardsticks in the same run: mq_index_build
of the whole column (the only route to the k extreme rows without the operator; the k
entries are then read off its end) and mq_stream_read of the column, whose time multiplied
by the select path's reads (levels + 1 collect read) is that path's own traffic floor.
Result: one JSON object, to --out.
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "topk_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
KS = [1, 10, 1000, 1 << 20]
COLLECT_READS = 1


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


vals = dev(n)
o_v, o_p = dev(max(KS)), dev(max(KS))
iv, ip = dev(n), dev(n, torch.int64)
swb = L.mq_scan_workspace_bytes(n)
sws = dev(swb, torch.uint8)


def fill(name):
    if name == "uniform_full":  # two 31-bit draws, one shifted into the sign bit's half
        mq.check(L.mq_gen_uniform(vals.data_ptr(), n, 42, 1 << 31, 0))
        mq.check(L.mq_gen_uniform(iv.data_ptr(), n, 43, 2, 0))
        step = 1 << 26
        for a in range(0, n, step):  # in pieces: no large temporary
            vals[a:a + step] -= iv[a:a + step] << 31
    elif name == "uniform_100":
        mq.check(L.mq_gen_uniform(vals.data_ptr(), n, 42, 100, 0))
    elif name == "all_equal":
        vals.fill_(12345)
    elif name == "sorted":
        step = 1 << 26
        for a in range(0, n, step):
            i = torch.arange(a, min(a + step, n), dtype=torch.int64, device="cuda")
            vals[a:a + len(i)] = (i - n // 2).to(torch.int32)
    torch.cuda.synchronize()


def topk(k, desc, info):
    mq.check(L.mq_topk(vals.data_ptr(), None, n, k, desc, mq.MQ_TOPK_AUTO, 0, o_v.data_ptr(), o_p.data_ptr(),
                       C.byref(info), 0))


def stream():
    rd = C.c_uint64()
    mq.check(L.mq_stream_read(vals.data_ptr(), n, sws.data_ptr(), swb, C.byref(rd), 0))


res = {"rows": n, "reps": args.reps, "default_cap": L.mq_topk_default_cap(), "sort_div": mq.MQ_TOPK_SORT_DIV,
       "collect_reads": COLLECT_READS, "columns": {}}
for name in ("uniform_full", "uniform_100", "all_equal", "sorted"):
    fill(name)
    r = {"stream_read": timed(stream)}
    r["stream_read"]["gbs"] = 4 * n / r["stream_read"]["ms"] / 1e6
    r["index_build"] = timed(lambda: mq.check(L.mq_index_build(vals.data_ptr(), n, iv.data_ptr(), ip.data_ptr(), 0)))
    for desc in (0, 1):
        for k in KS:
            info = mq.MqTopkInfo()
            t = timed(lambda: topk(k, desc, info))
            t.update(path={mq.MQ_TOPK_SELECT: "select", mq.MQ_TOPK_SORT: "sort"}[info.path], levels=info.levels,
                     candidates=info.candidates, ties=info.ties)
            t["of_index_build"] = t["ms"] / r["index_build"]["ms"]
            if info.path == mq.MQ_TOPK_SELECT:
                floor = (info.levels + COLLECT_READS) * r["stream_read"]["ms"]
                t["traffic_floor_ms"] = floor
                t["over_traffic_floor"] = t["ms"] / floor
            r[f"{'desc' if desc else 'asc'}_k{k}"] = t
    res["columns"][name] = r
    print(name, json.dumps(r), flush=True)

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
