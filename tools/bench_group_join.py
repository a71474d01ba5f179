"""group_aggregate_join at full size (not product code, run by no test): mq_group_join_plan at
--rows fact rows (the sweep is meant for 1e9 and 2^28), joined to dense dimensions of 2^10,
2^16, 2^20 and 2^24 keys that carry 25 and 2000 different attributes, with no range predicate
and behind a leading range that passes 10 % and 1 % of a uniform column. Every fact key has a
partner. Each point stands beside what is not the code under test: (a) the chain it replaces,
mq_where_positions (and one mq_fetch of the foreign keys, when there is a range) ->
mq_join_build / mq_join_probe / mq_join_write -> mq_fetch x 2 -> mq_group_plan; (b)
mq_group_where_plan on a prejoined attribute column with the same bounds (the same stream with
no lookups: the floor; with no range, one always-true range on the leading column); (c)
mq_keymap_build alone. The legs of one comparison alternate; host clock around
device-synchronised work, median of --reps after one warm-up. Result: one JSON object, to --out.
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
ap.add_argument("--dims", default="10,16,20,24", help="log2 of the dimension sizes")
ap.add_argument("--cards", default="25,2000", help="attribute cardinalities")
ap.add_argument("--chain-max-rows", type=int, default=1 << 28, help="largest fact table the join chain is run at")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_join_bench.json"))
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


def ranges(*r):
    return (mq.MqRange * len(r))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in r])


def ptrs(*t):
    return (C.c_void_p * len(t))(*[x.data_ptr() for x in t])


lead, fkey, val, pre = dev(n), dev(n), dev(n), dev(n)  # lead: uniform over [0, 1000); pre: the prejoined attributes
mq.check(L.mq_gen_uniform(lead.data_ptr(), n, 42, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
wsb = max(L.mq_where_workspace_bytes(n), L.mq_scan_workspace_bytes(n))
ws = dev(wsb, torch.uint8)
cnt = dev(2, torch.int64)
LEADS = [("none", None), ("10%", (0, 100)), ("1%", (0, 10))]
result = {"rows": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "points": [], "build": []}
with_chain = n <= args.chain_max_rows
if with_chain:
    pos, fk, o1, o2, ja, jv = (dev(n) for _ in range(6))


def group_of(plan):
    """Run a plan call, return its groups and free the handle."""
    h, g, path, rows = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    mq.check(plan(h, g, path, rows))
    mq.check(L.mq_group_free(h))
    return g.value, path.value, rows.value


for dl in [int(x) for x in args.dims.split(",")]:
    n1 = 1 << dl
    dkeys, dattrs, iota = dev(n1), dev(n1), dev(n1)
    mq.check(L.mq_gen_iota(dkeys.data_ptr(), n1, None))  # a dense span: the keys are 0 .. n1 - 1
    mq.check(L.mq_gen_iota(iota.data_ptr(), n1, None))
    mq.check(L.mq_gen_uniform(fkey.data_ptr(), n, 99 + dl, n1, 0))
    for card in [int(x) for x in args.cards.split(",")]:
        mq.check(L.mq_gen_uniform(dattrs.data_ptr(), n1, 5 + dl, card, 0))
        km, info = C.c_void_p(), mq.MqKeymapInfo()
        mq.check(L.mq_keymap_build(dkeys.data_ptr(), dattrs.data_ptr(), n1, 0, 0, 0, C.byref(km), C.byref(info), None), "mq_keymap_build")
        mq.check(L.mq_keymap_lookup(km, fkey.data_ptr(), None, n, 0, pre.data_ptr(), None, None), "mq_keymap_lookup")
        bounds = (C.c_int32 * 2)(info.attr_lo, info.attr_hi)

        def build():
            h = C.c_void_p()
            mq.check(L.mq_keymap_build(dkeys.data_ptr(), dattrs.data_ptr(), n1, 0, 0, 0, C.byref(h), None, None))
            L.mq_keymap_free(h)

        point = {"dim_log2": dl, "card": card, "map_bytes": int(info.bytes), "ms": timed({"keymap_build": build})}
        result["build"].append(point)
        print(json.dumps(point), flush=True)
        for lname, lr in LEADS:
            cols, rr = ((lead,), (lr,)) if lr else ((), ())
            fcols, fr = (cols, rr) if lr else ((lead,), ((None, None),))

            def fused():
                return group_of(lambda h, g, p, r: L.mq_group_join_plan(
                    ptrs(*cols) if cols else None, ranges(*rr) if rr else None, len(cols), fkey.data_ptr(), km, val.data_ptr(), n,
                    None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g), C.byref(p), C.byref(r), None))

            def floor():
                return group_of(lambda h, g, p, r: L.mq_group_where_plan(
                    ptrs(*fcols), ranges(*fr), len(fcols), pre.data_ptr(), val.data_ptr(), n, bounds, mq.MQ_GROUP_AUTO, C.byref(h),
                    C.byref(g), C.byref(p), C.byref(r), None))

            def chain():
                k, probe = n, fkey
                if lr:
                    mq.check(L.mq_where_positions(ptrs(*cols), ranges(*rr), 1, None, n, pos.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                                  wsb, None))
                    sync()
                    k = int(cnt[0].item())
                    mq.check(L.mq_fetch(fkey.data_ptr(), pos.data_ptr(), k, fk.data_ptr(), None))
                    probe = fk
                j, m = C.c_void_p(), C.c_uint64()
                mq.check(L.mq_join_build(dkeys.data_ptr(), iota.data_ptr(), n1, C.byref(j), None))
                mq.check(L.mq_join_probe(j, probe.data_ptr(), k, C.byref(m), None))
                mq.check(L.mq_join_write(j, pos.data_ptr() if lr else None, o1.data_ptr(), o2.data_ptr() if lr else None, None))
                mq.check(L.mq_fetch(dattrs.data_ptr(), o1.data_ptr(), m.value, ja.data_ptr(), None))
                if lr:
                    mq.check(L.mq_fetch(val.data_ptr(), o2.data_ptr(), m.value, jv.data_ptr(), None))
                out = group_of(lambda h, g, p, r: L.mq_group_plan(
                    ja.data_ptr(), jv.data_ptr() if lr else val.data_ptr(), m.value, bounds, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g),
                    C.byref(p), None))
                sync()
                L.mq_join_free(j)
                return out

            legs = {"group_join_plan": fused, "group_where_plan_prejoined_floor": floor}
            if with_chain:
                legs["join_chain"] = chain
            g, path, rows = fused()
            assert (g, rows) == floor()[::2], "the fused plan and the prejoined floor disagree"
            point = {"dim_log2": dl, "card": card, "lead": lname, "groups": g, "path": path, "joined_rows": rows, "ms": timed(legs)}
            if with_chain:
                t = point["ms"]
                point["ratio_to_chain"] = t["group_join_plan"]["ms"] / t["join_chain"]["ms"]
            result["points"].append(point)
            print(json.dumps(point), flush=True)
        sync()
        L.mq_keymap_free(km)
    del dkeys, dattrs, iota

with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
