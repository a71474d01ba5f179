"""group_aggregate_measures at full size (not product code, run by no test): one
mq_group_measures_plan + mq_group_measures_write at --rows fact rows (the sweep is meant for 1e9,
or the largest size that fits) with nmeas 1, 2 and 4 over price, qty, disc and tax columns, on a
Q1-like shape (2 plain keys of 3 x 2 values, 6 tuples, behind a range that passes 98 % of a
uniform column) and an SSB-like shape (2 key maps of 2^16 keys whose attributes span 7 x 25
values, 175 tuples, behind a range that passes 10 %). Each point stands beside what is not the
code under test: (a) the chain the single-value plan offers, nmeas x mq_group_star_plan +
mq_group_by_write with mq_sub / mq_add into an n-row column first for SUB / ADD, on inputs where
int32 does not wrap (MUL has no chain: such a point's chain covers the other measures only and
says so); (b) mq_stream_read over the distinct columns the plan touches, the floor. The legs of
one comparison alternate; host clock around device-synchronised work, median of --reps after one
warm-up. Result: one JSON object, to --out.
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
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "measures_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
COL, ADD, SUB, MUL = mq.MQ_MEAS_COL, mq.MQ_MEAS_ADD, mq.MQ_MEAS_SUB, mq.MQ_MEAS_MUL


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
    return (C.c_void_p * len(t))(*[x if isinstance(x, int) or x is None else x.data_ptr() for x in t])


lead, k0, k1, tmp = dev(n), dev(n), dev(n), dev(n)
price, qty, disc, tax = dev(n), dev(n), dev(n), dev(n)
mq.check(L.mq_gen_uniform(lead.data_ptr(), n, 42, 1000, None))
for t, seed, mod in ((price, 1, 100_000), (qty, 2, 50), (disc, 3, 11), (tax, 4, 9)):  # no int32 wrap in a + b, a - b
    mq.check(L.mq_gen_uniform(t.data_ptr(), n, seed, mod, None))
ws = dev(8192)
MEASURES = {1: [(MUL, price, disc)], 2: [(MUL, price, disc), (COL, qty, None)],
            4: [(MUL, price, disc), (COL, qty, None), (SUB, price, tax), (ADD, price, qty)]}
MAXG = 256
keys_out = [dev(MAXG) for _ in range(2)]
count_out = dev(MAXG, torch.int64)
agg_out = [[dev(MAXG, torch.int64) for _ in range(4)] for _ in range(3)]
mn32, mx32 = dev(MAXG), dev(MAXG)
result = {"rows": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "points": []}


def shape(name):
    """(terms, bounds, leading range, the columns the terms read, what to free)"""
    if name == "q1":
        mq.check(L.mq_gen_uniform(k0.data_ptr(), n, 11, 3, None))
        mq.check(L.mq_gen_uniform(k1.data_ptr(), n, 12, 2, None))
        return [mq.MqStarTerm(k0.data_ptr(), None, None), mq.MqStarTerm(k1.data_ptr(), None, None)], [0, 2, 0, 1], (0, 980), []
    n1, maps, bounds = 1 << 16, [], []
    dkeys = dev(n1)
    mq.check(L.mq_gen_iota(dkeys.data_ptr(), n1, None))
    for j, (fk, card) in enumerate(((k0, 7), (k1, 25))):
        a = dev(n1)
        mq.check(L.mq_gen_uniform(a.data_ptr(), n1, 21 + j, card, None))
        mq.check(L.mq_gen_uniform(fk.data_ptr(), n, 31 + j, n1, None))
        km, info = C.c_void_p(), mq.MqKeymapInfo()
        mq.check(L.mq_keymap_build(dkeys.data_ptr(), a.data_ptr(), n1, 0, 0, 0, C.byref(km), C.byref(info), None), "mq_keymap_build")
        maps.append(km)
        bounds += [info.attr_lo, info.attr_hi]
    return [mq.MqStarTerm(k0.data_ptr(), maps[0].value, None), mq.MqStarTerm(k1.data_ptr(), maps[1].value, None)], bounds, (0, 100), maps


for sname in ("q1", "ssb"):
    terms, bounds_list, lr, maps = shape(sname)
    tarr = (mq.MqStarTerm * 2)(*terms)
    bounds = (C.c_int32 * 4)(*bounds_list)
    cols, rr = ptrs(lead), ranges(lr)
    for nmeas, meas in MEASURES.items():
        marr = (mq.MqMeasure * nmeas)(*[mq.MqMeasure(a.data_ptr(), b.data_ptr() if b is not None else None, op, 0) for op, a, b in meas])
        info = {}

        def fused():
            h, g, p, r = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
            mq.check(L.mq_group_measures_plan(cols, rr, 1, tarr, 2, marr, nmeas, n, bounds, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g),
                                              C.byref(p), C.byref(r), None), "mq_group_measures_plan")
            assert g.value <= MAXG
            mq.check(L.mq_group_measures_write(h, ptrs(*keys_out), count_out.data_ptr(), *[ptrs(*agg_out[i][:nmeas]) for i in range(3)],
                                               None), "mq_group_measures_write")
            mq.check(L.mq_group_measures_free(h))
            info.update(groups=g.value, path=p.value, joined_rows=r.value)

        chained = [m for m in meas if m[0] != MUL]

        def chain():
            for op, a, b in chained:
                v = a
                if op != COL:
                    mq.check((L.mq_sub if op == SUB else L.mq_add)(a.data_ptr(), b.data_ptr(), n, tmp.data_ptr(), None))
                    v = tmp
                h, g, p, r = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
                mq.check(L.mq_group_star_plan(cols, rr, 1, tarr, 2, v.data_ptr(), n, bounds, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g),
                                              C.byref(p), C.byref(r), None), "mq_group_star_plan")
                mq.check(L.mq_group_by_write(h, ptrs(*keys_out), count_out.data_ptr(), agg_out[0][0].data_ptr(), mn32.data_ptr(),
                                             mx32.data_ptr(), None), "mq_group_by_write")
                mq.check(L.mq_group_free(h))

        touched = {id(t): t for t in [lead, k0, k1] + [x for _, a, b in meas for x in (a, b) if x is not None]}

        def floor():
            got = C.c_uint64()
            for t in touched.values():
                mq.check(L.mq_stream_read(t.data_ptr(), n, ws.data_ptr(), 8192 * 4, C.byref(got), None), "mq_stream_read")

        legs = {"group_measures_plan_write": fused, "stream_read_floor": floor}
        if chained:
            legs["star_plan_chain"] = chain
        t = timed(legs)
        point = {"shape": sname, "nmeas": nmeas, "ops": [op for op, _, _ in meas], "columns_touched": len(touched), **info, "ms": t,
                 "chain_measures": len(chained), "chain_covers_every_measure": len(chained) == nmeas,
                 "ratio_to_floor": t["group_measures_plan_write"]["ms"] / t["stream_read_floor"]["ms"],
                 "ratio_to_chain": t["group_measures_plan_write"]["ms"] / t["star_plan_chain"]["ms"] if chained else None}
        result["points"].append(point)
        print(json.dumps(point), flush=True)
    sync()
    for km in maps:
        L.mq_keymap_free(km)

with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
