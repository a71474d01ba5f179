"""group_aggregate_star at full size (not product code, run by no test): mq_group_star_plan at
--rows fact rows (the sweep is meant for 1e9 and 2^28), joined to 2 and 3 dense dimensions of
2^10, 2^16 and 2^20 keys whose attributes span 25 x 80 and 7 x 5 x 40 values, with no range
predicate and behind a leading range that passes 10 % of a uniform column, and with one more
dimension joined only as a filter that passes 50 % of the rows. Every fact key of a grouped
dimension has a partner. Each point stands beside what is not the code under test: (a) the chain
it replaces, one mq_keymap_lookup per dimension into an n-row attribute column (`missing` below
the map's attr_lo; the filtering dimension through a map of zeros) and then
mq_group_by_where_plan with one added range per attribute column; (b) mq_group_by_where_plan on
prejoined attribute columns with the same bounds (the same stream with no lookups: the floor;
the filter is a range on its prejoined column). The legs of one comparison alternate; host clock
around device-synchronised work, median of --reps after one warm-up. Result: one JSON object, to
--out.
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
ap.add_argument("--dims", default="10,16,20", help="log2 of the dimension sizes")
ap.add_argument("--spaces", default="25x80,7x5x40", help="attribute cardinalities of the grouped dimensions")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "star_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
MAX_DIMS = 4  # three grouped and the filtering one


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
    return (C.c_void_p * len(t))(*[x if isinstance(x, int) else x.data_ptr() for x in t])


def group_of(plan):
    """Run a plan call, return its groups, path and rows and free the handle."""
    h, g, path, rows = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint64()
    mq.check(plan(h, g, path, rows))
    mq.check(L.mq_group_free(h))
    return g.value, path.value, rows.value


lead, val = dev(n), dev(n)  # lead: uniform over [0, 1000)
fkeys = [dev(n) for _ in range(MAX_DIMS)]
pre = [dev(n) for _ in range(MAX_DIMS)]   # the prejoined attribute columns (the floor reads them, the chain rewrites them)
mq.check(L.mq_gen_uniform(lead.data_ptr(), n, 42, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
LEADS = [("none", None), ("10%", (0, 100))]
result = {"rows": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "points": []}

for dl in [int(x) for x in args.dims.split(",")]:
    n1 = 1 << dl
    dkeys = dev(n1)
    mq.check(L.mq_gen_iota(dkeys.data_ptr(), n1, None))  # a dense span: the keys are 0 .. n1 - 1
    for j in range(MAX_DIMS - 1):
        mq.check(L.mq_gen_uniform(fkeys[j].data_ptr(), n, 99 + dl + j, n1, 0))
    mq.check(L.mq_gen_uniform(fkeys[-1].data_ptr(), n, 7 + dl, 2 * n1, 0))  # half of them past the filter's keys
    for space in args.spaces.split(","):
        cards = [int(x) for x in space.split("x")]
        maps, infos, attrs = [], [], []
        for j, card in enumerate(cards):
            a = dev(n1)
            mq.check(L.mq_gen_uniform(a.data_ptr(), n1, 5 + dl + j, card, 0))
            km, info = C.c_void_p(), mq.MqKeymapInfo()
            mq.check(L.mq_keymap_build(dkeys.data_ptr(), a.data_ptr(), n1, 0, 0, 0, C.byref(km), C.byref(info), None), "mq_keymap_build")
            maps.append(km), infos.append(info), attrs.append(a)
        zeros = torch.zeros(n1, dtype=torch.int32, device="cuda")
        fmap = C.c_void_p()
        mq.check(L.mq_keymap_build(dkeys.data_ptr(), zeros.data_ptr(), n1, 0, 0, 0, C.byref(fmap), None, None), "mq_keymap_build")
        fset = L.mq_keymap_keyset(fmap)
        bounds_list = []
        for info in infos:
            bounds_list += [info.attr_lo, info.attr_hi]
        bounds = (C.c_int32 * len(bounds_list))(*bounds_list)
        nd = len(cards)

        def lookups(with_filter):
            for j in range(nd):
                mq.check(L.mq_keymap_lookup(maps[j], fkeys[j].data_ptr(), None, n, infos[j].attr_lo - 1, pre[j].data_ptr(), None, None))
            if with_filter:
                mq.check(L.mq_keymap_lookup(fmap, fkeys[-1].data_ptr(), None, n, -1, pre[-1].data_ptr(), None, None))

        lookups(True)
        for with_filter in (False, True):
            for lname, lr in LEADS:
                cols, rr = ((lead,), (lr,)) if lr else ((), ())
                terms = [mq.MqStarTerm(fkeys[-1].data_ptr(), None, fset)] if with_filter else []  # the filter first
                terms += [mq.MqStarTerm(fkeys[j].data_ptr(), maps[j].value, None) for j in range(nd)]
                tarr = (mq.MqStarTerm * len(terms))(*terms)
                # the chain's and the floor's predicates: the leading range (or one always-true range), one per attribute column
                ccols = list(cols) if lr else [lead]
                crr = list(rr) if lr else [(None, None)]
                if with_filter:
                    ccols.append(pre[-1]), crr.append((0, None))
                fcols, frr = list(ccols), list(crr)  # the floor: every grouped row has a partner, no range per attribute needed
                for j in range(nd):
                    ccols.append(pre[j]), crr.append((infos[j].attr_lo, None))
                keys = ptrs(*pre[:nd])

                def fused():
                    return group_of(lambda h, g, p, r: L.mq_group_star_plan(
                        ptrs(*cols) if cols else None, ranges(*rr) if rr else None, len(cols), tarr, len(terms), val.data_ptr(), n,
                        None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(g), C.byref(p), C.byref(r), None))

                def floor():
                    return group_of(lambda h, g, p, r: L.mq_group_by_where_plan(
                        ptrs(*fcols), ranges(*frr), len(fcols), keys, nd, val.data_ptr(), n, bounds, mq.MQ_GROUP_AUTO, C.byref(h),
                        C.byref(g), C.byref(p), C.byref(r), None))

                def chain():
                    lookups(with_filter)
                    return group_of(lambda h, g, p, r: L.mq_group_by_where_plan(
                        ptrs(*ccols), ranges(*crr), len(ccols), keys, nd, val.data_ptr(), n, bounds, mq.MQ_GROUP_AUTO, C.byref(h),
                        C.byref(g), C.byref(p), C.byref(r), None))

                g, path, rows = fused()
                assert (g, rows) == floor()[::2] == chain()[::2], "the fused plan, the chain and the prejoined floor disagree"
                t = timed({"group_star_plan": fused, "lookup_chain": chain, "group_by_where_plan_prejoined_floor": floor})
                point = {"dim_log2": dl, "space": space, "filter_dim": with_filter, "lead": lname, "groups": g, "path": path,
                         "joined_rows": rows, "ms": t, "ratio_to_chain": t["group_star_plan"]["ms"] / t["lookup_chain"]["ms"],
                         "ratio_to_floor": t["group_star_plan"]["ms"] / t["group_by_where_plan_prejoined_floor"]["ms"]}
                result["points"].append(point)
                print(json.dumps(point), flush=True)
        sync()
        for km in maps + [fmap]:
            L.mq_keymap_free(km)
        del attrs, zeros
    del dkeys

with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
