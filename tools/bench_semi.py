"""select_where_in at full size (not product code, run by no test): mq_semi_positions and
mq_semi_agg at --rows probe rows, for key sets of 2^10 .. 2^32 values of span with 1 % and 50 %
of the values present, semi and anti, with no range predicate and behind a leading range that
passes 10 % and 1 % of a uniform column. Each point stands beside what is not the code under
test: (a) mq_where_positions / mq_where_agg on the same columns with the IN predicate replaced
by a range of the same selectivity on a uniform column (the same stream with no lookups: the
floor); (b) the chain mq_join_build -> mq_join_probe -> mq_join_counts -> mq_select_positions
over the counts, what a caller writes today, for the semi positions form with no range and the
sizes it can hold; (c) mq_keyset_build alone at 2^20, 2^24 and 2^28 build rows. A second sweep
runs bitmaps of 2^14 .. 2^17 bytes through both forced paths: the largest size at which LDS is
not slower than global is what kSemiLdsBytes should be. The legs of one comparison alternate;
host clock around device-synchronised work, median of --reps after one warm-up. Result: one
JSON object, to --out.
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
ap.add_argument("--spans", default="10,16,17,18,19,20,22,25,28,32", help="log2 of the set spans")
ap.add_argument("--chain-max-rows", type=int, default=1 << 28, help="largest probe the join chain is run at")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "semi_bench.json"))
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


lead, uni, key, val = dev(n), dev(n), dev(n), dev(n)  # lead, uni: uniform over [0, 1000)
out = dev(n)
cnt, agg = dev(2, torch.int64), dev(8, torch.int64)
wsb = max(L.mq_semi_workspace_bytes(n), L.mq_scan_workspace_bytes(n))
ws = dev(wsb, torch.uint8)
mq.check(L.mq_gen_uniform(lead.data_ptr(), n, 42, 1000, 0))
mq.check(L.mq_gen_uniform(uni.data_ptr(), n, 43, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
LEADS = [("none", None), ("10%", (0, 100)), ("1%", (0, 10))]
result = {"rows": n, "reps": args.reps, "device": torch.cuda.get_device_name(0), "lds_auto_bytes": None, "points": [],
          "lds_sweep": [], "build": []}
t = 16
while L.mq_semi_auto_path(t * 2) == mq.MQ_SEMI_LDS:
    t *= 2
result["lds_auto_bytes_pow2_floor"] = t


def build_set(span_log2, present):
    """A key set of `present` (0.01 or 0.5) of 2^span_log2 values: (handle, info, build keys)."""
    span = 1 << span_log2
    m = min(max(int(span * present), 2), 1 << 28)  # distinct draws are a little fewer: info.distinct says
    keys = dev(m)
    mq.check(L.mq_gen_uniform(keys.data_ptr(), m, 5 + span_log2, min(span, 1 << 32), 0))
    if span_log2 == 32:
        keys ^= -(1 << 31)  # [0, 2^32) read as int32 is already the whole range
    keys[0], keys[1] = (0, span - 1) if span_log2 < 32 else (-(1 << 31), (1 << 31) - 1)
    h, info = C.c_void_p(), mq.MqKeysetInfo()
    mq.check(L.mq_keyset_build(keys.data_ptr(), m, 0, 0, 0, C.byref(h), C.byref(info), None), "mq_keyset_build")
    return h, info, keys


def probe_keys(span_log2):
    """The probe's key column: uniform over the set's span, so the hit rate is the set's density."""
    span = 1 << span_log2
    mq.check(L.mq_gen_uniform(key.data_ptr(), n, 99, min(span, 1 << 32), 0))


def sel_range(frac):
    return (0, max(int(round(1000 * frac)), 1))


for sl in [int(x) for x in args.spans.split(",")]:
    probe_keys(sl)
    for present in (0.01, 0.5):
        h, info, bkeys = build_set(sl, present)
        density = info.distinct / float(1 << sl)
        for lname, lr in LEADS:
            cols, rr = ((lead,), (lr,)) if lr else ((), ())
            for anti in (0, 1):
                frac = 1 - density if anti else density
                floor_cols, floor_r = cols + (uni,), rr + (sel_range(frac),)
                legs = {
                    "semi_positions": lambda: mq.check(L.mq_semi_positions(
                        ptrs(*cols) if cols else None, ranges(*rr) if rr else None, len(cols), key.data_ptr(), h, anti,
                        mq.MQ_SEMI_AUTO, None, n, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, None)),
                    "where_positions_floor": lambda: mq.check(L.mq_where_positions(
                        ptrs(*floor_cols), ranges(*floor_r), len(floor_cols), None, n, out.data_ptr(), cnt.data_ptr(),
                        ws.data_ptr(), wsb, None)),
                    "semi_agg": lambda: mq.check(L.mq_semi_agg(
                        ptrs(*cols) if cols else None, ranges(*rr) if rr else None, len(cols), key.data_ptr(), h, anti,
                        mq.MQ_SEMI_AUTO, val.data_ptr(), n, agg.data_ptr(), ws.data_ptr(), wsb, None)),
                    "where_agg_floor": lambda: mq.check(L.mq_where_agg(
                        ptrs(*floor_cols), ranges(*floor_r), len(floor_cols), val.data_ptr(), n, agg.data_ptr(),
                        ws.data_ptr(), wsb, None)),
                }
                point = {"span_log2": sl, "set_bytes": int(info.bytes), "distinct": int(info.distinct), "density": density,
                         "path": int(L.mq_semi_auto_path(info.bytes)), "lead": lname, "anti": anti, "ms": timed(legs)}
                result["points"].append(point)
                print(json.dumps(point), flush=True)
        if n <= args.chain_max_rows:  # (b) today's spelling of the semi positions form with no range
            m = bkeys.numel()
            iota, counts = dev(m), dev(n)
            mq.check(L.mq_gen_iota(iota.data_ptr(), m, None))

            def chain():
                j, pairs = C.c_void_p(), C.c_uint64()
                mq.check(L.mq_join_build(bkeys.data_ptr(), iota.data_ptr(), m, C.byref(j), None))
                mq.check(L.mq_join_probe(j, key.data_ptr(), n, C.byref(pairs), None))
                mq.check(L.mq_join_counts(j, counts.data_ptr(), None))
                mq.check(L.mq_select_positions(counts.data_ptr(), None, n, 1, 1, 0, 0, out.data_ptr(), cnt.data_ptr(),
                                               ws.data_ptr(), wsb, None))
                sync()
                L.mq_join_free(j)

            def ours():
                hh = C.c_void_p()
                mq.check(L.mq_keyset_build(bkeys.data_ptr(), m, 0, 0, 0, C.byref(hh), None, None))
                mq.check(L.mq_semi_positions(None, None, 0, key.data_ptr(), hh, 0, mq.MQ_SEMI_AUTO, None, n, out.data_ptr(),
                                             cnt.data_ptr(), ws.data_ptr(), wsb, None))
                sync()
                L.mq_keyset_free(hh)

            point = {"span_log2": sl, "present": present, "build_rows": m, "chain_vs_build_plus_probe": timed({"join_chain": chain, "keyset_build_and_semi": ours})}
            result["points"].append(point)
            print(json.dumps(point), flush=True)
            del iota, counts
        sync()
        L.mq_keyset_free(h)
        del bkeys

# kSemiLdsBytes: both forced paths on bitmaps of 2^14 .. 2^17 bytes, no range, semi, 50 % present
for bl in (14, 15, 16, 17):
    sl = bl + 3
    probe_keys(sl)
    h, info, bkeys = build_set(sl, 0.5)
    legs = {}
    for pname, path in (("lds", mq.MQ_SEMI_LDS), ("global", mq.MQ_SEMI_GLOBAL)):
        legs[pname + "_positions"] = lambda path=path: mq.check(L.mq_semi_positions(
            None, None, 0, key.data_ptr(), h, 0, path, None, n, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, None))
        legs[pname + "_agg"] = lambda path=path: mq.check(L.mq_semi_agg(
            None, None, 0, key.data_ptr(), h, 0, path, val.data_ptr(), n, agg.data_ptr(), ws.data_ptr(), wsb, None))
    point = {"set_bytes": int(info.bytes), "ms": timed(legs)}
    result["lds_sweep"].append(point)
    print(json.dumps(point), flush=True)
    sync()
    L.mq_keyset_free(h)
    del bkeys

# (c) the build alone
for rl in (20, 24, 28):
    m = 1 << rl
    keys = dev(m)
    for sl in (16, 24, 32):
        mq.check(L.mq_gen_uniform(keys.data_ptr(), m, 3, min(1 << sl, 1 << 32), 0))

        def build():
            hh = C.c_void_p()
            mq.check(L.mq_keyset_build(keys.data_ptr(), m, 0, 0, 0, C.byref(hh), None, None))
            L.mq_keyset_free(hh)

        point = {"build_rows": m, "span_log2": sl, "ms": timed({"keyset_build": build})}
        result["build"].append(point)
        print(json.dumps(point), flush=True)
    del keys

with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
