"""group_aggregate_where at full size (not product code, run by no test): mq_group_where_plan
+ mq_group_write + mq_group_free against the device-level chain it replaces
(mq_where_positions -> the count read back -> mq_fetch x 2 -> mq_group_plan + write + free,
with the same bounds), at --rows resident rows per column. The leading predicate passes 0.1,
1, 10, 50 and 100 % of a uniform column, then of a sorted one; with P = 2 a second predicate
passes half of a uniform column. Keys: uniform in [0, 100), uniform in [0, S), sorted with
100 keys; key bounds given and not given. At 100 % with P = 1 the predicate is also left
unbounded (no predicate column is read) and compared with plain mq_group_plan, of this
library and, with --parent-lib, of another build's. The legs of one comparison alternate
in one process; host clock around device-synchronised work, median of --reps after one
warm-up. Per comparison: the milliseconds, the fused plan's algorithmic bytes (4n per column
times the share of its 128-byte lines that are requested; without bounds the predicate and
key lines twice) and the rate they give as a share of mq_stream_read's in the same run.
Result: one JSON object, to --out.
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
ap.add_argument("--lib", default=None, help="the libmq.so under test (default: the tree's)")
ap.add_argument("--parent-lib", default=None, help="another build of libmq.so whose mq_group_plan is timed at 100 %%")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "group_where_bench.json"))
args = ap.parse_args()

L = mq.load(os.path.abspath(args.lib)) if args.lib else mq.load()
mq.check(L.mq_init(0))
n = args.rows
S = L.mq_group_dense_slots()
AUTO = mq.MQ_GROUP_AUTO
STEP = 1 << 26  # rows per piece of the torch-side work: no large temporary
LEADS = [("0.1%", 1), ("1%", 10), ("10%", 100), ("50%", 500), ("100%", 1000)]  # [0, width) of [0, 1000)
LATER = (0, 500)


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


lead_uniform, lead_sorted, second, val = dev(n), dev(n), dev(n), dev(n)
keysets = {"u100": (dev(n), 100), "uS": (dev(n), S), "sorted100": (dev(n), 100)}
pos, fk, fv = dev(n), dev(n), dev(n)
cnt = dev(2, torch.int64)
outs = [dev(S), dev(S, torch.int64), dev(S, torch.int64), dev(S), dev(S)]  # keys, count, sum, min, max
wsb = max(L.mq_where_workspace_bytes(n), L.mq_scan_workspace_bytes(n))
ws = dev(wsb, torch.uint8)

mq.check(L.mq_gen_uniform(lead_uniform.data_ptr(), n, 42, 1000, 0))
mq.check(L.mq_gen_uniform(second.data_ptr(), n, 43, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
mq.check(L.mq_gen_uniform(keysets["u100"][0].data_ptr(), n, 5, 100, 0))
mq.check(L.mq_gen_uniform(keysets["uS"][0].data_ptr(), n, 6, S, 0))
for a in range(0, n, STEP):  # ascending, uniform over [0, 1000) and over [0, 100)
    i = torch.arange(a, min(a + STEP, n), dtype=torch.int64, device="cuda")
    lead_sorted[a:a + len(i)] = (i * 1000 // n).to(torch.int32)
    keysets["sorted100"][0][a:a + len(i)] = (i * 100 // n).to(torch.int32)
torch.cuda.synchronize()


def ptrs(cs):
    return (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs])


def ranges(rs):
    return (mq.MqRange * len(rs))(*[mq.MqRange(lo is not None, lo or 0, hi is not None, hi or 0) for lo, hi in rs])


def c_bounds(b):
    return None if b is None else (C.c_int32 * 2)(*b)


def write_free(lib, h):
    mq.check(lib.mq_group_write(h, *[o.data_ptr() for o in outs], 0))
    mq.check(lib.mq_group_free(h))


def fused(cs, rs, keys, bounds):
    h, g, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
    mq.check(L.mq_group_where_plan(ptrs(cs), ranges(rs), len(cs), keys.data_ptr(), val.data_ptr(), n, c_bounds(bounds), AUTO,
                                   C.byref(h), C.byref(g), None, C.byref(rows), 0))
    write_free(L, h)
    return g.value, rows.value


def chain(cs, rs, keys, bounds):
    mq.check(L.mq_where_positions(ptrs(cs), ranges(rs), len(cs), None, n, pos.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, 0))
    k = int(cnt[0].item())
    mq.check(L.mq_fetch(keys.data_ptr(), pos.data_ptr(), k, fk.data_ptr(), 0))
    mq.check(L.mq_fetch(val.data_ptr(), pos.data_ptr(), k, fv.data_ptr(), 0))
    h, g = C.c_void_p(), C.c_uint64()
    mq.check(L.mq_group_plan(fk.data_ptr(), fv.data_ptr(), k, c_bounds(bounds), AUTO, C.byref(h), C.byref(g), None, 0))
    write_free(L, h)
    return g.value, k


def plain(lib, keys, bounds):
    h, g = C.c_void_p(), C.c_uint64()
    mq.check(lib.mq_group_plan(keys.data_ptr(), val.data_ptr(), n, c_bounds(bounds), AUTO, C.byref(h), C.byref(g), None, 0))
    write_free(lib, h)
    return g.value


def snapshot():
    sync()
    return [o.clone() for o in outs]


def live_line_shares(cs, rs):
    """Per predicate column the share of its 32-row lines that are requested (1 for the
    first), the share of lines with a final survivor (the key and value lines), and K."""
    shares, live_final, k, lines = [0] * len(cs), 0, 0, 0
    for a in range(0, n, STEP):
        b = min(a + STEP, n)
        m = torch.ones(b - a, dtype=torch.bool, device="cuda")
        pad = (-(b - a)) % 32
        for j, (c, (lo, hi)) in enumerate(zip(cs, rs)):
            mm = torch.nn.functional.pad(m, (0, pad)) if pad else m
            shares[j] += int(mm.view(-1, 32).any(1).sum().item())
            m &= (c[a:b] >= lo) & (c[a:b] < hi)
        mm = torch.nn.functional.pad(m, (0, pad)) if pad else m
        live_final += int(mm.view(-1, 32).any(1).sum().item())
        lines += (b - a + 31) // 32
        k += int(m.sum().item())
    return [s / lines for s in shares], live_final / lines, k


def stream_ms(c):
    rd = C.c_uint64()
    t = timed_legs({"s": lambda: mq.check(L.mq_stream_read(c.data_ptr(), n, ws.data_ptr(), wsb, C.byref(rd), 0))})["s"]
    t["gbs"] = rd.value / t["ms"] / 1e6
    return t


res = {"rows": n, "reps": args.reps, "dense_slots": S, "second_predicate": "half of a uniform column",
       "k_stream_read": stream_ms(lead_uniform), "sweep": {}, "pass_everything": {}}
stream_gbs = res["k_stream_read"]["gbs"]
print("k_stream_read", json.dumps(res["k_stream_read"]), flush=True)

for lead_name, lead in (("uniform", lead_uniform), ("sorted", lead_sorted)):
    for P in (1, 2):
        cs = [lead] + [second] * (P - 1)
        for sel, width in LEADS:
            rs = [(0, width)] + [LATER] * (P - 1)
            shares, live_final, k = live_line_shares(cs, rs)
            for kname, (keys, width_k) in keysets.items():
                for bounds in ((0, width_k - 1), None):
                    g1, rows = fused(cs, rs, keys, bounds)
                    a = snapshot()
                    g2, kc = chain(cs, rs, keys, bounds)
                    b = snapshot()
                    assert (g1, rows) == (g2, kc) and rows == k, "the fused plan and the chain differ"
                    assert all(torch.equal(x[:g1], y[:g1]) for x, y in zip(a, b)), "the fused plan and the chain differ"
                    t = timed_legs({"fused": lambda: fused(cs, rs, keys, bounds), "chain": lambda: chain(cs, rs, keys, bounds)})
                    passes = 1 if bounds else 2  # without bounds the predicate and key lines are read twice
                    bytes_ = int(4 * n * (passes * sum(shares) + (passes + 1) * live_final))
                    r = {"K": k, "groups": g1, "live_line_share": shares + [live_final], "algorithmic_bytes": bytes_, **t}
                    r["fused"]["gbs"] = bytes_ / r["fused"]["ms"] / 1e6
                    r["fused"]["of_stream_read"] = r["fused"]["gbs"] / stream_gbs
                    r["fused_over_chain"] = r["fused"]["ms"] / r["chain"]["ms"]
                    name = f"{lead_name}_P{P}_{sel}_{kname}_{'bounds' if bounds else 'nobounds'}"
                    res["sweep"][name] = r
                    print(name, json.dumps(r), flush=True)

# every row passes and no predicate column is read: the fused kernel against k_group_dense
parent = None
if args.parent_lib:
    parent = mq.load(os.path.abspath(args.parent_lib))
    mq.check(parent.mq_init(0))
for kname, (keys, width_k) in keysets.items():
    for bounds in ((0, width_k - 1), None):
        cs, rs = [lead_uniform], [(None, None)]
        g1, rows = fused(cs, rs, keys, bounds)
        a = snapshot()
        g2 = plain(L, keys, bounds)
        b = snapshot()
        assert g1 == g2 and rows == n and all(torch.equal(x[:g1], y[:g1]) for x, y in zip(a, b))
        legs = {"fused": lambda: fused(cs, rs, keys, bounds), "plain": lambda: plain(L, keys, bounds)}
        if parent:
            legs["plain_parent"] = lambda: plain(parent, keys, bounds)
        t = timed_legs(legs)
        bytes_ = 4 * n * (2 if bounds else 3)
        r = {"groups": g1, "algorithmic_bytes": bytes_, **t}
        for leg in r:
            if isinstance(r[leg], dict):
                r[leg]["of_stream_read"] = bytes_ / r[leg]["ms"] / 1e6 / stream_gbs
        r["fused_over_plain"] = r["fused"]["ms"] / r["plain"]["ms"]
        name = f"{kname}_{'bounds' if bounds else 'nobounds'}"
        res["pass_everything"][name] = r
        print("pass_everything", name, json.dumps(r), flush=True)

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
