"""select_where at full size (not product code, run by no test): mq_where_positions for 2 and
3 predicates against the device-level chain it replaces (mq_select_positions -> mq_fetch ->
mq_select_positions with a payload -> ..., the counts read back between the stages as the
chain needs them), and mq_where_agg for one predicate plus a value column against
mq_select_fetch_agg, at --rows resident rows per column. The leading predicate passes 0.1,
1, 10 and 50 % of a uniform column, then of a sorted one; every later predicate passes half
of a uniform column. A leading predicate that passes every row (its column still read) is
the no-skip yardstick: every line of the later columns is then requested. The legs of one
comparison alternate; host clock around device-synchronised work, median of --reps after
one warm-up. Per leg: the milliseconds, the algorithmic bytes (4n per column times the share
of its 128-byte lines that still hold a survivor, the bitmap, counts and scan of the
positions form, the output) and the rate those bytes give as a share of mq_stream_read's on
the same column. Result: one JSON object, to --out.
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
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "where_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n = args.rows
STEP = 1 << 26  # rows per piece of the torch-side work: no large temporary
LEADS = [("0.1%", 1), ("1%", 10), ("10%", 100), ("50%", 500), ("100%", 1000)]  # [0, width) of [0, 1000)
LATER = (0, 500)


def dev(count, dtype=torch.int32):
    return torch.empty(max(count, 1), dtype=dtype, device="cuda")


def sync():
    mq.check(L.mq_device_sync())


def timed_pair(legs, reps=args.reps):
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


cols = [dev(n) for _ in range(3)]
lead_sorted = dev(n)
val = dev(n)
pos_a, pos_b, fetched, out = dev(n), dev(n), dev(n), dev(n)
cnt = dev(2, torch.int64)
agg = dev(8, torch.int64)
wsb = max(L.mq_where_workspace_bytes(n), L.mq_scan_workspace_bytes(n))
ws = dev(wsb, torch.uint8)

for j, c in enumerate(cols):
    mq.check(L.mq_gen_uniform(c.data_ptr(), n, 42 + j, 1000, 0))
mq.check(L.mq_gen_uniform(val.data_ptr(), n, 77, 1 << 20, 0))
for a in range(0, n, STEP):  # ascending, uniform over [0, 1000)
    i = torch.arange(a, min(a + STEP, n), dtype=torch.int64, device="cuda")
    lead_sorted[a:a + len(i)] = (i * 1000 // n).to(torch.int32)
torch.cuda.synchronize()


def ptrs(cs):
    return (C.c_void_p * len(cs))(*[c.data_ptr() for c in cs])


def ranges(rs):
    return (mq.MqRange * len(rs))(*[mq.MqRange(1, lo, 1, hi) for lo, hi in rs])


def count():
    return int(cnt[0].item())


def where_positions(cs, rs):
    mq.check(L.mq_where_positions(ptrs(cs), ranges(rs), len(cs), None, n, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                  wsb, 0))
    return count()


def chain_positions(cs, rs):
    """The parent commit's route: a select, then per further predicate a gather and a select
    with the positions as payload; each stage needs the count of the one before."""
    mq.check(L.mq_select_positions(cs[0].data_ptr(), None, n, 1, rs[0][0], 1, rs[0][1], pos_a.data_ptr(), cnt.data_ptr(),
                                   ws.data_ptr(), wsb, 0))
    k, cur, nxt = count(), pos_a, pos_b
    for c, (lo, hi) in zip(cs[1:], rs[1:]):
        mq.check(L.mq_fetch(c.data_ptr(), cur.data_ptr(), k, fetched.data_ptr(), 0))
        mq.check(L.mq_select_positions(fetched.data_ptr(), cur.data_ptr(), k, 1, lo, 1, hi, nxt.data_ptr(), cnt.data_ptr(),
                                       ws.data_ptr(), wsb, 0))
        k, cur, nxt = count(), nxt, cur
    return k, cur


def live_line_shares(cs, rs):
    """Per column the share of its 32-row lines in which the predicates before it left a row
    (1 for the first), the share of lines with a final survivor, and K."""
    shares, live_final, k = [0] * len(cs), 0, 0
    lines = 0
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
    t = timed_pair({"s": lambda: mq.check(L.mq_stream_read(c.data_ptr(), n, ws.data_ptr(), wsb, C.byref(rd), 0))})["s"]
    t["gbs"] = rd.value / t["ms"] / 1e6
    return t


# the positions form's own traffic besides the columns: the bitmap written and read (n / 8
# each), a count per 256 rows written, read twice and written by the scan and read by the
# expand kernel (5 n / 64)
BITMAP_BYTES = 2 * n // 8 + 5 * n // 64

res = {"rows": n, "reps": args.reps, "later_predicates": "half of a uniform column each", "bitmap_bytes": BITMAP_BYTES,
       "k_stream_read": stream_ms(cols[0]), "positions": {}, "aggregate": {}}
stream_gbs = res["k_stream_read"]["gbs"]
print("k_stream_read", json.dumps(res["k_stream_read"]), flush=True)

for lead_name, lead in (("uniform", cols[0]), ("sorted", lead_sorted)):
    for P in (2, 3):
        cs = [lead] + cols[1:P]
        for sel, width in LEADS:
            rs = [(0, width)] + [LATER] * (P - 1)
            shares, _, k = live_line_shares(cs, rs)
            assert where_positions(cs, rs) == k
            kc, cur = chain_positions(cs, rs)
            assert kc == k and torch.equal(cur[:k], out[:k]), "the chain and mq_where_positions differ"
            t = timed_pair({"where": lambda: where_positions(cs, rs), "chain": lambda: chain_positions(cs, rs)})
            bytes_ = int(4 * n * sum(shares)) + BITMAP_BYTES + 4 * k
            r = {"K": k, "live_line_share": shares, "algorithmic_bytes": bytes_, **t}
            r["where"]["gbs"] = bytes_ / r["where"]["ms"] / 1e6
            r["where"]["of_stream_read"] = r["where"]["gbs"] / stream_gbs
            r["where_over_chain"] = r["where"]["ms"] / r["chain"]["ms"]
            res["positions"][f"{lead_name}_P{P}_{sel}"] = r
            print(lead_name, P, sel, json.dumps(r), flush=True)

for lead_name, lead in (("uniform", cols[0]), ("sorted", lead_sorted)):
    for sel, width in LEADS:
        rs = [(0, width)]
        _, live_final, k = live_line_shares([lead], rs)

        def fused():
            mq.check(L.mq_select_fetch_agg(lead.data_ptr(), val.data_ptr(), n, 1, 0, 1, width, agg.data_ptr(), ws.data_ptr(),
                                           wsb, 0))

        def where():
            mq.check(L.mq_where_agg(ptrs([lead]), ranges(rs), 1, val.data_ptr(), n, agg.data_ptr(), ws.data_ptr(), wsb, 0))

        fused()
        sync()
        want = agg[:3].tolist()
        where()
        sync()
        assert agg[:3].tolist() == want and want[0] == k, "mq_select_fetch_agg and mq_where_agg differ"
        t = timed_pair({"where": where, "select_fetch_agg": fused})
        bytes_ = int(4 * n * (1 + live_final))
        r = {"K": k, "live_line_share": [1.0, live_final], "algorithmic_bytes": bytes_, **t}
        r["where"]["gbs"] = bytes_ / r["where"]["ms"] / 1e6
        r["where"]["of_stream_read"] = r["where"]["gbs"] / stream_gbs
        r["where_over_select_fetch_agg"] = r["where"]["ms"] / r["select_fetch_agg"]["ms"]
        res["aggregate"][f"{lead_name}_{sel}"] = r
        print("agg", lead_name, sel, json.dumps(r), flush=True)

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
