"""Row deletes and updates at full size (not product code, run by no test): the plan,
the column compaction and the index step of a delete at --rows rows x --cols columns
with 1 % and 50 % of the rows deleted, and an update of the 1 % list's rows, HIP events,
median of --reps after one warm-up. Two yardsticks in the same run: mq_memcpy_d2d of the
same read-plus-write bytes (the copy rate README quotes for dense position writes), and
the only route without these operators: compacting the host rows (numpy, one column)
and uploading the column again with mq_column_upload. The host write-back of the
compacted rows over PCIe is timed on its own. Result: one JSON object, to --out.
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
from refapi import make_column, mq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000_000)
ap.add_argument("--cols", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-host", action="store_true", help="skip the host-route yardstick")
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "dml_bench.json"))
args = ap.parse_args()

L = mq.load()
mq.check(L.mq_init(0))
n, ncols = args.rows, args.cols


def dev(count, dtype=torch.int32):
    return torch.empty(max(count, 1), dtype=dtype, device="cuda")


def timed(fn, reps=args.reps):
    """Median ms of fn() between two events on the null stream, after one warm-up."""
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


cols = [dev(n) for _ in range(ncols)]
for j, c in enumerate(cols):
    mq.check(L.mq_gen_uniform(c.data_ptr(), n, 42 + j, n, 0))
outs = [dev(n) for _ in range(ncols)]
iv, ip = dev(n), dev(n, torch.int64)
mq.check(L.mq_index_build(cols[0].data_ptr(), n, iv.data_ptr(), ip.data_ptr(), 0))
ov, op = dev(n), dev(n, torch.int64)
wsb = L.mq_delete_workspace_bytes(n)
ws = dev(wsb, torch.uint8)
swb = L.mq_scan_workspace_bytes(n)
sws = dev(swb, torch.uint8)
cnt = dev(1, torch.int64)
res = {"rows": n, "cols": ncols, "reps": args.reps, "delete": {}}

for label, hi in (("1pct", n // 100), ("50pct", n // 2)):
    # the ids: ascending positions of column 0's values in [0, hi)
    pos = dev(n)
    mq.check(L.mq_select_positions(cols[0].data_ptr(), None, n, 1, 0, 1, hi, pos.data_ptr(), cnt.data_ptr(),
                                   sws.data_ptr(), swb, 0))
    k = int(cnt.item())
    deleted, bad = C.c_uint64(), C.c_uint64()

    def plan():
        mq.check(L.mq_delete_plan(pos.data_ptr(), k, n, C.byref(deleted), C.byref(bad), ws.data_ptr(), wsb, 0))

    def columns():
        mq.check(L.mq_delete_columns(ws.data_ptr(), ptrs(cols), ncols, ptrs(outs), 0))

    def index():
        mq.check(L.mq_delete_index(ws.data_ptr(), iv.data_ptr(), ip.data_ptr(), ov.data_ptr(), op.data_ptr(), 0))

    r = {"ids": k, "plan_ms": timed(plan)}
    d = deleted.value
    left = n - d
    r["deleted"] = d
    r["columns_ms"] = timed(columns)
    r["index_ms"] = timed(index)
    # the same bytes as a plain copy: a copy of B bytes reads B and writes B
    col_bytes = ncols * (4 * n + 4 * left)
    idx_bytes = 2 * 8 * n + 4 * n + 12 * left  # positions twice (count, write), values, both outputs
    r["columns_bytes"], r["index_bytes"] = col_bytes, idx_bytes
    r["copy_columns_ms"] = timed(lambda: [mq.check(L.mq_memcpy_d2d(outs[j].data_ptr(), cols[j].data_ptr(),
                                                                   col_bytes // ncols // 2, 0)) for j in range(ncols)])
    r["copy_index_ms"] = timed(lambda: mq.check(L.mq_memcpy_d2d(op.data_ptr(), ip.data_ptr(),
                                                                min(idx_bytes // 2, 8 * n), 0)))
    r["copy_index_bytes"] = 2 * min(idx_bytes // 2, 8 * n)
    r["columns_gbs"] = col_bytes / r["columns_ms"] / 1e6
    r["copy_columns_gbs"] = col_bytes / r["copy_columns_ms"] / 1e6
    r["columns_fraction_of_copy"] = r["copy_columns_ms"] / r["columns_ms"]
    r["index_gbs"] = idx_bytes / r["index_ms"] / 1e6
    r["copy_index_gbs"] = r["copy_index_bytes"] / r["copy_index_ms"] / 1e6
    r["index_fraction_of_copy"] = r["index_gbs"] / r["copy_index_gbs"]
    # the write-back of one column's surviving rows to host memory, apart from the device time
    mq.check(L.mq_delete_columns(ws.data_ptr(), ptrs(cols), ncols, ptrs(outs), 0))
    torch.cuda.synchronize()
    host = np.empty(left, dtype=np.int32)
    host[:] = 0  # pages touched before the clock starts
    t0 = time.perf_counter()
    mq.check(L.mq_memcpy_d2h(host.ctypes.data, outs[0].data_ptr(), 4 * left, 0))
    mq.check(L.mq_stream_sync(0))
    r["writeback_one_column_ms"] = 1e3 * (time.perf_counter() - t0)
    if not args.no_host:
        # the route without these operators, one column: compact the host rows, upload again
        full = np.empty(n, dtype=np.int32)
        mq.check(L.mq_memcpy_d2h(full.ctypes.data, cols[0].data_ptr(), 4 * n, 0))
        mq.check(L.mq_stream_sync(0))
        ids = np.empty(k, dtype=np.int32)
        mq.check(L.mq_memcpy_d2h(ids.ctypes.data, pos.data_ptr(), 4 * k, 0))
        mq.check(L.mq_stream_sync(0))
        t0 = time.perf_counter()
        keep = np.ones(n, dtype=bool)
        keep[ids] = False
        kept = full[keep]
        full[:len(kept)] = kept
        t1 = time.perf_counter()
        c = make_column(full[:len(kept)])
        mq.check(L.mq_column_upload(C.byref(c)))
        mq.check(L.mq_device_sync())
        t2 = time.perf_counter()
        L.mq_column_invalidate(C.byref(c))
        assert np.array_equal(kept, host), "device compaction differs from the host's"
        r["host_route_one_column"] = {"compact_ms": 1e3 * (t1 - t0), "upload_ms": 1e3 * (t2 - t1),
                                      "total_ms": 1e3 * (t2 - t0)}
        r["host_route_over_device_one_column"] = 1e3 * (t2 - t0) / ((r["plan_ms"] + r["columns_ms"]) / ncols)
        del full, keep, kept
    res["delete"][label] = r
    if label == "1pct":
        # update: the 1 % list's rows of one column
        res["update"] = {"ids": k, "ms": timed(lambda: mq.check(L.mq_update_rows(outs[1].data_ptr(), n, pos.data_ptr(), k,
                                                                                 -10, None, 0)))}
    del pos

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
