"""Batched row inserts at full size (not product code, run by no test): the insertion
points, the plan, the column expansion and the index merge of an insert of 1 % and 50 %
new rows into --rows rows x --cols columns, HIP events, median of --reps after one
warm-up. Yardsticks in the same run: mq_memcpy_d2d of half the expansion's read-plus-write
bytes (the yardstick of tools/bench_dml.py); for the index merge, building the index again
over the n + k rows with mq_index_build_ref; and for an append, the only route without the
operator: the new rows written to the host column and the whole column uploaded again with
mq_column_upload. The host write-back of one interleaved column over PCIe is timed on its
own. Result: one JSON object, to --out.
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
ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "insert_bench.json"))
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
# the sorted index of column 0: the clustered keys of the expansion, and the index merged into
iv, ip = dev(n), dev(n, torch.int64)
mq.check(L.mq_index_build(cols[0].data_ptr(), n, iv.data_ptr(), ip.data_ptr(), 0))
res = {"rows": n, "cols": ncols, "reps": args.reps, "insert": {}}

for label, k in (("1pct", n // 100), ("50pct", n // 2)):
    m = n + k
    new = [dev(k) for _ in range(ncols)]
    for j, c in enumerate(new):
        mq.check(L.mq_gen_uniform(c.data_ptr(), k, 142 + j, n, 0))
    outs = [dev(m) for _ in range(ncols)]
    spare = dev(m)
    skeys, order, ins, npos = dev(k), dev(k, torch.int64), dev(k), dev(k, torch.int64)
    ov, op = dev(m), dev(m, torch.int64)
    wsb = L.mq_insert_workspace_bytes(n, k)
    ws = dev(wsb, torch.uint8)
    bad = C.c_uint64()

    def sort_batch():
        mq.check(L.mq_index_build(new[0].data_ptr(), k, skeys.data_ptr(), order.data_ptr(), 0))

    def points():
        mq.check(L.mq_insert_points(iv.data_ptr(), n, skeys.data_ptr(), k, ins.data_ptr(), 0))

    def plan():
        mq.check(L.mq_insert_plan(ins.data_ptr(), k, n, C.byref(bad), ws.data_ptr(), wsb, 0))

    def columns():
        mq.check(L.mq_insert_columns(ws.data_ptr(), ptrs(cols), ptrs(new), ncols, ptrs(outs), 0))

    def positions():
        mq.check(L.mq_insert_positions(None, n, order.data_ptr(), k, npos.data_ptr(), 0))

    def index(ren):
        mq.check(L.mq_insert_index(ws.data_ptr(), iv.data_ptr(), ip.data_ptr(), skeys.data_ptr(), npos.data_ptr(),
                                   ins.data_ptr() if ren else None, k if ren else 0, ov.data_ptr(), op.data_ptr(), 0))

    r = {"new_rows": k, "sort_batch_ms": timed(sort_batch), "points_ms": timed(points), "plan_ms": timed(plan)}
    r["columns_ms"] = timed(columns)
    r["positions_ms"] = timed(positions)
    r["index_ms"] = timed(lambda: index(False))
    r["index_renumbered_ms"] = timed(lambda: index(True))
    r["merge_total_ms"] = r["sort_batch_ms"] + r["points_ms"] + r["plan_ms"] + r["positions_ms"] + r["index_ms"]
    # the yardstick of the merge: the index built again over the n + k rows (outs[0] holds them)
    exact = C.c_int()
    r["rebuild_ms"] = timed(lambda: mq.check(L.mq_index_build_ref(outs[0].data_ptr(), m, ov.data_ptr(), op.data_ptr(),
                                                                  0, C.byref(exact), 0)))
    r["rebuild_over_merge"] = r["rebuild_ms"] / r["merge_total_ms"]
    # the same bytes as a plain copy: a copy of B bytes reads B and writes B
    col_bytes = ncols * 8 * m  # 4n + 4k read, 4(n + k) written, per column
    r["columns_bytes"] = col_bytes
    r["copy_columns_ms"] = timed(lambda: [mq.check(L.mq_memcpy_d2d(outs[j].data_ptr(), spare.data_ptr(), 4 * m, 0))
                                          for j in range(ncols)])
    r["columns_gbs"] = col_bytes / r["columns_ms"] / 1e6
    r["copy_columns_gbs"] = col_bytes / r["copy_columns_ms"] / 1e6
    r["columns_fraction_of_copy"] = r["copy_columns_ms"] / r["columns_ms"]
    idx_bytes = 2 * 12 * m  # values and positions, read and written
    r["index_bytes"] = idx_bytes
    r["index_gbs"] = idx_bytes / r["index_ms"] / 1e6
    # an append on the device, one column: the old copy and the k new values (uploaded) into a new buffer
    host_new = np.empty(k, dtype=np.int32)
    host_new[:] = 7
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mq.check(L.mq_memcpy_d2d(spare.data_ptr(), cols[0].data_ptr(), 4 * n, 0))
    mq.check(L.mq_memcpy_h2d(spare.data_ptr() + 4 * n, host_new.ctypes.data, 4 * k, 0))
    mq.check(L.mq_stream_sync(0))
    r["append_device_one_column_ms"] = 1e3 * (time.perf_counter() - t0)
    # the write-back of one interleaved column to host memory, apart from the device time
    columns()
    torch.cuda.synchronize()
    host = np.empty(m, dtype=np.int32)
    host[:] = 0  # pages touched before the clock starts
    t0 = time.perf_counter()
    mq.check(L.mq_memcpy_d2h(host.ctypes.data, outs[0].data_ptr(), 4 * m, 0))
    mq.check(L.mq_stream_sync(0))
    r["writeback_one_column_ms"] = 1e3 * (time.perf_counter() - t0)
    if not args.no_host:
        # the route without the operator, one column: write the new rows, upload the column again
        mq.check(L.mq_memcpy_d2h(host.ctypes.data, cols[0].data_ptr(), 4 * n, 0))
        mq.check(L.mq_stream_sync(0))
        t0 = time.perf_counter()
        host[n:] = host_new
        t1 = time.perf_counter()
        c = make_column(host)
        mq.check(L.mq_column_upload(C.byref(c)))
        mq.check(L.mq_device_sync())
        t2 = time.perf_counter()
        L.mq_column_invalidate(C.byref(c))
        r["host_route_one_column"] = {"write_ms": 1e3 * (t1 - t0), "upload_ms": 1e3 * (t2 - t1),
                                      "total_ms": 1e3 * (t2 - t0)}
        r["host_route_over_device_append"] = 1e3 * (t2 - t0) / r["append_device_one_column_ms"]
    res["insert"][label] = r
    del new, outs, spare, skeys, order, ins, npos, ov, op, ws, host, host_new
    torch.cuda.empty_cache()

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
