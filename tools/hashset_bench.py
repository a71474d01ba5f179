"""Hashset bulk-insert timing (not product code).

For n uniformly random int32 keys and a table of the smallest prime >= 1.5 n slots:
  device   mq_hashset_insert with keys and table resident: HIP events on the library
           stream, 5 warm-up runs, median of 20 (the table is zeroed outside the events);
  gpu_api  mq_hashset_insert_many forced onto the GPU path (MQ_HASHSET_GPU_MIN=1):
           table up, build, table down; wall clock, median of --api-reps;
  host     mq_hashset_insert_many forced onto the host loop; wall clock, same reps.
n sweeps from 2^--log2 down by --step bits to 2^--min-log2; the crossover printed at the
end is the smallest n of the sweep from which gpu_api is no slower than host at every
larger n. One JSON line per n.

  python tools/hashset_bench.py [--log2 24] [--min-log2 10] [--step 2] [--api-reps 9]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from refapi import mq  # noqa: E402


def next_prime(x: int) -> int:
    x = max(x, 2)
    while True:
        if x < 4 or (x % 2 and all(x % d for d in range(3, int(x ** 0.5) + 1, 2))):
            return x
        x += 1


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def traffic_bytes(size: int, n: int, slots: int) -> int:
    """Least HBM bytes of one build, from the kernels' access patterns (no counters): the
    streamed passes (expand 4+8 per slot, scratch fill 8 and its scan 8 per scratch
    slot, keys 4 each, pack 8+4 per slot) plus one 64-byte sector read and written back
    per key for the scratch claim and again for the table slot it settles in."""
    return 12 * size + 16 * slots + 4 * n + 12 * size + 2 * 2 * 64 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=24)
    ap.add_argument("--min-log2", type=int, default=10)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--api-reps", type=int, default=9)
    a = ap.parse_args()
    L = mq.load()
    mq.check(L.mq_init(0))

    class Hashset(C.Structure):
        _fields_ = [("keys", C.POINTER(C.c_int32)), ("size", C.c_int)]
    L.create_hashset.restype = C.POINTER(Hashset)
    L.create_hashset.argtypes = [C.c_int]
    L.free_hashset.argtypes = [C.POINTER(Hashset)]
    L.free_hashset.restype = None

    st = L.mq_default_stream()
    ts = torch.cuda.ExternalStream(st)
    rng = np.random.default_rng(42)
    all_keys = rng.integers(-2**31, 2**31 - 1, 1 << a.log2, dtype=np.int64).astype(np.int32)
    rows = []
    for lg in range(a.log2, a.min_log2 - 1, -a.step):
        n = 1 << lg
        size = next_prime((3 * n + 1) // 2)
        keys = np.ascontiguousarray(all_keys[:n])
        d_keys = torch.from_numpy(keys).cuda()
        d_tab = torch.zeros(size, dtype=torch.int32, device="cuda")
        ws_bytes = L.mq_hashset_insert_workspace_bytes(size, n)
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        ms = []
        for r in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            mq.check(L.mq_memset(d_tab.data_ptr(), 0, size * 4, st))
            e0.record(ts)
            mq.check(L.mq_hashset_insert(d_tab.data_ptr(), size, d_keys.data_ptr(), n, d_cnt.data_ptr(),
                                         d_ws.data_ptr(), ws_bytes, st))
            e1.record(ts)
            torch.cuda.synchronize()
            if r >= 5:
                ms.append(e0.elapsed_time(e1))
        dev_table = d_tab.cpu().numpy()
        stored = int(d_cnt.item())
        del d_ws
        api = {}
        for path, gpu_min in (("gpu_api", "1"), ("host", str(2**62))):
            os.environ["MQ_HASHSET_GPU_MIN"] = gpu_min
            t = []
            for r in range(a.api_reps + 1):
                hs = L.create_hashset(size)
                t0 = time.perf_counter()
                rc = L.mq_hashset_insert_many(hs, keys.ctypes.data, n)
                t.append(1e3 * (time.perf_counter() - t0))
                assert rc == 0, rc
                if r == 0:  # the warm-up run is also the check against the device build
                    tab = np.ctypeslib.as_array(hs.contents.keys, shape=(size,))
                    assert np.array_equal(tab, dev_table), path
                L.free_hashset(hs)
            api[path] = median(t[1:])
            api[path + "_range"] = [round(min(t[1:]), 4), round(max(t[1:]), 4)]
        slots = 2
        while slots < 2 * n:
            slots <<= 1
        dev = median(ms)
        row = {"n": n, "size": size, "stored": stored, "device_ms": round(dev, 4),
               "gpu_api_ms": round(api["gpu_api"], 4), "host_ms": round(api["host"], 4),
               "gpu_api_min_max": api["gpu_api_range"], "host_min_max": api["host_range"],
               "est_bytes": traffic_bytes(size, n, slots),
               "est_gb_s": round(traffic_bytes(size, n, slots) / (dev * 1e-3) / 1e9, 1),
               "ws_bytes": ws_bytes}
        rows.append(row)
        print(json.dumps(row), flush=True)
    cross = None
    for row in rows:  # descending n: stop at the first n where the GPU path is slower
        if row["gpu_api_ms"] > row["host_ms"]:
            break
        cross = row["n"]
    print(json.dumps({"crossover_n": cross, "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
