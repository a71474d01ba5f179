"""Child of test_gpu_threads.py::test_first_use_from_many_threads: a fresh process in which
eight threads make their first libmq call at the same moment.

Each thread waits at a barrier, then calls mq_stream_create (the first libmq call of the
process races the device's first-use initialisation) and runs one folded aggregate,
mq_select_agg, on that stream (the occupancy cache's first fill for k_scan and eight
creations of arrival counters). Every aggregate is compared exactly with numpy. Prints one
JSON line; exits 0 only when all eight match, 3 when a thread is stuck.
"""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refapi import mq  # noqa: E402

THREADS, N, DEADLINE = 8, 70_001, 60.0


def main():
    L = mq.load()  # dlopen only: no libmq function has been called yet
    bar = threading.Barrier(THREADS)
    cols = [np.random.default_rng(100 + i).integers(-1000, 1000, N).astype(np.int32) for i in range(THREADS)]
    bounds = [(-500 + 40 * i, 300 + 50 * i) for i in range(THREADS)]
    got, errors = [None] * THREADS, [None] * THREADS

    def body(i):
        try:
            s, col, ws, out = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            bar.wait(DEADLINE)
            mq.check(L.mq_stream_create(C.byref(s)), "mq_stream_create")
            ws_bytes = L.mq_scan_workspace_bytes(N)
            for p, nbytes in ((col, 4 * N), (ws, ws_bytes), (out, 32)):
                mq.check(L.mq_malloc(C.byref(p), nbytes), "mq_malloc")
            mq.check(L.mq_memcpy_h2d(col, cols[i].ctypes.data, 4 * N, s), "h2d")
            lo, hi = bounds[i]
            mq.check(L.mq_select_agg(col, N, 1, lo, 1, hi, out, ws, ws_bytes, s), "mq_select_agg")
            a = mq.MqAgg()
            mq.check(L.mq_memcpy_d2h(C.byref(a), out, 32, s), "d2h")
            got[i] = [int(a.count), int(a.sum), int(a.min), int(a.max)]
            for p in (col, ws, out):
                L.mq_free(p)
            mq.check(L.mq_stream_destroy(s), "mq_stream_destroy")
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors[i] = repr(e)
            bar.abort()
        finally:
            L.mq_thread_release()

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(DEADLINE)
    stuck = [i for i, t in enumerate(threads) if t.is_alive()]
    want = []
    for v, (lo, hi) in zip(cols, bounds):
        m = v[(v >= lo) & (v < hi)].astype(np.int64)
        want.append([len(m), int(m.sum()), int(m.min()), int(m.max())])
    wrong = [i for i in range(THREADS) if got[i] != want[i]]
    ok = not stuck and not wrong and not any(errors)
    print(json.dumps({"ok": ok, "threads": THREADS, "wrong": wrong, "stuck": stuck, "errors": [e for e in errors if e]}), flush=True)
    os._exit(0 if ok else 3 if stuck else 1)  # a stuck daemon thread must not hold the exit up


if __name__ == "__main__":
    main()
