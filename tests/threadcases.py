"""The worker harness and the per-family jobs of test_gpu_threads.py.

A job owns its device inputs, its workspace and its guarded outputs (all made on the main
thread), knows what the suite's models say its outputs are (`want`, bytes), and runs once
on a stream: `run(stream, rnd)` returns the outputs' bytes. Every output buffer is filled
with 0x5A before each run and is followed by GUARD words that must stay 0x5A, as in
test_gpu_join_regimes.py, so a thread that writes into another thread's buffers is caught.
One job is run by one thread at a time.
"""
import ctypes as C
import struct
import threading
import time

import numpy as np

import distinctcases as dcs
import groupbywherecases as gbw
import groupcases as gc
import joincases as jc
import measurecases as mc
import semicases as sc
import starcases as stc
import topk64cases as t64
import topkcases as tk
import wherecases as wc
from devbuf import Dev
from refapi import mq

N = 70_001            # the odd size of the drop-in tests: past one 1024-row tile, a ragged tail
WORKERS = 8
ROUNDS = 20
GUARD = 64            # int32 words past every output's end
FILL = 0x5A
PER_THREAD = 2        # hipStreamPerThread, as a void* stream
DEADLINE_FLOOR = 30.0
DEADLINE_FACTOR = 20.0

HUNG = []             # non-empty once a worker missed its deadline: nothing more runs on the GPU


def deadline_for(serial_seconds):
    """Generous on purpose: it tells a hang from slowness, it asserts no performance."""
    return max(DEADLINE_FLOOR, DEADLINE_FACTOR * serial_seconds)


def c_ranges(ranges):
    return (mq.MqRange * max(len(ranges), 1))(*[mq.MqRange(*mq.bounds(lo, hi)) for lo, hi in ranges])


def c_ptrs(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def c_i32(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def agg_bytes(a):
    """(count, sum, min, max) as the first 24 bytes of an mq_agg."""
    return struct.pack("<Qqii", *a)


def padded(want, cap):
    """`want` followed by the untouched fill of an output of `cap` elements."""
    want = np.ascontiguousarray(want)
    assert len(want) <= cap
    return want.tobytes() + bytes([FILL]) * ((cap - len(want)) * want.itemsize)


class Out:
    """A device array of n elements of `dtype` with GUARD words behind it."""

    def __init__(self, L, n, dtype=np.int32):
        self.L, self.n, self.dtype = L, int(n), np.dtype(dtype)
        self.bytes = self.n * self.dtype.itemsize
        self.total = (self.bytes + 15) // 16 * 16 + GUARD * 4
        self.dev = Dev(self.total)
        self.ptr = self.dev.ptr

    def arm(self, stream):
        mq.check(self.L.mq_memset(self.ptr, FILL, self.total, stream), "mq_memset")

    def read(self, stream):
        """The n elements' bytes once `stream` has drained; the guard must be as it was."""
        raw = np.empty(self.total, np.uint8)
        mq.check(self.L.mq_memcpy_d2h(raw.ctypes.data, self.ptr, self.total, stream), "d2h")
        assert np.all(raw[self.bytes:] == FILL), "guard words written"
        return raw[:self.bytes].tobytes()


class AggOut(Out):
    """An mq_agg (32 bytes); read: its count, sum, min and max (24 bytes)."""

    def __init__(self, L):
        super().__init__(L, 8)

    def read(self, stream):
        return super().read(stream)[:24]


class KeySet:
    """A key set built on the calling thread (the NULL stream) from a numpy column; `h` is immutable."""

    def __init__(self, L, keys):
        self.L, self.keys = L, np.ascontiguousarray(keys, np.int32)
        self.dev, h = Dev.of(self.keys), C.c_void_p()
        mq.check(L.mq_keyset_build(self.dev.ptr, len(self.keys), 0, 0, 0, C.byref(h), None, None), "mq_keyset_build")
        self.h = h.value

    def free(self):
        """Once every probe has completed."""
        mq.check(self.L.mq_device_sync(), "mq_device_sync")
        mq.check(self.L.mq_keyset_free(self.h), "mq_keyset_free")


class KeyMap:
    """A key map built on the calling thread (the NULL stream) from a dimension's numpy columns."""

    def __init__(self, L, keys, attrs):
        self.L = L
        self.keys, self.attrs = np.ascontiguousarray(keys, np.int32), np.ascontiguousarray(attrs, np.int32)
        self.dk, self.da, h = Dev.of(self.keys), Dev.of(self.attrs), C.c_void_p()
        mq.check(L.mq_keymap_build(self.dk.ptr, self.da.ptr, len(self.keys), 0, 0, 0, C.byref(h), None, None), "mq_keymap_build")
        self.h = h.value

    def free(self):
        mq.check(self.L.mq_device_sync(), "mq_device_sync")
        mq.check(self.L.mq_keymap_free(self.h), "mq_keymap_free")


class Job:
    """outs: the guarded outputs; want: their expected bytes, in the same order."""
    name = "job"

    def arm(self, stream):
        for o in self.outs:
            o.arm(stream)

    def read(self, stream):
        return [o.read(stream) for o in self.outs]

    def run(self, stream, rnd=0):
        self.arm(stream)
        extra = self.launch(stream, rnd) or []
        return self.read(stream) + extra

    def free(self):
        pass


class WhereJob(Job):
    """mq_where_positions (with a payload) + mq_where_agg on one workspace."""
    name = "where"

    def __init__(self, L, n=N, case="uniform_50", ncols=3):
        self.L, self.n = L, n
        self.cols, self.ranges = wc.case(case, n, ncols)
        pay, val = wc.payload_of(n), wc.values_of(n)
        self.keep = {id(c): Dev.of(c) for c in self.cols}
        self.ptrs = [self.keep[id(c)].ptr for c in self.cols]
        self.pay, self.val = Dev.of(pay), Dev.of(val)
        self.ws_bytes = L.mq_where_workspace_bytes(n)
        self.ws = Dev(self.ws_bytes)
        self.outs = [Out(L, n), Out(L, 1, np.uint64), AggOut(L)]
        w = wc.positions(self.cols, self.ranges, pay)
        self.want = [padded(w, n), struct.pack("<Q", len(w)), agg_bytes(wc.aggregate(self.cols, self.ranges, val))]

    def launch(self, s, rnd):
        L, o = self.L, self.outs
        cp, cr, k = c_ptrs(self.ptrs), c_ranges(self.ranges), len(self.ptrs)
        mq.check(L.mq_where_positions(cp, cr, k, self.pay.ptr, self.n, o[0].ptr, o[1].ptr, self.ws.ptr, self.ws_bytes, s), "where_positions")
        mq.check(L.mq_where_agg(cp, cr, k, self.val.ptr, self.n, o[2].ptr, self.ws.ptr, self.ws_bytes, s), "where_agg")


class SemiJob(Job):
    """Semi / anti (by round) positions and aggregate. own_set: the key set is built and freed
    inside every run (mq_keyset_build, from the pool); else `ks` is a shared, immutable handle."""
    name = "semi"

    def __init__(self, L, n=N, set_name="dense_small", ks=None, set_keys=None, key=None, ncols=1, seed_case="uniform_50"):
        self.L, self.n = L, n
        if key is None:
            key, set_keys = sc.keyset(set_name, n)
        self.cols, self.ranges = sc.case(seed_case, n, ncols)
        val = wc.values_of(n)
        self.keep = {id(c): Dev.of(c) for c in self.cols}
        self.ptrs = [self.keep[id(c)].ptr for c in self.cols]
        self.key, self.val, self.set = Dev.of(key), Dev.of(val), Dev.of(set_keys)
        self.n1, self.ks = len(set_keys), ks
        self.ws_bytes = L.mq_semi_workspace_bytes(n)
        self.ws = Dev(self.ws_bytes)
        self.outs = [Out(L, n), Out(L, 1, np.uint64), AggOut(L)]
        self.wants = []
        for anti in (False, True):
            w = sc.positions(self.cols, self.ranges, key, set_keys, anti)
            self.wants.append([padded(w, n), struct.pack("<Q", len(w)),
                               agg_bytes(sc.aggregate(self.cols, self.ranges, key, set_keys, val, anti))])
        self.want = self.wants[0]

    def want_of(self, rnd):
        return self.wants[rnd & 1]

    def launch(self, s, rnd):
        L, o, anti = self.L, self.outs, rnd & 1
        ks = self.ks
        if ks is None:
            h = C.c_void_p()
            mq.check(L.mq_keyset_build(self.set.ptr, self.n1, 0, 0, 0, C.byref(h), None, s), "keyset_build")
            ks = h
        cp, cr, k = (c_ptrs(self.ptrs), c_ranges(self.ranges), len(self.ptrs)) if self.ptrs else (None, None, 0)
        path = mq.MQ_SEMI_AUTO if rnd & 2 else mq.MQ_SEMI_GLOBAL
        mq.check(L.mq_semi_positions(cp, cr, k, self.key.ptr, ks, anti, path, None, self.n, o[0].ptr, o[1].ptr,
                                     self.ws.ptr, self.ws_bytes, s), "semi_positions")
        mq.check(L.mq_semi_agg(cp, cr, k, self.key.ptr, ks, anti, path, self.val.ptr, self.n, o[2].ptr,
                               self.ws.ptr, self.ws_bytes, s), "semi_agg")
        if self.ks is None:
            mq.check(L.mq_stream_sync(s), "sync")  # every probe of the handle has completed
            mq.check(L.mq_keyset_free(ks), "keyset_free")


GROUP_DT = [np.int32, np.uint64, np.int64, np.int32, np.int32]


class GroupJob(Job):
    """mq_group_plan without bounds (one mq_reduce on the stream), dense and sort by round."""
    name = "group"

    def __init__(self, L, n=N, keyset="uniform_100"):
        self.L, self.n = L, n
        keys = gc.keys_of(keyset, n, L.mq_group_dense_slots())
        vals = gc.values_of("uniform", keys)
        self.dk, self.dv = Dev.of(keys), Dev.of(vals)
        w = gc.group(keys, vals)
        self.g = len(w[0])
        self.outs = [Out(L, self.g, dt) for dt in GROUP_DT]
        self.want = [np.ascontiguousarray(a, dt).tobytes() for a, dt in zip(w, GROUP_DT)]

    def plan(self, s, rnd):
        h, groups, taken = C.c_void_p(), C.c_uint64(), C.c_int(-1)
        path = mq.MQ_GROUP_SORT if rnd & 1 else mq.MQ_GROUP_DENSE
        mq.check(self.L.mq_group_plan(self.dk.ptr, self.dv.ptr, self.n, None, path, C.byref(h), C.byref(groups),
                                      C.byref(taken), s), "group_plan")
        assert (groups.value, taken.value) == (self.g, path), (groups.value, taken.value)
        return h

    def write(self, h, s):
        mq.check(self.L.mq_group_write(h, *[o.ptr for o in self.outs], s), "group_write")

    def launch(self, s, rnd):
        h = self.plan(s, rnd)
        self.write(h, s)
        mq.check(self.L.mq_group_free(h), "group_free")


AGG_DT = [np.uint64, np.int64, np.int32, np.int32]


class GroupByWhereJob(Job):
    """mq_group_by_where_plan over two key columns without bounds + mq_group_by_write."""
    name = "group_by_where"

    def __init__(self, L, n=N):
        self.L, self.n = L, n
        self.cols, self.ranges = wc.case("uniform_50", n, 2)
        rng = np.random.default_rng(n + 77)
        keys = [np.ascontiguousarray(rng.integers(-5, 20, n), np.int32), np.ascontiguousarray(rng.integers(100, 140, n), np.int32)]
        vals = wc.values_of(n)
        self.keep = [Dev.of(a) for a in self.cols + keys + [vals]]
        self.pc, self.dks, self.dv = [d.ptr for d in self.keep[:2]], [d.ptr for d in self.keep[2:4]], self.keep[4].ptr
        w = gbw.model(self.cols, self.ranges, keys, vals)
        self.g = len(w[1])
        self.rows = int(w[1].sum())
        self.outs = [Out(L, self.g) for _ in keys] + [Out(L, self.g, dt) for dt in AGG_DT]
        self.want = [np.ascontiguousarray(k, np.int32).tobytes() for k in w[0]] + \
                    [np.ascontiguousarray(a, dt).tobytes() for a, dt in zip(w[1:], AGG_DT)]

    def launch(self, s, rnd):
        L = self.L
        h, groups, taken, rows = C.c_void_p(), C.c_uint64(), C.c_int(-1), C.c_uint64()
        path = mq.MQ_GROUP_SORT if rnd & 1 else mq.MQ_GROUP_AUTO
        mq.check(L.mq_group_by_where_plan(c_ptrs(self.pc), c_ranges(self.ranges), 2, c_ptrs(self.dks), 2, self.dv, self.n, None,
                                          path, C.byref(h), C.byref(groups), C.byref(taken), C.byref(rows), s), "group_by_where_plan")
        assert (groups.value, rows.value) == (self.g, self.rows), (groups.value, rows.value)
        mq.check(L.mq_group_by_write(h, c_ptrs([o.ptr for o in self.outs[:2]]), *[o.ptr for o in self.outs[2:]], s), "group_by_write")
        mq.check(L.mq_group_free(h), "group_free")


class MeasuresJob(Job):
    """mq_group_measures_plan (a plain and a key map term, Q1's four measures), dense and sort
    by round, + write. The terms' map is built here on the main thread."""
    name = "measures"

    def __init__(self, L, n=N, seed=0):
        self.L, self.n = L, n
        self.cols, self.ranges = wc.case("uniform_50", n, 1)
        self.terms = stc.make("plain_km", (16, 16), n, seed=seed)
        assert [t.kind for t in self.terms] == ["plain", "km"]
        ops = mc.columns(n, seed=seed)
        meas = mc.q1_measures(ops, 4)
        self.keep = {id(a): Dev.of(a) for a in self.cols + ops + [t.col for t in self.terms]}
        self.km = KeyMap(L, self.terms[1].dim_keys, self.terms[1].dim_attrs)
        self.star = (mq.MqStarTerm * 2)(mq.MqStarTerm(self.keep[id(self.terms[0].col)].ptr, None, None),
                                        mq.MqStarTerm(self.keep[id(self.terms[1].col)].ptr, self.km.h, None))
        self.pc = [self.keep[id(c)].ptr for c in self.cols]
        self.meas = (mq.MqMeasure * 4)()
        for i, q in enumerate(meas):
            self.meas[i] = mq.MqMeasure(self.keep[id(q.a)].ptr, self.keep[id(q.b)].ptr if q.b is not None else None, mc.OPS[q.op], 0)
        keys, count, aggs = mc.model(self.cols, self.ranges, self.terms, meas)
        self.g, self.rows = len(count), int(count.sum())
        self.outs = self.new_outs()
        self.want = [k.tobytes() for k in keys] + [count.tobytes()] + \
                    [np.ascontiguousarray(aggs[m][i], np.int64).tobytes() for i in range(3) for m in range(4)]

    def new_outs(self):
        L, g = self.L, self.g
        return [Out(L, g), Out(L, g), Out(L, g, np.uint64)] + [Out(L, g, np.int64) for _ in range(12)]

    def plan(self, s, path):
        L = self.L
        h, groups, taken, rows = C.c_void_p(), C.c_uint64(), C.c_int(-1), C.c_uint64()
        mq.check(L.mq_group_measures_plan(c_ptrs(self.pc), c_ranges(self.ranges), 1, self.star, 2, self.meas, 4, self.n, None,
                                          path, C.byref(h), C.byref(groups), C.byref(taken), C.byref(rows), s), "measures_plan")
        assert (groups.value, rows.value, taken.value) == (self.g, self.rows, path), (groups.value, rows.value, taken.value)
        return h

    def write(self, h, s, outs=None):
        o = outs or self.outs
        arr = lambda ds: c_ptrs([d.ptr for d in ds])  # noqa: E731
        mq.check(self.L.mq_group_measures_write(h, arr(o[0:2]), o[2].ptr, arr(o[3:7]), arr(o[7:11]), arr(o[11:15]), s), "measures_write")

    def launch(self, s, rnd):
        h = self.plan(s, mq.MQ_GROUP_SORT if rnd & 1 else mq.MQ_GROUP_DENSE)
        self.write(h, s)
        mq.check(self.L.mq_group_measures_free(h), "measures_free")

    def free(self):
        self.km.free()


class DistinctJob(Job):
    """mq_group_distinct_plan under two predicates, the lds and the sort path by round, + write."""
    name = "distinct"

    def __init__(self, L, n=N):
        self.L, self.n = L, n
        self.cols, self.ranges = dcs.predicates(n, 2)
        keys, vals = dcs.table(n, [5, 7], -3, 40, seed=n)
        self.keep = [Dev.of(a) for a in self.cols + keys + [vals]]
        self.pc, self.dks, self.dv = [d.ptr for d in self.keep[:2]], [d.ptr for d in self.keep[2:4]], self.keep[4].ptr
        wk, wcnt, self.rows, self.pairs = dcs.model(self.cols, self.ranges, keys, vals)
        self.g = len(wcnt)
        self.outs = [Out(L, self.g), Out(L, self.g), Out(L, self.g, np.uint64)]
        self.want = [k.tobytes() for k in wk] + [wcnt.tobytes()]

    def plan(self, s, rnd):
        L = self.L
        h, groups, info = C.c_void_p(), C.c_uint64(), mq.MqGdistinctInfo()
        path = mq.MQ_GDISTINCT_SORT if rnd & 1 else mq.MQ_GDISTINCT_LDS
        mq.check(L.mq_group_distinct_plan(c_ptrs(self.pc), c_ranges(self.ranges), 2, c_ptrs(self.dks), 2, self.dv, self.n, None, None,
                                          path, C.byref(h), C.byref(groups), C.byref(info), s), "distinct_plan")
        assert (groups.value, info.path, info.rows, info.pairs) == (self.g, path, self.rows, self.pairs), (groups.value, info.path)
        return h

    def write(self, h, s):
        mq.check(self.L.mq_group_distinct_write(h, c_ptrs([o.ptr for o in self.outs[:2]]), self.outs[2].ptr, s), "distinct_write")

    def launch(self, s, rnd):
        h = self.plan(s, rnd)
        self.write(h, s)
        mq.check(self.L.mq_group_distinct_free(h), "distinct_free")


class TopkJob(Job):
    """mq_topk on its select path (a candidate cap below n), then mq_topk64 on its select path
    with a cap of 1 over 55 shared bits (six histogram levels, each a sync and a host read-back)
    and on its sort path (two mq_index_build runs inside)."""
    name = "topk"
    K, K64 = 1000, 100

    def __init__(self, L, n=N):
        self.L, self.n = L, n
        vals, pay = tk.values_of("full_range", n), tk.payload_of(n)
        v64 = t64.values_of("shared_55", n)
        self.dv, self.dp, self.d64 = Dev.of(vals), Dev.of(pay), Dev.of(v64)
        self.outs = [Out(L, self.K), Out(L, self.K), Out(L, self.K64, np.int64), Out(L, self.K64, np.uint32),
                     Out(L, self.K64, np.int64), Out(L, self.K64, np.uint32)]
        self.wants = []
        for desc in (False, True):
            wv, wp = tk.topk(vals, pay, self.K, desc)
            idx = t64.topk64(v64, None, (None, None), self.K64, desc)
            w64 = [v64[idx].tobytes(), idx.astype(np.uint32).tobytes()]
            self.wants.append([wv.tobytes(), wp.tobytes()] + w64 + w64)
        self.want = self.wants[0]

    def want_of(self, rnd):
        return self.wants[rnd & 1]

    def launch(self, s, rnd):
        L, o, desc = self.L, self.outs, rnd & 1
        info = mq.MqTopkInfo()
        mq.check(L.mq_topk(self.dv.ptr, self.dp.ptr, self.n, self.K, desc, mq.MQ_TOPK_SELECT, 64, o[0].ptr, o[1].ptr,
                           C.byref(info), s), "topk")
        assert (info.m, info.path) == (self.K, mq.MQ_TOPK_SELECT), (info.m, info.path)
        i64 = mq.MqTopk64Info()
        mq.check(L.mq_topk64(self.d64.ptr, None, None, self.n, self.K64, desc, mq.MQ_TOPK_SELECT, 1, o[2].ptr, o[3].ptr,
                             C.byref(i64), s), "topk64 select")
        assert (i64.m, i64.path, i64.levels) == (self.K64, mq.MQ_TOPK_SELECT, 6), (i64.m, i64.path, i64.levels)
        mq.check(L.mq_topk64(self.d64.ptr, None, None, self.n, self.K64, desc, mq.MQ_TOPK_SORT, 0, o[4].ptr, o[5].ptr,
                             C.byref(i64), s), "topk64 sort")
        assert (i64.m, i64.path) == (self.K64, mq.MQ_TOPK_SORT), (i64.m, i64.path)


class JoinJob(Job):
    """mq_join_build -> probe -> counts -> write -> free on joincases' many-to-many "dups"."""
    name = "join"

    def __init__(self, L, case="dups"):
        self.L = L
        c1, p1, c2, p2 = jc.named_inputs(case)
        self.n1, self.n2 = len(c1), len(c2)
        self.d = [Dev.of(a) for a in (c1, p1, c2, p2)]
        w1, w2 = jc.join_pairs(c1, p1, c2, p2)
        self.m = len(w1)
        self.outs = [Out(L, self.n2, np.uint32), Out(L, self.m), Out(L, self.m)]
        self.want = [jc.join_counts(c1, c2).tobytes(), w1.tobytes(), w2.tobytes()]

    def build(self, s):
        h = C.c_void_p()
        mq.check(self.L.mq_join_build(self.d[0].ptr, self.d[1].ptr, self.n1, C.byref(h), s), "join_build")
        return h

    def probe_write(self, h, s):
        L, o, m = self.L, self.outs, C.c_uint64()
        mq.check(L.mq_join_probe(h, self.d[2].ptr, self.n2, C.byref(m), s), "join_probe")
        assert m.value == self.m, m.value
        mq.check(L.mq_join_counts(h, o[0].ptr, s), "join_counts")
        mq.check(L.mq_join_write(h, self.d[3].ptr, o[1].ptr, o[2].ptr, s), "join_write")

    def launch(self, s, rnd):
        h = self.build(s)
        self.probe_write(h, s)
        mq.check(self.L.mq_stream_sync(s), "sync")
        mq.check(self.L.mq_join_free(h), "join_free")


FAMILIES = [WhereJob, SemiJob, GroupJob, GroupByWhereJob, MeasuresJob, DistinctJob, TopkJob, JoinJob]


def want_of(job, rnd):
    return job.want_of(rnd) if hasattr(job, "want_of") else job.want


def new_stream(L):
    s = C.c_void_p()
    mq.check(L.mq_stream_create(C.byref(s)), "mq_stream_create")
    return s


def serial_pass(L, jobs, rounds=(0, 1)):
    """Every job once per round of `rounds` on the main thread, on a stream of its own: the
    outputs (kept, per job and round) must equal the model, or the bug is a single-thread one.
    Returns (outputs, seconds)."""
    s = new_stream(L)
    t0 = time.perf_counter()
    try:
        got = {}
        for j, job in enumerate(jobs):
            for r in rounds:
                got[j, r] = job.run(s, r)
                assert got[j, r] == want_of(job, r), ("single-thread result differs from the model", job.name, r)
    finally:
        mq.check(L.mq_stream_destroy(s), "mq_stream_destroy")
    return got, time.perf_counter() - t0


GRACE = 5.0           # after the deadline, for workers that left a timed-out barrier to exit


class Ctx:
    def __init__(self, i, crew):
        self.i, self.crew, self.stream = i, crew, None

    def barrier(self):
        """Waits until the crew's deadline at the latest, not a full deadline from now."""
        self.crew.bar.wait(max(0.05, self.crew.end - time.monotonic()))


class Crew:
    """n daemon threads, a stream each (`streams[i]`: "new", None for the NULL stream, or
    PER_THREAD), started together by a barrier. A worker records its own exception, marks the
    crew failed and breaks the barrier so the others stop; `run` re-raises on the main thread.
    Every barrier wait ends at the crew's deadline. A barrier that breaks with no failure
    recorded has timed out: some worker is stuck inside libmq, HUNG is set, and the workers that
    leave make no further libmq call (no mq_stream_destroy, no mq_thread_release: both may
    synchronise or free on the device). `run` joins until the deadline and GRACE seconds more;
    a worker alive then, or a timed-out barrier, fails the test with HUNG set."""

    def __init__(self, L, n, deadline, streams=None):
        self.L, self.n, self.deadline = L, n, deadline
        self.streams = streams or ["new"] * n
        self.bar = threading.Barrier(n)
        self.errors = [None] * n
        self.failed = False
        self.end = time.monotonic() + deadline

    def _worker(self, i, body):
        L, ctx, made = self.L, Ctx(i, self), None
        try:
            if self.streams[i] == "new":
                made = new_stream(L)
                ctx.stream = made
            else:
                ctx.stream = self.streams[i]
            ctx.barrier()
            body(ctx)
        except threading.BrokenBarrierError as e:
            self.errors[i] = e
            if not self.failed:  # nobody failed: a wait ran into the deadline
                HUNG.append(("barrier timed out", i))
        except BaseException as e:  # noqa: BLE001 (re-raised on the main thread)
            self.errors[i] = e
            self.failed = True
            self.bar.abort()
        if HUNG:
            return  # nothing more on the GPU, this thread's epilogue included
        if made is not None:
            L.mq_stream_destroy(made)
        L.mq_thread_release()  # a worker's last libmq call

    def run(self, bodies):
        import pytest
        assert not HUNG
        threads = [threading.Thread(target=self._worker, args=(i, b), daemon=True) for i, b in enumerate(bodies)]
        self.end = time.monotonic() + self.deadline
        for t in threads:
            t.start()
        for t in threads:
            t.join(max(0.0, self.end + GRACE - time.monotonic()))
        stuck = [i for i, t in enumerate(threads) if t.is_alive()]
        if stuck:
            HUNG.append(("stuck", stuck))
        if HUNG:
            pytest.fail(f"deadline of {self.deadline:.0f} s missed (still inside libmq: workers {stuck}): nothing more is started on the GPU")
        real = [e for e in self.errors if e is not None and not isinstance(e, threading.BrokenBarrierError)]
        if real:
            raise real[0]
        broken = [e for e in self.errors if e is not None]
        if broken:
            raise broken[0]
