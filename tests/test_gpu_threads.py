"""The device API from concurrent host threads, one stream each (-m gpu).

include/mq_device.h promises per-thread state (the last error, the delete and insert plans,
shared_select's count state, the staging), shared state behind locks (the pool, the arrival
counters, the occupancy cache) and handles that may be probed or written from any stream. The
row shards depend on all of it; here several threads are inside libmq at once:

  1. first use of the library from eight threads at the same moment (a fresh process);
  2. the folded one-launch forms (arrival counters) on created, NULL and per-thread streams;
  3. eight operator families at once, fixed and then rotating over the workers;
  4. per-thread plans and errors do not cross (barrier-stepped, deterministic);
  5. one key set and two key maps (a dense dimension, a span past 2^31) probed by eight threads;
  6. one measures handle written from eight threads;
  7. handles planned by one thread, written and freed by another;
  8. staged downloads from four threads.

Expected values come from the suite's models (threadcases.py builds them on the main thread
before any worker starts); every comparison is exact; the main thread's serial pass over the
same jobs is a second comparison. A worker that misses its deadline fails its test and makes
every later test of this module skip: nothing more is started on the GPU after a hang.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import dmlcases as dc
import groupjoincases as gj
import insertcases as ic
import starcases as stc
import threadcases as tc
import wherecases as wc
from devbuf import Dev
from refapi import mq
from threadcases import FILL, N, ROUNDS, WORKERS, Crew, Out, c_ptrs, new_stream, padded, want_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    return L


@pytest.fixture(autouse=True)
def not_after_a_hang():
    if tc.HUNG:
        pytest.skip("a worker of an earlier test is stuck inside libmq: nothing more is started on the GPU")


@pytest.fixture
def cu_limit(lib):
    """limit(cus) before the workers start; reset after they have joined and the device is idle
    (the hook's contract: no other thread is inside libmq). After a hang only the host-side
    reset is made."""
    def limit(cus):
        if cus:
            mq.check(lib.mq_test_set_cu_limit(cus), "mq_test_set_cu_limit")
    try:
        yield limit
    finally:
        if not tc.HUNG:
            mq.check(lib.mq_device_sync(), "mq_device_sync")
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def report(what, serial):
    print(f"[threads] {what}: serial pass {serial:.3f} s, join deadline {tc.deadline_for(ROUNDS * serial):.0f} s")


# ---------------------------------------------------------------------------
# 1. first use from many threads at once
# ---------------------------------------------------------------------------
def test_first_use_from_many_threads(lib):
    """A child process (this one initialised libmq long ago): eight threads make mq_stream_create
    their first libmq call at one barrier and run mq_select_agg on the new stream, racing the
    device's first-use initialisation, the occupancy cache's first fill and eight creations of
    arrival counters. The child compares with numpy and exits 0 only if all eight match."""
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "threads_first_use.py")], capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        tc.HUNG.append("first-use child")
        pytest.fail("the first-use child did not finish in 180 s: nothing more is started on the GPU")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    rep = json.loads(lines[-1])
    if rep["stuck"]:
        tc.HUNG.append("first-use child")
    assert p.returncode == 0 and rep == {"ok": True, "threads": 8, "wrong": [], "stuck": [], "errors": []}, (p.returncode, rep, p.stderr[-2000:])


# ---------------------------------------------------------------------------
# 2. the arrival-counter family on every kind of stream
# ---------------------------------------------------------------------------
class FoldedJob(tc.Job):
    """The entry points that fold their partials inside one launch (block_arrive_last on the
    stream's arrival counters): mq_select_agg, mq_reduce (an unbounded mq_select_agg),
    mq_select_fetch_agg and mq_select_sum, each on this job's column and range. (mq_topk and
    mq_topk64 take no arrival counters: their histograms are folded by atomics.)"""
    name = "folded"

    def __init__(self, L, i, n=N):
        self.L, self.n = L, n
        rng = np.random.default_rng(500 + i)
        sel = rng.integers(-1000, 1000, n).astype(np.int32)
        val = wc.values_of(n + i)[:n]
        self.lo, self.hi = -700 + 37 * i, 100 + 41 * i
        self.ds, self.dval = Dev.of(sel), Dev.of(val)
        self.ws_bytes = L.mq_scan_workspace_bytes(n)
        self.ws = Dev(self.ws_bytes)
        self.outs = [tc.AggOut(L) for _ in range(4)]
        r = [(self.lo, self.hi)]
        a = wc.aggregate([sel], r, sel)
        self.want = [tc.agg_bytes(a), tc.agg_bytes(wc.aggregate([sel], [(None, None)], sel)),
                     tc.agg_bytes(wc.aggregate([sel], r, val)), tc.agg_bytes((a[0], a[1], wc.I32_MAX, wc.I32_MIN))]

    def launch(self, s, rnd):
        L, o, n, ws, wb = self.L, self.outs, self.n, self.ws.ptr, self.ws_bytes
        mq.check(L.mq_select_agg(self.ds.ptr, n, 1, self.lo, 1, self.hi, o[0].ptr, ws, wb, s), "mq_select_agg")
        mq.check(L.mq_reduce(self.ds.ptr, n, o[1].ptr, ws, wb, s), "mq_reduce")
        mq.check(L.mq_select_fetch_agg(self.ds.ptr, self.dval.ptr, n, 1, self.lo, 1, self.hi, o[2].ptr, ws, wb, s), "mq_select_fetch_agg")
        mq.check(L.mq_select_sum(self.ds.ptr, n, 1, self.lo, 1, self.hi, o[3].ptr, ws, wb, s), "mq_select_sum")


def looping(job, serial, rounds=ROUNDS):
    def body(ctx):
        for r in range(rounds):
            ctx.barrier()
            got = job.run(ctx.stream, r)
            assert got == want_of(job, r), (job.name, ctx.i, r, "differs from the model")
            assert got == serial[r & 1], (job.name, ctx.i, r, "differs from the serial pass")
    return body


@pytest.mark.parametrize("cus", [0, 2])
def test_folded_forms_on_every_kind_of_stream(lib, cu_limit, cus):
    """Twelve workers, each looping count / sum / min / max of its own column and range through
    the four folded forms: eight on created streams, two on the NULL stream (one counter block,
    launches in order) and two on the per-thread default stream, the one case where the counter
    table is keyed by thread. Exact every round. The per-thread workers end with
    mq_thread_release, which drops their entries; two new threads then do the same work on that
    handle and find fresh ones. Under a CU limit of 2 the same launches have
    the grid of two CUs: more rows a block, another number of arrivals and of partials to fold."""
    cu_limit(cus)
    jobs = [FoldedJob(lib, i) for i in range(12)]
    got, secs = tc.serial_pass(lib, jobs)
    report(f"folded forms (cu limit {cus})", secs)
    streams = ["new"] * 8 + [None, None, tc.PER_THREAD, tc.PER_THREAD]
    bodies = [looping(j, [got[i, 0], got[i, 1]]) for i, j in enumerate(jobs)]
    Crew(lib, 12, tc.deadline_for(ROUNDS * secs), streams).run(bodies)
    Crew(lib, 2, tc.deadline_for(ROUNDS * secs), [tc.PER_THREAD] * 2).run(bodies[10:])


# ---------------------------------------------------------------------------
# 3. all operator families at once
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [0, 2])
def test_all_families_at_once(lib, cu_limit, cus):
    """Eight workers, eight families (where, semi with a key set built every round, group dense /
    sort, group_by_where, measures dense / sort, distinct lds / sort, top_k + top_k64 select and
    sort, the many-to-many join). Ten rounds with worker i on family i, then ten with worker i on
    family (i + round) mod 8, so that every thread touches every family's per-thread state and
    every stream's scratch moves through the pool. After its last round a worker takes a block of a
    size of its own from the pool and frees it in its stream's order; once the workers have gone
    (their streams destroyed) the pool hands exactly those eight blocks out again and allocates
    nothing."""
    cu_limit(cus)
    jobs = [F(lib) for F in tc.FAMILIES]
    try:
        got, secs = tc.serial_pass(lib, jobs)
        report(f"all families (cu limit {cus})", secs)
        blocks = [None] * WORKERS

        def body(ctx):
            for r in range(ROUNDS):
                ctx.barrier()
                j = ctx.i if r < ROUNDS // 2 else (ctx.i + r) % WORKERS
                out = jobs[j].run(ctx.stream, r)
                assert out == want_of(jobs[j], r), (jobs[j].name, ctx.i, r, "differs from the model")
                assert out == got[j, r & 1], (jobs[j].name, ctx.i, r, "differs from the serial pass")
            p = C.c_void_p()
            mq.check(lib.mq_pool_malloc(C.byref(p), block_bytes(ctx.i)), "mq_pool_malloc")
            blocks[ctx.i] = p.value
            ctx.barrier()  # every worker holds its block before the first is freed: eight different blocks
            mq.check(lib.mq_memset(p, ctx.i, block_bytes(ctx.i), ctx.stream), "mq_memset")
            mq.check(lib.mq_pool_free_on(p, ctx.stream), "mq_pool_free_on")

        Crew(lib, WORKERS, tc.deadline_for(ROUNDS * secs)).run([body] * WORKERS)
        mq.check(lib.mq_device_sync(), "mq_device_sync")
        again = []
        try:
            for i in range(WORKERS):
                p = C.c_void_p()
                mq.check(lib.mq_pool_malloc(C.byref(p), block_bytes(i)), "mq_pool_malloc")
                again.append(p.value)
            assert len(set(blocks)) == WORKERS and sorted(again) == sorted(blocks), \
                "the pool allocated anew instead of handing out the workers' blocks"
        finally:
            for b in again:
                mq.check(lib.mq_pool_free(b), "mq_pool_free")
    finally:
        if not tc.HUNG:
            for j in jobs:
                j.free()


def block_bytes(i):
    """Larger than twice any scratch these jobs take: the pool hands out a block of at most twice
    the size asked for, so no block of the library's own fits such a request and a worker's block
    fits no request of the library's."""
    return (64 << 20) + (1 << 20) * i


# ---------------------------------------------------------------------------
# 4. per-thread plans do not cross
# ---------------------------------------------------------------------------
def stepped(lib, steps_a, steps_b, extra=()):
    """Two (or more) workers walk lists of equal length, one barrier before every step; a None
    step only waits. The barriers fix the order of the calls: the test is deterministic."""
    lists = [steps_a, steps_b] + list(extra)
    assert len({len(s) for s in lists}) == 1

    def body_of(steps):
        def body(ctx):
            for step in steps:
                ctx.barrier()
                if step:
                    step(ctx)
        return body
    Crew(lib, len(lists), tc.DEADLINE_FLOOR * 2).run([body_of(s) for s in lists])


class DeleteSide:
    """One thread's table, index, position set, workspace and outputs of a delete."""

    def __init__(self, L, n, set_name, seed):
        self.L, self.n = L, n
        cols = dc.table(n, 2, seed=seed)
        ids = dc.delete_sets(n)[set_name]
        self.pos = dc.position_list(ids, "shuffled", seed=seed)
        key = (np.random.default_rng(seed).permutation(n) % 7).astype(np.int32)
        iv, ip = dc.index_of(key)
        self.left, self.deleted = n - len(ids), len(ids)
        self.dcols, self.dpos, self.div, self.dip = [Dev.of(c) for c in cols], Dev.of(self.pos), Dev.of(iv), Dev.of(ip)
        self.ws = Dev(L.mq_delete_workspace_bytes(n))
        self.outs = [Out(L, self.left), Out(L, self.left), Out(L, self.left), Out(L, self.left, np.uint64)]
        wv, wp = dc.delete_index(iv, ip, ids, n)
        self.want = [c.tobytes() for c in dc.delete_rows(cols, ids)] + [wv.tobytes(), wp.tobytes()]

    def plan(self, ctx):
        deleted, bad = C.c_uint64(~0), C.c_uint64(~0)
        mq.check(self.L.mq_delete_plan(self.dpos.ptr, len(self.pos), self.n, C.byref(deleted), C.byref(bad), self.ws.ptr,
                                       self.ws.nbytes, ctx.stream), "mq_delete_plan")
        assert (deleted.value, bad.value) == (self.deleted, 0)
        for o in self.outs:
            o.arm(ctx.stream)

    def apply(self, ctx):
        L, o, s = self.L, self.outs, ctx.stream
        mq.check(L.mq_delete_columns(self.ws.ptr, c_ptrs([d.ptr for d in self.dcols]), 2, c_ptrs([o[0].ptr, o[1].ptr]), s), "mq_delete_columns")
        mq.check(L.mq_delete_index(self.ws.ptr, self.div.ptr, self.dip.ptr, o[2].ptr, o[3].ptr, s), "mq_delete_index")

    def check(self, ctx):
        assert [o.read(ctx.stream) for o in self.outs] == self.want, "the delete ran on another thread's plan"


def test_delete_plans_do_not_cross(lib):
    """A plans, B plans, A applies to its columns and index, B applies: each result is dmlcases'
    for its own position set, table and workspace, twenty times over."""
    a, b = DeleteSide(lib, N, "random_50pct", 1), DeleteSide(lib, 3 * 8192 + 17, "every_second", 2)
    rnd_a = [a.plan, None, a.apply, None, a.check]
    rnd_b = [None, b.plan, None, b.apply, b.check]
    stepped(lib, rnd_a * ROUNDS, rnd_b * ROUNDS)


class UpdateSide:
    def __init__(self, L, n, seed, value):
        self.L, self.n, self.value = L, n, value
        self.col = dc.table(n, 1, seed=seed)[0]
        ids = np.random.default_rng(seed).integers(0, n, n // 3).astype(np.int32)
        self.k = len(ids)
        self.dcol, self.dpos = Out(L, n), Dev.of(ids)
        self.want = dc.update_rows(self.col, ids, value).tobytes()

    def load(self, ctx):
        self.dcol.arm(ctx.stream)
        mq.check(self.L.mq_memcpy_h2d(self.dcol.ptr, self.col.ctypes.data, 4 * self.n, ctx.stream), "h2d")

    def apply(self, ctx):
        mq.check(self.L.mq_update_rows(self.dcol.ptr, self.n, self.dpos.ptr, self.k, self.value, None, ctx.stream), "mq_update_rows")

    def check(self, ctx):
        assert self.dcol.read(ctx.stream) == self.want


def test_updates_do_not_cross(lib):
    """The same steps through mq_update_rows, which keeps no plan: each column is dmlcases' for
    its own position list and value."""
    a, b = UpdateSide(lib, N, 3, -77), UpdateSide(lib, 3 * 8192 + 17, 4, 2**31 - 1)
    rnd_a = [a.load, None, a.apply, None, a.check]
    rnd_b = [None, b.load, None, b.apply, b.check]
    stepped(lib, rnd_a * ROUNDS, rnd_b * ROUNDS)


class InsertSide:
    """One thread's old table and index, batch, points, workspace and outputs of an insert."""

    def __init__(self, L, n, set_name, seed):
        self.L, self.n = L, n
        cols = dc.table(n, 2, seed=seed)
        self.points = ic.insertion_points(n)[set_name]
        k = self.k = len(self.points)
        new = dc.table(k, 2, seed=seed + 10)
        m = n + k
        rng = np.random.default_rng(seed)
        iv = np.sort(rng.integers(-1000, 1000, n)).astype(np.int32)
        ip = rng.permutation(n).astype(np.uint64)
        nv = np.sort(rng.integers(-1000, 1000, k)).astype(np.int32)
        np_ = (n + rng.permutation(k)).astype(np.uint64)
        ipoints = np.searchsorted(iv, nv, side="right").astype(np.uint32)  # mq_insert_points' rule
        self.dold, self.dnew = [Dev.of(c) for c in cols], [Dev.of(c) for c in new]
        self.dpts, self.dipts = Dev.of(self.points), Dev.of(ipoints)
        self.div, self.dip, self.dnv, self.dnp = Dev.of(iv), Dev.of(ip), Dev.of(nv), Dev.of(np_)
        self.ws, self.iws = Dev(L.mq_insert_workspace_bytes(n, k)), Dev(L.mq_insert_workspace_bytes(n, k))
        self.outs = [Out(L, m), Out(L, m), Out(L, m), Out(L, m, np.uint64)]
        wv, wp = ic.insert_index(iv, ip, nv, np_)
        self.want = [ic.expand(cols[j], self.points, new[j]).tobytes() for j in range(2)] + [wv.tobytes(), wp.tobytes()]

    def _plan(self, d, ws, s):
        bad = C.c_uint64(~0)
        mq.check(self.L.mq_insert_plan(d.ptr, self.k, self.n, C.byref(bad), ws.ptr, ws.nbytes, s), "mq_insert_plan")
        assert bad.value == 0

    def plan(self, ctx):
        self._plan(self.dpts, self.ws, ctx.stream)
        for o in self.outs:
            o.arm(ctx.stream)

    def apply(self, ctx):
        L, o, s = self.L, self.outs, ctx.stream
        mq.check(L.mq_insert_columns(self.ws.ptr, c_ptrs([d.ptr for d in self.dold]), c_ptrs([d.ptr for d in self.dnew]), 2,
                                     c_ptrs([o[0].ptr, o[1].ptr]), s), "mq_insert_columns")

    def plan_index(self, ctx):
        self._plan(self.dipts, self.iws, ctx.stream)

    def apply_index(self, ctx):
        o = self.outs
        mq.check(self.L.mq_insert_index(self.iws.ptr, self.div.ptr, self.dip.ptr, self.dnv.ptr, self.dnp.ptr, None, 0,
                                        o[2].ptr, o[3].ptr, ctx.stream), "mq_insert_index")

    def check(self, ctx):
        assert [o.read(ctx.stream) for o in self.outs] == self.want, "the insert ran on another thread's plan"


def test_insert_plans_do_not_cross(lib):
    """A plans, B plans, A expands its columns, B expands; then the same around the index's own
    plan and mq_insert_index: each result is insertcases' for its own points."""
    a, b = InsertSide(lib, N, "random_50pct", 5), InsertSide(lib, 3 * 8192 + 17, "random_1pct", 6)
    rnd_a = [a.plan, None, a.apply, None, a.plan_index, None, a.apply_index, None, a.check]
    rnd_b = [None, b.plan, None, b.apply, None, b.plan_index, None, b.apply_index, b.check]
    stepped(lib, rnd_a * ROUNDS, rnd_b * ROUNDS)


class SharedSide:
    """One thread's column, q ranges, workspace and outputs of the two-step shared select."""

    def __init__(self, L, refcpu, n, q, seed):
        self.L, self.n, self.q = L, n, q
        rng = np.random.default_rng(seed)
        d = rng.integers(0, 10 ** 6, n).astype(np.int32)
        lows = rng.integers(0, 500_000, q).astype(np.int32)
        highs = (lows + rng.integers(100_000, 500_000, q)).astype(np.int32)
        self.lo, self.hi = c_i32s(lows), c_i32s(highs)
        lists = refcpu.shared_select(d, lows, highs)
        self.counts = [len(w) for w in lists]
        self.dcol = Dev.of(d)
        self.ws = Dev(L.mq_shared_select_workspace_bytes(n, q))
        self.outs = [Out(L, k) for k in self.counts]
        self.want = [np.ascontiguousarray(w, np.int32).tobytes() for w in lists]

    def count(self, ctx):
        k = (C.c_uint64 * self.q)()
        mq.check(self.L.mq_shared_select_count(self.dcol.ptr, self.n, self.lo, self.hi, self.q, k, self.ws.ptr, self.ws.nbytes,
                                               ctx.stream), "mq_shared_select_count")
        assert [int(x) for x in k] == self.counts
        for o in self.outs:
            o.arm(ctx.stream)

    def write(self, ctx):
        mq.check(self.L.mq_shared_select_write(self.ws.ptr, c_ptrs([o.ptr for o in self.outs]), ctx.stream), "mq_shared_select_write")

    def check(self, ctx):
        assert [o.read(ctx.stream) for o in self.outs] == self.want, "the write ran on another thread's count"


def c_i32s(a):
    return (C.c_int32 * len(a))(*[int(x) for x in a])


def test_shared_select_states_do_not_cross(lib, refcpu):
    """A counts with Q = 3, B counts with Q = 7, A writes, B writes: each thread's write runs on
    the workspace of its own count; the positions are refcpu.shared_select's."""
    a, b = SharedSide(lib, refcpu, N, 3, 7), SharedSide(lib, refcpu, 50_021, 7, 8)
    rnd_a = [a.count, None, a.write, None, a.check]
    rnd_b = [None, b.count, None, b.write, b.check]
    stepped(lib, rnd_a * ROUNDS, rnd_b * ROUNDS)


def test_last_errors_do_not_cross(lib):
    """A and B each make one call that its argument checks refuse (a misaligned workspace; a path
    that is none of the three: nothing reaches a kernel), then, after a barrier, each finds its
    own message in mq_last_error(). A third thread that has never failed reads the empty string."""
    ws, col = Dev(lib.mq_where_workspace_bytes(1024) + 16), Dev(4096)
    cnt, out = Dev(16), Dev(4096)
    seen = {}

    def a_fails(ctx):
        rc = lib.mq_where_positions(c_ptrs([col.ptr]), tc.c_ranges([(0, 5)]), 1, None, 1024, out.ptr, cnt.ptr, ws.ptr + 4,
                                    ws.nbytes - 16, ctx.stream)
        assert rc == mq.MQ_EINVAL

    def b_fails(ctx):
        h, g = C.c_void_p(), C.c_uint64()
        rc = lib.mq_group_plan(col.ptr, col.ptr, 1024, None, 9, C.byref(h), C.byref(g), None, ctx.stream)
        assert rc == mq.MQ_EINVAL

    def read(ctx):
        seen[ctx.i] = lib.mq_last_error()

    stepped(lib, [a_fails, None, read], [None, b_fails, read], extra=[[None, None, read]])
    assert seen[0] == b"mq_where_positions: workspace NULL, short or not 16-byte aligned", seen
    assert seen[1] == b"mq_group_plan: path 9", seen
    assert seen[2] == b"", seen


def test_an_apply_step_needs_a_plan_of_its_own_thread(lib, refcpu):
    """A makes a delete plan, an insert plan and a shared-select count; C, which has made none,
    then calls every apply step on A's workspaces with valid arguments of its own: each is
    refused with MQ_EINVAL and the message the code defines, and C's outputs stay untouched.
    A's own apply steps still work afterwards."""
    d, ins, sh = DeleteSide(lib, 8193, "random_50pct", 11), InsertSide(lib, 8193, "random_50pct", 12), SharedSide(lib, refcpu, 8193, 7, 13)
    spare = [Out(lib, N + 8193, np.uint64) for _ in range(7)]

    def a_plans(ctx):
        d.plan(ctx)
        ins.plan(ctx)
        sh.count(ctx)

    def c_applies(ctx):
        L, s = lib, ctx.stream
        for o in spare:
            o.arm(s)
        two = c_ptrs([spare[0].ptr, spare[1].ptr])
        calls = [
            (lambda: L.mq_delete_columns(d.ws.ptr, c_ptrs([x.ptr for x in d.dcols]), 2, two, s),
             b"mq_delete_columns: no plan of this thread on this workspace"),
            (lambda: L.mq_delete_index(d.ws.ptr, d.div.ptr, d.dip.ptr, spare[0].ptr, spare[1].ptr, s),
             b"mq_delete_index: no plan of this thread on this workspace"),
            (lambda: L.mq_insert_columns(ins.ws.ptr, c_ptrs([x.ptr for x in ins.dold]), c_ptrs([x.ptr for x in ins.dnew]), 2, two, s),
             b"mq_insert_columns: no plan of this thread on this workspace"),
            (lambda: L.mq_insert_index(ins.ws.ptr, ins.div.ptr, ins.dip.ptr, ins.dnv.ptr, ins.dnp.ptr, None, 0, spare[0].ptr,
                                       spare[1].ptr, s),
             b"mq_insert_index: no plan of this thread on this workspace"),
            (lambda: L.mq_shared_select_write(sh.ws.ptr, c_ptrs([o.ptr for o in spare]), s),
             b"mq_shared_select_write: no matching mq_shared_select_count"),
        ]
        for call, message in calls:
            rc = call()
            assert (rc, L.mq_last_error()) == (mq.MQ_EINVAL, message), (rc, L.mq_last_error(), message)
        for o in spare:
            assert o.read(s) == bytes([FILL]) * o.bytes, "a refused apply step wrote its outputs"

    def a_applies(ctx):
        d.apply(ctx)
        ins.apply(ctx)
        ins.plan_index(ctx)
        ins.apply_index(ctx)
        sh.write(ctx)
        d.check(ctx)
        ins.check(ctx)
        sh.check(ctx)

    stepped(lib, [a_plans, None, a_applies], [None, c_applies, None])


# ---------------------------------------------------------------------------
# 5. one immutable handle, many probing threads
# ---------------------------------------------------------------------------
class ProbeJob(tc.Job):
    """On shared handles (a key map, its key set): mq_keymap_lookup, mq_group_join_plan + write
    and mq_group_star_plan with the map as one term beside a plain one + write, on this job's
    own fact columns."""
    name = "probe"

    def __init__(self, L, km, fact_name, n, seed):
        self.L, self.n, self.km = L, n, km.h
        fkey = gj.fact_keys(fact_name, n, km.keys)
        vals = wc.values_of(n + seed)[:n]
        plain = np.ascontiguousarray(np.random.default_rng(seed).integers(0, 5, n) + 100, np.int32)
        self.dfk, self.dv, self.dpl = Dev.of(fkey), Dev.of(vals), Dev.of(plain)
        attr, hit = gj.lookup(fkey, km.keys, km.attrs, missing=-9)
        wj = gj.model([], [], fkey, km.keys, km.attrs, vals)
        terms = [stc.Term("plain", plain), stc.Term("km", fkey, km.keys, km.attrs)]
        ws = stc.model([], [], terms, vals)
        self.gj_, self.gs = len(wj[0]), len(ws[1])
        self.terms = (mq.MqStarTerm * 2)(mq.MqStarTerm(self.dpl.ptr, None, None), mq.MqStarTerm(self.dfk.ptr, km.h, None))
        self.outs = [Out(L, n), Out(L, n, np.uint8)] + [Out(L, self.gj_, dt) for dt in tc.GROUP_DT] + \
                    [Out(L, self.gs), Out(L, self.gs)] + [Out(L, self.gs, dt) for dt in tc.AGG_DT]
        self.want = [attr.tobytes(), hit.tobytes()] + [np.ascontiguousarray(a, dt).tobytes() for a, dt in zip(wj, tc.GROUP_DT)] + \
                    [np.ascontiguousarray(k, np.int32).tobytes() for k in ws[0]] + \
                    [np.ascontiguousarray(a, dt).tobytes() for a, dt in zip(ws[1:], tc.AGG_DT)]

    def launch(self, s, rnd):
        L, o, n = self.L, self.outs, self.n
        mq.check(L.mq_keymap_lookup(self.km, self.dfk.ptr, None, n, -9, o[0].ptr, o[1].ptr, s), "mq_keymap_lookup")
        h, g, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        path = mq.MQ_GROUP_SORT if rnd & 1 else mq.MQ_GROUP_AUTO
        mq.check(L.mq_group_join_plan(None, None, 0, self.dfk.ptr, self.km, self.dv.ptr, n, None, path, C.byref(h), C.byref(g), None,
                                      C.byref(rows), s), "mq_group_join_plan")
        assert g.value == self.gj_, g.value
        if h:
            mq.check(L.mq_group_write(h, *[x.ptr for x in o[2:7]], s), "mq_group_write")
            mq.check(L.mq_group_free(h), "mq_group_free")
        h = C.c_void_p()
        mq.check(L.mq_group_star_plan(None, None, 0, self.terms, 2, self.dv.ptr, n, None, path, C.byref(h), C.byref(g), None,
                                      C.byref(rows), s), "mq_group_star_plan")
        assert g.value == self.gs, g.value
        if h:
            mq.check(L.mq_group_by_write(h, c_ptrs([o[7].ptr, o[8].ptr]), *[x.ptr for x in o[9:13]], s), "mq_group_by_write")
            mq.check(L.mq_group_free(h), "mq_group_free")


def both(a, b):
    """One worker's two jobs as one."""
    class Pair(tc.Job):
        name = a.name + "+" + b.name

        def run(self, s, rnd=0):
            return a.run(s, rnd) + b.run(s, rnd)

        def want_of(self, rnd):
            return want_of(a, rnd) + want_of(b, rnd)
    return Pair()


def test_one_key_set_and_two_key_maps_probed_by_many_threads(lib):
    """The main thread builds a dense dimension of 2048 keys and a sparse one over a span past
    2^31 as key maps (four workers each), and one key set. Eight workers, each with its own stream, fact columns and
    workspace, run semi / anti positions and aggregate (on the map's own key set and on the
    separate set), the lookup, the group-join plan and the star plan on them at once, exact
    against semicases, groupjoincases and starcases. The handles are freed on the main thread
    after the workers have joined."""
    dims = [gj.dimension("dense", card=7, n1=2048), gj.dimension("sparse_wide", card=2048)]
    maps = [tc.KeyMap(lib, dk, da) for dk, da in dims]
    key, set_keys = tc.sc.keyset("sparse_wide", N)
    ks = tc.KeySet(lib, set_keys)
    try:
        jobs = []
        for i in range(WORKERS):
            km = maps[i & 1]
            fact = gj.FACT_SETS[(i >> 1) % 4]
            n = N + 32 * i + i
            semi_map = tc.SemiJob(lib, n, ks=lib.mq_keymap_keyset(km.h), set_keys=km.keys, key=gj.fact_keys("half_present", n, km.keys))
            jobs.append(both(both(semi_map, tc.SemiJob(lib, N, ks=ks.h, set_keys=set_keys, key=np.roll(key, 97 * i))), ProbeJob(lib, km, fact, n, i)))
        got, secs = tc.serial_pass(lib, jobs)
        report("shared handles", secs)
        Crew(lib, WORKERS, tc.deadline_for(ROUNDS * secs)).run([looping(j, [got[i, 0], got[i, 1]]) for i, j in enumerate(jobs)])
    finally:
        if not tc.HUNG:
            ks.free()
            for m in maps:
                m.free()


# ---------------------------------------------------------------------------
# 6. one group handle written from many threads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", [mq.MQ_GROUP_DENSE, mq.MQ_GROUP_SORT])
def test_one_measures_handle_written_from_many_threads(lib, path):
    """mq_group_measures_write "may be repeated (on any stream of the device)": the main thread
    plans, eight workers write the handle at once into outputs of their own on streams of their
    own, twenty times; every output is the model's and the serial write's. (The other handle
    kinds promise repeated writes only: they are serial-only)"""
    job = tc.MeasuresJob(lib)
    try:
        h = job.plan(None, path)
        t0 = time.perf_counter()
        job.arm(None)
        job.write(h, None)
        serial = job.read(None)
        secs = time.perf_counter() - t0
        assert serial == job.want, "single-thread write differs from the model"
        report("measures write", secs)
        outs = [job.new_outs() for _ in range(WORKERS)]

        def body(ctx):
            mine = outs[ctx.i]
            for r in range(ROUNDS):
                for o in mine:
                    o.arm(ctx.stream)
                ctx.barrier()
                job.write(h, ctx.stream, mine)
                got = [o.read(ctx.stream) for o in mine]
                assert got == job.want and got == serial, (ctx.i, r)

        Crew(lib, WORKERS, tc.deadline_for(ROUNDS * secs)).run([body] * WORKERS)
        mq.check(lib.mq_device_sync(), "mq_device_sync")
        # the buffers are freed in the order of the last write's stream, and the workers' streams are
        # gone: the last write is one on the NULL stream
        job.arm(None)
        job.write(h, None)
        assert job.read(None) == job.want
        mq.check(lib.mq_group_measures_free(h), "mq_group_measures_free")
    finally:
        if not tc.HUNG:
            job.free()


# ---------------------------------------------------------------------------
# 7. handles that change threads
# ---------------------------------------------------------------------------
def test_handles_planned_by_one_thread_written_and_freed_by_another(lib):
    """A plans a group, a measures and a distinct handle and builds a join on its stream and
    writes the first three into its own outputs; after a barrier B writes the handles on its
    stream into its outputs, frees them (their buffers go back in the order of B's stream, the
    last write's) and at once plans the same shapes again, which takes same-sized scratch from
    the pool, while A is reading its own outputs back. Both threads' results are exact."""
    ga, gb_ = tc.GroupJob(lib), tc.GroupJob(lib)
    ma, mb = tc.MeasuresJob(lib), tc.MeasuresJob(lib)
    da, db = tc.DistinctJob(lib), tc.DistinctJob(lib)
    jb = tc.JoinJob(lib)
    hs = {}
    try:
        def a_plans(ctx):
            s = ctx.stream
            for j in (ga, ma, da):
                j.arm(s)
            hs["g"], hs["m"], hs["d"] = ga.plan(s, 1), ma.plan(s, mq.MQ_GROUP_SORT), da.plan(s, 1)
            ga.write(hs["g"], s)
            ma.write(hs["m"], s)
            da.write(hs["d"], s)
            hs["j"] = jb.build(s)
            mq.check(lib.mq_stream_sync(s), "sync")  # the handles leave this thread with no work of its own queued on them

        def a_reads(ctx):
            for j in (ga, ma, da):
                assert j.read(ctx.stream) == j.want, (j.name, "planner's own outputs")

        def b_writes(ctx):
            s = ctx.stream
            for j in (gb_, mb, db, jb):
                j.arm(s)
            gb_.write(hs["g"], s)
            mb.write(hs["m"], s)
            db.write(hs["d"], s)
            jb.probe_write(hs["j"], s)
            mq.check(lib.mq_group_free(hs["g"]), "mq_group_free")
            mq.check(lib.mq_group_measures_free(hs["m"]), "mq_group_measures_free")
            mq.check(lib.mq_group_distinct_free(hs["d"]), "mq_group_distinct_free")
            first = [j.read(s) for j in (gb_, mb, db, jb)]
            mq.check(lib.mq_join_free(hs["j"]), "mq_join_free")
            again = [j.run(s, 1) for j in (gb_, mb, db)]  # the same shapes, planned afresh
            for j, f in zip((gb_, mb, db, jb), first):
                assert f == j.want, (j.name, "written by the other thread")
            for j, f in zip((gb_, mb, db), again):
                assert f == want_of(j, 1), (j.name, "planned again")

        rnd_a = [a_plans, a_reads]
        rnd_b = [None, b_writes]
        stepped(lib, rnd_a * 5, rnd_b * 5)
    finally:
        if not tc.HUNG:
            ma.free()
            mb.free()


# ---------------------------------------------------------------------------
# 8. staged downloads from several threads
# ---------------------------------------------------------------------------
class DownloadJob:
    """mq_select_positions + mq_memcpy_d2h_staged, then mq_select_positions_download with 1, 3
    and 8 segments, into guarded host buffers of this job's own."""

    def __init__(self, L, refcpu, i, n=N):
        self.L, self.n, self.i = L, n, i
        col = np.random.default_rng(900 + i).integers(0, 1000, n).astype(np.int32)
        self.lo, self.hi = 100 + 10 * i, 600 + 30 * i
        self.wpos = refcpu.select_scan(col, self.lo, self.hi)
        self.dcol, self.dpos, self.dcnt = Dev.of(col), Out(L, n), Out(L, 1, np.uint64)
        self.ws_bytes = L.mq_scan_workspace_bytes(n)
        self.ws = Dev(self.ws_bytes)
        self.host = np.empty(n + tc.GUARD, np.int32)

    def run(self, s):
        L, n, k = self.L, self.n, len(self.wpos)
        guard = np.frombuffer(bytes([FILL]) * 4, np.int32)[0]
        self.dpos.arm(s)
        self.dcnt.arm(s)
        mq.check(L.mq_select_positions(self.dcol.ptr, None, n, 1, self.lo, 1, self.hi, self.dpos.ptr, self.dcnt.ptr, self.ws.ptr,
                                       self.ws_bytes, s), "mq_select_positions")
        assert self.dcnt.read(s) == np.uint64(k).tobytes()
        self.host[:] = guard
        mq.check(L.mq_memcpy_d2h_staged(self.host.ctypes.data, self.dpos.ptr, 4 * k, s), "mq_memcpy_d2h_staged")
        assert np.array_equal(self.host[:k], self.wpos) and np.all(self.host[k:] == guard), (self.i, "staged")
        assert self.dpos.read(s) == padded(self.wpos, n)
        for segs in (1, 3, 8):
            self.host[:] = guard
            self.dpos.arm(s)
            h_seg, h_rows = (C.c_uint64 * segs)(), (C.c_uint64 * (segs + 1))()
            mq.check(L.mq_select_positions_download(self.dcol.ptr, n, 1, self.lo, 1, self.hi, segs, self.dpos.ptr, self.host.ctypes.data,
                                                    h_seg, h_rows, self.ws.ptr, self.ws_bytes, s), "mq_select_positions_download")
            rows = [int(x) for x in h_rows]
            assert rows[0] == 0 and rows[-1] == n and rows == sorted(rows), (self.i, segs, rows)
            want_seg = [int(np.count_nonzero((self.wpos >= a) & (self.wpos < b))) for a, b in zip(rows, rows[1:])]
            assert [int(x) for x in h_seg] == want_seg, (self.i, segs)
            assert np.array_equal(self.host[:k], self.wpos) and np.all(self.host[k:] == guard), (self.i, segs, "download")


def test_staged_downloads_from_several_threads(lib, refcpu):
    """Four workers each select, download through the staged D2H and through the pipelined
    segmented form (1, 3 and 8 segments) into host buffers of their own: the positions are
    refcpu's and no guard word behind a host buffer changes. Every worker ends with
    mq_thread_release; one more download from a new thread still works."""
    jobs = [DownloadJob(lib, refcpu, i) for i in range(5)]
    s = new_stream(lib)
    t0 = time.perf_counter()
    for j in jobs:
        j.run(s)
    secs = time.perf_counter() - t0
    mq.check(lib.mq_stream_destroy(s), "mq_stream_destroy")
    report("staged downloads", secs)

    def body_of(job, rounds):
        def body(ctx):
            for _ in range(rounds):
                ctx.barrier()
                job.run(ctx.stream)
        return body
    Crew(lib, 4, tc.deadline_for(ROUNDS * secs)).run([body_of(j, ROUNDS) for j in jobs[:4]])
    Crew(lib, 1, tc.deadline_for(secs)).run([body_of(jobs[4], 1)])
