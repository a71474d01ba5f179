"""The hash join where its suite never went, every comparison exact (-m gpu).

  a. hot keys: runs of 4096 / 4097 / 65 536 / 65 537 / 131 073 build rows through the
     per-row write (k_join_write lists a run past 4096 rows as 65 536-pair chunks, which
     k_join_write_long copies with one block each): more than one chunk a run, the chunk
     end at exactly one chunk, reservations of several entries from lanes of one wave and
     of different blocks, and, under a CU limit of 1, a list longer than the grid;
  b. mq_pjoin_place, which copies the scheme, with the same lengths;
  c. mq_join_counts in every state a probe can leave, before and after the write, and the
     build-positions-only write;
  d. mq_hash_join, the one-call form: capacity, NULL outputs, M = 0, a stream of its own;
  e. the join's grid-stride kernels past one sweep (mq_test_set_cu_limit, as
     test_gpu_regimes.py).

Expected values come from joincases.py (numpy, pinned to the oracle by test_join_host.py).
Every test asserts its regime through mq_join_state / mq_scan_geometry before it compares;
every output is prefilled with 0x5A bytes and followed by guard words that must stay.
"""
import ctypes as C

import numpy as np
import pytest

import joincases as jc
from devbuf import Dev
from refapi import mq
from test_gpu_parity import JOIN_PATHS, JOIN_PROBE_MODES
from test_gpu_regimes import SENT, _geometry, hardware, lib, limit  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 64  # int32 words past every output's end
PART, DUPW, PACKED, RS, PRUNS, RUN2, DEFERRED, ROW_WRITE = (
    mq.MQ_JOIN_STATE_PART, mq.MQ_JOIN_STATE_DUPW, mq.MQ_JOIN_STATE_PACKED, mq.MQ_JOIN_STATE_RS,
    mq.MQ_JOIN_STATE_PRUNS, mq.MQ_JOIN_STATE_RUN2, mq.MQ_JOIN_STATE_DEFERRED, mq.MQ_JOIN_STATE_ROW_WRITE)
FORCE_PART = {"MQ_JOIN_PART_MIN": "65536", "MQ_JOIN_PART_DIV": "1000000"}


class Out:
    """A device array of n elements, 0x5A-filled, with GUARD sentinel words behind it."""

    def __init__(self, lib, n, dtype=np.int32):
        self.lib, self.n, self.dtype = lib, int(n), dtype
        self.dev = Dev((self.n + GUARD) * 4)
        mq.check(lib.mq_memset(self.dev.ptr, 0x5A, (self.n + GUARD) * 4, None), "mq_memset")
        mq.check(lib.mq_stream_sync(None), "sync")
        self.ptr = self.dev.ptr

    def get(self, tag=None):
        """The n elements; the guard words must be as they were."""
        mq.check(self.lib.mq_device_sync(), "mq_device_sync")
        a = self.dev.get(np.uint32, self.n + GUARD)
        assert np.all(a[self.n:] == SENT), ("guard words written", tag)
        return a[:self.n].view(self.dtype)

    def untouched(self):
        mq.check(self.lib.mq_device_sync(), "mq_device_sync")
        return bool(np.all(self.dev.get(np.uint32, self.n + GUARD) == SENT))


class Join:
    """mq_join_build .. mq_join_free over host arrays (kept on the device until free())."""

    def __init__(self, lib, c1, p1, stream=None):
        self.lib, self.stream, self.h = lib, stream, C.c_void_p()
        self.d1 = [Dev.of(c1), Dev.of(p1)]
        self.d2 = None
        self.m = self.n2 = 0
        mq.check(lib.mq_join_build(self.d1[0].ptr, self.d1[1].ptr, len(c1), C.byref(self.h), stream), "join_build")

    def probe(self, c2):
        self.d2 = Dev.of(c2)
        m = C.c_uint64()
        mq.check(self.lib.mq_join_probe(self.h, self.d2.ptr, len(c2), C.byref(m), self.stream), "join_probe")
        self.m, self.n2 = m.value, len(c2)
        return self.m

    def state(self):
        out = (C.c_uint32 * mq.MQ_JOIN_STATE_WORDS)()
        mq.check(self.lib.mq_join_state(self.h, out), "mq_join_state")
        return out[0], out[1], out[2]

    def counts(self, tag=None):
        cnt = Out(self.lib, self.n2, np.uint32)
        mq.check(self.lib.mq_join_counts(self.h, cnt.ptr, self.stream), "join_counts")
        return cnt.get(tag)

    def write(self, p2, tag=None, p2_offset=0):
        """(out1, out2); p2 None: the build-positions-only write, (out1, None). p2_offset:
        p2 that many elements past a 16-byte boundary."""
        o1 = Out(self.lib, self.m)
        o2 = Out(self.lib, self.m) if p2 is not None else None
        dp2 = Dev.of(p2, offset_elems=p2_offset) if p2 is not None else None
        mq.check(self.lib.mq_join_write(self.h, dp2.ptr if dp2 else None, o1.ptr, o2.ptr if o2 else None,
                                        self.stream), "join_write")
        return o1.get(tag), (o2.get(tag) if o2 else None)

    def free(self):
        if self.h:
            mq.check(self.lib.mq_join_free(self.h), "join_free")
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def want_hot():
    """join_pairs of hot_keys, both directions (computed once)."""
    c1, p1, c2, p2, _ = jc.hot_keys()
    return jc.join_pairs(c1, p1, c2, p2), jc.join_pairs(c2, p2, c1, p1)


def blocks_under(lib, cus):
    """The limit holds: the geometry's grid is that of `cus` CUs (8 blocks each)."""
    blocks, _ = _geometry(lib, 1 << 30)
    assert 0 < blocks <= 8 * cus, (cus, blocks)
    return blocks


# ---------------------------------------------------------------------------
# a. hot keys through every build path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [0, 1])
@pytest.mark.parametrize("path", list(JOIN_PATHS))
def test_hot_keys_per_row_write(lib, limit, monkeypatch, want_hot, path, cus):
    setenv(monkeypatch, JOIN_PATHS[path])
    c1, p1, c2, p2, _ = jc.hot_keys()
    (w1, w2), (v1, v2) = want_hot
    entries = jc.long_entries(jc.join_counts(c1, c2))
    assert entries == 21
    if cus:
        limit(cus)
        assert entries > 8 * cus >= blocks_under(lib, cus)  # k_join_write_long's 8 blocks a CU: a longer list
    with Join(lib, c1, p1) as j:
        assert j.probe(c2) == len(w1)
        o1, o2 = j.write(p2, (path, cus))
        unique, flags, nlong = j.state()
        # a key on 15 or more rows sends the windowed and partitioned duplicate forms to the
        # sorted runs (or, MQ_JOIN_RUNS=0, the global-CAS table), whose write is the per-row one
        assert flags & ROW_WRITE and nlong == entries, (path, cus, unique, flags, nlong)
        if path == "cas":
            assert unique == 0 and not flags & (PART | DUPW | PRUNS | DEFERRED), (unique, flags)
        else:
            assert unique == 2 and flags & RS and not flags & (PART | DUPW | PRUNS | DEFERRED), (unique, flags)
        assert np.array_equal(o1, w1) and np.array_equal(o2, w2), (path, cus)
        cnt = j.counts((path, cus))  # per-row lengths, after the write
        assert np.array_equal(cnt, jc.join_counts(c1, c2)), (path, cus)
    # roles swapped: a hot probe-side key (4096 .. 131 073 probe rows) hits short build runs
    with Join(lib, c2, p2) as j:
        assert j.probe(c1) == len(v1)
        h1, h2 = j.write(p1, (path, cus, "swapped"))
        assert np.array_equal(h1, v1) and np.array_equal(h2, v2), (path, cus, "swapped")


# ---------------------------------------------------------------------------
# b. mq_pjoin_place with the same lengths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [0, 1])
def test_place_hot_lengths(lib, limit, cus):
    cntp, out1p, inv, p2 = jc.hot_place()
    n, m = len(cntp), len(out1p)
    assert jc.long_entries(cntp) == 21
    if cus:
        limit(cus)
        blocks = blocks_under(lib, cus)
        assert 21 > blocks and n > 8 * blocks * 256  # k_pj_place_long and the row kernels: many sweeps
    w1, w2 = jc.place(cntp, out1p, inv, p2)
    D = [Dev.of(x) for x in (cntp, out1p, inv, p2)]
    o1, o2 = Out(lib, m), Out(lib, m)
    mq.check(lib.mq_pjoin_place(D[0].ptr, D[1].ptr, D[2].ptr, D[3].ptr, n, m, o1.ptr, o2.ptr, None), "mq_pjoin_place")
    assert np.array_equal(o1.get(cus), w1) and np.array_equal(o2.get(cus), w2)


# ---------------------------------------------------------------------------
# c. mq_join_counts in every state the probe can leave
# ---------------------------------------------------------------------------
def _spread(rng, n):
    return rng.choice(1 << 30, n, replace=False).astype(np.int32)


def _unique_build(n1):
    def make(rng):
        keys = _spread(rng, n1 + 5000)
        return keys[:n1], keys[:n1], keys[n1:]  # build, keys to hit, keys never built
    return make


def _short_runs_build(rng):
    """dups_short_runs's build, smaller: 70 000+ rows, runs of 1 to 14 in input order."""
    keys = _spread(rng, 25_000)
    reps = rng.integers(1, 15, 20_000)
    c1 = np.repeat(keys[:20_000], reps)
    return c1[rng.permutation(len(c1))], keys[:20_000][reps >= 2], keys[20_000:]


def _dups_build(rng):
    c1 = rng.integers(0, 5000, 30_000, dtype=np.int32)
    return c1, np.arange(5000, dtype=np.int32), np.arange(5000, 6000, dtype=np.int32)


# state: (env, build, (unique, flags set, flags clear) after the probe)
COUNT_STATES = {
    "unique_table": ({}, _unique_build(5_000), (1, 0, PART | DEFERRED | PRUNS)),
    "unique_part_deferred": (FORCE_PART, _unique_build(70_001), (1, PART | DEFERRED, DUPW | PRUNS)),
    "unique_materialized": ({"MQ_JOIN_PART_MIN": "65536", "MQ_JOIN_PART_DIV": "1"}, _unique_build(80_003),
                            (1, 0, PART | DEFERRED | PRUNS)),
    "windowed_packed_runs": ({}, _short_runs_build, (2, PACKED | PRUNS, PART | DUPW | RS | RUN2 | DEFERRED)),
    "part_dup_run2": (FORCE_PART, _short_runs_build, (2, PART | DUPW | PRUNS | RUN2 | DEFERRED, RS)),
    "part_dup_packed": (dict(FORCE_PART, MQ_JOIN_RUN2="0"), _short_runs_build,
                        (2, PACKED | PRUNS, PART | DUPW | RS | RUN2 | DEFERRED)),
    "sorted_runs": ({"MQ_JOIN_WINRUNS": "0"}, _dups_build, (2, RS, PART | DUPW | PRUNS | DEFERRED)),
    "global_cas": ({"MQ_JOIN_RUNS": "0"}, _dups_build, (0, 0, PART | DUPW | PRUNS | DEFERRED)),
}


@pytest.mark.parametrize("n2", [1, 63, 64, 65, 4097, 70_001])
@pytest.mark.parametrize("state", list(COUNT_STATES))
def test_join_counts_in_every_probe_state(lib, monkeypatch, state, n2):
    env, build, (unique, on, off) = COUNT_STATES[state]
    setenv(monkeypatch, env)
    rng = np.random.default_rng(n2 + 100_000 * list(COUNT_STATES).index(state))
    c1, hits, misses = build(rng)
    assert state not in ("unique_part_deferred", "unique_materialized", "windowed_packed_runs", "part_dup_run2",
                         "part_dup_packed") or len(c1) >= 65536  # the windowed builds
    assert state != "unique_materialized" or n2 < len(c1)
    # row 0 always hits (a duplicated key where the build has any: the partitioned forms
    # turn to their duplicate-key form only when a probe row meets one); the last row too
    c2 = np.where(rng.random(n2) < 0.6, rng.choice(hits, n2), rng.choice(misses, n2)).astype(np.int32)
    c2[0] = c2[-1] = hits[0]
    p1 = rng.integers(-10 ** 7, 10 ** 7, len(c1), dtype=np.int32)
    p2 = rng.integers(0, 10 ** 7, n2, dtype=np.int32)
    w1, w2 = jc.join_pairs(c1, p1, c2, p2)
    wc = jc.join_counts(c1, c2)
    tag = (state, n2)

    def probed():
        j = Join(lib, c1, p1)
        assert j.probe(c2) == len(w1), tag
        u, f, _ = j.state()
        assert u == unique and f & on == on and not f & off, (tag, u, f)
        return j

    with probed() as j:  # no counts call: the write as the probe left it
        a1, a2 = j.write(p2, tag)
    with probed() as j:  # ... and its build-positions-only form
        b1, _ = j.write(None, tag)
    with probed() as j:
        cnt = j.counts(tag)
        assert not j.state()[1] & DEFERRED, tag  # (the deferred forms: finished the classic way)
        assert np.array_equal(cnt, wc) and int(cnt.astype(np.int64).sum()) == j.m, tag
        c1_, c2_ = j.write(p2, tag)
        assert np.array_equal(j.counts(tag), wc), tag  # again after the write
        d1, _ = j.write(None, tag)
        if state in ("sorted_runs", "global_cas"):
            assert j.state()[1] & ROW_WRITE, tag
    assert np.array_equal(a1, w1) and np.array_equal(a2, w2), tag
    assert np.array_equal(c1_, w1) and np.array_equal(c2_, w2), tag  # counts first: the same pairs
    assert np.array_equal(b1, w1) and np.array_equal(d1, w1), tag


def test_join_counts_edges(lib):
    rng = np.random.default_rng(5)
    c1 = rng.permutation(1000).astype(np.int32)
    c2 = rng.integers(0, 2000, 300, dtype=np.int32)
    empty = np.zeros(0, np.int32)
    with Join(lib, empty, empty) as j:  # n1 == 0: the probe ran nothing, the counts are zeros
        assert j.probe(c2) == 0
        assert np.array_equal(j.counts(), np.zeros(len(c2), np.uint32))
    cnt = Out(lib, 300, np.uint32)
    with Join(lib, c1, c1) as j:
        assert j.probe(empty) == 0  # n2 == 0: nothing to write, with or without d_cnt
        assert lib.mq_join_counts(j.h, cnt.ptr, None) == mq.MQ_OK
        assert lib.mq_join_counts(j.h, None, None) == mq.MQ_OK
        assert cnt.untouched()
        assert j.probe(c2) == int(jc.join_counts(c1, c2).sum())
        assert lib.mq_join_counts(j.h, None, None) == mq.MQ_EINVAL  # n2 > 0 and no d_cnt
        assert lib.mq_join_counts(None, cnt.ptr, None) == mq.MQ_EINVAL  # no handle
        assert cnt.untouched()
        assert np.array_equal(j.counts(), jc.join_counts(c1, c2))


# ---------------------------------------------------------------------------
# d. mq_hash_join, the one-call form
# ---------------------------------------------------------------------------
def _hash_join(lib, D, n1, n2, o1, o2, cap, stream=None, h_m=True):
    m = C.c_uint64(0xDEAD)
    rc = lib.mq_hash_join(D[0].ptr, D[1].ptr, n1, D[2].ptr, D[3].ptr, n2, o1.ptr if o1 else None,
                          o2.ptr if o2 else None, cap, C.byref(m) if h_m else None, stream)
    return rc, m.value


def _one_call_inputs(name):
    if name == "hot_keys":
        return jc.hot_keys()[:4]
    if name == "dups":
        return jc.named_inputs("dups")
    rng = np.random.default_rng(20)  # unique_part: 2^20 + 333 unique build rows, a third of the probe hits
    n1 = (1 << 20) + 333
    keys = _spread(rng, n1 + 200_000)
    c1 = keys[:n1]
    c2 = np.concatenate([rng.choice(c1, 100_000), keys[n1:]])[rng.permutation(300_000)]
    return c1, rng.integers(-10 ** 7, 10 ** 7, n1, dtype=np.int32), c2, rng.integers(0, 10 ** 7, len(c2), dtype=np.int32)


@pytest.mark.parametrize("name", ["unique_part", "dups", "hot_keys"])
def test_hash_join_one_call(lib, name):
    c1, p1, c2, p2 = _one_call_inputs(name)
    n1, n2 = len(c1), len(c2)
    w1, w2 = jc.join_pairs(c1, p1, c2, p2)
    M = len(w1)
    assert M > 0
    # the regime, from the three-step form under the same (default) settings
    with Join(lib, c1, p1) as j:
        assert j.probe(c2) == M
        unique, flags, _ = j.state()
        if name == "unique_part":  # the default partitioned probe, whose write is the fused one
            assert unique == 1 and flags & PART and flags & DEFERRED, (unique, flags)
        t1, t2 = j.write(p2, name)
        if name == "hot_keys":
            assert j.state()[1] & ROW_WRITE and j.state()[2] == 21
    assert np.array_equal(t1, w1) and np.array_equal(t2, w2), name
    D = [Dev.of(x) for x in (c1, p1, c2, p2)]
    sp = C.c_void_p()
    mq.check(lib.mq_stream_create(C.byref(sp)), "mq_stream_create")
    try:
        for stream in (None, sp.value):  # cap == M succeeds, on the null stream and on one of its own
            o1, o2 = Out(lib, M), Out(lib, M)
            rc, m = _hash_join(lib, D, n1, n2, o1, o2, M, stream)
            assert (rc, m) == (mq.MQ_OK, M), (name, stream, rc, m)
            assert np.array_equal(o1.get(name), w1) and np.array_equal(o2.get(name), w2), (name, stream)
    finally:
        mq.check(lib.mq_stream_destroy(sp.value), "mq_stream_destroy")
    o1, o2 = Out(lib, M), Out(lib, M)
    assert _hash_join(lib, D, n1, n2, o1, o2, M - 1) == (mq.MQ_ECAP, M)  # one pair short
    assert _hash_join(lib, D, n1, n2, None, o2, M) == (mq.MQ_ECAP, M)
    assert _hash_join(lib, D, n1, n2, o1, None, M) == (mq.MQ_ECAP, M)
    assert _hash_join(lib, D, n1, n2, o1, o2, M, h_m=False)[0] == mq.MQ_EINVAL
    assert o1.untouched() and o2.untouched(), name
    # M == 0: MQ_OK whatever the outputs (an all-miss probe; no probe rows)
    absent = np.arange(-1000, 0, dtype=np.int32)
    assert not np.isin(absent, c1).any()
    miss = Dev.of(absent)
    for d2, k2 in ((miss, 1000), (D[2], 0)):
        for a, b in ((o1, o2), (None, o2), (o1, None), (None, None)):
            rc, m = _hash_join(lib, [D[0], D[1], d2, D[3]], n1, k2, a, b, 0)
            assert (rc, m) == (mq.MQ_OK, 0), (name, k2, a is None, b is None, rc, m)
    assert o1.untouched() and o2.untouched(), name


# ---------------------------------------------------------------------------
# e. the grid-stride kernels past one sweep
# ---------------------------------------------------------------------------
def _sweeps(lib, limit, cus, n2):
    limit(cus)
    blocks = blocks_under(lib, cus)
    assert n2 > 8 * cus * 256 >= blocks * 256, (cus, blocks, n2)  # every stream_grid kernel: j += stride runs


@pytest.mark.parametrize("cus", [1, 2])
@pytest.mark.parametrize("path", list(JOIN_PATHS))
@pytest.mark.parametrize("case", ["dups", "dups_short_runs", "marker", "neg"])
def test_build_paths_many_sweeps(lib, limit, monkeypatch, case, path, cus):
    setenv(monkeypatch, JOIN_PATHS[path])
    c1, p1, c2, p2 = jc.named_inputs(case)
    assert len(c1) <= 300_000 and len(c2) <= 300_000
    _sweeps(lib, limit, cus, len(c2))
    w1, w2 = jc.join_pairs(c1, p1, c2, p2)
    with Join(lib, c1, p1) as j:
        assert j.probe(c2) == len(w1)
        unique, flags, _ = j.state()
        if case == "dups" and path in ("sorted", "cas"):  # (under 2^16 build rows: no windowed runs build)
            assert unique == (2 if path == "sorted" else 0) and not flags & PRUNS, (unique, flags)
        cnt = j.counts((case, path, cus))
        o1, o2 = j.write(p2, (case, path, cus))
    assert np.array_equal(cnt, jc.join_counts(c1, c2)), (case, path, cus)
    assert np.array_equal(o1, w1) and np.array_equal(o2, w2), (case, path, cus)


@pytest.mark.parametrize("cus", [1, 2])
@pytest.mark.parametrize("mode", list(JOIN_PROBE_MODES))
@pytest.mark.parametrize("case", jc.PROBE_CASES)
def test_probe_modes_many_sweeps(lib, limit, refcpu, monkeypatch, case, mode, cus):
    monkeypatch.setenv("MQ_JOIN_SAMPLE", "0")
    setenv(monkeypatch, JOIN_PROBE_MODES[mode])
    c1, p1, c2, p2 = jc.probe_inputs(case, refcpu.gen_join)
    assert len(c2) < len(c1)
    _sweeps(lib, limit, cus, len(c2))
    w1, w2 = jc.join_pairs(c1, p1, c2, p2)
    with Join(lib, c1, p1) as j:
        assert j.probe(c2) == len(w1)
        unique, flags, _ = j.state()
        if case != "dup_probed":  # (n2 < n1: MQ_JOIN_PART_DIV=1 stores the windows as the global table)
            assert unique == 1 and bool(flags & DEFERRED) == (mode in ("part", "part_wide")), (case, mode, unique, flags)
            assert bool(flags & PART) == (mode in ("part", "part_wide")), (case, mode, flags)
        else:  # the probe met the duplicate key: no longer the unique table
            assert unique != 1, (case, mode, unique, flags)
        o1, o2 = j.write(p2, (case, mode, cus))
        if not flags & DEFERRED:  # p2 off 16-byte alignment: k_join_write_hits, one row a lane
            u1, u2 = j.write(p2, (case, mode, cus, "unaligned"), p2_offset=1)
            assert np.array_equal(u1, w1) and np.array_equal(u2, w2), (case, mode, cus, "unaligned")
    assert np.array_equal(o1, w1) and np.array_equal(o2, w2), (case, mode, cus)


@pytest.mark.parametrize("dup", [False, True])
def test_sampled_build_many_sweeps(lib, limit, dup):
    """Builds of 2^20 rows and more check a strided sample of 2^18 keys for duplicates first
    (k_sample_dups): under a limit of 2 CUs its grid takes 64 sweeps. Unique keys stay on the
    partitioned unique build; every key twice goes straight to the partitioned duplicate form."""
    c1, p1, c2, p2 = _one_call_inputs("unique_part")
    if dup:
        c1 = c1.copy()  # (a key's two rows 2^19 apart: the sample's stride of 4 rows takes both)
        c1[1 << 19:1 << 20] = c1[:1 << 19]
    _sweeps(lib, limit, 2, 1 << 18)
    w1, w2 = jc.join_pairs(c1, p1, c2, p2)
    with Join(lib, c1, p1) as j:
        unique, flags, _ = j.state()  # decided by the build, before any probe
        assert (unique, bool(flags & DUPW)) == ((2, True) if dup else (1, False)) and flags & PART, (dup, unique, flags)
        assert j.probe(c2) == len(w1)
        assert j.state()[1] & DEFERRED
        o1, o2 = j.write(p2, dup)
    assert np.array_equal(o1, w1) and np.array_equal(o2, w2), dup
