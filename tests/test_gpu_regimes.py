"""The full-size regimes of the streaming kernels at small sizes, every comparison exact.

Every streaming kernel sizes its grid from the device's CU count, so on a 256-CU MI355X
a column of a few million rows leaves a block or wave almost no rows: k_scan's unrolled
main loop, k_select_stage's ring + spill and its switch to bitmap mode, the long
wave-chunks of shared select and of k_group_dense then run only in the 1e9-row tests,
which check properties on uniform data. mq_test_set_cu_limit (mq_device.h) lowers the CU
count the geometry uses; with 1, 2 or 7 CUs a column of 0.3-4 M rows gives each block
what a 1e9-row column gives it on the whole device. Expected values come from numpy, the
refcpu oracle and groupcases.py; each test asserts first that its regime is reached.
"""
import ctypes as C

import numpy as np
import pytest

import groupcases as gc
from devbuf import Dev
from refapi import mq
from test_gpu_parity import BOUNDS, I32MAX, I32MIN, _data

pytestmark = pytest.mark.gpu

LIMITS = [1, 2, 7]
SCAN_N = 300_007     # rows per limited CU: 37 tiles a block (kSum: 4 unrolled groups + 5 tail tiles)
STAGE_N = 4_000_037
ROW_BASE = 1_000_003
SENT = 0x5A5A5A5A    # what mq_memset(0x5A) leaves in an int32


def _geometry(L, n):
    b, r = C.c_uint32(), C.c_uint64()
    L.mq_scan_geometry(n, C.byref(b), C.byref(r))
    return b.value, r.value


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    yield L
    L.mq_test_set_cu_limit(0)


@pytest.fixture(scope="module")
def hardware(lib):
    """mq_scan_geometry before this module sets any limit."""
    return {n: _geometry(lib, n) for n in (1, SCAN_N, STAGE_N, 1 << 30)}


@pytest.fixture
def limit(lib, hardware):
    """limit(cus) sets the CU limit for the test; the hardware count is back afterwards,
    whatever the test did."""
    def set_limit(cus):
        mq.check(lib.mq_device_sync(), "mq_device_sync")
        mq.check(lib.mq_test_set_cu_limit(cus), "mq_test_set_cu_limit")
        blocks, _ = _geometry(lib, 1 << 30)
        assert 0 < blocks <= 8 * cus, (cus, blocks)  # the limit is what the geometry uses
    try:
        yield set_limit
    finally:
        lib.mq_device_sync()
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def _agg_of(out):
    a = mq.MqAgg.from_buffer_copy(out.get(np.uint8, 32).tobytes())
    return a.count, a.sum, a.min, a.max


def _mask(d, lo, hi):
    m = np.ones(len(d), dtype=bool)
    if lo is not None:
        m &= d >= lo
    if hi is not None:
        m &= d < hi
    return m


def _want_agg(v):
    """(count, int64 sum, min, max) of the selected values, as mq_agg reports them."""
    if len(v) == 0:
        return 0, 0, I32MAX, I32MIN
    return len(v), int(v.astype(np.int64).sum()), int(v.min()), int(v.max())


def _is_empty_range(lo, hi):
    return (I32MAX + 1 if hi is None else hi) - (I32MIN if lo is None else lo) <= 0


# ---------------------------------------------------------------------------
# a. the scan family: k_scan<kSum / kAgg> and k_scan_gather
# ---------------------------------------------------------------------------
def _wide(n, seed):
    """Full-range int32 with INT32_MIN, INT32_MAX and INT32_MAX - 1 planted every 10 007
    rows, a third of the period apart: each lands in the unrolled groups of every block
    (a block owns at least 24 576 rows, and its tail is at most 7 tiles)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(I32MIN, I32MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
    d[0::10_007] = I32MIN
    d[3_331::10_007] = I32MAX
    d[6_673::10_007] = I32MAX - 1
    return d


def _scan_column(kind, n):
    return _wide(n, 31 * n + 1) if kind == "wide" else _data(n, n)


def _scan_regime(lib, n):
    blocks, rpb = _geometry(lib, n)
    assert rpb >= 3 * 8192, (n, blocks, rpb)  # several unrolled groups a block, accumulators live
    return blocks


@pytest.mark.parametrize("cus", LIMITS)
@pytest.mark.parametrize("kind", ["wide", "narrow"])
def test_scan_main_loop(lib, limit, kind, cus):
    """mq_select_sum, mq_select_agg and the two-launch form (mq_select_partials +
    mq_combine_partials, both want_minmax values) where every block runs its unrolled
    main loop several times and then a tail: columns 16-byte aligned and +4 B, the whole
    bounds matrix. SCAN_N rows for each limited CU keep 37 tiles a block."""
    limit(cus)
    n = SCAN_N * cus
    blocks = _scan_regime(lib, n)
    d = _scan_column(kind, n)
    want = {b: _want_agg(d[_mask(d, *b)]) for b in BOUNDS}
    ws, out = Dev(lib.mq_scan_workspace_bytes(n)), Dev(32)
    for off in (0, 1):
        dd = Dev.of(d, offset_elems=off)
        for lo, hi in BOUNDS:
            tag = (kind, cus, off, lo, hi)
            w = want[(lo, hi)]
            args = (dd.ptr, n) + mq.bounds(lo, hi)
            mq.check(lib.mq_select_sum(*args, out.ptr, ws.ptr, ws.nbytes, None))
            assert _agg_of(out) == (w[0], w[1], I32MAX, I32MIN), tag
            mq.check(lib.mq_select_agg(*args, out.ptr, ws.ptr, ws.nbytes, None))
            assert _agg_of(out) == w, tag
            for minmax in (0, 1):
                nb = C.c_uint32(0)
                mq.check(lib.mq_select_partials(*args, minmax, ws.ptr, ws.nbytes, C.byref(nb), None))
                if _is_empty_range(lo, hi):
                    assert nb.value >= 1, tag
                else:
                    assert nb.value == blocks, tag + (minmax,)
                mq.check(lib.mq_combine_partials(ws.ptr, nb.value, out.ptr, None))
                assert _agg_of(out) == (w if minmax else (w[0], w[1], I32MAX, I32MIN)), tag + (minmax,)


@pytest.mark.parametrize("cus", LIMITS)
@pytest.mark.parametrize("kind", ["wide", "narrow"])
def test_fused_select_fetch_agg_main_loop(lib, limit, kind, cus):
    """k_scan_gather over the same chunks: the select column wide or narrow, the value
    column full-range with the INT32 extremes planted; the narrow column's wide ranges
    fill and drain the per-wave LDS buffer many times a block."""
    limit(cus)
    n = SCAN_N * cus
    _scan_regime(lib, n)  # k_scan_gather launches no more blocks than k_scan does
    sel, val = _scan_column(kind, n), _wide(n, 77 * n + 5)
    ws, out = Dev(lib.mq_scan_workspace_bytes(n)), Dev(32)
    for off in (0, 1):
        ds, dv = Dev.of(sel, offset_elems=off), Dev.of(val, offset_elems=off)
        for lo, hi in BOUNDS:
            w = _want_agg(val[_mask(sel, lo, hi)])
            mq.check(lib.mq_select_fetch_agg(ds.ptr, dv.ptr, n, *mq.bounds(lo, hi), out.ptr, ws.ptr, ws.nbytes,
                                             None))
            assert _agg_of(out) == w, (kind, cus, off, lo, hi)


# ---------------------------------------------------------------------------
# b. k_select_stage: positions, the payload form, a row base
# ---------------------------------------------------------------------------
LO, HI = -1000, 1000  # the range every pattern's matching rows lie in


def _bursts(n):
    """Runs of exactly 1023, 1024, 1025 and 2049 matching rows, 60 013 others between."""
    m = np.zeros(n, dtype=bool)
    at, k = 0, 0
    while at < n:
        run = (1023, 1024, 1025, 2049)[k % 4]
        m[at:at + run] = True
        at += run + 60_013
        k += 1
    return m


def _window(n, start):
    m = np.zeros(n, dtype=bool)
    m[start:start + 10_000] = True
    return m


# name -> (match mask over the row index, period of a one-in-p pattern or None)
PATTERNS = {
    # uniform densities by row index, periods unrelated to the 2048-row granule
    "one_in_199": (lambda i, n: i % 199 == 0, 199),     # 0.5 %: the ring alone
    "one_in_49": (lambda i, n: i % 49 == 0, 49),        # 2 %: ring + spill
    "one_in_33": (lambda i, n: i % 33 == 0, 33),        # 3 %: spill near its allowance
    "one_in_32": (lambda i, n: i % 32 == 0, 32),        # 8 a tile: the allowance exactly
    "one_in_25": (lambda i, n: i % 25 == 0, 25),        # 4 %: spills, then the switch
    "half": (lambda i, n: i % 14 < 7, None),
    "all": (lambda i, n: np.ones(n, dtype=bool), None),
    # 1 % for 70 001 rows then every row for 30 011: spills, then a switch off any 8-tile edge
    "sparse_then_dense": (lambda i, n: np.where(i % 100_012 < 70_001, i % 100_012 % 100 == 0, True), None),
    # a ring exactly full and one past full, then long all-zero bitmap tiles
    "bursts": (lambda i, n: _bursts(n), None),
    # isolated matches: cross-block prefixes over zero counts
    "row_0": (lambda i, n: i == 0, None),
    "row_last": (lambda i, n: i == n - 1, None),
    "tile_last_rows": (lambda i, n: i % 256 == 255, None),
    "window_start": (lambda i, n: _window(n, 0), None),
    "window_middle": (lambda i, n: _window(n, n // 2 - 5_000), None),
    "window_end": (lambda i, n: _window(n, n - 10_000), None),
}

_stage_cache = {}


def _stage_case(name):
    """The pattern's column and payload on the host and on the device (aligned and +4 B)
    and the expected positions: made once, shared by the three limits, never changed."""
    if name not in _stage_cache:
        _stage_cache.clear()
        n = STAGE_N
        rng = np.random.default_rng(sorted(PATTERNS).index(name))
        m = np.asarray(PATTERNS[name][0](np.arange(n, dtype=np.int64), n), dtype=bool)
        inside = rng.integers(LO, HI, n, dtype=np.int32)
        inside[::7], inside[3::7] = LO, HI - 1
        outside = np.array([I32MIN, LO - 1, HI, I32MAX, -123_456_789, 123_456_789],
                           dtype=np.int32)[rng.integers(0, 6, n)]
        col = np.where(m, inside, outside).astype(np.int32)
        want = np.flatnonzero(m).astype(np.int32)
        assert np.array_equal(want, np.flatnonzero((col >= LO) & (col < HI)))
        pay = (np.arange(n, dtype=np.int64) * 7 - 5).astype(np.int32)
        _stage_cache[name] = dict(
            n=n, want=want, want_pay=pay[want], cols=[Dev.of(col), Dev.of(col, offset_elems=1)],
            pays=[Dev.of(pay), Dev.of(pay, offset_elems=1)], ws=Dev(mq.load().mq_scan_workspace_bytes(n)),
            out=Dev((n + 8) * 4), cnt=Dev(8))
    return _stage_cache[name]


def _stage_rows_per_wave(n, cus):
    """A lower bound of k_select_stage's rows per wave: whole 2048-row granules dealt to
    at most 8 resident blocks of 4 waves a CU."""
    granules = -(-n // 2048)
    return -(-granules // (32 * cus)) * 2048


def _stage_run(lib, c, col, out_off, want, tag, payload=None, row_base=None):
    n, out, cnt, ws = c["n"], c["out"], c["cnt"], c["ws"]
    k = len(want)
    mq.check(lib.mq_memset(out.ptr, 0x5A, (n + 8) * 4, None))
    optr = out.ptr + 4 * out_off
    if row_base is None:
        mq.check(lib.mq_select_positions(col, payload, n, 1, LO, 1, HI, optr, cnt.ptr, ws.ptr, ws.nbytes, None))
    else:
        mq.check(lib.mq_select_positions_at(col, payload, n, row_base, 1, LO, 1, HI, optr, cnt.ptr, ws.ptr,
                                            ws.nbytes, None))
    assert int(cnt.get(np.uint64, 1)[0]) == k, tag
    got = out.get(np.int32, out_off + k + 4)
    assert np.all(got[:out_off] == SENT) and np.all(got[out_off + k:] == SENT), tag + ("wrote outside the list",)
    assert np.array_equal(got[out_off:out_off + k], want), tag


@pytest.mark.parametrize("cus", LIMITS)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_select_stage_regimes(lib, limit, name, cus):
    """mq_select_positions on an aligned and a +4 B column and into an output 4 / 8 / 12 B
    past a 16-byte boundary, the payload form with the payload aligned and +4 B, and
    mq_select_positions_at with a row base, on patterns that wave boundaries cut
    everywhere. With one limited CU a wave owns at least 126 976 rows, the 1e9-row run's
    regime (122 880)."""
    limit(cus)
    c = _stage_case(name)
    n, want = c["n"], c["want"]
    rw = _stage_rows_per_wave(n, cus)
    # more than 64 bitmap tiles a wave (the expansion loop repeats) and many iterations of
    # the unrolled loop (the pending bitmap record is carried from one to the next)
    assert rw > 64 * 256, (cus, rw)
    if cus <= 2:
        assert rw > 32768, (cus, rw)  # ring + spill is reachable: 1024 matches below 1/32
    period = PATTERNS[name][1]
    if cus == 1 and period not in (None, 199):
        assert rw // period > 1024 + 64, (name, rw // period)  # the ring overflows: a wave spills
    (col0, col1), (pay0, pay1) = [x.ptr for x in c["cols"]], [x.ptr for x in c["pays"]]
    _stage_run(lib, c, col0, 0, want, (name, cus, "aligned"))
    _stage_run(lib, c, col1, 0, want, (name, cus, "column +4 B"))
    for out_off in (1, 2, 3):
        _stage_run(lib, c, col0, out_off, want, (name, cus, "output +", out_off))
    _stage_run(lib, c, col0, 0, c["want_pay"], (name, cus, "payload"), payload=pay0)
    _stage_run(lib, c, col1, 1, c["want_pay"], (name, cus, "payload +4 B"), payload=pay1)
    _stage_run(lib, c, col0, 0, want + np.int32(ROW_BASE), (name, cus, "row base"), row_base=ROW_BASE)


# ---------------------------------------------------------------------------
# c. shared select: the count, scatter and column passes over long wave-chunks
# ---------------------------------------------------------------------------
_shared_cache = {}


def _shared_case(refcpu, kind, q):
    """Column, query ranges (the sparse150 and dense rules of
    test_shared_select_many_queries) and refcpu.shared_select's lists, made once."""
    if (kind, q) not in _shared_cache:
        _shared_cache.clear()
        n = STAGE_N
        rng = np.random.default_rng(1000 * q + len(kind))
        d = rng.integers(0, 10 ** 6, n).astype(np.int32)
        if kind == "sparse":
            lows = rng.integers(0, 10 ** 6 - 1000, q)
            highs = lows + 1000
        else:
            lows = rng.integers(0, 500_000, q)
            highs = lows + rng.integers(100_000, 500_000, q)
        lows, highs = lows.astype(np.int32), highs.astype(np.int32)
        _shared_cache[(kind, q)] = (d, Dev.of(d), lows, highs, refcpu.shared_select(d, lows, highs, nthreads=16))
    return _shared_cache[(kind, q)]


@pytest.mark.parametrize("twopass", [False, True])
@pytest.mark.parametrize("cus", [1, 2])
@pytest.mark.parametrize("q", [2, 16, 150])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_shared_select_long_chunks(lib, refcpu, limit, monkeypatch, kind, q, cus, twopass):
    """mq_shared_select_count + _write where a wave-chunk is 60 K rows and more (1e9 rows
    on the whole device: 120 K): the pair-listing count pass and the scatter, the dense
    ranges' pair-slice overflow into the column pass, and the column pass forced."""
    if twopass:
        monkeypatch.setenv("MQ_SS_TWOPASS", "1")
    limit(cus)
    d, dd, lows, highs, want = _shared_case(refcpu, kind, q)
    n = len(d)
    assert -(-n // (32 * cus)) >= 60_000, cus  # rows a wave-chunk: at most 8 blocks of 4 waves a CU
    ws = Dev(lib.mq_shared_select_workspace_bytes(n, q))  # sized under the limit
    k = (C.c_uint64 * q)()
    lo_c, hi_c = (C.c_int32 * q)(*lows.tolist()), (C.c_int32 * q)(*highs.tolist())
    mq.check(lib.mq_shared_select_count(dd.ptr, n, lo_c, hi_c, q, k, ws.ptr, ws.nbytes, None))
    assert [int(x) for x in k] == [len(w) for w in want], (kind, q, cus, twopass)
    outs = [Dev((int(x) + 4) * 4) for x in k]
    for o in outs:
        mq.check(lib.mq_memset(o.ptr, 0x5A, o.nbytes, None))
    ptrs = (C.c_void_p * q)(*[o.ptr for o in outs])
    mq.check(lib.mq_shared_select_write(ws.ptr, ptrs, None))
    for j in range(q):
        got = outs[j].get(np.int32, int(k[j]) + 4)
        assert np.array_equal(got[:int(k[j])], want[j]), (kind, q, cus, twopass, j)
        assert np.all(got[int(k[j]):] == SENT), (kind, q, cus, twopass, j, "wrote past the list")


# ---------------------------------------------------------------------------
# d. k_group_dense: long chunks, runs of wave-uniform tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("keyset", ["sorted_runs", "uniform_100"])
def test_group_dense_long_chunks(lib, limit, keyset):
    """mq_group_plan / _write on the dense path with one limited CU: every block runs its
    unrolled loop many times. sorted_runs: 62 keys of [0, 2048), both ends among them,
    sorted, so most wave tiles hold one key and a run of them is folded in registers and
    flushed where the key changes, mid-tile; uniform_100: every row an LDS atomic."""
    limit(1)
    n = SCAN_N
    _, rpb = _geometry(lib, n)
    assert rpb >= 3 * 8192, rpb  # k_group_dense launches at most 4 blocks a CU: no fewer rows a block
    rng = np.random.default_rng(5)
    if keyset == "sorted_runs":
        picks = np.unique(np.concatenate([[0, 2047], rng.choice(2048, 60, replace=False)]))
        keys = np.sort(picks[rng.integers(0, len(picks), n)]).astype(np.int32)
        tiles = keys[: n // 256 * 256].reshape(-1, 256)
        assert (tiles.min(axis=1) == tiles.max(axis=1)).sum() > len(tiles) // 2
    else:
        keys = rng.integers(0, 100, n).astype(np.int32)
    assert gc.key_range(keys) <= lib.mq_group_dense_slots()
    vals = gc.values_of("uniform", keys)
    want = gc.group(keys, vals)
    names = ["keys", "count", "sum", "min", "max"]
    dtypes = [np.int32, np.uint64, np.int64, np.int32, np.int32]
    for ko, vo in ((0, 0), (1, 0), (0, 1)):
        dk, dv = Dev.of(keys, offset_elems=ko), Dev.of(vals, offset_elems=vo)
        h, groups, taken = C.c_void_p(), C.c_uint64(0), C.c_int(-1)
        mq.check(lib.mq_group_plan(dk.ptr, dv.ptr, n, None, mq.MQ_GROUP_AUTO, C.byref(h), C.byref(groups),
                                   C.byref(taken), None), "mq_group_plan")
        assert taken.value == mq.MQ_GROUP_DENSE and groups.value == len(want[0]), (keyset, ko, vo)
        g = groups.value
        outs = [Dev((g + 1) * np.dtype(t).itemsize) for t in dtypes]
        mq.check(lib.mq_group_write(h, *[o.ptr for o in outs], None), "mq_group_write")
        for nm, t, o, w in zip(names, dtypes, outs, want):
            assert np.array_equal(o.get(t, g), w), (keyset, ko, vo, nm)
        mq.check(lib.mq_group_free(h), "mq_group_free")


# ---------------------------------------------------------------------------
# e. the hook itself
# ---------------------------------------------------------------------------
def test_cu_limit_restores_and_never_raises(lib, limit, hardware):
    """After mq_test_set_cu_limit(0) mq_scan_geometry answers as before any limit; a
    limit above the hardware count changes nothing; a negative one is refused and leaves
    the limit as it was."""
    now = lambda: {n: _geometry(lib, n) for n in hardware}
    limit(1)
    assert now() != hardware and _geometry(lib, 1 << 30)[0] <= 8
    assert lib.mq_test_set_cu_limit(-1) == mq.MQ_EINVAL
    assert _geometry(lib, 1 << 30)[0] <= 8
    mq.check(lib.mq_test_set_cu_limit(0))
    assert now() == hardware
    mq.check(lib.mq_test_set_cu_limit(1 << 20))
    assert now() == hardware
    mq.check(lib.mq_test_set_cu_limit(0))
    assert now() == hardware
