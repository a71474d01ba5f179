"""The full-size regimes of the streaming kernels at small sizes, every comparison exact.

Every streaming kernel sizes its grid from the device's CU count, so on a 256-CU MI355X
a column of a few million rows leaves a block or wave almost no rows: k_scan's unrolled
main loop, k_select_stage's ring + spill and its switch to bitmap mode, the long
wave-chunks of shared select and of k_group_dense then run only in the 1e9-row tests,
which check properties on uniform data. mq_test_set_cu_limit (mq_device.h) lowers the CU
count the geometry uses; with 1, 2 or 7 CUs a column of 0.3-4 M rows gives each block
what a 1e9-row column gives it on the whole device. The grid-stride operators (fetch,
add / sub, gather, histogram, hashset lookup, and the insert and update kernels of
mq_dml.hip) take a second step of their loops only past 524 288 work items on the whole
device; under a limit a few thousand are enough. Expected values come from numpy, the
refcpu oracle, groupcases.py, dmlcases.py and insertcases.py; each test asserts first that
its regime is reached.
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
# e. the grid-stride operators: fetch, add / sub, gather, histogram, hashset lookup
#
# stream_grid launches min(ceil(work / 256), 8 x CUs) blocks of 256 threads, so under a
# limit the grid has S = lanes(cus) lanes and a lane's loop repeats once the work passes S
# items: on the whole device that takes 524 288.
# ---------------------------------------------------------------------------
PAD = 8  # sentinel words kept after every output


def lanes(cus):
    return 8 * cus * 256


def _refill(lib, d):
    mq.check(lib.mq_memset(d.ptr, 0x5A, d.nbytes, None), "mq_memset")


def _check_out(out, off, want, tag):
    """out holds `want` from word `off` on and 0x5A everywhere else."""
    got = out.get(np.int32, off + len(want) + PAD)
    assert np.array_equal(got[off:off + len(want)], want), tag
    assert np.all(got[:off] == SENT) and np.all(got[off + len(want):] == SENT), tag + ("wrote outside the output",)


_fetch_cache = {}


def _fetch_data():
    """A 500 000-row full-range column, aligned and +4 B, and the most positions any case
    uses (random with repeats), made once."""
    if not _fetch_cache:
        rng = np.random.default_rng(41)
        col = rng.integers(I32MIN, I32MAX, 500_000, dtype=np.int64, endpoint=True).astype(np.int32)
        col[:2], col[-2:] = (I32MIN, I32MAX), (I32MAX, I32MIN)
        kmax = 4 * (11 * lanes(max(LIMITS)) + 5) + 3
        pos = rng.integers(0, len(col), kmax).astype(np.int32)
        pos[::1001], pos[7::1001] = 0, len(col) - 1
        _fetch_cache.update(col=col, pos=pos, cols=[Dev.of(col), Dev.of(col, offset_elems=1)],
                            poss=[Dev.of(pos), Dev.of(pos, offset_elems=1)], out=Dev(4 * (kmax + 2 * PAD)))
    return _fetch_cache


@pytest.mark.parametrize("cus", LIMITS)
def test_fetch_unrolled_steps(lib, limit, cus):
    """k_fetch where its unrolled step (4 groups of 4 positions a lane), the one-group loop
    and the tail hand over to each other: k4 groups at and around 3S, 4S, between and far
    past, k = 4 k4 + {0, 3}; all pointers aligned (k_fetch<true>), the positions or the
    output alone 4 B off (k_fetch<false>), the column 4 B off; positions descending once."""
    limit(cus)
    S = lanes(cus)
    groups = [3 * S, 3 * S + 1, 4 * S, 4 * S + 1, 5 * S + S // 2, 11 * S + 5]
    # at 3S groups no lane takes the unrolled step and every lane the one-group loop 3 times;
    # from 3S + 1 on the unrolled step runs, at 11S + 5 twice and then the one-group loop
    assert min(groups) >= 3 * S and max(groups) > 2 * 4 * S + 3 * S
    c = _fetch_data()
    col, pos, out = c["col"], c["pos"], c["out"]
    # (column, positions, output) offsets in dwords
    layouts = {"aligned": (0, 0, 0), "pos +4 B": (0, 1, 0), "out +4 B": (0, 0, 1), "col +4 B": (1, 0, 0)}
    for k4 in groups:
        for r in (0, 3):
            k = 4 * k4 + r
            want = col[pos[:k]]
            for name, (co, po, oo) in layouts.items():
                _refill(lib, out)
                mq.check(lib.mq_fetch(c["cols"][co].ptr, c["poss"][po].ptr, k, out.ptr + 4 * oo, None), "mq_fetch")
                _check_out(out, oo, want, (cus, k4, r, name))
    k = 4 * groups[-1] + 3
    desc = np.sort(pos[:k])[::-1].copy()
    dd = Dev.of(desc)
    _refill(lib, out)
    mq.check(lib.mq_fetch(c["cols"][0].ptr, dd.ptr, k, out.ptr, None), "mq_fetch")
    _check_out(out, 0, col[desc], (cus, "descending"))


def test_fetch_at_row_base(lib, limit):
    """mq_fetch_at on a 50 000-row shard whose rows start at 1 000 003: out = shard[pos -
    row_base], past the unrolled step; row base 0 is mq_fetch; a negative one is refused."""
    limit(1)
    S = lanes(1)
    k = 4 * (4 * S + 1) + 3
    assert k // 4 > 3 * S
    rng = np.random.default_rng(43)
    shard = rng.integers(I32MIN, I32MAX, 50_000, dtype=np.int64, endpoint=True).astype(np.int32)
    local = rng.integers(0, len(shard), k).astype(np.int32)
    local[:4] = (0, len(shard) - 1, 0, len(shard) - 1)
    ds, out = Dev.of(shard), Dev(4 * (k + 2 * PAD))
    for base in (ROW_BASE, 0):
        dp = Dev.of(local + np.int32(base))
        _refill(lib, out)
        mq.check(lib.mq_fetch_at(ds.ptr, base, dp.ptr, k, out.ptr, None), "mq_fetch_at")
        _check_out(out, 0, shard[local], ("fetch_at", base))
        if base == 0:
            at = out.get(np.int32, k + PAD)
            _refill(lib, out)
            mq.check(lib.mq_fetch(ds.ptr, dp.ptr, k, out.ptr, None), "mq_fetch")
            assert np.array_equal(out.get(np.int32, k + PAD), at)
    _refill(lib, out)
    assert lib.mq_fetch_at(ds.ptr, -1, dp.ptr, k, out.ptr, None) == mq.MQ_EINVAL
    assert np.all(out.get(np.int32, k + PAD) == SENT)


ADDSUB_PAIRS = [(I32MIN, I32MIN), (I32MAX, I32MAX), (I32MIN, I32MAX), (I32MAX, I32MIN), (-1, I32MIN)]
_addsub_cache = {}


def _addsub_data(refcpu, n, S):
    """Full-range a and b of n rows with the wrap-around pairs planted in every sweep of
    4 S rows (from its row 6 on, across two groups of 4), and the oracle's a + b and a - b."""
    if n not in _addsub_cache:
        rng = np.random.default_rng(n)
        a = rng.integers(I32MIN, I32MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
        b = rng.integers(I32MIN, I32MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
        planted = 0
        for at in range(6, n - len(ADDSUB_PAIRS) + 1, 4 * S):
            for j, (x, y) in enumerate(ADDSUB_PAIRS):
                a[at + j], b[at + j] = x, y
            planted += 1
        assert planted >= n // (4 * S)
        _addsub_cache[n] = (a, b, refcpu.add(a, b), refcpu.sub(a, b))
    return _addsub_cache[n]


@pytest.mark.parametrize("layout", ["aligned", "a +4 B", "b +4 B", "out +4 B"])
def test_add_sub_sweeps_and_layouts(lib, refcpu, limit, layout):
    """mq_add and mq_sub over one to six sweeps of the grid with all pointers 16-byte aligned
    (k_addsub<*, true>) and with a, b or the output alone 4 B off (k_addsub<*, false>, the
    scalar instance), two's-complement wrap at the INT32 extremes in every sweep."""
    limit(1)
    S = lanes(1)
    sizes = [4 * S, 4 * S + 1, 4 * (2 * S + 1) + 3, 4 * (5 * S + 77) + 2]
    assert min(sizes) // 4 >= S and max(sizes) // 4 > 5 * S  # the grid is full; up to 6 sweeps
    ao, bo, oo = {"aligned": (0, 0, 0), "a +4 B": (1, 0, 0), "b +4 B": (0, 1, 0), "out +4 B": (0, 0, 1)}[layout]
    for n in sizes:
        a, b, want_add, want_sub = _addsub_data(refcpu, n, S)
        assert np.array_equal(want_add, (a.astype(np.int64) + b).astype(np.int32))  # the oracle wraps
        da, db, out = Dev.of(a, offset_elems=ao), Dev.of(b, offset_elems=bo), Dev(4 * (n + 2 * PAD))
        for fn, want in ((lib.mq_add, want_add), (lib.mq_sub, want_sub)):
            _refill(lib, out)
            mq.check(fn(da.ptr, db.ptr, n, out.ptr + 4 * oo, None), "mq_add/mq_sub")
            _check_out(out, oo, want, (layout, n, "add" if fn is lib.mq_add else "sub"))


@pytest.mark.parametrize("cus", [1, 2])
def test_gather_u64_full_steps(lib, limit, cus):
    """k_gather_u64 around one full grid step of G = lanes x 8 rows and past three: its
    unguarded main loop repeats and the guarded last step follows it."""
    limit(cus)
    G = lanes(cus) * 8
    assert G == 8 * cus * 2048
    sizes = [G - 1, G, G + 1, 3 * G + 2049]
    assert max(sizes) > 3 * G + 7 * 256  # some lanes take a fourth full step
    rng = np.random.default_rng(47 + cus)
    col = rng.integers(I32MIN, I32MAX, 300_000, dtype=np.int64, endpoint=True).astype(np.int32)
    pos = rng.integers(0, len(col), max(sizes)).astype(np.uint64)
    pos[:2], pos[-2:] = (0, len(col) - 1), (len(col) - 1, 0)
    dc, dp, out = Dev.of(col), Dev.of(pos), Dev(4 * (max(sizes) + 2 * PAD))
    for n in sizes:
        _refill(lib, out)
        mq.check(lib.mq_gather_u64(dc.ptr, dp.ptr, n, out.ptr, None), "mq_gather_u64")
        _check_out(out, 0, col[pos[:n].astype(np.int64)], (cus, n))


def test_histogram_many_sweeps(lib, refcpu, limit):
    """k_histogram where every lane counts 146 rows: the (min, bin) pairs of
    test_gather_and_histogram_vs_oracle, and a full-range column binned from INT32_MIN."""
    limit(1)
    n = 300_000
    assert n > 100 * lanes(1)
    rng = np.random.default_rng(9)
    col = rng.integers(-10**6, 10**6, n).astype(np.int32)
    wide = _wide(n, 53)
    cases = [(col, int(col.min()), (int(col.max()) - int(col.min())) // 99), (col, 0, 7), (col, -10, -3),
             (wide, I32MIN, 43_383_508)]
    h = Dev(8 * (101 + 2))
    dcs = {id(col): Dev.of(col), id(wide): Dev.of(wide)}
    for c, mn, bs in cases:
        assert bs not in (0, -1)  # INT32_MIN / -1 traps in the oracle
        _refill(lib, h)
        mq.check(lib.mq_histogram(dcs[id(c)].ptr, n, mn, bs, h.ptr, None), "mq_histogram")
        got = h.get(np.uint64, 103)
        want = refcpu.histogram(c, mn, bs)
        assert int(want.sum()) == n
        assert np.array_equal(got[:101], want), (mn, bs)
        assert np.all(got[101:] == np.uint64(0x5A5A5A5A5A5A5A5A)), (mn, bs, "wrote past the counts")


def test_hashset_lookup_many_sweeps(lib, refcpu, limit):
    """k_hashset_lookup on 300 000 probes (146 a lane): members, keys that share a member's
    home slot, non-members, 0 and negatives, on the tables of hashsetcases.py that are at
    most half full, against the restatement's lookup."""
    import hashsetcases as hc
    limit(1)
    nprobe = 300_000
    assert nprobe > 100 * lanes(1)
    tables = {name: (size, keys) for name, (size, keys) in hc.LISTS.items()
              if len({int(k) for k in keys} - {0}) * 2 <= size}
    assert len(tables) >= 3, sorted(tables)
    found = Dev(nprobe + 16)
    for name, (size, keys) in sorted(tables.items()):
        t = hc.expected_table(refcpu, size, keys)
        rng = np.random.default_rng(size)
        members = np.array([k for k in keys if k != 0], dtype=np.int64)
        pool = np.concatenate([members, members + size, members - size, members + 7 * size, -members,
                               rng.integers(I32MIN, I32MAX, 4000, endpoint=True), np.arange(-50, 50),
                               [0, I32MIN, I32MAX, I32MIN + 1, size, -size]])
        pool = pool[(pool >= I32MIN) & (pool <= I32MAX)].astype(np.int32)
        probes = pool[rng.integers(0, len(pool), nprobe)]
        probes[:len(pool)] = pool
        answer = {int(k): refcpu.hashset_lookup(t, int(k)) for k in np.unique(probes)}
        want = np.array([answer[int(k)] for k in probes.tolist()], dtype=np.uint8)
        assert 0 < want.sum() < nprobe and all(answer[int(k)] for k in members)
        dt, dp = Dev.of(t), Dev.of(probes)
        _refill(lib, found)
        mq.check(lib.mq_hashset_lookup(dt.ptr, size, dp.ptr, nprobe, found.ptr, None), "mq_hashset_lookup")
        got = found.get(np.uint8, nprobe + 16)
        assert np.array_equal(got[:nprobe], want), name
        assert np.all(got[nprobe:] == 0x5A), (name, "wrote past the answers")


# ---------------------------------------------------------------------------
# f. the grid-stride insert and update operators: k_ins_points, k_ins_slots,
#    k_ins_positions, k_ins_index, k_dml_update
#
# The same stream_grid loops: with one limited CU the grid has lanes(1) = 2048 lanes, and a
# few tens of thousands of items give every lane more than 10 steps and a ragged last one.
# ---------------------------------------------------------------------------
def _many_steps(*counts):
    S = lanes(1)
    for c in counts:
        assert c > 10 * S and c % S not in (0, S - 1), (c, S)  # every lane past 10 steps; a ragged last step


def test_insert_points_many_steps(lib, limit):
    """mq_insert_points of 25 003 sorted new keys into 60 001 old ones with duplicates and
    both INT32 ends, against np.searchsorted."""
    limit(1)
    n, k = 60_001, 25_003
    _many_steps(k)
    rng = np.random.default_rng(61)
    old = rng.integers(-4000, 4000, n) * 3
    old[:2], old[-2:] = I32MIN, I32MAX
    old = np.sort(old).astype(np.int32)
    new = np.concatenate([rng.integers(-12_500, 12_500, k - 6), [I32MIN, I32MIN, I32MAX, I32MAX, -12_001, 12_001]])
    new = np.sort(new).astype(np.int32)
    dold, dnew, dins = Dev.of(old), Dev.of(new), Dev(4 * (k + PAD))
    _refill(lib, dins)
    mq.check(lib.mq_insert_points(dold.ptr, n, dnew.ptr, k, dins.ptr, None), "mq_insert_points")
    got = dins.get(np.uint32, k + PAD)
    assert np.array_equal(got[:k], np.searchsorted(old, new, side="right"))
    assert np.all(got[k:] == SENT), "wrote past the points"


def test_insert_index_slots_positions_many_steps(lib, limit):
    """test_gpu_insert's index merge (mq_insert_slots with an order, mq_insert_positions
    from slots and from a base, mq_insert_index with and without renumbering) with 30 011
    new entries on 45 007 old ones: 75 018 slots, 36 steps a lane. Then mq_insert_slots
    without an order."""
    from test_gpu_insert import check_insert_index
    limit(1)
    n, k = 45_007, 30_011
    _many_steps(k, n + k)
    check_insert_index(lib, n, k)
    ins = np.sort(np.random.default_rng(67).integers(0, n + 1, k)).astype(np.uint32)
    dins, dslots = Dev.of(ins), Dev(8 * (k + PAD))
    _refill(lib, dslots)
    mq.check(lib.mq_insert_slots(dins.ptr, None, k, dslots.ptr, None), "mq_insert_slots")
    got = dslots.get(np.uint64, k + PAD)
    assert np.array_equal(got[:k], ins.astype(np.uint64) + np.arange(k, dtype=np.uint64))
    assert np.all(got[k:] == np.uint64(0x5A5A5A5A5A5A5A5A)), "wrote past the slots"


def test_update_rows_many_steps(lib, limit):
    """mq_update_rows with 40 009 ids (repeats, five of them outside the column) on 100 003
    rows: the listed rows change, no other does, the ids outside are counted."""
    import dmlcases as dc
    limit(1)
    n, k = 100_003, 40_009
    _many_steps(k)
    rng = np.random.default_rng(71)
    col = dc.table(n, 1)[0]
    ids = rng.integers(0, n, 30_003).astype(np.int32)
    ids = np.concatenate([ids, ids[::3]])  # repeats
    assert len(ids) == k - 5
    wild = np.concatenate([ids, [-1, n, n + 1, I32MAX, I32MIN]]).astype(np.int32)
    rng.shuffle(wild)
    # the steps touch disjoint rows: a step that repeated another would leave rows unchanged
    assert len(np.unique(wild[-lanes(1):])) > lanes(1) // 2
    d, dp, bad = Dev.of(np.concatenate([col, [4242, 4242]]).astype(np.int32)), Dev.of(wild), Dev.of(np.array([99], np.uint64))
    mq.check(lib.mq_update_rows(d.ptr, n, dp.ptr, k, -10, bad.ptr, None), "mq_update_rows")
    got = d.get(np.int32, n + 2)
    assert np.array_equal(got[:n], dc.update_rows(col, ids, -10)) and np.all(got[n:] == 4242)
    assert bad.get(np.uint64, 1)[0] == 5


# ---------------------------------------------------------------------------
# g. the hook itself
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
