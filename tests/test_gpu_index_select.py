"""mq_index_select (k_index_bounds + k_index_copy, csrc/mq_kernels.hip) against the oracle's
restatement of the sorted-index select (refcpu.index_select, pinned to the reference's own
select_column_sorted_index in test_oracle_index.py). Every comparison is exact equality.
Every output is pre-filled with 0x5A bytes and compared whole, so a word written past the
selected run fails like a wrong position does.

No run of equal values is longer than 4096 rows (4097 in the all-equal column of that
size): k_index_bounds walks a run of `low` or `high` on one lane, and what a longer run
costs has not been measured.
"""
import ctypes as C

import numpy as np
import pytest

from devbuf import Dev
from refapi import mq

pytestmark = pytest.mark.gpu

I32MIN, I32MAX = -(2 ** 31), 2 ** 31 - 1
SENT = 0x5A5A5A5A              # what mq_memset(0x5A) leaves in an int32
SENT64 = 0x5A5A5A5A5A5A5A5A
PAD = 4                        # sentinel words kept after each query's n output words
SIZES = [0, 1, 2, 63, 64, 65, 4097, 100_003]
MAX_RUN = 4096
LANES_1CU = 8 * 256            # k_index_copy's lanes under a CU limit of 1 (stream_grid)


@pytest.fixture(scope="module")
def lib():
    L = mq.load()
    mq.check(L.mq_init(0), "mq_init")
    return L


# ---------------------------------------------------------------------------
# columns (sorted values) and bounds
# ---------------------------------------------------------------------------
def _ascending(count, rng):
    """count strictly ascending int32 with gaps of 2..4 (so v - 1 and v + 1 are absent),
    negative and positive."""
    return (np.cumsum(rng.integers(2, 5, count)) - 2 * count).astype(np.int32)


def _runs(n, rng):
    """Runs of 1..4096 equal values, longer ones the more rows there are: from 8192 rows on
    a single row and a run of exactly 4096 come first, so a walk over a whole longest run
    starts at row 1."""
    small = [1, 1, 2, 3, 5, 17]
    lengths = [1, MAX_RUN] if n >= 2 * MAX_RUN else []
    pick = small if n <= 65 else small + [64, 257, 1000] if n < 2 * MAX_RUN else small + [64, 257, 1000, MAX_RUN]
    while sum(lengths) < n:
        lengths.append(int(rng.choice(pick)))
    v = np.repeat(_ascending(len(lengths), rng), lengths)[:n]
    return np.ascontiguousarray(v)


_columns = {}


def columns(n):
    """name -> sorted int32 values of n rows; made once per n, never changed."""
    if n not in _columns:
        rng = np.random.default_rng(1000 + n)
        c = {"distinct": _ascending(n, rng), "runs": _runs(n, rng)}
        if n <= 4097:
            c["equal"] = np.full(n, 7, dtype=np.int32)
        if n == 1:
            c["int32_min"] = np.array([I32MIN], dtype=np.int32)
            c["int32_max"] = np.array([I32MAX], dtype=np.int32)
        else:
            e = _runs(n, rng)
            e[0], e[-1] = I32MIN, I32MAX
            c["extremes"] = e
        for name, v in c.items():
            assert len(v) == n and np.all(v[1:] >= v[:-1]), name
            edges = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1], [True]]))
            # the all-equal column of 4097 rows is the one run a row longer than the rest
            assert np.diff(edges).max() <= (MAX_RUN + 1 if name == "equal" else MAX_RUN), name
        _columns[n] = c
    return _columns[n]


def permutation(n):
    return np.random.default_rng(7 * n + 1).permutation(n).astype(np.uint64)


def _clip(cands):
    return sorted({int(c) for c in cands if I32MIN <= c <= I32MAX})


def all_pairs(v):
    """n <= 65: every value present, each -1 and +1, INT32_MIN and INT32_MAX, in all pairs."""
    cand = _clip([int(x) + d for x in np.unique(v) for d in (-1, 0, 1)] + [I32MIN, I32MAX])
    return [(lo, hi) for lo in cand for hi in cand]


def special_pairs(v):
    """The cases by name, where the column allows them (a column that starts at INT32_MIN has
    nothing below its first value)."""
    u = np.unique(v)
    v0, vmax, mid = int(u[0]), int(u[-1]), int(u[len(u) // 2])
    s = {"low == high present": (mid, mid), "low > high": (int(v[3 * len(v) // 4]), int(v[len(v) // 4]))}
    if mid - 1 not in u and mid - 1 >= I32MIN:
        s["high present, [low, high) empty"] = (mid - 1, mid)
    if v0 > I32MIN:
        s["low below the first value"] = (v0 - 1, mid)
        s["high below the first value"] = (mid, v0 - 1)
        s["both below the first value"] = (v0 - 1, v0 - 1)
    if vmax < I32MAX - 1:
        s["both above the last value"] = (vmax + 1, vmax + 2)
    s["everything"] = (I32MIN, I32MAX)
    return s


def seeded_pairs(v, seed):
    """64 pairs: bounds at present values and their neighbours (run edges), low <= high mostly,
    and 8 drawn from the whole int32 range."""
    rng = np.random.default_rng(seed)
    a = v[rng.integers(0, len(v), 56)].astype(np.int64) + rng.integers(-1, 2, 56)
    b = v[rng.integers(0, len(v), 56)].astype(np.int64) + rng.integers(-1, 2, 56)
    swap = (a > b) & (rng.random(56) < 0.8)
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    wide = rng.integers(I32MIN, I32MAX, (8, 2), endpoint=True)
    pairs = [(int(x), int(y)) for x, y in zip(np.clip(a, I32MIN, I32MAX), np.clip(b, I32MIN, I32MAX))]
    return pairs + [(int(x), int(y)) for x, y in wide]


def bounds_for(v, seed):
    if len(v) <= 65:
        return all_pairs(v)
    return seeded_pairs(v, seed) + list(special_pairs(v).values())


# ---------------------------------------------------------------------------
# running a batch of queries
# ---------------------------------------------------------------------------
class Index:
    """One sorted index on the device and the buffers for batches of queries on it."""

    def __init__(self, lib, refcpu, values, positions, batch):
        self.lib, self.refcpu = lib, refcpu
        self.values, self.positions, self.n = values, positions, len(values)
        self.dv, self.dp = Dev.of(values), Dev.of(positions)
        self.slot = self.n + PAD
        self.batch = batch
        self.out = Dev(4 * self.slot * batch)
        self.cnt = Dev(8 * (batch + 1))

    def check(self, pairs, tag):
        for at in range(0, len(pairs), self.batch):
            self._check(pairs[at:at + self.batch], tag)

    def _check(self, pairs, tag):
        L, n, slot, q = self.lib, self.n, self.slot, len(pairs)
        mq.check(L.mq_memset(self.out.ptr, 0x5A, 4 * slot * q, None), "mq_memset")
        mq.check(L.mq_memset(self.cnt.ptr, 0x5A, 8 * (q + 1), None), "mq_memset")
        for j, (lo, hi) in enumerate(pairs):
            rc = L.mq_index_select(self.dv.ptr, self.dp.ptr, n, lo, hi, self.out.ptr + 4 * slot * j,
                                   self.cnt.ptr + 8 * j, None)
            assert rc == mq.MQ_OK, tag + (lo, hi, L.mq_last_error())
            if j % 16 == 15:  # keeps the calls in flight, and so the pool's scratch blocks, few
                mq.check(L.mq_stream_sync(None), "sync")
        want = np.full(slot * q, SENT, dtype=np.int32)
        want_k = np.full(q + 1, SENT64, dtype=np.uint64)
        for j, (lo, hi) in enumerate(pairs):
            w = self.refcpu.index_select(self.values, self.positions, lo, hi)
            want[slot * j:slot * j + len(w)] = w
            want_k[j] = len(w)
        got_k = self.cnt.get(np.uint64, q + 1)
        if not np.array_equal(got_k, want_k):
            j = int(np.flatnonzero(got_k != want_k)[0])
            raise AssertionError(tag + ("count", pairs[j] if j < q else "past the counts", int(got_k[j]), int(want_k[j])))
        got = self.out.get(np.int32, slot * q)
        if not np.array_equal(got, want):
            j = int(np.flatnonzero(got != want)[0]) // slot
            k = int(want_k[j])
            g = got[slot * j:slot * (j + 1)]
            what = "positions" if not np.array_equal(g[:k], want[slot * j:slot * j + k]) else "wrote past the run"
            raise AssertionError(tag + (what, pairs[j], k))


def _batch_for(n):
    return max(1, min(4096, (32 << 20) // (4 * (n + PAD))))  # at most 32 MiB of outputs a batch


@pytest.mark.parametrize("n", SIZES)
def test_index_select_vs_oracle(lib, refcpu, n):
    """Every column kind at n rows, positions a seeded permutation. n <= 65: all pairs of the
    values present, their neighbours and the INT32 extremes; above: 64 seeded pairs and the
    named cases. n = 0 runs with NULL pointers and selects nothing."""
    if n == 0:
        cnt = Dev(16)
        for lo, hi in ((0, 10), (I32MIN, I32MAX), (5, 5), (7, 3)):
            mq.check(lib.mq_memset(cnt.ptr, 0x5A, 16, None), "mq_memset")
            mq.check(lib.mq_index_select(None, None, 0, lo, hi, None, cnt.ptr, None), "mq_index_select")
            assert cnt.get(np.uint64, 2).tolist() == [0, SENT64], (lo, hi)
        return
    pos = permutation(n)
    named = set()
    for name, v in columns(n).items():
        pairs = bounds_for(v, seed=n)
        if n > 65:
            named |= set(special_pairs(v))
        Index(lib, refcpu, v, pos, _batch_for(n)).check(pairs, (n, name))
    if n > 65:  # every named case ran on some column of this size
        assert named >= {"low == high present", "high present, [low, high) empty", "low > high",
                         "low below the first value", "high below the first value",
                         "both above the last value"}, named


def test_index_select_truncates_wide_positions(lib, refcpu):
    """size_t positions at 2^31 and above 2^32: the output is their (int) truncation, as the
    reference's int result array holds them."""
    n = 4097
    v = columns(n)["runs"]
    pos = permutation(n)
    pos[0::3] += np.uint64(1 << 31)
    pos[1::3] += np.uint64((1 << 32) + 5)
    pos[2::7] += np.uint64(3 << 33)
    pos[n // 2] = np.uint64(1 << 31)
    assert (pos.astype(np.int32) < 0).any() and (pos > np.uint64(1 << 32)).any()
    Index(lib, refcpu, v, pos, _batch_for(n)).check(bounds_for(v, seed=99), ("wide positions",))


def test_index_copy_many_sweeps(lib, refcpu):
    """k_index_copy's grid-stride loop past 20 sweeps: 100 003 rows under a CU limit of 1
    (2048 lanes) and ranges that select at least 50 000 rows."""
    n = 100_003
    pos = permutation(n)
    mq.check(lib.mq_device_sync(), "mq_device_sync")
    mq.check(lib.mq_test_set_cu_limit(1), "mq_test_set_cu_limit")
    try:
        for name in ("runs", "distinct"):
            v = columns(n)[name]
            lo, hi = int(v[n // 4]), int(v[n // 4 + 60_000])
            pairs = [(lo, hi), (lo - 1, hi + 1), (I32MIN, I32MAX), (int(v[0]), int(v[-1]))]
            for a, b in pairs:
                k = len(refcpu.index_select(v, pos, a, b))
                assert k >= 50_000 and k > 20 * LANES_1CU, (name, a, b, k)
            Index(lib, refcpu, v, pos, len(pairs)).check(pairs, ("sweeps", name))
    finally:
        lib.mq_device_sync()
        mq.check(lib.mq_test_set_cu_limit(0), "mq_test_set_cu_limit(0)")


def test_index_select_two_streams_one_thread(lib, refcpu):
    """One thread queues mq_index_select on stream A and, before A has run, on stream B with
    another range, 8 rounds: each call's {first row, K} hand-over between its two kernels is
    its own, so both outputs are right. (With one shared hand-over buffer the second call's
    bounds could replace the first's before its copy had read them; whether they did was a
    matter of timing.)"""
    n = 100_003
    v, pos = columns(n)["runs"], permutation(n)
    dv, dp = Dev.of(v), Dev.of(pos)
    sa, sb = C.c_void_p(), C.c_void_p()
    mq.check(lib.mq_stream_create(C.byref(sa)), "mq_stream_create")
    mq.check(lib.mq_stream_create(C.byref(sb)), "mq_stream_create")
    outs = [Dev(4 * (n + PAD)), Dev(4 * (n + PAD))]
    cnts = [Dev(16), Dev(16)]
    rng = np.random.default_rng(5)
    try:
        for rnd in range(8):
            a0, b0 = int(rng.integers(0, n // 2)), int(rng.integers(0, n // 2))
            ranges = [(int(v[a0]), int(v[a0 + n // 3 + rnd])), (int(v[b0]) + 1, int(v[b0 + n // 2 - rnd]))]
            assert ranges[0] != ranges[1]
            for st, out, cnt in zip((sa, sb), outs, cnts):
                mq.check(lib.mq_memset(out.ptr, 0x5A, 4 * (n + PAD), st), "mq_memset")
                mq.check(lib.mq_memset(cnt.ptr, 0x5A, 16, st), "mq_memset")
            for st, out, cnt, (lo, hi) in zip((sa, sb), outs, cnts, ranges):
                mq.check(lib.mq_index_select(dv.ptr, dp.ptr, n, lo, hi, out.ptr, cnt.ptr, st), "mq_index_select")
            mq.check(lib.mq_stream_sync(sa), "sync A")
            mq.check(lib.mq_stream_sync(sb), "sync B")
            for which, out, cnt, (lo, hi) in zip("AB", outs, cnts, ranges):
                w = refcpu.index_select(v, pos, lo, hi)
                assert len(w) > 10_000, (rnd, which, len(w))
                assert cnt.get(np.uint64, 2).tolist() == [len(w), SENT64], (rnd, which, lo, hi)
                got = out.get(np.int32, n + PAD)
                assert np.array_equal(got[:len(w)], w), (rnd, which, lo, hi)
                assert np.all(got[len(w):] == SENT), (rnd, which, lo, hi, "wrote past the run")
    finally:
        mq.check(lib.mq_stream_destroy(sa), "mq_stream_destroy")
        mq.check(lib.mq_stream_destroy(sb), "mq_stream_destroy")
