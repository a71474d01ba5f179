"""hash join: a numpy model of the operator and the named inputs, shared by the host and
GPU tests of the join (mq_join_*, mq_hash_join, mq_pjoin_place, mq_shard_join).

The model is the reference's output contract (query.c:652-696 over multimap.c) stated
without a table: pairs in probe-major order and, for one probe row, the build rows with
its key in ascending build row order (the multimap's insertion order). It has no loop
over rows, so it also serves inputs the oracle's restated `key % size` multimap is too
slow for. tests/test_join_host.py pins it to the oracle on the CPU.
"""
from __future__ import annotations

import numpy as np

K_LONG_RUN = 4096      # mq_join.hip / mq_pjoin.hip: a longer run is listed for a block ...
K_LONG_CHUNK = 65536   # ... as chunks of this many pairs
HOT_LENGTHS = (4096, 4097, 65536, 65537, 131073)  # 0, 1, 1, 2 and 3 list entries
HOT_ROWS = 3           # probe rows per hot key


def long_entries(lengths) -> int:
    """Entries the per-row write lists for rows with these pair counts."""
    L = np.asarray(lengths, dtype=np.int64)
    return int(((L[L > K_LONG_RUN] + K_LONG_CHUNK - 1) // K_LONG_CHUNK).sum())


def _i32(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x).astype(np.int32))


def _runs(c1, c2):
    """The stable key order of the build rows and, per probe row, its run [lo, hi) in it."""
    c1, c2 = np.asarray(c1, dtype=np.int32), np.asarray(c2, dtype=np.int32)
    order = np.argsort(c1, kind="stable")
    s = c1[order]
    return order, np.searchsorted(s, c2, side="left"), np.searchsorted(s, c2, side="right")


def join_counts(c1, c2) -> np.ndarray:
    """Per probe row, the number of build rows with its key."""
    _, lo, hi = _runs(c1, c2)
    return (hi - lo).astype(np.uint32)


def join_pairs(c1, p1, c2, p2):
    """(out1, out2): p1 of the build row and p2 of the probe row of every pair."""
    order, lo, hi = _runs(c1, c2)
    cnt = hi - lo
    m = int(cnt.sum())
    first = np.cumsum(cnt) - cnt  # a probe row's first pair
    src = np.repeat(lo - first, cnt) + np.arange(m, dtype=np.int64)
    return _i32(np.asarray(p1)[order[src]]), _i32(np.repeat(np.asarray(p2), cnt))


def place(cntp, out1p, inv, p2):
    """mq_pjoin_place in closed form: row r has cntp[inv[r]] pairs, which lie in the
    partitioned stream out1p behind those of the partitioned rows before inv[r]; the
    output holds the rows' pairs in row order, out2 = p2[r]."""
    cntp = np.asarray(cntp).astype(np.int64)
    inv = np.asarray(inv).astype(np.int64)
    poff = np.cumsum(cntp) - cntp
    cnt_row = cntp[inv]
    m = int(cnt_row.sum())
    roff = np.cumsum(cnt_row) - cnt_row
    src = np.repeat(poff[inv] - roff, cnt_row) + np.arange(m, dtype=np.int64)
    return _i32(np.asarray(out1p)[src]), _i32(np.repeat(np.asarray(p2), cnt_row))


# ---------------------------------------------------------------------------
# the inputs of test_hash_join_vs_oracle (tests/test_gpu_parity.py), which builds them
# from here with its own generator
# ---------------------------------------------------------------------------
ORACLE_CASES = ["unique", "dups", "skew", "neg", "tiny", "empty", "marker", "unique_partitioned",
                "dups_partitioned", "ragged_hits", "dups_short_runs", "dups_run_of_15"]
# the ones small enough for the host test (the partitioned pair has 5 M build rows)
HOST_ORACLE_CASES = ["unique", "dups", "skew", "neg", "tiny", "empty", "marker", "ragged_hits",
                     "dups_run_of_15"]


def oracle_inputs(case: str, rng, gen_join=None):
    """(c1, p1, c2, p2) of a named case, drawn from rng in a fixed order. gen_join:
    refcpu.gen_join, for the two partitioned cases."""
    if case == "unique":
        c1 = rng.permutation(200_000).astype(np.int32)
        c2 = rng.integers(0, 400_000, 150_000, dtype=np.int32)
    elif case == "dups":
        c1 = rng.integers(0, 5000, 100_000, dtype=np.int32)
        c2 = rng.integers(0, 6000, 30_000, dtype=np.int32)
    elif case == "skew":  # one huge group plus a long tail
        c1 = np.where(rng.random(50_000) < 0.5, 7, rng.integers(0, 10 ** 6, 50_000)).astype(np.int32)
        c2 = np.concatenate([[7, 7, 3], rng.integers(0, 10 ** 6, 2000)]).astype(np.int32)
    elif case == "neg":
        c1 = rng.integers(-(2 ** 31), 2 ** 31 - 1, 20_000, dtype=np.int64).astype(np.int32)
        c1[:4] = [-(2 ** 31), 2 ** 31 - 1, 0, -1]
        c2 = np.concatenate([c1[::3], rng.integers(-100, 100, 500)]).astype(np.int32)
    elif case == "tiny":  # the reference's full-table hang shapes (multimap.c:65-71)
        c1 = np.array([5, 9], dtype=np.int32)
        c2 = np.array([1, 9, 5, 5, 2], dtype=np.int32)
    elif case == "marker":  # unique keys, one build row {key -1, position -1} = the
        c1 = (rng.permutation(3000) - 1500).astype(np.int32)  # packed table's empty word
        c2 = rng.integers(-1600, 1600, 5000, dtype=np.int32)
    elif case == "ragged_hits":  # unique keys, probe rows 64k+1 with hits at the word edges
        c1 = rng.permutation(1000).astype(np.int32)
        c2 = np.concatenate([np.arange(129), rng.integers(500, 2000, 64 * 7 + 1), [999]]).astype(np.int32)
    elif case == "dups_short_runs":  # > 2^16 rows, runs of 1..14 rows in input order
        # (spread keys: the oracle's `key % size` multimap goes quadratic on dense ones)
        keys = rng.choice(1 << 30, 90_000, replace=False).astype(np.int32)
        c1 = np.repeat(keys[:60_000], rng.integers(1, 15, 60_000))[:300_000]
        c1 = c1[rng.permutation(len(c1))]
        c2 = np.concatenate([rng.choice(keys[:60_000], 100_000), keys[60_000:80_000]]).astype(np.int32)
    elif case == "dups_run_of_15":  # one key on 15 rows: not packable, the window flags
        keys = rng.choice(1 << 30, 250_000, replace=False).astype(np.int32)
        c1 = keys[:200_000].copy()
        c1[1 + rng.choice(len(c1) - 1, 14, replace=False)] = c1[0]
        c2 = rng.choice(keys, 100_000)
        c2[:5] = c1[0]
    elif case in ("unique_partitioned", "dups_partitioned"):
        # > 2^22 build rows: the window-partitioned insert. Keys from the spread
        # config-5 generator: the oracle restates the reference's `key % size`
        # multimap, which goes quadratic on dense or arithmetic key runs.
        c1 = rng.permutation(gen_join(5_000_000, "build"))
        c2 = gen_join(3_000_000, "probe")
        if case == "dups_partitioned":  # one duplicate, seen only after partitioning
            c1[4_999_999] = c1[17]
    else:
        c1 = np.array([], dtype=np.int32)
        c2 = np.array([1, 2], dtype=np.int32)
    p1 = rng.integers(0, 10 ** 7, len(c1), dtype=np.int32)
    p2 = rng.integers(0, 10 ** 7, len(c2), dtype=np.int32)
    if case == "marker":
        p1[np.nonzero(c1 == -1)[0][0]] = -1
    return c1, p1, c2, p2


def named_inputs(case: str):
    """oracle_inputs with the case's own fixed seed (the host test and the regime tests)."""
    return oracle_inputs(case, np.random.default_rng(1000 + ORACLE_CASES.index(case)))


# ---------------------------------------------------------------------------
# three inputs of test_hash_join_partitioned_probe (unique builds of 200 003 spread keys),
# restated for the many-sweeps test with the probe side cut to 150 001 rows (fewer than the
# build's, so that MQ_JOIN_PART_DIV=1 still stores the windows as the global table)
# ---------------------------------------------------------------------------
PROBE_CASES = ["n2_4097", "one_pass", "dup_probed"]


def probe_inputs(case: str, gen_join):
    rng = np.random.default_rng(2000 + PROBE_CASES.index(case))
    n1 = 200_003
    c1 = rng.permutation(gen_join(n1, "build"))
    if case == "n2_4097":
        n2 = 4097
        c2 = np.concatenate([rng.choice(c1, n2 // 2), rng.integers(-2 ** 31, 2 ** 31 - 1, n2 - n2 // 2)])
        c2 = c2.astype(np.int64).astype(np.int32)[rng.permutation(n2)]
    elif case == "dup_probed":  # one key on two build rows, met by the probe's last row
        c1[n1 - 5] = c1[100]
        c2 = rng.choice(c1, 150_000)
        c2 = np.concatenate([c2, [c1[100]]]).astype(np.int32)
    else:  # one_pass: about half the rows hit
        c2 = np.concatenate([rng.choice(c1, 70_000), gen_join(1 << 20, "probe")[:80_001]]).astype(np.int32)
        c2 = c2[rng.permutation(len(c2))]
    p1 = rng.integers(-10 ** 7, 10 ** 7, len(c1), dtype=np.int32)
    p2 = rng.integers(0, 10 ** 7, len(c2), dtype=np.int32)
    return c1, p1, c2, p2


# ---------------------------------------------------------------------------
# hot keys: runs at and around the long-run limit and the chunk size
# ---------------------------------------------------------------------------
def hot_rows(n2: int) -> np.ndarray:
    """The probe rows of the hot keys, [key, occurrence]: the first occurrences share one
    64-row word (rows 640..644), the second end a word each in five different 256-row
    blocks, the third start a word each, the last of them in the ragged last word."""
    rows = np.empty((len(HOT_LENGTHS), HOT_ROWS), dtype=np.int64)
    for i in range(len(HOT_LENGTHS)):
        rows[i] = [640 + i, 5_055 + 1_024 * i, (n2 - 1) // 64 * 64 - 2_048 * (4 - i)]
    return rows


_hot = None


def hot_keys():
    """(c1, p1, c2, p2, info). Build: five keys on HOT_LENGTHS rows each, scattered by a
    permutation among 60 000 spread filler keys on 1 to 3 rows. Probe: 20 001 rows, each hot
    key on HOT_ROWS of them (hot_rows), the rest filler hits and keys never built. Computed
    once; callers must not modify it."""
    global _hot
    if _hot is None:
        rng = np.random.default_rng(4096)
        keys = rng.choice(1 << 30, 80_000 + len(HOT_LENGTHS), replace=False).astype(np.int32)
        hot, filler, absent = keys[:5], keys[5:60_005], keys[60_005:]
        reps = rng.integers(1, 4, len(filler))
        c1 = np.concatenate([np.repeat(filler, reps), np.repeat(hot, HOT_LENGTHS)])
        c1 = c1[rng.permutation(len(c1))]
        n2 = 20_001
        c2 = np.where(rng.random(n2) < 0.7, rng.choice(filler, n2), rng.choice(absent, n2)).astype(np.int32)
        rows = hot_rows(n2)
        for i in range(len(hot)):
            c2[rows[i]] = hot[i]
        p1 = rng.integers(0, 10 ** 7, len(c1), dtype=np.int32)
        p2 = rng.integers(0, 10 ** 7, n2, dtype=np.int32)
        for a in (c1, p1, c2, p2):
            a.setflags(write=False)
        _hot = (c1, p1, c2, p2, {"hot": hot, "rows": rows, "filler_rows": int(reps.sum())})
    return _hot


def hot_place(n: int = 50_001):
    """(cntp, out1p, inv, p2) for mq_pjoin_place: the partitioned counts carry each hot
    length on HOT_ROWS rows among counts 0 to 3; inv is a random bijection."""
    rng = np.random.default_rng(65536)
    cntp = rng.integers(0, 4, n).astype(np.uint32)
    at = rng.choice(n, len(HOT_LENGTHS) * HOT_ROWS, replace=False)
    cntp[at] = np.repeat(np.array(HOT_LENGTHS, dtype=np.uint32), HOT_ROWS)
    m = int(cntp.astype(np.int64).sum())
    out1p = rng.integers(0, 10 ** 9, m, dtype=np.int32)
    inv = rng.permutation(n).astype(np.uint32)
    p2 = rng.integers(0, 10 ** 9, n, dtype=np.int32)
    return cntp, out1p, inv, p2
