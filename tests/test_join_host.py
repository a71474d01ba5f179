"""joincases.py on the CPU: the numpy join model against the oracle (refcpu.hash_join, the
restatement of query.c:652-696 over multimap.c), and every hot-key input checked for what
it claims. The GPU tests (test_gpu_join_regimes.py) take their expected values from here.
"""
import numpy as np
import pytest

import joincases as jc


@pytest.mark.parametrize("case", jc.HOST_ORACLE_CASES)
def test_join_pairs_equals_oracle(refcpu, case):
    c1, p1, c2, p2 = jc.named_inputs(case)
    w1, w2 = refcpu.hash_join(c1, p1, c2, p2)
    g1, g2 = jc.join_pairs(c1, p1, c2, p2)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2)
    # (not with the roles swapped: the oracle's multimap goes quadratic on the dense probe
    # keys of `unique` as a build side, 84 s)


@pytest.mark.parametrize("case", jc.HOST_ORACLE_CASES + ["dups_short_runs", "hot_keys"])
def test_join_counts_equal_the_pairs_per_row(case):
    c1, p1, c2, p2 = jc.hot_keys()[:4] if case == "hot_keys" else jc.named_inputs(case)
    cnt = jc.join_counts(c1, c2)
    assert cnt.dtype == np.uint32 and len(cnt) == len(c2)
    rows = np.arange(len(c2), dtype=np.int32)
    o1, o2 = jc.join_pairs(c1, p1, c2, rows)
    assert int(cnt.astype(np.int64).sum()) == len(o1) == len(o2)
    assert np.array_equal(np.bincount(o2, minlength=len(c2)).astype(np.uint32), cnt)
    # every pair joins equal keys; inside a probe row the build rows ascend
    b1, _ = jc.join_pairs(c1, np.arange(len(c1), dtype=np.int32), c2, rows)
    assert np.array_equal(c1[b1], c2[o2])
    same = o2[1:] == o2[:-1]
    assert np.all(o2[1:] >= o2[:-1]) and np.all(b1[1:][same] > b1[:-1][same])


def test_long_entries():
    assert [jc.long_entries([L]) for L in jc.HOT_LENGTHS] == [0, 1, 1, 2, 3]
    assert jc.long_entries([0, 1, 4096, 4097, 65536 * 2, 65536 * 2 + 1]) == 1 + 2 + 3
    assert jc.long_entries(np.repeat(jc.HOT_LENGTHS, jc.HOT_ROWS)) == 21


def test_hot_keys_is_what_it_claims():
    c1, p1, c2, p2, info = jc.hot_keys()
    hot, rows = info["hot"], info["rows"]
    # the build: the five lengths exactly, every other key on 1 to 3 rows
    keys, runs = np.unique(c1, return_counts=True)
    assert [int(runs[keys == k][0]) for k in hot] == list(jc.HOT_LENGTHS)
    rest = runs[~np.isin(keys, hot)]
    assert len(rest) == 60_000 and rest.min() == 1 and rest.max() == 3
    assert len(c1) == sum(jc.HOT_LENGTHS) + info["filler_rows"] and 380_000 < len(c1) < 400_000
    # ... scattered: no hot key's rows are one stretch of the input
    for k in hot:
        at = np.nonzero(c1 == k)[0]
        assert at[-1] - at[0] > 300_000
    # the probe: each hot key on exactly its three rows
    assert len(c2) == 20_001
    for i, k in enumerate(hot):
        assert np.array_equal(np.nonzero(c2 == k)[0], np.sort(rows[i]))
    assert len(set((rows[:, 0] // 64).tolist())) == 1              # five hot rows in one 64-row word
    assert len(set((rows[:, 1] // 256).tolist())) == 5             # ... in five different blocks
    assert np.all(rows[:, 1] % 64 == 63) and np.all(rows[:, 2] % 64 == 0)
    assert rows[4, 2] // 64 == (len(c2) - 1) // 64 and len(c2) % 64  # the ragged last word
    cnt = jc.join_counts(c1, c2)
    assert int((cnt == 0).sum()) > 4000 and int(((cnt > 0) & (cnt <= 3)).sum()) > 10_000
    assert jc.long_entries(cnt) == 21
    m = int(cnt.astype(np.int64).sum())
    assert m == jc.HOT_ROWS * sum(jc.HOT_LENGTHS) + int(cnt[cnt <= 3].sum()) and 800_000 < m < 900_000
    # the list's capacity (mq_join_write): m / 4096 + m / 65536 + 2
    assert 21 <= m // jc.K_LONG_RUN + m // jc.K_LONG_CHUNK + 2
    # swapped roles: the 20 001 rows build, a hot key is a run of three met by 4096+ probe rows
    assert jc.long_entries(jc.join_counts(c2, c1)) == 0


def test_hot_keys_against_the_oracle(refcpu):
    """The oracle's `key % size` multimap on the hot-key input (spread filler keys): both
    directions."""
    c1, p1, c2, p2, _ = jc.hot_keys()
    w1, w2 = refcpu.hash_join(c1, p1, c2, p2)
    g1, g2 = jc.join_pairs(c1, p1, c2, p2)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2)
    v1, v2 = refcpu.hash_join(c2, p2, c1, p1)
    h1, h2 = jc.join_pairs(c2, p2, c1, p1)
    assert np.array_equal(h1, v1) and np.array_equal(h2, v2)


def test_hot_place_is_what_it_claims():
    cntp, out1p, inv, p2 = jc.hot_place()
    n = len(cntp)
    assert n == 50_001 and np.array_equal(np.sort(inv), np.arange(n, dtype=np.uint32))
    big = np.sort(cntp[cntp > 3])
    assert np.array_equal(big, np.repeat(np.array(jc.HOT_LENGTHS, dtype=np.uint32), jc.HOT_ROWS))
    assert jc.long_entries(cntp) == 21 and len(out1p) == int(cntp.astype(np.int64).sum())
    o1, o2 = jc.place(cntp, out1p, inv, p2)
    # row by row, the definition: row r's pairs are out1p[poff[inv[r]] : + cntp[inv[r]]]
    poff = np.concatenate([[0], np.cumsum(cntp.astype(np.int64))])
    want1 = np.concatenate([out1p[poff[q]:poff[q + 1]] for q in inv.tolist()])
    assert np.array_equal(o1, want1)
    assert np.array_equal(o2, np.repeat(p2, cntp[inv]))


def test_place_equals_the_host_phases_restatement(refcpu):
    """joincases.place against HostPhases.place (test_pjoin_dist.py), which the distributed
    join's host restatement is pinned by."""
    import torch

    from test_pjoin_dist import HostPhases
    cntp, out1p, inv, p2 = jc.hot_place(5_001)
    m = int(cntp.astype(np.int64).sum())
    t = lambda x, d: torch.from_numpy(x.astype(d))
    w1, w2 = HostPhases(refcpu).place(t(cntp, np.int32), t(out1p, np.int32), t(inv, np.int32), t(p2, np.int32), m)
    o1, o2 = jc.place(cntp, out1p, inv, p2)
    assert np.array_equal(o1, w1.numpy()) and np.array_equal(o2, w2.numpy())
