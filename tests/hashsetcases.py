"""Key lists shared by the bulk-insert tests (test_hashset_many.py, test_gpu_hashset_build.py):
test_hashset.py's CASES plus its negative and full lists, and the reference's own
insert_hashset loop where the reference defines the case."""
import ctypes as C

import numpy as np

from test_hashset import CASES, _bind, _table

LISTS = dict(CASES)
LISTS["negative"] = (10, [-1, -11, -21, 9, -5, 0, -2**31])  # test_libmq_negative_and_full
LISTS["full"] = (4, [1, 2, 3, 4, 5])


def reference_defined(size: int, keys) -> bool:
    """hashset.c indexes keys[negative] for a negative key and probes a full table
    forever: defined are non-negative keys in a table that never fills."""
    return all(int(k) >= 0 for k in keys) and len({int(k) for k in keys} - {0}) < size


def reference_table(refcpu, size: int, keys):
    """The slots the reference's insert_hashset loop leaves on zeroed slots, or None
    where the reference library is not built or the case is undefined in it."""
    if not refcpu.have_reference() or not reference_defined(size, keys):
        return None
    ref = _bind(refcpu.reference())
    hs = ref.create_hashset(size)
    C.memset(hs.contents.keys, 0, size * 4)  # the reference leaves them uninitialised
    for k in keys:
        ref.insert_hashset(hs, int(k))
    t = _table(hs)
    ref.free_hashset(hs)
    return t


def expected_table(refcpu, size: int, keys) -> np.ndarray:
    """refcpu.hashset_table, cross-checked against the reference where it applies."""
    want = refcpu.hashset_table(keys, size)
    ref = reference_table(refcpu, size, keys)
    assert ref is None or np.array_equal(ref, want), "restatement differs from the reference"
    return want


def thirds(keys):
    """keys as three consecutive batches (some may be empty)."""
    a, b = len(keys) // 3, 2 * len(keys) // 3
    return [keys[:a], keys[a:b], keys[b:]]
