"""The sort in numpy: the executable statement of include/rivulus_gpu.h's rv_sort_indices comment.

A key column is (dtype, values, valid): dtype "i64" / "f64" / "null", values a numpy array of int64 / float64 (anything for "null"), valid a
bool array or None (no nulls).  Every function returns numpy int64 permutations; a stable sort has exactly one, so tests compare for equality.
"""
import numpy as np

DESCENDING, NULLS_LAST = 1, 2
SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def order_key(bits, is_float):
    """The order map of csrc/order_key.hpp over uint64 bit patterns: Int64 the sign bit flipped; Float64 sign bit set -> every bit flipped,
    otherwise the sign bit set; every NaN -> the largest key."""
    bits = np.asarray(bits, np.uint64)
    if not is_float:
        return bits ^ SIGN
    mapped = np.where((bits >> np.uint64(63)).astype(bool), ~bits, bits | SIGN)
    nan = (bits & ~SIGN) > np.uint64(0x7FF0000000000000)
    return np.where(nan, ALL, mapped)


def working_keys(col, flags):
    """(class, key) per row.  class orders the nulls against the values (nulls first: 0 for a null, 1 for a value; nulls last: the other way
    round); key is the mapped key, complemented when descending, and 0 under a null -- whatever lies there is never looked at."""
    dtype, values, valid = col
    n = len(values)
    if dtype == "null":
        valid = np.zeros(n, bool)
    elif valid is None:
        valid = np.ones(n, bool)
    valid = np.asarray(valid, bool)
    keys = np.zeros(n, np.uint64)
    if dtype != "null" and n:
        bits = np.ascontiguousarray(values).view(np.uint64)
        mapped = order_key(bits, dtype == "f64")
        if flags & DESCENDING:
            mapped = ~mapped
        keys = np.where(valid, mapped, np.uint64(0))
    null_class = 1 if flags & NULLS_LAST else 0
    cls = np.where(valid, 1 - null_class, null_class).astype(np.uint8)
    return cls, keys


def sort_indices(col, flags=0, prior=None):
    """rv_sort_indices: `prior` (default: the identity) reordered stably by the key at its rows."""
    n = len(col[1])
    prior = np.arange(n, dtype=np.int64) if prior is None else np.asarray(prior, np.int64)
    assert len(prior) == n and (n == 0 or (prior.min() >= 0 and prior.max() < n))
    cls, keys = working_keys(col, flags)
    cls, keys = cls[prior], keys[prior]
    by_key = np.argsort(keys, kind="stable")
    by_class = np.argsort(cls[by_key], kind="stable")
    return prior[by_key[by_class]]


def sort_frame(cols, keys):
    """rv_sort's permutation: keys a list of (column index, flags), the first the most significant -- the chain from the last to the first."""
    perm = None
    for c, flags in reversed(keys):
        perm = sort_indices(cols[c], flags, perm)
    return perm


def lexsort_frame(cols, keys):
    """The same by np.lexsort over (class, key) of every key: a second statement of the multi-key order."""
    columns = []
    for c, flags in reversed(keys):
        cls, k = working_keys(cols[c], flags)
        columns += [k, cls]
    return np.lexsort(columns).astype(np.int64)


def column_of(dtype, cells):
    """A key column from a JSON cell list: null -> a null cell; Float64 cells may be spelled "nan", "-nan", "inf", "-inf", "-0.0" or a hex
    bit pattern "0x...". """
    n = len(cells)
    if dtype == "null":
        return "null", np.zeros(n, np.int64), None
    valid = np.array([c is not None for c in cells], bool)
    if dtype == "i64":
        values = np.array([0 if c is None else int(c) for c in cells], np.int64)
    else:
        bits = np.zeros(n, np.uint64)
        for i, c in enumerate(cells):
            if c is None:
                continue
            if isinstance(c, str) and c.startswith("0x"):
                bits[i] = int(c, 16)
            elif c == "-nan":
                bits[i] = 0xFFF8000000000000
            else:
                bits[i] = np.array([float(c)], np.float64).view(np.uint64)[0]
        values = bits.view(np.float64)
    return dtype, values, (None if valid.all() else valid)
