"""Top-k in numpy: the executable statement of include/rivulus_gpu.h's rv_top_k_indices comment.

The DEFINITION is two lines -- the sort's model cut at k (top_k_indices, top_k_frame).  The rest restates the device's radix select
(rivulus_amd/csrc/topk_rule.hpp, topk.hip): the null class, the bin rule and the stop rule, so that tests know which path a call takes,
how many passes over the key column it runs ("top_k_last_passes") and how many candidate rows it sorts ("top_k_last_candidates").
Columns and flags are sort_model's.
"""
import numpy as np

import sort_model as M


def top_k_indices(col, flags=0, k=0):
    return M.sort_indices(col, flags)[:k]


def top_k_frame(cols, keys, k):
    return M.sort_frame(cols, keys)[:k]


# ---- the select -------------------------------------------------------------------------------------------------------------------------
NULLS_ONLY, VALUES, EVERY_ROW = 0, 1, 2


def null_class(n, v, k, nulls_last):
    """(kind, values owed, nulls taken) for 0 < k < n = m + v: which rows the first k of the sort can come from, by the counts alone."""
    m = n - v
    if not nulls_last:
        if m >= k:
            return NULLS_ONLY, 0, False
        return VALUES, k - m, m > 0
    if v >= k:
        return VALUES, k, False
    return EVERY_ROW, 0, False


def choose_bin(hist, r):
    """(bin, count strictly below it, its count): the smallest bin whose inclusive prefix count reaches r, 1 <= r <= sum(hist)."""
    below = 0
    for b in range(255):
        c = int(hist[b])
        if below + c >= r:
            return b, below, c
        below += c
    return 255, below, int(hist[255])


def digits(keys, pos):
    return ((keys >> np.uint64(8 * pos)) & np.uint64(0xFF)).astype(np.int64)


def high_from(keys, pos):
    return keys >> np.uint64(8 * pos)


class Select:
    """What one call does: `selected` False -- the whole column is sorted (passes 0, every row a candidate); True -- `passes` passes over the
    key column, and `candidates`, the ascending row ids that are gathered and sorted."""

    def __init__(self, n, selected, passes=0, candidates=None):
        self.selected, self.passes = selected, passes if selected else 0
        self.candidates = candidates if selected else np.arange(n, dtype=np.int64)
        self.count = len(self.candidates)


def select(col, flags, k, select_from_rows, divisor):
    """The select over the FIRST key `col` for a call that asks for k rows."""
    n = len(col[1])
    k = min(k, n)
    if k == 0:
        return Select(0, True, 0, np.zeros(0, np.int64))  # nothing runs: no pass, no candidate
    if n < select_from_rows or 2 * k >= n:
        return Select(n, False)
    cls, keys = M.working_keys(col, flags)
    nulls_last = bool(flags & M.NULLS_LAST)
    valid = cls == (0 if nulls_last else 1)
    vkeys = keys[valid]
    v = len(vkeys)
    mask = [pos for pos in range(8) if v and (digits(vkeys, pos) != digits(vkeys[:1], pos)[0]).any()]  # where two non-null keys differ
    kind, r, nulls_taken = null_class(n, v, k, nulls_last)
    passes = 1
    if kind == EVERY_ROW:
        return Select(n, False)
    if kind == NULLS_ONLY:
        cand = np.flatnonzero(~valid)
    else:
        pos = max(mask) if mask else 0
        live = np.ones(v, bool)  # the values that still tie with the cut above `pos`
        below_total, prefix_high = 0, None
        while True:
            b, below, in_bin = choose_bin(np.bincount(digits(vkeys[live], pos), minlength=256), r)
            below_total += below
            r -= below
            live &= digits(vkeys, pos) == b
            count = (n - v if nulls_taken else 0) + below_total + in_bin
            prefix_high = high_from(vkeys[live][0], pos)
            remaining = [p for p in mask if p < pos]
            if not (remaining and count > n // divisor):
                break
            pos = max(remaining)
            passes += 1
        is_cand = np.zeros(n, bool)
        is_cand[valid] = high_from(keys[valid], pos) <= prefix_high
        if nulls_taken:
            is_cand |= ~valid
        cand = np.flatnonzero(is_cand)
        assert len(cand) == count
    if len(cand) >= n or len(cand) > n // 2:
        return Select(n, False)
    return Select(n, True, passes, cand.astype(np.int64))
