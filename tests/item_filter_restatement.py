"""The item-filter contract of include/t4r_hip_filter.h restated in numpy: the predicate, the packed bit words, the mask, the
ranking rule of t4r_topk (value descending, ties to the lower id) and the tail rule.  It is the oracle of
tests/test_item_filter_gpu.py and uses none of the device code; tests/test_item_filter_cpu.py checks it against hand-written
cases."""
import numpy as np


def allow_words(V):
    """words of a bit array over V items: one 64-item collect tile's worth"""
    return 2 * ((V + 63) // 64) if V > 0 else 0


def pack_bits(allow):
    """allow [V] (non-zero = allowed) -> uint32 [allow_words(V)]: bit (v & 31) of word (v >> 5), pad bits zero"""
    allow = np.asarray(allow) != 0
    words = np.zeros(allow_words(allow.shape[0]), dtype=np.uint32)
    for v in np.flatnonzero(allow):
        words[v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    return words


def allowed(n_rows, V, allow=None, excl=None):
    """bool [n_rows, V]: (no allow array or allow[v]) and v not in excl[row]; entries of excl outside [0, V) are ignored"""
    ok = np.ones((n_rows, V), dtype=bool)
    if allow is not None:
        ok &= (np.asarray(allow) != 0)[None, :]
    if excl is not None:
        excl = np.asarray(excl)
        assert excl.shape[0] == n_rows
        for r in range(n_rows):
            e = excl[r]
            e = e[(e >= 0) & (e < V)]
            ok[r, e] = False
    return ok


def mask(scores, ok):
    """a copy of scores with -inf where not ok, whatever the column held"""
    out = np.array(scores, dtype=np.float32, copy=True)
    out[~ok] = -np.inf
    return out


def rank(scores, k):
    """(values [n, k], ids [n, k]) of the k best columns per row: value descending, ties to the lower id (a stable sort)"""
    scores = np.asarray(scores, dtype=np.float32)
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(scores, order, axis=1), order.astype(np.int64)


def tail(vals, ids):
    """the tail rule: id -1 in every slot whose value is -inf"""
    ids = np.array(ids, dtype=np.int64, copy=True)
    ids[np.isneginf(vals)] = -1
    return vals, ids


def filtered_topk(scores, k, allow=None, excl=None):
    """what every filtered route must return for the materialised scores [n, V]"""
    n, V = scores.shape
    return tail(*rank(mask(scores, allowed(n, V, allow, excl)), k))
