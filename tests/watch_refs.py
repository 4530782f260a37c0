"""Standing queries: numpy models of ``cone_watch_plan`` and ``cone_watch_store``, the validity rule written a second time from
the window geometry, the dictated lists and stamps the kernel tests run on, and the planted errors with the case that catches
each.

The rule the kernels implement (include/cone_hip.h): at the current ``ctx_l`` entry (q, wi) is valid iff ``stamp == ctx_l`` or
``stamp > 0 and (wi - 1) S + W <= stamp``, ``S = W // 2``.  ``valid_by_ranges`` says the same thing without the formula: the
clips ``cone_window_table`` gives the window now are the clips it gave it when the entry was stamped.  The two agree wherever a
stamp can come from a real poll (``0 <= stamp <= ctx_l``: a video only grows between two resets); the kernel tests also dictate
stamps above ``ctx_l``, where only the formula is the contract."""
import numpy as np

NEW_SYMBOLS = ("cone_watch_plan", "cone_watch_store")
N_ARGS = {"cone_watch_plan": 17, "cone_watch_store": 11}
NINF = np.float32(-np.inf)


def num_windows(ctx_l, W):
    S = W // 2
    return -(-ctx_l // S) + 1


def clip_range(wi, ctx_l, W):
    """The clips of window ``wi`` of a video of ``ctx_l`` clips (window_table_kernel: window 0 is the half window ahead)."""
    S = W // 2
    return max((wi - 1) * S, 0), min((wi - 1) * S + W, ctx_l)


def valid_rule(wi, stamp, ctx_l, W, mut=()):
    e = (wi - 1) * (W // 2) + W
    full = e < stamp if "lt_for_le" in mut else e <= stamp
    return bool(stamp == ctx_l or (stamp > 0 and full))


def valid_by_ranges(wi, stamp, ctx_l, W):
    """Brute force: the entry was computed (stamp > 0) on exactly the clips the window has now."""
    if stamp <= 0:
        return False
    then, now = clip_range(wi, stamp, W), clip_range(wi, ctx_l, W)
    return then == now and list(range(*then)) == list(range(*now))


def plan_ref(widx, wval, stamp, ctx_l, W, Nq, mut=()):
    """``cone_watch_plan``: (miss_widx, miss_wval, n_miss, seg_off, seg_cand, seg_n, seg_tag)."""
    nq, K = widx.shape
    n_win = stamp.shape[1]
    miss_widx = np.full((nq, K), -1, np.int32)
    miss_wval = np.full((nq, K), NINF, np.float32)
    n_miss = np.zeros(nq, np.int32)
    seg_cand, seg_n = np.zeros(nq * K, np.int64), np.zeros(nq * K, np.int32)
    for q in range(nq):
        found = []
        for j in range(K):
            wi = int(widx[q, j])
            if not 0 <= wi < n_win:
                continue
            seg_cand[q * K + j], seg_n[q * K + j] = (q * n_win + wi) * Nq, Nq
            if not valid_rule(wi, int(stamp[q, wi]), ctx_l, W, mut):
                found.append(j)
        if "unstable_order" in mut:
            found = found[::-1]
        n_miss[q] = len(found)
        miss_widx[q, :len(found)] = widx[q, found]
        miss_wval[q, :len(found)] = wval[q, found]
    return miss_widx, miss_wval, n_miss, np.arange(nq + 1, dtype=np.int32) * K, seg_cand, seg_n, np.zeros(nq * K, np.int32)


def store_ref(cand, miss_widx, n_miss, ctx_l, Nq, cache, stamp, mut=()):
    """``cone_watch_store`` on copies of ``cache`` (nq, n_win, Nq, 4) and ``stamp`` (nq, n_win): what they hold afterwards."""
    cache, stamp = cache.copy(), stamp.copy()
    nq, K = miss_widx.shape
    n_win = stamp.shape[1]
    cand = cand.reshape(-1, Nq, 4)
    first = 0
    for q in range(nq):
        n = min(max(int(n_miss[q]), 0), K)
        for m in range(n):
            wi = int(miss_widx[q, m])
            if 0 <= wi < n_win:
                cache[q, wi] = cand[first + m]
                stamp[q, wi] = ctx_l - 1 if "stamp_off_by_one" in mut else ctx_l
        first += n
    return cache, stamp


def cand_rows(n_miss, K, Nq):
    """A candidate buffer for the store: every word names its own (window row, slot, column)."""
    total = int(sum(min(max(int(n), 0), K) for n in n_miss))
    return (np.arange(max(total, 1) * Nq * 4, dtype=np.float32) + 1.0).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ dictated lists and stamps
W_DICTATED = 90
PATTERNS = ("all_valid", "all_missing", "alternating", "pad_middle", "out_of_range", "threshold", "short_equal", "zero_between")
KS = (1, 2, 63, 64, 65, 255, 256)
N_QUERIES = (1, 5, 64)
SLOTS = (3, 5, 10)


def dictated(nq, K, pattern, seed=0):
    """(widx (nq, K) int32, wval (nq, K) fp32, stamp (nq, n_win) int32, ctx_l): every query lists K distinct windows of a video
    of ``n_win = K + 7`` windows in an order of its own; the last window is short (3 clips are missing)."""
    W, S = W_DICTATED, W_DICTATED // 2
    n_win = K + 7
    ctx_l = (n_win - 1) * S - 3
    assert num_windows(ctx_l, W) == n_win
    rng = np.random.default_rng(1000 * K + 10 * nq + seed)
    widx = np.stack([rng.permutation(n_win)[:K] for _ in range(nq)]).astype(np.int32)
    wval = np.sort(rng.standard_normal((nq, K)).astype(np.float32), axis=1)[:, ::-1].copy()
    stamp = np.zeros((nq, n_win), np.int32)
    even = (np.arange(K) % 2 == 0)
    for q in range(nq):
        if pattern == "all_valid":
            stamp[q] = ctx_l
        elif pattern in ("alternating", "pad_middle", "out_of_range"):
            stamp[q, widx[q, even]] = ctx_l
        elif pattern == "threshold":            # the window's end exactly (valid: it was full) and one clip short of it
            for j in range(K):
                wi = int(widx[q, j])
                stamp[q, wi] = (wi - 1) * S + W - (j % 2)
        elif pattern == "short_equal":          # stamp == ctx_l keeps the short last window; one clip earlier it does not
            stamp[q] = ctx_l if q % 2 == 0 else ctx_l - 1
            if n_win - 1 not in widx[q]:
                widx[q, K // 2] = n_win - 1
        elif pattern == "zero_between":         # queries without a miss between queries with some
            if q % 3 == 1:
                stamp[q] = ctx_l
            else:
                stamp[q, widx[q, even]] = ctx_l
    if pattern == "pad_middle" and K >= 3:
        for q in range(nq):
            at = [K // 2] if K < 8 else [1, K // 2, K // 2 + 1, K - 2]
            widx[q, at], wval[q, at] = -1, NINF
    if pattern == "out_of_range":
        for q in range(nq):
            bad = [n_win, -2, n_win + 5, -7, 1 << 30]
            for i, j in enumerate(range(q % 2 if K > 1 else 0, K, max(K // 5, 1))):
                widx[q, j] = bad[i % len(bad)]
    return widx, wval, stamp, ctx_l


# ------------------------------------------------------------------------------------------------ planted errors
# mutation -> (pattern, K, nq): the dictated case on which the mutated model differs from the contract
MUTATIONS = ("lt_for_le", "unstable_order", "stamp_off_by_one")
CAUGHT_BY = {
    "lt_for_le": ("threshold", 64, 5),              # a stamp exactly at the window's end: `<` runs a full window again
    "unstable_order": ("alternating", 65, 5),       # two or more misses per query: their list order is the call's row order
    "stamp_off_by_one": ("all_missing", 2, 1),      # the short last window is valid only by stamp == ctx_l
}
