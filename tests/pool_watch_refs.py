"""Standing queries over a library: numpy models of ``cone_watch_pool_plan`` and ``cone_watch_pool_store`` written from the
contract in include/cone_hip.h ("standing queries over a library"), not from the kernels, and the dictated inputs the kernel
tests run on.

The contract in short.  The chosen windows of query q in pool order: the budget's pairs in their order, of pair i the list
positions ``0 .. pair_k - 1`` of ``(q, pair_slot[i])``.  Ordinal t with entry ``wi`` in slot ``s`` is listed when
``0 <= wi < v_cap[s]`` (and lies inside the axis), missing when listed and ``stamp[q][v_win0[s] + wi]`` is not valid at
``v_ctx_l[s]`` by the single-video rule (tests/watch_refs.py: ``valid_rule``).  ``n_pairs`` is clamped into ``[0, Wb]``, ``pair_k``
into ``[0, K]``, a slot outside ``[0, V)`` is an empty pair, ordinals past ``Wb`` do not exist."""
import numpy as np

from watch_refs import NINF, num_windows, valid_rule

NEW_SYMBOLS = ("cone_watch_pool_plan", "cone_watch_pool_store")
N_ARGS = {"cone_watch_pool_plan": 24, "cone_watch_pool_store": 15}
POISON = 0x7EADBEEF
W_DICTATED = 90

PATTERNS = ("all_valid", "all_missing", "alternating", "one_pair_all", "pairs_of_one", "pair_seam", "threshold", "per_video_ctx",
            "out_of_slab", "short_budget", "hostile")
BUDGETS = (1, 2, 63, 64, 65, 255, 256)
KS = (1, 20, 256)
VS = (1, 3, 300)
N_QUERIES = (1, 5, 64)
SLOTS = (3, 5, 10)


def _clamp(x, lo, hi):
    return min(max(int(x), lo), hi)


def chosen(n_pairs, pair_slot, pair_k, q, V, K):
    """The planned pairs of query ``q``: ``[(pair index, slot, first ordinal, planned windows), ...]``, the clamps applied."""
    Wb = pair_slot.shape[1]
    out, t = [], 0
    for i in range(_clamp(n_pairs[q], 0, Wb)):
        slot, k = int(pair_slot[q, i]), _clamp(pair_k[q, i], 0, K)
        if not 0 <= slot < V:
            continue
        planned = min(k, Wb - t)
        if planned > 0:
            out.append((i, slot, t, planned))
            t += planned
    return out


def listed(wi, slot, v_win0, v_cap, n_tot):
    return 0 <= wi < int(v_cap[slot]) and int(v_win0[slot]) >= 0 and int(v_win0[slot]) + wi < n_tot


def plan_ref(widx, wval, n_pairs, pair_slot, pair_k, v_ctx_l, v_win0, v_cap, stamp, W, Nq, miss_widx=None, miss_wval=None):
    """``cone_watch_pool_plan``: (miss_widx, miss_wval, pair_miss, seg_off, seg_cand, seg_n, seg_tag).  ``miss_widx`` /
    ``miss_wval`` (nq, V, K) are what the buffers held before (poison when not given): the entries the contract does not name
    keep those words."""
    nq, V, K = widx.shape
    Wb, n_tot = pair_slot.shape[1], stamp.shape[1]
    mw = np.full((nq, V, K), POISON, np.int32) if miss_widx is None else miss_widx.copy()
    mv = np.full((nq, V, K), POISON, np.int32).view(np.float32) if miss_wval is None else miss_wval.copy()
    pair_miss = np.zeros((nq, Wb), np.int32)
    seg_cand, seg_n, seg_tag = np.zeros(nq * Wb, np.int64), np.zeros(nq * Wb, np.int32), np.zeros(nq * Wb, np.int32)
    for q in range(nq):
        for i, slot, t0, planned in chosen(n_pairs, pair_slot, pair_k, q, V, K):
            found = []
            for j in range(planned):
                wi, seg = int(widx[q, slot, j]), q * Wb + t0 + j
                seg_tag[seg] = slot
                if listed(wi, slot, v_win0, v_cap, n_tot):
                    at = int(v_win0[slot]) + wi
                    seg_cand[seg], seg_n[seg] = (q * n_tot + at) * Nq, Nq
                    if not valid_rule(wi, int(stamp[q, at]), int(v_ctx_l[slot]), W):
                        found.append(j)
            mw[q, slot, :len(found)], mv[q, slot, :len(found)] = widx[q, slot, found], wval[q, slot, found]
            mw[q, slot, len(found):planned], mv[q, slot, len(found):planned] = -1, NINF
            pair_miss[q, i] = len(found)
    return mw, mv, pair_miss, np.arange(nq + 1, dtype=np.int32) * Wb, seg_cand, seg_n, seg_tag


def store_ref(cand, jobs, miss_widx, v_ctx_l, v_win0, v_cap, Nq, cache, stamp):
    """``cone_watch_pool_store`` on copies of ``cache`` (nq, n_tot, Nq, 4) and ``stamp`` (nq, n_tot): what they hold afterwards."""
    cache, stamp = cache.copy(), stamp.copy()
    nq, V, K = miss_widx.shape
    n_tot = stamp.shape[1]
    rows = cand.reshape(-1, 4)
    for q, slot, n, first in np.asarray(jobs).reshape(-1, 4).tolist():
        if not (0 <= q < nq and 0 <= slot < V and first >= 0):
            continue
        for m in range(_clamp(n, 0, K)):
            wi = int(miss_widx[q, slot, m])
            if listed(wi, slot, v_win0, v_cap, n_tot):
                at = int(v_win0[slot]) + wi
                cache[q, at] = rows[first + m * Nq:first + (m + 1) * Nq]
                stamp[q, at] = v_ctx_l[slot]
    return cache, stamp


def jobs_for(pair_miss, n_pairs, pair_slot, pair_k, V, K, Nq):
    """The host's job table for a plan: one job per planned pair that misses something, sorted by slot (the order of the calls a
    host plans by video), each pair's rows behind those of the jobs before it.  Returns (jobs (n, 4) int32, candidate rows)."""
    nq = pair_miss.shape[0]
    todo = [(slot, q, int(pair_miss[q, i])) for q in range(nq) for i, slot, _, _ in chosen(n_pairs, pair_slot, pair_k, q, V, K)
            if pair_miss[q, i] > 0]
    jobs, first = [], 0
    for slot, q, n in sorted(todo):
        jobs.append((q, slot, n, first))
        first += n * Nq
    return np.asarray(jobs, np.int32).reshape(-1, 4), first


def cand_rows(n_rows):
    """A candidate buffer for the store: every word names its own (row, column)."""
    return (np.arange(max(n_rows, 1) * 4, dtype=np.float32) + 1.0).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ dictated inputs
def dictated(nq, V, K, Wb, pattern):
    """A dict of the plan's inputs.  Slots 0 .. 3 hold videos of ``K + 3`` windows (every list entry is a real window), the others
    videos of 6 windows (their lists are padded with -1 / -inf past 6); every video's last window is short; slabs have 0 .. 2
    windows of headroom and do not touch.  Some patterns need a shape of their own and enlarge ``V`` or ``K`` (the dict says what
    they took).  Stamps start at 0 (never computed) and the pattern sets those of the planned entries."""
    assert pattern in PATTERNS
    W, S = W_DICTATED, W_DICTATED // 2
    if pattern == "one_pair_all":
        K = max(K, Wb)
    if pattern == "pairs_of_one":
        V = max(V, Wb)
    if pattern == "pair_seam":
        K, V = max(K, 64), max(V, 8)
    if pattern == "per_video_ctx":
        V = max(V, 2)
    slots = np.arange(V)
    n_win = np.where(slots < 4, K + 3, 6)
    v_ctx_l = ((n_win - 1) * S - 3 - (slots % 2 if pattern == "per_video_ctx" else slots % 5)).astype(np.int32)
    assert all(num_windows(int(c), W) == int(n) for c, n in zip(v_ctx_l[:8], n_win[:8]))
    v_cap = (n_win + slots % 3).astype(np.int32)
    v_win0 = (np.cumsum(v_cap + slots % 2) - v_cap).astype(np.int32)
    n_tot = int(v_win0[-1] + v_cap[-1]) + 2
    j = np.arange(K)
    widx = (n_win[None, :, None] - 1 - j[None, None, :] - np.arange(nq)[:, None, None] - slots[None, :, None]) % n_win[None, :, None]
    real = np.broadcast_to(j[None, None, :] < n_win[None, :, None], widx.shape)
    widx = np.where(real, widx, -1).astype(np.int32)
    wval = np.where(real, 1.0 - j[None, None, :] / (K + 1.0) - 1e-3 * slots[None, :, None] - 1e-5 * np.arange(nq)[:, None, None],
                    -np.inf).astype(np.float32)
    # ---- the pairs
    n_pairs = np.zeros(nq, np.int32)
    pair_slot, pair_k = np.full((nq, Wb), -1, np.int32), np.zeros((nq, Wb), np.int32)
    for q in range(nq):
        if pattern == "one_pair_all":
            ks = [Wb]
        elif pattern == "pairs_of_one":
            ks = [1] * Wb
        elif pattern == "pair_seam":
            ks = [63, 1, 1, 62, 1, 40, 1, 87]                   # ends at ordinals 63, 64, 65, 127, 128, 168, 169, 256
        else:
            P = min(V, Wb, 5 + q % 3)
            ks = [min(K, Wb // P + (1 if i < Wb % P else 0)) for i in range(P)]
            if pattern == "short_budget":
                ks = [] if q % 3 == 0 else [max(k // 2, 1) for k in ks[:max(len(ks) - 1, 1)]]
                if sum(ks) >= Wb:
                    ks = []
        out, left = [], Wb
        for k in ks:                                            # a budget never spends more than Wb
            if left > 0:
                out.append(min(k, left, K))
                left -= out[-1]
        n_pairs[q] = len(out)
        stride = 1 if V < 5 else 3 if V % 3 else 7 if V % 7 else 11
        pair_slot[q, :len(out)] = [(q + i * stride) % V for i in range(len(out))]     # distinct: the plan's precondition
        pair_k[q, :len(out)] = out
    assert all(len(set(pair_slot[q, :n_pairs[q]].tolist())) == n_pairs[q] for q in range(nq))
    # ---- out-of-slab list entries
    if pattern == "out_of_slab":
        bad = [-1, -5, None, None, 1 << 30]                     # None: the slot's own v_cap, and 7 past it
        for q in range(nq):
            for i in range(n_pairs[q]):
                s = int(pair_slot[q, i])
                for n, jj in enumerate(range(i % 2, int(pair_k[q, i]), 3)):
                    b = bad[(n + q) % 5]
                    widx[q, s, jj] = (int(v_cap[s]) + (7 if (n + q) % 5 == 3 else 0)) if b is None else b
    # ---- the stamps of the planned entries
    stamp = np.zeros((nq, n_tot), np.int32)
    if pattern == "per_video_ctx":
        for s in range(V):                                      # one stamp value a slab: the smaller of the two clip counts
            stamp[:, v_win0[s]:v_win0[s] + v_cap[s]] = (n_win[s] - 1) * S - 4
    elif pattern != "all_missing":
        for q in range(nq):
            for i, s, t0, planned in chosen(n_pairs, pair_slot, pair_k, q, V, K):
                for jj in range(planned):
                    wi, t = int(widx[q, s, jj]), t0 + jj
                    if not listed(wi, s, v_win0, v_cap, n_tot):
                        continue
                    at = int(v_win0[s]) + wi
                    if pattern == "all_valid":
                        stamp[q, at] = v_ctx_l[s]
                    elif pattern == "threshold":                # the window's end exactly (valid) and one clip short of it; the
                        end = (wi - 1) * S + W                  # short last window holds only at stamp == ctx_l
                        stamp[q, at] = v_ctx_l[s] - (t % 2) if end > v_ctx_l[s] else end - (t % 2)
                    elif t % 2 == 0:
                        stamp[q, at] = v_ctx_l[s]
    # ---- hostile device words (after the stamps: they describe what a sane host never sends)
    if pattern == "hostile":
        for q in range(nq):
            n = int(n_pairs[q])
            if q % 4 == 0:
                n_pairs[q] = Wb + 5                              # rows past the real pairs are -1 / 0: empty
            elif q % 4 == 1:
                n_pairs[q] = -3
            if n >= 1:
                pair_k[q, 0] = K + 9 if q % 2 == 0 else -4      # above K (and maybe across the cap of Wb), below 0
            if n >= 2:
                pair_slot[q, 1] = V + 3 if q % 2 == 0 else -2   # an empty pair
            if n < Wb:
                pair_slot[q, n], pair_k[q, n] = V, 7            # read only where n_pairs says so
    return dict(nq=nq, V=V, K=K, Wb=Wb, W=W, n_tot=n_tot, widx=widx, wval=wval, n_pairs=n_pairs, pair_slot=pair_slot, pair_k=pair_k,
                v_ctx_l=v_ctx_l, v_win0=v_win0, v_cap=v_cap, stamp=stamp, n_win=n_win)


def plan_args(d):
    return (d["widx"], d["wval"], d["n_pairs"], d["pair_slot"], d["pair_k"], d["v_ctx_l"], d["v_win0"], d["v_cap"], d["stamp"], d["W"])


def shape_for(a, b):
    """(K, V, nq) for the a-th budget and the b-th pattern: every value of each meets every budget and every pattern's family."""
    return KS[(a + b) % 3], VS[(a + 2 * b + 1) % 3], N_QUERIES[(2 * a + b) % 3]
