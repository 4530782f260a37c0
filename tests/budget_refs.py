"""Models and named cases for library window budgets (cone_library_budget, cone_library_localize_ragged; plan_ragged_calls and
search_windows of cone_amd/library.py).  Pure numpy / Python, no GPU: shared by tests/test_library_budget_cpu.py and
tests/test_library_budget_gpu.py."""
import numpy as np

NEW_SYMBOLS = ("cone_library_budget_workspace", "cone_library_budget", "cone_library_localize_ragged_workspace",
               "cone_library_localize_ragged")
N_ARGS = dict(cone_library_budget_workspace=4, cone_library_budget=12, cone_library_localize_ragged_workspace=9,
              cone_library_localize_ragged=22)

NINF = np.float32("-inf")


# ------------------------------------------------------------------------------------------------ the contract
def ranked_order(wval):
    """(nq, n_videos, scan_K) fp32 -> (nq, n_videos * scan_K) flat indices slot * scan_K + j, per query in THE order: value
    descending, ties to the lower flat index (-0.0 == +0.0: numpy compares numbers).  NaN sorts last (never chosen)."""
    flat = np.asarray(wval, dtype=np.float32).reshape(len(wval), -1)
    key = np.where(np.isnan(flat), NINF, flat)
    return np.stack([np.lexsort((np.arange(flat.shape[1]), -row)) for row in key])


def budget_ref(wval, W, order=None):
    """The contract of cone_library_budget.  Per query: the entries > -inf in THE order, the first min(W, count) are chosen;
    pairs in order of first appearance; pair_k = entries chosen from the slot, pair_best = the value of its first (its bits).
    Returns (n_pairs (nq), pair_slot, pair_k (nq, W) int32, pair_best (nq, W) fp32); rows past n_pairs are -1 / 0 / -inf.
    ``order`` = ranked_order(wval) when the caller has it."""
    wval = np.asarray(wval, dtype=np.float32)
    nq, _, K = wval.shape
    flat = wval.reshape(nq, -1)
    order = ranked_order(wval) if order is None else order
    n_pairs = np.zeros(nq, dtype=np.int32)
    slot = np.full((nq, W), -1, dtype=np.int32)
    count = np.zeros((nq, W), dtype=np.int32)
    best = np.full((nq, W), NINF, dtype=np.float32)
    for q in range(nq):
        where = {}
        for i in order[q][:W]:
            v = flat[q, i]
            if not v > NINF:            # (-inf and NaN: behind every number in THE order -- nothing after them is chosen either)
                break
            s = int(i) // K
            if s not in where:
                where[s] = len(where)
                slot[q, where[s]], best[q, where[s]] = s, v
            count[q, where[s]] += 1
        n_pairs[q] = len(where)
    return n_pairs, slot, count, best


# ------------------------------------------------------------------------------------------------ dictated lists
SHAPES = ((1, 1), (3, 20), (7, 5), (410, 20), (33, 256))        # (n_videos, scan_K); the last two: flat rows of 8 200 / 8 448 > 8 192
BUDGETS = (1, 2, 63, 64, 65, 255, 256)
N_QUERIES = (1, 5, 64)
FAMILIES = ("distinct", "all_equal", "two_identical", "tie_at_w_raised", "tie_at_w_lowered", "dead_slot", "plus_inf", "signed_zeros")


def list_lengths(V, K):
    """Entries per list: full, except for the (7, 5) shape, whose lists are padded (1 .. 5 entries, then -1 / -inf)."""
    return [(s % K) + 1 if (V, K) == (7, 5) else K for s in range(V)]


def dictated(V, K, nq, family, W, seed=0):
    """(wval, widx) (nq, V, K): descending per (query, slot), padded with -inf / -1 behind list_lengths."""
    rng = np.random.default_rng(1000 * V + K + seed)
    n = V * K
    lens = list_lengths(V, K)
    live = np.concatenate([np.arange(K) < m for m in lens])                     # (n) which flat entries exist
    wval = np.full((nq, n), NINF, dtype=np.float32)
    for q in range(nq):
        vals = (rng.permutation(n).astype(np.float32) - n / 3) / 64              # distinct in fp32, both signs
        if family == "all_equal":
            vals[:] = 0.25
        elif family == "signed_zeros":
            vals = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0))
        rows = -np.sort(-vals.reshape(V, K), axis=1)                            # every list descending
        rows = np.where(np.arange(K)[None, :] < np.asarray(lens)[:, None], rows, NINF)
        if family == "two_identical" and V >= 2:
            rows[V - 1] = rows[0]
            if lens[V - 1] != lens[0]:
                rows[V - 1, lens[V - 1]:] = NINF
        if family == "dead_slot":
            rows[V // 2] = NINF
        if family == "plus_inf":
            rows[::2, 0] = np.inf                                                # several +inf heads: they tie, the lower slot first
        if family in ("tie_at_w_raised", "tie_at_w_lowered") and int(live.sum()) > W:
            order = ranked_order(rows[None])[0]
            a, b = order[W - 1], order[W]                                        # the W-th and the (W + 1)-th entry
            flat = rows.reshape(-1)
            if family == "tie_at_w_raised":
                flat[b] = flat[a]       # (every entry before b in its list is among the first W: >= flat[a] -- still descending)
            else:
                flat[a] = flat[b]       # (every entry behind a in its list is at most flat[b])
        wval[q] = rows.reshape(-1)
    wval = wval.reshape(nq, V, K)
    assert (np.diff(np.nan_to_num(wval.astype(np.float64), posinf=1e300, neginf=-1e300), axis=2) <= 0).all()
    widx = np.where(wval > NINF, np.arange(K, dtype=np.int32)[None, None, :], np.int32(-1)).astype(np.int32)
    return wval, widx


# ------------------------------------------------------------------------------------------------ the planner
def check_ragged_plan(video_of, k_of, calls, limit, max_windows):
    """What plan_ragged_calls promises: every pair once; both limits; a video's pairs adjacent in the concatenation and in the
    caller's order; the videos ascending."""
    flat = [i for idx in calls for i in idx]
    assert sorted(flat) == list(range(len(k_of)))
    assert all(idx for idx in calls)
    for idx in calls:
        assert len(idx) <= limit and sum(k_of[i] for i in idx) <= max_windows
    vids = [video_of[i] for i in flat]
    assert vids == sorted(vids)
    for v in set(vids):
        mine = [i for i in flat if video_of[i] == v]
        assert mine == sorted(mine)                     # stable
    for a, b in zip(calls, calls[1:]):                  # greedy: the next pair did not fit
        assert len(a) == limit or sum(k_of[i] for i in a) + k_of[b[0]] > max_windows
