"""Certified library budgets (include/cone_hip.h, "certified library budgets"): a numpy / float64 model of
``cone_library_scan_certified`` written from the header's contract, not from the kernels, and the dictated inputs its tests run
on.  Pure numpy / torch on the CPU, no GPU: shared by tests/test_library_certified_cpu.py and the two GPU files.

The pipeline in the model's words.  A table of videos ``[(row0, ctx_l), ...]`` by ascending row0; window j of slot v is flat entry
``win_off[v] + j``.  ``coarse`` / ``exact`` are flat window rows (nq, total_win): the max of a window's frame scores, taken from
the bf16 shadow resp. the fp32 rows.  Per query: the ``n_cand`` best coarse entries (score descending, ties to the lower flat
index, a NaN never chosen) are the candidates; ordered by (exact descending, flat ascending) they are walked, skipping a candidate
whose slot has already given ``min(K, windows of the slot)``, until ``W`` are taken; ``t`` = the last taken exact score, ``c_last`` =
the smallest coarse score of the set; certified iff every window is a candidate, or W were taken and ``t - c_last > E`` with all
of them finite.  The emitted lists hold, per slot, its taken candidates in walk order, -1 / -inf elsewhere.

Planted errors.  ``certified_model`` / ``table_measures`` take ONE named fault at a time (``FAULTS``); ``DICTATED`` are named one-clip
cases that run on the model (tests/test_library_certified_cpu.py computes which case tells which fault from the contract:
``catches()`` must equal ``CATCHES``) and, unchanged, on the device against the fault-free model
(tests/test_library_certified_gpu.py).  What no model fault stands for -- a half-block or the odd-W term crossing a video's end,
rows of unlisted videos, the passes' seams, the merge levels, the chunk seam -- the GPU file holds by comparing with
cone_library_scan on arenas whose holes and unlisted rows are poisoned in both planes; no catch is claimed for those here.
"""
import numpy as np
import torch

import prefilter_certified_ref as C
import prefilter_stage_refs as P

NEW_SYMBOLS = ("cone_library_shadow_bytes", "cone_library_shadow_open", "cone_library_shadow_index",
               "cone_library_scan_certified_workspace", "cone_library_scan_certified")
N_ARGS = dict(cone_library_shadow_bytes=1, cone_library_shadow_open=4, cone_library_shadow_index=6,
              cone_library_scan_certified_workspace=8, cone_library_scan_certified=22)
NINF = np.float32("-inf")
MAX_CAND = 4096


# ------------------------------------------------------------------------------------------------ the table
def num_windows(ctx_l, W):
    S = W // 2
    return -(-ctx_l // S) + 1


def table_brute(videos, W):
    """``(order, row0, ctx, hb_off, win_off)`` by counting, one video at a time: slots by ascending row0."""
    S = W // 2
    order = sorted(range(len(videos)), key=lambda i: videos[i][0])
    hb, win = [0], [0]
    for i in order:
        n = videos[i][1]
        halves = sum(1 for h in range(n) if h * S < n)                      # half-blocks that hold a row
        hb.append(hb[-1] + halves)
        win.append(win[-1] + sum(1 for j in range(n + 2) if max((j - 1) * S, 0) < n and (j - 1) * S < n))
    return order, [videos[i][0] for i in order], [videos[i][1] for i in order], hb, win


def stacked(lengths, gaps=None, start=0):
    """Videos of ``lengths`` back to back from ``start`` (``gaps[i]`` free rows before video i): ([(row0, n), ...], capacity)."""
    out, at = [], start
    for i, n in enumerate(lengths):
        at += gaps[i] if gaps else 0
        out.append((at, n))
        at += n
    return out, at


# ------------------------------------------------------------------------------------------------ windows
def flat_windows(frame_scores, videos_by_slot, W):
    """``frame_scores[s]`` (nq, ctx_l of slot s) float64/float32 tensors -> (nq, total_win): every slot's window row
    (prefilter_stage_refs.windows_of: the max over the numbers of a window's frames, -inf without one), concatenated."""
    return torch.cat([P.windows_of(fs, W) for fs in frame_scores], dim=1).numpy()


def honest_rows(arena, videos_by_slot, cls, W):
    """The two flat window rows of HONEST arenas in float64: exact from the fp32 rows, coarse from both operands' bf16."""
    v, q = arena.double(), cls.double()
    ex = [(q @ v[r:r + n].t()) for r, n in videos_by_slot]
    co = [(C.bf16(cls) @ C.bf16(arena[r:r + n]).t()) for r, n in videos_by_slot]
    return flat_windows(co, videos_by_slot, W), flat_windows(ex, videos_by_slot, W)


def row_measures(arena):
    """Per row (r, n) in float64, inflated as the device inflates them: (rows, 2)."""
    v, vh = arena.float().double(), C.bf16(arena)
    r = (v - vh).norm(dim=1) * C.INFLATE + 2.0 ** -55
    n = torch.maximum(v.norm(dim=1), vh.norm(dim=1)) * C.INFLATE + 2.0 ** -55
    return torch.stack([r, n], dim=1)


def table_measures(err, videos_by_slot, fault=None):
    """(R, N) = the maxima of the per-row measures over exactly the table's rows; a NaN sticks (``nan_dropped``: fmaxf's way)."""
    rows = torch.cat([err[r:r + n] for r, n in videos_by_slot]).double()
    if fault == "nan_dropped":
        rows = torch.where(torch.isnan(rows), torch.zeros_like(rows), rows)
    if bool(torch.isnan(rows).any()):
        bad = torch.isnan(rows).any(dim=0)
        return tuple(float("nan") if bool(bad[i]) else float(rows[:, i].max()) for i in range(2))
    return float(rows[:, 0].max()), float(rows[:, 1].max())


# ------------------------------------------------------------------------------------------------ the candidate set and the walk
FAULTS = ("tie_higher_index", "certify_ge", "cmin_from_exact", "capped_counts", "short_certified", "nan_dropped")


def candidate_set(coarse_row, n_cand, fault=None):
    """Flat indices of the n_cand best coarse entries: score descending, ties to the lower index, a NaN never chosen."""
    row = np.asarray(coarse_row, dtype=np.float64)
    live = np.flatnonzero(~np.isnan(row))
    order = live[np.lexsort((-live if fault == "tie_higher_index" else live, -row[live]))]
    return order[:n_cand]


def default_n_cand(W, total_win):
    return min(total_win, max(4 * W, 128))


def certified_model(coarse, exact, win_off, K, W, n_cand, E, fault=None):
    """The contract on flat rows ``coarse`` / ``exact`` (nq, total_win): returns ``(widx, wval (nq, V, K), flags (nq), margin (nq))``
    -- ``margin`` = ``t - c_last`` (NaN where W were not taken or something is not finite), ``E`` a float or one per query."""
    coarse, exact = np.asarray(coarse), np.asarray(exact, dtype=np.float32)
    nq, total = coarse.shape
    V = len(win_off) - 1
    n_cand = n_cand or default_n_cand(W, total)
    slot_of = np.searchsorted(np.asarray(win_off), np.arange(total), side="right") - 1
    widx = np.full((nq, V, K), -1, dtype=np.int32)
    wval = np.full((nq, V, K), NINF, dtype=np.float32)
    flags, margin = np.zeros(nq, dtype=np.int32), np.full(nq, np.nan)
    Es = np.broadcast_to(np.asarray(E, dtype=np.float64), (nq,))
    for q in range(nq):
        cand = candidate_set(coarse[q], n_cand, fault)
        ex = np.where(np.isnan(exact[q, cand]), NINF, exact[q, cand])
        walk = cand[np.lexsort((cand, -ex.astype(np.float64)))]
        given, taken = {}, []
        for f in walk:
            s = int(slot_of[f])
            cap = min(K, int(win_off[s + 1] - win_off[s]))
            if given.get(s, 0) >= cap:
                if fault == "capped_counts":
                    taken.append(-1)                                    # (the skipped candidate uses up a place of the budget)
                    if len(taken) == W:
                        break
                continue
            widx[q, s, given.get(s, 0)], wval[q, s, given.get(s, 0)] = f - win_off[s], exact[q, f]
            given[s] = given.get(s, 0) + 1
            taken.append(f)
            if len(taken) == W:
                break
        c_last = float(np.min(coarse[q, cand])) if len(cand) == n_cand else float("-inf")
        if fault == "cmin_from_exact":
            c_last = float(np.min(ex)) if len(cand) == n_cand else float("-inf")
        real = [f for f in taken if f >= 0]
        if (len(taken) == W or fault == "short_certified") and real:
            t = float(exact[q, real[-1]])
            if np.isfinite(t) and np.isfinite(c_last) and np.isfinite(Es[q]):
                margin[q] = t - c_last
        proved = not np.isnan(margin[q]) and (margin[q] >= Es[q] if fault == "certify_ge" else margin[q] > Es[q])
        flags[q] = 1 if total <= n_cand or proved else 0
    return widx, wval, flags, margin


def full_lists(exact, win_off, K):
    """cone_library_scan's lists from a flat exact row: per slot the first K of (score descending, window ascending)."""
    exact = np.asarray(exact, dtype=np.float32)
    nq, V = exact.shape[0], len(win_off) - 1
    widx = np.full((nq, V, K), -1, dtype=np.int32)
    wval = np.full((nq, V, K), NINF, dtype=np.float32)
    for q in range(nq):
        for s in range(V):
            row = exact[q, win_off[s]:win_off[s + 1]]
            order = np.lexsort((np.arange(len(row)), -row.astype(np.float64)))[:K]
            widx[q, s, :len(order)], wval[q, s, :len(order)] = order, row[order]
    return widx, wval


def chosen_prefixes_equal(pairs_n, pairs_slot, pairs_k, got, want, q):
    """The lists' contract for query q: ``got`` / ``want`` = (widx, wval); the first pair_k entries of every chosen slot agree as
    words."""
    for i in range(int(pairs_n[q])):
        s, k = int(pairs_slot[q, i]), int(pairs_k[q, i])
        if not (np.array_equal(got[0][q, s, :k], want[0][q, s, :k])
                and np.array_equal(got[1][q, s, :k].view(np.int32), want[1][q, s, :k].view(np.int32))):
            return False
    return True


# ------------------------------------------------------------------------------------------------ dictated, decoupled arenas
def dictated_arenas(videos_by_slot, capacity, coarse_fs, exact_fs, dv=256, hole=1e30):
    """Frame f of slot s scores ``exact_fs[s][q][f]`` in the fp32 arena and ``coarse_fs[s][q][f]`` (bf16 values) in the shadow, for
    query q = e_q: row = sum_q x[q][f] e_q.  Rows outside the videos hold ``hole`` in both.  Returns (arena fp32, shadow rows as
    bf16, cls (nq, dv))."""
    nq = coarse_fs[0].shape[0]
    arena = torch.full((capacity, dv), hole, dtype=torch.float32)
    shadow = torch.full((capacity, dv), hole, dtype=torch.float32)
    for (r, n), c, x in zip(videos_by_slot, coarse_fs, exact_fs):
        c, x = torch.as_tensor(c, dtype=torch.float32), torch.as_tensor(x, dtype=torch.float32)
        fin = torch.isfinite(c)
        assert torch.equal(c[fin].bfloat16().float(), c[fin]), "coarse: bf16 values only"
        arena[r:r + n], shadow[r:r + n] = 0.0, 0.0
        arena[r:r + n, :nq], shadow[r:r + n, :nq] = x.t(), c.t()
    cls = torch.zeros(nq, dv)
    cls[torch.arange(nq), torch.arange(nq)] = 1.0
    return arena, shadow.bfloat16(), cls


def unit_query_bound(R, N, dv):
    """E of a query e_q (|q| = |qh| = 1, qh = q) for dictated measures."""
    return C.device_bound(torch.eye(1, dv)[0], R, N, dv)


# ------------------------------------------------------------------------------------------------ named dictated cases
E_EXACT = 2.0 ** -6 * (1 + 2.0 ** -10)       # E of a query e_q at R = 2^-6, N = 0: (R + 0)(1 + 2^-10) + 2^-114 * 2, and the last term
                                             # is below half an ulp of the rest in fp64 -- the same bits in numpy and on the device


def _ladder(V=40):
    return np.arange(V, 0, -1, dtype=np.float32) * 4                     # 160, 156, ...: bf16 values, candidates by slot


def _threshold(extra):
    """K = 1, W = 4, 10 candidates = slots 0 .. 4 (c_last = 144): the walk's 4th window is slot 3 at 144 + E + extra; fp32 holds
    144 + 2^-6 + 2^-16 (+ 2^-16) exactly."""
    c = _ladder()
    x = c.copy()
    x[3] = np.float32(144 + E_EXACT + extra)
    x[4] = x[3] - np.float32(0.125)
    assert float(x[3]) - 144 == E_EXACT + extra
    return dict(coarse=c, exact=x, K=1, W=4, n_cand=10, R=2.0 ** -6, N=0.0)


def _dictated_cases():
    cases = {"threshold_eq": _threshold(0.0), "threshold_above": _threshold(2.0 ** -16)}
    c = np.full(12, 1.0, dtype=np.float32)
    c[[2, 4, 6, 7, 9]] = [9, 8, 5, 5, 5]                                 # the tie at 5: flat 12, 13 | 14, 15 | 18, 19
    x = c.copy()
    x[7], x[9] = 7.5, 7.75
    for n_cand in (5, 6, 7):
        cases[f"tie_at_{n_cand}"] = dict(coarse=c, exact=x, K=2, W=5, n_cand=n_cand, R=2.0 ** -6, N=1.0)
    c = _ladder(10)
    cases["cap_all_candidates"] = dict(coarse=c, exact=c.copy(), K=1, W=3, n_cand=20, R=2.0 ** -6, N=1.0)
    x = c.copy()
    x[2] += 1.0                                                          # (the last taken window clears c_last: only the count says no)
    cases["cap_short"] = dict(coarse=c, exact=x, K=1, W=5, n_cand=6, R=2.0 ** -6, N=1.0)            # three slots cannot give five
    cases["cap_counts"] = dict(coarse=c, exact=c.copy(), K=1, W=3, n_cand=8, R=2.0 ** -6, N=1.0)    # W is reached only past the capped
    nan = dict(coarse=c, exact=c.copy(), K=2, W=2, n_cand=6, R=2.0 ** -6, N=1.0, nan_slot=1)        # a listed row's measures are NaN
    cases["nan_measure"] = nan
    return cases


DICTATED = _dictated_cases()
CATCHES = {"tie_higher_index": ("tie_at_5", "tie_at_6", "tie_at_7"), "certify_ge": ("threshold_eq",),
           "cmin_from_exact": ("threshold_eq",),
           "capped_counts": ("cap_all_candidates", "cap_counts", "cap_short", "threshold_above", "threshold_eq"),
           "short_certified": ("cap_short",), "nan_dropped": ("nan_measure",)}


def case_inputs(case):
    """(flat coarse, flat exact (1, 2 V), win_off, err (V, 2)) of a one-clip case: slot s has windows 2 s and 2 s + 1, both on its
    one clip."""
    V = len(case["coarse"])
    flat = lambda x: np.repeat(np.asarray(x, dtype=np.float32)[None, :], 2, axis=1)
    err = torch.tensor([[case["R"], case["N"]]] * V, dtype=torch.float32)
    if "nan_slot" in case:
        err[case["nan_slot"]] = float("nan")
    return flat(case["coarse"]), flat(case["exact"]), np.arange(0, 2 * V + 1, 2), err


def run_case(case, fault=None):
    """The model's outcome of a case: (widx, wval, flags)."""
    coarse, exact, win_off, err = case_inputs(case)
    V = len(case["coarse"])
    Rm, Nm = table_measures(err, [(s, 1) for s in range(V)], fault)
    E = unit_query_bound(Rm, Nm, 256)
    return certified_model(coarse, exact, win_off, case["K"], case["W"], case["n_cand"], E, fault)[:3]


def catches():
    """fault -> the names of the cases whose outcome (flags, and the lists of certified queries or of every query the fault-free
    model certifies) differs under that fault: what running the case against the fault-free model would notice."""
    out = {}
    for fault in FAULTS:
        hit = []
        for name, case in DICTATED.items():
            a, b = run_case(case), run_case(case, fault)
            same = np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
            if not same:
                hit.append(name)
        out[fault] = tuple(sorted(hit))
    return out
