"""Shared by tests/test_library_search_cpu.py and tests/test_library_search_gpu.py: a first-principles model of the scan's
table, a float64 numpy model of the whole scan -- frame scores, windows, stable order, video ranking -- from the reference's
own definition of a window (cone/inference.py:284-299), the scan's ALGORITHM (flat half-block planes, windows from two planes)
with a switch per planted error, and the case lists both files walk.  Nothing here touches the library."""
import numpy as np

NEW_SYMBOLS = ("cone_library_scan_workspace", "cone_library_scan", "cone_library_localize_ranked_workspace",
               "cone_library_localize_ranked")

# ---- the issue's shapes -------------------------------------------------------------------------------------------------
TABLE_LENGTHS = (1, 44, 45, 46, 89, 90, 91, 900)                                  # the table's lengths at S = 45
KERNEL_LENGTHS = (1, 3, 4, 5, 15, 16, 17, 44, 45, 46, 89, 90, 91, 135, 333, 900)  # 4-row wave slot, 16-row workgroup, the seam
LONG_VIDEO = 45 * 1100                                                            # 1 101 windows: past the 1 024 counted in LDS
WINDOWS = (90, 125)
N_VIDEOS = (1, 2, 7, 65, 300)
N_QUERIES = (1, 4, 5, 64)
TOPK = (1, 20, 30)


def num_windows(ctx_l, W):
    S = W // 2
    return -(-ctx_l // S) + 1


# ---- the table from first principles ----------------------------------------------------------------------------------------
def table_model(videos, S):
    """One entry per half-block, by walking every video's rows: ``videos`` = [(row0, ctx_l), ...] in any order.  Returns
    (order, units) with order[slot] = index into ``videos`` by ascending row0 and units = [(slot, h, first row, rows), ...] in
    the order the scan's flat list has them."""
    order = sorted(range(len(videos)), key=lambda i: videos[i][0])
    units = []
    for slot, i in enumerate(order):
        row0, ctx_l = videos[i]
        h, r = 0, 0
        while r < ctx_l:
            units.append((slot, h, row0 + r, min(S, ctx_l - r)))
            h, r = h + 1, r + S
    return order, units


def stacked(lengths, gaps=None, start=0):
    """[(row0, ctx_l), ...] for videos laid out in the order given, ``gaps[i]`` free rows in front of video i (default none)."""
    out, at = [], start
    for i, n in enumerate(lengths):
        at += gaps[i] if gaps else 0
        out.append((at, n))
        at += n
    return out


# ---- the reference's definition, float64 ------------------------------------------------------------------------------------
def _fmax_reduce(x):
    """max that drops NaN (fmaxf), -inf for nothing or for NaN only."""
    x = x[~np.isnan(x)]
    return x.max() if x.size else -np.inf


def frame_scores(arena, cls):
    """(nq, rows) float64 <row, query>, every row by the same summation whatever surrounds it (a row sum over the products: no
    BLAS blocking), so equal rows score equal and both models below read the same numbers."""
    c64 = cls.astype(np.float64)
    out = np.empty((cls.shape[0], arena.shape[0]))
    for r0 in range(0, arena.shape[0], 4096):
        a64 = arena[r0:r0 + 4096].astype(np.float64)
        for q in range(cls.shape[0]):
            out[q, r0:r0 + a64.shape[0]] = (a64 * c64[q]).sum(axis=1)
    return out


def windows_truth(fs, W):
    """(nq, num_window) float64 from ONE video's frame scores fs (nq, ctx_l): window i = max over clips [max((i - 1) S, 0),
    min((i - 1) S + W, ctx_l)) (cone/inference.py:286-292); a NaN frame score is dropped by the max, as fmaxf drops it."""
    S = W // 2
    ctx_l = fs.shape[1]
    nw = num_windows(ctx_l, W)
    win = np.full((fs.shape[0], nw), -np.inf)
    for i in range(nw):
        s, e = max((i - 1) * S, 0), min((i - 1) * S + W, ctx_l)
        blk = np.where(np.isnan(fs[:, s:e]), -np.inf, fs[:, s:e])
        win[:, i] = blk.max(axis=1)
    return win


def stable_topk(row, k, higher_index_first=False):
    """First k of the stable descending order (ties to the LOWER index), padded with (-1, -inf).  Never sees a NaN: a window
    score is a max that drops them."""
    assert not np.isnan(row).any()
    idx = sorted(range(len(row)), key=lambda i: (-row[i], -i if higher_index_first else i))[:k]
    pad = k - len(idx)
    return np.asarray(idx + [-1] * pad, dtype=np.int64), np.asarray([row[i] for i in idx] + [-np.inf] * pad)


def scan_truth(arena, videos, cls, W, K, n_rank):
    """The whole scan from the definition: per slot (videos by ascending row0) and query the stable top-K windows of that
    video's rows ALONE; best = first value; the n_rank best slots by (score desc, slot asc).  Returns dict(widx (nq, V, K),
    wval, rank_slot (nq, n_rank), rank_val, order, win = per slot the (nq, num_window) window scores)."""
    order = sorted(range(len(videos)), key=lambda i: videos[i][0])
    nq, V = cls.shape[0], len(videos)
    widx, wval = np.full((nq, V, K), -1, dtype=np.int64), np.full((nq, V, K), -np.inf)
    fs_all, wins = frame_scores(arena, cls), []
    for slot, i in enumerate(order):
        row0, ctx_l = videos[i]
        win = windows_truth(fs_all[:, row0:row0 + ctx_l], W)
        wins.append(win)
        for q in range(nq):
            widx[q, slot], wval[q, slot] = stable_topk(win[q], K)
    rank_slot, rank_val = np.zeros((nq, n_rank), dtype=np.int64), np.zeros((nq, n_rank))
    for q in range(nq):
        rank_slot[q], rank_val[q] = stable_topk(wval[q, :, 0], n_rank)
    return dict(widx=widx, wval=wval, rank_slot=rank_slot, rank_val=rank_val, order=order, win=wins)


# ---- the scan's algorithm, with a switch per planted error ------------------------------------------------------------------
PLANTED = ("window_leaks_a_row", "wrong_hb_off", "ties_by_value", "odd_term_from_next_video")


def scan_algorithm(arena, videos, cls, W, K, n_rank, planted=None):
    """What the kernels do, in float64: the flat list of half-blocks (hb_off = prefix sums of ceil(ctx_l / S)), two planes --
    hm[g] = max of the unit's frame scores, fr[g] = its first frame's --, win[i] = max(hm[i - 1], hm[i], W odd: fr[i + 1]) over
    the video's OWN units, stable top-K per (query, slot), stable ranking of the slots.  ``planted``:
      window_leaks_a_row        a video's last half-block reads one row past the video's end;
      wrong_hb_off              a video's units are taken from hb_off[slot] + 1 on (an off-by-one in the owner search);
      ties_by_value             equal best scores rank the HIGHER slot first;
      odd_term_from_next_video  the odd-W term fr[i + 1] is taken whenever unit i + 1 exists in the flat list.
    Same return value as scan_truth."""
    assert planted is None or planted in PLANTED
    S, odd = W // 2, W & 1
    order = sorted(range(len(videos)), key=lambda i: videos[i][0])
    nq, V = cls.shape[0], len(videos)
    nh = [-(-videos[i][1] // S) for i in order]
    hb_off = np.concatenate([[0], np.cumsum(nh)]).astype(np.int64)
    total = int(hb_off[-1])
    fs_all = frame_scores(arena, cls)
    hm, fr = np.full((nq, total), -np.inf), np.full((nq, total), -np.inf)
    for slot, i in enumerate(order):
        row0, ctx_l = videos[i]
        for h in range(nh[slot]):
            lo, hi = row0 + h * S, row0 + min((h + 1) * S, ctx_l)
            if planted == "window_leaks_a_row" and h == nh[slot] - 1 and hi < arena.shape[0]:
                hi += 1
            fs = fs_all[:, lo:hi]
            for q in range(nq):
                hm[q, hb_off[slot] + h] = _fmax_reduce(fs[q])
                fr[q, hb_off[slot] + h] = fs[q, 0]
    widx, wval = np.full((nq, V, K), -1, dtype=np.int64), np.full((nq, V, K), -np.inf)
    for slot in range(V):
        off = int(hb_off[slot]) + (1 if planted == "wrong_hb_off" and hb_off[slot] + nh[slot] < total else 0)
        for q in range(nq):
            a, f = hm[q, off:], fr[q, off:]
            win = np.full(nh[slot] + 1, -np.inf)
            for i in range(nh[slot] + 1):
                parts = []
                if i >= 1:
                    parts.append(a[i - 1])
                if i < nh[slot]:
                    parts.append(a[i])
                inside = i + 1 < nh[slot]
                if planted == "odd_term_from_next_video":
                    inside = off + i + 1 < total
                if odd and inside:
                    parts.append(f[i + 1])
                win[i] = _fmax_reduce(np.asarray(parts))
            widx[q, slot], wval[q, slot] = stable_topk(win, K)
    rank_slot, rank_val = np.zeros((nq, n_rank), dtype=np.int64), np.zeros((nq, n_rank))
    for q in range(nq):
        rank_slot[q], rank_val[q] = stable_topk(wval[q, :, 0], n_rank, higher_index_first=planted == "ties_by_value")
    return dict(widx=widx, wval=wval, rank_slot=rank_slot, rank_val=rank_val, order=order)


def same_scan(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("widx", "wval", "rank_slot", "rank_val"))


# ---- value families -----------------------------------------------------------------------------------------------------
QNAN32 = np.uint32(0x7FC00000).view(np.float32)


def unit_rows(n, dv, seed):
    x = np.random.default_rng(seed).standard_normal((n, dv)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def build_arena(videos, dv, seed, capacity=None, hole=QNAN32):
    """(capacity, dv) float32: N(0, 1) unit rows inside the videos, ``hole`` everywhere else."""
    capacity = capacity or max(r + n for r, n in videos)
    arena = np.full((capacity, dv), hole, dtype=np.float32)
    for i, (row0, n) in enumerate(videos):
        arena[row0:row0 + n] = unit_rows(n, dv, seed * 1000 + i)
    return arena


def family(name, dv=256, W=90, seed=3):
    """A named small case of the planted-error table and of the GPU value families: (arena, videos, cls, W).  Query 0 is a unit
    vector; a "peak" is a row equal to 3 x query 0 (score 3: above every N(0, 1) unit row's |score| <= 1).
      random        seven videos of TABLE-like lengths with gaps;
      seam          two adjacent videos, no gap: a peak in video 0's LAST row and a double peak in video 1's FIRST row (W even);
      seam_odd      the same with W = 125 and the double peak in video 1's first row only: the odd term must not reach it from video 0;
      half_first    one video among three, W = 125: a peak in the first row of its half-block 2 (seen by window 1 through fr only);
      twins         two byte-identical videos between two others: equal best scores, ties across videos go to the lower slot;
      flat          a video whose rows are all equal: ties within a video go to the lower window index;
      nan_row       a NaN row inside one video (its frame score is dropped);
      all_nan       a video that is all NaN (every window -inf, listed 0 .. K - 1)."""
    S = W // 2
    q = unit_rows(3, dv, seed + 77)
    peak = 3 * q[0]
    if name == "random":
        videos = stacked([91, 1, 46, 333, 45, 89, 135], gaps=[0, 3, 0, 17, 0, 1, 5])
        arena = build_arena(videos, dv, seed, capacity=videos[-1][0] + 135 + 9)
    elif name in ("seam", "seam_odd"):
        W = 125 if name == "seam_odd" else 90
        S = W // 2
        videos = stacked([2 * S, 2 * S + 7, 50])                    # video 0 ends on a half-block boundary, video 1 follows at once
        arena = build_arena(videos, dv, seed)
        if name == "seam":
            arena[videos[0][1] - 1] = peak
        arena[videos[1][0]] = 2 * peak                              # (twice video 0's: a leak across the seam shows in video 0)
    elif name == "half_first":
        W, S = 125, 62
        videos = stacked([100, 4 * S, 80], gaps=[0, 0, 2])
        arena = build_arena(videos, dv, seed)
        arena[videos[1][0] + 2 * S] = peak
    elif name == "twins":
        videos = stacked([60, 140, 33, 140], gaps=[0, 0, 4, 0])
        arena = build_arena(videos, dv, seed)
        arena[videos[3][0]:videos[3][0] + 140] = arena[videos[1][0]:videos[1][0] + 140]
        arena[videos[1][0] + 70] = arena[videos[3][0] + 70] = peak
    elif name == "flat":
        videos = stacked([50, 333, 50])
        arena = build_arena(videos, dv, seed)
        arena[videos[1][0]:videos[1][0] + 333] = unit_rows(1, dv, seed + 5)[0]
    elif name == "nan_row":
        videos = stacked([91, 200, 46], gaps=[0, 1, 0])
        arena = build_arena(videos, dv, seed)
        arena[videos[1][0] + 45] = QNAN32                           # the first row of half-block 1: its fr is NaN
        arena[videos[1][0] + 130] = QNAN32
    elif name == "all_nan":
        videos = stacked([91, 200, 46])
        arena = build_arena(videos, dv, seed)
        arena[videos[1][0]:videos[1][0] + 200] = QNAN32
    else:
        raise KeyError(name)
    return arena, videos, q, W


FAMILIES = ("random", "seam", "seam_odd", "half_first", "twins", "flat", "nan_row", "all_nan")

# which family must tell which planted error from the truth (the CPU suite asserts this table)
CATCHES = {
    "window_leaks_a_row": ("seam",),
    "wrong_hb_off": ("random", "seam", "half_first"),
    "ties_by_value": ("twins",),
    "odd_term_from_next_video": ("seam_odd",),
}
