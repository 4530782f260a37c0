"""Plain references for the kernels that produce DECISIONS: the stable top-k forms of prefilter.hip and the proposal pooling +
cosine match of window_ops.hip (include/cone_hip.h: cone_topk_windows, cone_clip_matching[_gathered]).  Nothing here touches
the library; tests/test_index_kernels_cpu.py validates these helpers before the GPU tests rely on them.

    topk_reference           first k of the stable descending order of the non-NaN entries, (-1, -inf) padded
    topk_rows                named adversarial score rows (also the patterns of tools/topk_check.py)
    fast_select_survivors    how many values of a chunk's waves pass the threshold selection (which branch a row reaches)
    pooled_match_reference   float64 pooling + adapter + cosine of given spans, slices in exact rational arithmetic
    dyadic_spans             named edge-case spans whose boundaries are exact in fp32
    crafted_window / crafted_adapter_biases / slice_neighbours   inputs under which a slice moved by one clip is visible
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np
import torch

TK_CH = 4096            # scores per level-1 chunk of the two-level top-k; slot j of a chunk belongs to thread j % 256
TOL = 1e-4              # the project's figure for the matching column against the reference
POWER = 10 * TOL        # a slice moved by one clip must move the float64 value by at least this much


# ---- stable top-k ---------------------------------------------------------------------------------------------------------
def topk_reference(row, k: int):
    """(idx int32 (k,), val float32 (k,)): the first k entries of the stable descending order of the non-NaN entries of
    ``row`` -- ties, -0.0 against +0.0 included, to the lower index; a NaN is never selected (topk_kernel's "after the last
    pick" test and topk_chunk_kernel's ``x == x`` are both false for it); fewer than k numbers: (-1, -inf) padding."""
    x = torch.as_tensor(row, dtype=torch.float32).cpu().numpy()
    keep = np.flatnonzero(~np.isnan(x))
    order = keep[np.argsort(-x[keep], kind="stable")][:k]          # -(-0.0) and -(+0.0) compare equal: the tie stays a tie
    idx = np.full(k, -1, np.int32)
    val = np.full(k, -np.inf, np.float32)
    idx[:order.size] = order
    val[:order.size] = x[order]
    return torch.from_numpy(idx), torch.from_numpy(val)


def _planted(n: int, seed: int, slots):
    """Noise in (-1, 1) with the values 10, 10, 11, 11, ... (pairs tie) planted at chunk slots ``slots`` of one full chunk."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g) * 2 - 1
    full = n // TK_CH
    base = (seed % full) * TK_CH if full else 0
    at = [base + s for s in slots if base + s < n]
    for r, j in enumerate(at):
        x[j] = 10.0 + (len(at) - 1 - r) // 2
    return x


def topk_rows(n: int, k: int, seed: int = 0):
    """name -> one float32 score row of n windows, aimed at a top-k of size k.  Different seeds give different rows for every
    name.  No denormals: window scores are cosines."""
    g = torch.Generator().manual_seed(1000 + seed)
    inf = float("inf")
    rows = {
        "randint": torch.randint(0, 50, (n,), generator=g).float(),
        "randn": torch.randn(n, generator=g),
        "ascending": torch.arange(n, dtype=torch.float32) + seed,
        "descending": torch.arange(n, 0, -1, dtype=torch.float32) + seed,
        "constant": torch.full((n,), 3.0 + seed),
        "blocks": ((torch.arange(n) + 1000 * seed) // TK_CH).float(),
        # everything that matters sits in the last 4096 windows (two chunks of a two-level row share them)
        "one_hot_chunk": torch.cat([torch.zeros(max(n - TK_CH, 0)), torch.randn(min(n, TK_CH), generator=g) + 10]),
        "neg_inf": torch.where(torch.rand(n, generator=g) < 0.999, torch.tensor(-inf), torch.randn(n, generator=g)),
    }
    # the largest values in ONE thread of one chunk (slots t + 256 u: at most 16 of them)
    t = (37 + 5 * seed) % 256
    rows["one_lane"] = _planted(n, seed, [t + 256 * u for u in range(min(k, TK_CH // 256))])
    # ... and in a few lanes of ONE wave (slot mod 256 < 64), lane after lane, at least 6 whole lanes of 16: for 7 <= k <= 64
    # the threshold is then an ordinary lane's best, the 96 planted values all pass it and the selection overflows (> 64)
    lanes = -(-max(k, 96) // 16)
    rows["one_wave"] = _planted(n, seed, [l + 256 * u for l in range(min(lanes, 64)) for u in range(16)])
    x = torch.randint(0, 50, (n,), generator=g).float()
    rows["nan_sprinkled"] = torch.where(torch.rand(n, generator=g) < 0.1, torch.tensor(float("nan")), x)
    few = torch.full((n,), float("nan"))
    at = torch.randperm(n, generator=g)[:min(n, k) // 2]            # fewer than k numbers are left
    few[at] = torch.randint(0, 3, (at.numel(),), generator=g).float()
    rows["nan_few_left"] = few
    rows["all_nan"] = torch.full((n,), float("nan"))
    u = torch.rand(n, generator=g)
    rows["pos_inf"] = torch.where(u < 0.05, torch.tensor(inf), torch.where(u < 0.1, torch.tensor(-inf), torch.randn(n, generator=g)))
    if n >= 3:
        rows["pos_inf"][torch.randperm(n, generator=g)[:3]] = inf
    z = torch.randint(0, 8, (n,), generator=g)
    rows["signed_zero"] = torch.where(z < 3, torch.tensor(-0.0), torch.where(z < 6, torch.tensor(0.0),
                                      torch.where(z < 7, torch.tensor(1.0), torch.tensor(-1.0))))
    return {name: r.float().contiguous() for name, r in rows.items()}


NAN_FREE = ("randint", "randn", "ascending", "descending", "constant", "blocks", "one_hot_chunk", "neg_inf", "one_lane",
            "one_wave", "pos_inf", "signed_zero")
WITH_NAN = ("nan_sprinkled", "nan_few_left", "all_nan")


def fast_select_survivors(chunk, k: int):
    """The threshold selection of the two-level form (tk_wave_select_fast, k <= 64), restated to tell which branch a row
    reaches: per wave of the chunk's workgroup (slot j -> thread j % 256, wave = thread // 64) the number of values at or ahead
    of T = the k-th best of the 64 per-lane bests, in the order (score desc, index asc).  More than 64 -> the kernel falls
    back to the pass-based selection."""
    x = torch.as_tensor(chunk, dtype=torch.float32).numpy()
    out = []
    for wave in range(4):
        ent = [(-float(x[j]), j) for j in range(x.size) if (j % 256) // 64 == wave and not np.isnan(x[j])]
        best = {}
        for e in ent:
            lane = e[1] % 64
            if lane not in best or e < best[lane]:
                best[lane] = e
        lb = sorted(best.values())
        out.append(len(ent) if len(lb) < k else sum(e <= lb[k - 1] for e in ent))
    return out


# ---- proposal pooling + cosine match ---------------------------------------------------------------------------------------
def exact_slice(c, w, vlen: int):
    """(s, e) = (max(floor((c - w/2) vlen), 0), ceil((c + w/2) vlen)) in exact rational arithmetic from the fp32 values."""
    c, hw = Fraction(float(np.float32(c))), Fraction(float(np.float32(w))) / 2
    x1, x2 = (c - hw) * vlen, (c + hw) * vlen
    return max(x1.numerator // x1.denominator, 0), -((-x2.numerator) // x2.denominator)


def match_of_slice(rows, vlen: int, s: int, e_eff: int, cls, adapter=None) -> float:
    """float64 match value of the pooling over rows [s, e_eff) of the zero-padded window (rows past vlen are zero and count
    in the divisor); NaN for an empty slice."""
    if e_eff - s <= 0:
        return float("nan")
    rows = np.asarray(rows, np.float64)
    pf = rows[s:min(e_eff, vlen)].sum(axis=0) / (e_eff - s) if s < min(e_eff, vlen) else np.zeros(rows.shape[1])
    if adapter is not None:
        w0, b0, w1, b1 = (np.asarray(a, np.float64) for a in adapter)
        pf = w1 @ np.maximum(w0 @ pf + b0, 0.0) + b1 + pf
    cls = np.asarray(cls, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((pf / np.linalg.norm(pf)) @ (cls / np.linalg.norm(cls)))


def pooled_match_reference(vid_rows, vlen: int, pad_len: int, spans, cls, adapter=None):
    """cone/model.py:130-152, 178-210 for ONE window and given spans (nq, 2), in float64: the mean over rows
    s .. min(e, pad_len) of the window zero-padded to pad_len (NaN for an empty slice), the optional adapter pair
    (w0, b0, w1, b1) + residual, the cosine with cls / ||cls||.  Returns (match (nq,) float64, s (nq,), e (nq,))."""
    spans = np.asarray(spans, np.float32).reshape(-1, 2)
    se = [exact_slice(c, w, vlen) for c, w in spans]
    m = [match_of_slice(vid_rows, vlen, s, min(e, pad_len), cls, adapter) for s, e in se]
    return np.array(m), np.array([s for s, _ in se]), np.array([e for _, e in se])


def slice_neighbours(s: int, e_eff: int, pad_len: int):
    """The slices one clip away from [s, e_eff) that a pooling on this window can produce: start or effective end moved by one,
    0 <= start, end <= pad_len (an end past pad_len is clamped back onto the same slice).  A neighbour may be empty (NaN)."""
    out = []
    if s - 1 >= 0:
        out.append((s - 1, e_eff))
    out.append((s + 1, e_eff))
    if e_eff - 1 >= 0:
        out.append((s, e_eff - 1))
    if e_eff + 1 <= pad_len:
        out.append((s, e_eff + 1))
    return out


def _answer_key(s, e_eff, vlen, with_adapter):
    """What the value of the pooling over [s, e_eff) depends on: nothing for an empty slice (NaN); the real rows it holds --
    and, with an adapter only, the divisor: without one the cosine is scale-free, and a slice of zero rows alone is 0 / 0."""
    if e_eff - s <= 0:
        return None
    real = (s, min(e_eff, vlen)) if s < min(e_eff, vlen) else None
    if with_adapter:
        return (real, e_eff - s)
    return real


def power_of_case(rows, vlen, pad_len, s, e, cls, adapter=None):
    """(smallest float64 distance between the value of the right slice and of each neighbouring slice, neighbours compared).
    A NaN against a number counts as inf.  A neighbour that is the SAME answer by construction (``_answer_key``: both empty,
    or -- without an adapter -- the same real rows under another divisor) is not compared: no kernel error can show there."""
    e_eff = min(e, pad_len)
    right = match_of_slice(rows, vlen, s, e_eff, cls, adapter)
    worst, n = float("inf"), 0
    for s2, e2 in slice_neighbours(s, e_eff, pad_len):
        if _answer_key(s, e_eff, vlen, adapter is not None) == _answer_key(s2, e2, vlen, adapter is not None):
            continue
        other = match_of_slice(rows, vlen, s2, e2, cls, adapter)
        n += 1
        if np.isnan(right) != np.isnan(other):
            continue
        worst = min(worst, 0.0 if np.isnan(right) else abs(right - other))
    return worst, n


# named cases of one window shape: predicates over (a, b) = 128 (c - w/2), 128 (c + w/2), the slice (s, e) and the shape
def _case_table(vlen, pad):
    integral = lambda v: (v * vlen) % 128 == 0
    real = lambda s, e: 0 < s and e <= vlen
    tab = [
        ("both_integral", lambda a, b, s, e: integral(a) and integral(b) and 0 < s and e - s >= 2 and e <= vlen and b > a),
        ("negative_x1", lambda a, b, s, e: a < 0 and 1 <= e <= vlen),
    ]
    for L in (1, 7, 8, 9, 16, 17):
        tab.append((f"len_{L}", lambda a, b, s, e, L=L: real(s, e) and e - s == L and b > a))
    tab += [
        ("zero_rows", lambda a, b, s, e: vlen < e <= pad and s < vlen),
        ("clamped", lambda a, b, s, e: e > pad and s < vlen),
        ("empty_s_eq_end", lambda a, b, s, e: s == min(e, pad) and b > a),
        ("empty_s_gt_pad", lambda a, b, s, e: s > pad),
        ("w0_on_integer", lambda a, b, s, e: a == b and integral(a) and 0 < s <= vlen),
        ("w0_off_integer", lambda a, b, s, e: a == b and not integral(a) and e - s == 1 and 0 < s),
        ("full_window", lambda a, b, s, e: a == 0 and b == 128),
    ]
    return tab


def _candidates(vlen, pad_len, name, pred):
    """(c, w, in_range) of every span of the 2^-7 grid that is an instance of the named case, in a fixed scan order: c and w in
    [0, 1] first; the two empty slices that start at or past pad_len need c - w/2 >= pad_len / vlen >= 1 with w > 0, which no
    span in [0, 1] has, and are built with 1 < c <= 8 (the end stays positive: inside the reference's domain)."""
    for c_max in ((128, 1024) if name.startswith("empty_s_") else (128,)):
        for hw in range(0, 65):                                # w / 2 in [0, 1/2]
            for cc in range(0 if c_max == 128 else 129, c_max + 1):
                a, b = cc - hw, cc + hw
                s, e = max((a * vlen) // 128, 0), -((-b * vlen) // 128)
                if e >= 1 and pred(a, b, s, e):
                    yield cc / 128.0, 2 * hw / 128.0, c_max == 128


@functools.lru_cache(maxsize=None)
def dyadic_spans(vlen: int, pad_len: int):
    """[(name, c, w, in_range)]: the first span of the scan order for every named edge case that this window shape can reach,
    c and w / 2 multiples of 2^-7 (vlen <= 256: both products (c +- w/2) vlen are exact in fp32, floor / ceil the same in any
    evaluation order)."""
    assert 1 <= vlen <= pad_len <= 256
    out = []
    for name, pred in _case_table(vlen, pad_len):
        first = next(_candidates(vlen, pad_len, name, pred), None)
        if first is not None:
            out.append((name,) + first)
    return out


WINDOW_SHAPES = [(v, p) for v in (1, 45, 90, 128) for p in (v, v + 3, 256)]


def crafted_cases(rows, cls, adapter, max_tries: int = 200):
    """{(vlen, pad_len): [(name, c, w, cls index, in_range)]}: for every window shape and every named case it can reach, the
    first span of the scan order (and the first of the cls vectors) under which the case has POWER -- every neighbouring
    slice that is another answer lies at least 10 TOL away in float64, for these clip rows and this adapter.  A case for which
    the first ``max_tries`` spans hold no such instance is returned with its first span: the tests assert the power of every
    case they use, so it fails there rather than being left out."""
    out = {}
    for vlen, pad in WINDOW_SHAPES:
        lst = []
        for name, pred in _case_table(vlen, pad):
            pick = None
            for t, (c, w, inr) in enumerate(_candidates(vlen, pad, name, pred)):
                if t >= max_tries:
                    break
                s, e = exact_slice(c, w, vlen)
                for j in range(len(cls)):
                    if pick is None:
                        pick = (name, c, w, j, inr)
                    if power_of_case(rows[:vlen], vlen, pad, s, e, cls[j], adapter)[0] >= POWER:
                        pick = (name, c, w, j, inr)
                        break
                else:
                    continue
                break
            if pick is not None:
                lst.append(pick)
        out[(vlen, pad)] = lst
    return out


def crafted_window(dv: int, seed: int = 0, n_rows: int = 128):
    """(rows (n_rows, dv), cls (3, dv), r) float32: clip rows that alternate between two orthogonal unit directions q (even
    rows) and p (odd rows) with magnitudes 1 .. 1.75 and 1e-3 of shared noise; cls vectors in the plane of q and p, of
    different norms, at -0, -10 and 10 degrees from q; r a unit vector orthogonal to both.  A slice moved by one clip turns the
    pooled direction by ~1 / length radians in that plane -- per-row offsets far above the noise."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(dv)
    q /= np.linalg.norm(q)
    p = rng.standard_normal(dv)
    p -= (p @ q) * q
    p /= np.linalg.norm(p)
    r = rng.standard_normal(dv)
    r -= (r @ q) * q + (r @ p) * p
    r /= np.linalg.norm(r)
    rows = np.empty((n_rows, dv))
    for i in range(n_rows):
        rows[i] = (1.0 + 0.25 * (i % 4)) * (q if i % 2 == 0 else p) + 1e-3 * rng.standard_normal(dv)
    ang = np.deg2rad([0.0, -10.0, 10.0])
    cls = np.stack([(2.0 + j) * (np.cos(t) * q + np.sin(t) * p) for j, t in enumerate(ang)])
    return rows.astype(np.float32), cls.astype(np.float32), r.astype(np.float32)


def crafted_adapter_biases(sd, r, seed: int = 0):
    """A copy of state dict ``sd`` (numpy) whose second adapter bias is of the size of the pooled rows and orthogonal to them
    (b1 = r + 0.02 N(0, 1); b0 = 0.1 N(0, 1)): the adapter's output then depends on the SCALE of the pooled row, so a wrong
    divisor (zero rows miscounted) moves the match value as a wrong row does."""
    rng = np.random.default_rng(100 + seed)
    sd = dict(sd)
    d, dv = sd["adapter_layer.layers.0.weight"].shape
    sd["adapter_layer.layers.0.bias"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    sd["adapter_layer.layers.1.bias"] = (1.0 * r + 0.02 * rng.standard_normal(dv)).astype(np.float32)
    return sd


def adapter_of(sd):
    """(w0, b0, w1, b1) of a state dict with an adapter, else None."""
    if "adapter_layer.layers.0.weight" not in sd:
        return None
    return tuple(np.asarray(sd[f"adapter_layer.layers.{i}.{n}"]) for i in (0, 1) for n in ("weight", "bias"))


# (name, preset, make_opt overrides): adapter linear / none x 5 / 10 decoder slots x dv 256 (ego4d) / 512 (mad), and one model of
# another shape, whose adapter (d != dv) runs through the general GEMM
MATCH_VARIANTS = [(f"{preset}-{ad}-nq{nq}", preset, dict(adapter_module=ad, num_queries=nq))
                  for preset in ("ego4d", "mad") for ad in ("linear", "none") for nq in (5, 10)]
MATCH_VARIANTS.append(("shape128x4-linear-nq5", "ego4d", dict(hidden_dim=128, nheads=4, dim_feedforward=512)))


@functools.lru_cache(maxsize=None)
def matching_setup(variant: str, weight_seed: int = 0):
    """Everything the crafted matching tests of one model variant share, computed once: (opt, state dict (numpy, crafted adapter
    biases), rows, cls, adapter, entries).  ``entries``: the batch -- dicts(vlen, pad_len, cls_j, names, spans (nq, 2) fp32,
    ref (nq,) float64, s, e), each the window rows[:vlen] zero-padded to pad_len with nq crafted spans that share a cls
    vector; spare slots repeat the entry's first span."""
    from cone_amd import synth
    from cone_amd.config import make_opt
    _, preset, kw = next(v for v in MATCH_VARIANTS if v[0] == variant)
    opt = make_opt(preset, **kw)
    sd = synth.make_state_dict(opt, weight_seed)
    rows, cls, r = crafted_window(opt.v_appear_feat_dim, seed=weight_seed)
    if opt.adapter_module == "linear":
        sd = crafted_adapter_biases(sd, r, seed=weight_seed)
    adapter = adapter_of(sd)
    nq = opt.num_queries
    entries = []
    for (vlen, pad), lst in crafted_cases(rows, cls, adapter).items():
        for j in range(len(cls)):
            mine = [c for c in lst if c[3] == j]
            for i in range(0, len(mine), nq):
                grp = mine[i:i + nq]
                grp = grp + [grp[0]] * (nq - len(grp))
                spans = np.array([[c[1], c[2]] for c in grp], np.float32)
                ref, s, e = pooled_match_reference(rows[:vlen], vlen, pad, spans, cls[j], adapter)
                entries.append(dict(vlen=vlen, pad_len=pad, cls_j=j, names=[c[0] for c in grp], spans=spans, ref=ref, s=s, e=e))
    return opt, sd, rows, cls, adapter, entries


def assert_power(rows, cls, adapter, entries):
    """Every crafted case of ``entries`` has POWER (no case exempt); returns the smallest figure."""
    worst = float("inf")
    for en in entries:
        for name, s, e in zip(en["names"], en["s"], en["e"]):
            pw, n = power_of_case(rows[:en["vlen"]], en["vlen"], en["pad_len"], int(s), int(e), cls[en["cls_j"]], adapter)
            assert pw >= POWER, (name, en["vlen"], en["pad_len"], int(s), int(e), pw)
            assert n >= 1 or min(int(e), en["pad_len"]) - int(s) <= 0, (name, "no neighbour compared")
            worst = min(worst, pw)
    return worst
