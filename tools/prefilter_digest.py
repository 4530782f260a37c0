#!/usr/bin/env python3
"""Digests of the pre-filter's outputs on fixed seeded inputs, for a same-box A/B of two builds of the pre-filter sources
(cone_amd/csrc/prefilter.hip): every C entry (prefilter_scores: fp32 / split / bf16; both batched entries; PrefilterIndex.topk;
topk_windows) and every launch form of each (streaming QG x WPH x VPL, the many-query QT ladders and second passes, the
gated fallback, the three top-k forms), on the smallest shapes that reach them.
    python3 tools/prefilter_digest.py /tmp/pf_ab.pt       # first run (build A): saves every output there
    python3 tools/prefilter_digest.py /tmp/pf_ab.pt       # next run (build B): compares case by case, bit for bit
(tools/ab_on_box.sh runs the two builds one after the other.)  Prints one line per differing case (mismatching elements,
largest difference), the number of cases, and a digest of all outputs; exits 1 if a case differs."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cone_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1)
h = hashlib.sha1()
path = sys.argv[1] if len(sys.argv) > 1 else None
ref = torch.load(path) if path and os.path.exists(path) else None
out, bad = {}, []


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def case(key, **tensors):
    """Record the outputs of one case; against a saved run, compare them bit for bit (NaN and -inf included)."""
    cur = {k: v.cpu() for k, v in tensors.items() if v is not None}
    assert key not in out, key
    out[key] = cur
    for k in sorted(cur):
        h.update(cur[k].contiguous().numpy().tobytes())
    if ref is None:
        return
    msgs = []
    for k in sorted(cur):
        a, b = cur[k], ref[key][k]
        if a.shape != b.shape or not torch.equal(bits(a), bits(b)):
            n = int((bits(a) != bits(b)).sum()) if a.shape == b.shape else -1
            d = float((a.double() - b.double()).abs().nan_to_num(0.0).max()) if a.shape == b.shape else float("nan")
            msgs.append(f"{k} {n}/{a.numel()} differ (max {d:.2e})")
    if msgs:
        bad.append(key)
        print(f"{key}: " + ", ".join(msgs))


def unit(n, dv):
    return ops.l2_normalize(torch.randn(n, dv, device=dev, generator=g), 0.0)


def scores_case(tag, vid, nq, W, **kw):
    txt = unit(nq, vid.shape[1])
    fs, ws = ops.prefilter_scores(vid, txt, W, **kw)
    idx, val = ops.topk_windows(ws, min(30, ws.shape[1]))
    case(f"{tag}_ctx{vid.shape[0]}_dv{vid.shape[1]}_W{W}_q{nq}", ws=ws, idx=idx, val=val, fs=fs)


# ---- prefilter_scores, fp32: the streaming forms (1 - 4 queries) and the first many-query pass, with and without frame scores
# (300 017 x 512 at W = 125: 4 840 half windows, one wave each; the others: a workgroup per half window)
for ctx_l, dv, W in ((300_017, 512, 125), (44_001, 256, 90), (901, 256, 90), (37, 768, 90), (5_003, 1024, 7)):
    vid = unit(ctx_l, dv)
    for nq in (1, 2, 3, 4, 5, 7):
        for want_fs in (False, True):
            scores_case(f"fp32_fs{int(want_fs)}", vid, nq, W, frame_scores=want_fs)
    if dv == 1024:                                          # 40 queries at dv 1024: 32 per pass, and a second pass
        for want_fs in (False, True):
            scores_case(f"fp32mq_fs{int(want_fs)}", vid, 40, W, frame_scores=want_fs)
# the many-query passes at dv 512: 17 / 33 / 70 queries = 2 and 4 query tiles, and a second pass from query 64
vid = unit(44_001, 512)
for nq in (17, 33, 70):
    for want_fs in (False, True):
        scores_case(f"fp32mq_fs{int(want_fs)}", vid, nq, 90, frame_scores=want_fs)
for dv in (256, 768, 1024):                                 # one wave per half window (4 501 of them) at the other row widths
    vid = unit(9_001, dv)
    for nq in (1, 2, 3):
        scores_case("fp32_long", vid, nq, 4, frame_scores=False)

# ---- the split entry: 8 and 70 queries (a second pass), dv 256 / 512; 37 rows = one half window: eleven of the twelve waves
# have none; 44 001 = 977 x 45 + 36 and 20 011 = 322 x 62 + 47: a partial last half window
for ctx_l, dv, W in ((37, 256, 90), (44_001, 256, 90), (20_011, 512, 125), (500, 512, 90)):
    vid = unit(ctx_l, dv)
    for nq in (8, 70):
        scores_case("split", vid, nq, W, frame_scores=False, split_bf16=True)

# ---- the bf16 entry: streaming forms (1 - 4 queries; 9 001 rows at W = 4: one wave per half window), the many-query form
# (5, 17, 70); dv 96 and 288: no multiple of 256 -- a short last k-block --, dv 1024: two 16-B loads per lane
for ctx_l, dv, W in ((9_001, 96, 90), (9_001, 288, 4), (5_003, 1024, 7), (9_001, 1024, 4), (16_400, 512, 5)):
    vid16 = ops.rows_to_bf16(unit(ctx_l, dv))
    for nq in (1, 2, 3, 4, 5, 17, 70):
        scores_case("bf16", vid16, nq, W, frame_scores=False)


# ---- both batched entries: three videos of mixed lengths (2 600 rows at W = 4 / 5: 1 301 windows, the pass-based rows of the
# segmented top-k; the others: its counting rows), groups of 4, 1, 1 and 3 queries, an even and an odd W
def plan_of(lens, nqs, S):
    g_row0, g_ctx_l, g_q, q_ctx_l = [], [], [], []
    row0 = q = 0
    for n, c in zip(lens, nqs):
        for q0 in range(0, c, 4):
            ids = list(range(q + q0, q + min(q0 + 4, c)))
            g_row0.append(row0); g_ctx_l.append(n); g_q.append(ids + [-1] * (4 - len(ids)))
        q_ctx_l += [n] * c
        row0 += n; q += c
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=dev)
    nw = [(n + S - 1) // S + 1 for n in q_ctx_l]
    cum = lambda v: [sum(v[:i]) for i in range(len(v))]
    return dict(g_row0=t(g_row0, torch.int64), g_ctx_l=t(g_ctx_l, torch.int32), g_q=t(g_q, torch.int32), ng=len(g_row0),
                max_ctx_l=max(lens), q_fs_off=t(cum(q_ctx_l), torch.int64), q_win_off=t(cum(nw), torch.int64),
                q_ctx_l=t(q_ctx_l, torch.int32), fs_total=sum(q_ctx_l), win_total=sum(nw))


lens, nqs = (150, 37, 2_600), (5, 1, 3)
for dv, W in ((256, 4), (768, 5), (96, 4), (1024, 5)):
    arena, cls = unit(sum(lens), dv), unit(sum(nqs), dv)
    plan = plan_of(lens, nqs, W // 2)
    if dv % 256 == 0:
        idx, fs, ws = ops.prefilter_batched(arena, cls, plan, W, 30)
        case(f"batched_dv{dv}_W{W}", idx=idx, fs=fs, ws=ws)
    idx, _, ws = ops.prefilter_batched(ops.rows_to_bf16(arena), cls, plan, W, 30)
    case(f"batched_bf16_dv{dv}_W{W}", idx=idx, ws=ws)


# ---- PrefilterIndex.topk
def certified_case(tag, vid, cls, W, k, n_cand=None):
    idx, val, cert = ops.PrefilterIndex(vid).topk(cls, W, k, n_cand=n_cand)
    case(f"cert_{tag}_ctx{vid.shape[0]}_dv{vid.shape[1]}_W{W}_q{cls.shape[0]}_k{k}_c{n_cand}", idx=idx, val=val, cert=cert)
    return cert.cpu().tolist()


vid = unit(3_000, 256)
assert certified_case("all", vid, unit(3, 256), 4, 30) == [1, 1, 1]           # N(0,1) rows: every query certifies
certified_case("many", unit(3_000, 512), unit(17, 512), 5, 8)                 # the many-query coarse scan, an odd W
assert certified_case("small", unit(100, 256), unit(3, 256), 4, 30) == [1, 1, 1]        # 51 windows <= n_cand = 128
certified_case("sets", unit(16_400, 256), unit(3, 256), 4, 30, n_cand=2_000)  # candidates through cone_topk_windows_ws
# a query that cannot certify (tests/test_prefilter_certified_gpu.py): a video of identical rows -- every window ties, so the
# gated fp32 scan and the fallback's top-k run; with peaks planted along query 0 that one certifies and shares the call
for ctx_l, dv, W in ((600, 256, 4), (600, 512, 5), (600, 768, 4), (600, 1024, 5), (16_400, 256, 4), (16_400, 1024, 5)):
    rows = unit(6, dv)
    same = rows[:1].repeat(ctx_l, 1).contiguous()
    assert certified_case("tie", same, rows[1:4].contiguous(), W, 30) == [0, 0, 0]
    q0 = rows[4]
    for j, f in enumerate(range(10, ctx_l, ctx_l // 5)):
        a = 0.9 - 0.05 * j
        same[f] = a * q0 + (1 - a * a) ** 0.5 * same[f]
    cert = certified_case("mixed", same, torch.stack([q0, rows[1], rows[2], rows[3], rows[5]]), W, 4)
    assert 0 in cert, cert
certified_case("tie_k256", unit(1, 256).repeat(44_001, 1).contiguous(), unit(2, 256), 4, 256, n_cand=256)   # lists of 256: the pass-based selection

# ---- topk_windows: one workgroup of 256 per row (<= 4 096 windows), of 1 024 (<= 8 192, or k past the chunk lists), and
# the two-level chunk / merge form (more); scores quantised to 1 / 64 -- planted ties -- and a NaN, a +inf, a -inf per row
for nw, k in ((22, 22), (3_000, 30), (6_000, 30), (20_000, 30), (20_000, 64), (20_000, 65), (20_000, 300), (44_001, 30)):
    sc = (torch.randn(5, nw, device=dev, generator=g) * 64).round() / 64
    sc[:, nw // 2] = float("nan")
    sc[1, nw // 3] = float("inf")
    sc[2, nw // 4] = float("-inf")
    idx, val = ops.topk_windows(sc, k)
    case(f"topk_nw{nw}_k{k}", idx=idx, val=val)

torch.cuda.synchronize()
print(f"prefilter digest {h.hexdigest()}  ({len(out)} cases" + (f", {len(bad)} differ from {path})" if ref is not None else ")"))
if path and ref is None:
    torch.save(out, path)
sys.exit(1 if bad else 0)
