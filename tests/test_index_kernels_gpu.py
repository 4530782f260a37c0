"""The kernels that produce DECISIONS, pinned at their edge cases against the references of tests/index_refs.py (validated on
the CPU by test_index_kernels_cpu.py): every form of the stable top-k (prefilter.hip) bit for bit, and the proposal pooling +
cosine match (window_ops.hip) on crafted spans whose slices are exact, within TOL = 1e-4 of float64.  Needs an MI355X.

Which top-k path a case runs, from the dispatch in cone_topk_windows_ws / cone_topk_windows (TK_CH = 4096, TK_KMAX = 256):
  n <= 4096               -> topk_kernel<256>               (workspace 0: n <= 2 TK_CH)
  4096 < n <= 8192        -> topk_kernel<1024>              (workspace 0)
  n > 8192, k <= 256 and ceil(n / 4096) k <= 4096 -> topk_chunk_kernel + topk_merge_kernel; inside tk_block_select
        k <= 64 -> tk_wave_select_fast, which hands over to tk_wave_select when a wave has more than 64 survivors (``one_wave``:
                   test_index_kernels_cpu.test_threshold_selection_overflows_on_one_wave_and_not_on_noise)
        k > 64  -> tk_wave_select
  n = 8193, k = 257       -> k > TK_KMAX: the one-level topk_kernel<1024>
  n = 65537, k = 256      -> 17 chunks x 256 = 4352 > 4096 candidates: the one-level topk_kernel<1024>
topk_seg_kernel: n <= 1024 windows -> the counting rank, n > 1024 -> the pass branch (videos of 1024 and 1025 windows below).
"""
import numpy as np
import pytest
import torch

import index_refs as R
from cone_amd import _lib, ops
from test_gpu_parity import record_measured

pytestmark = pytest.mark.gpu

TOL = R.TOL
PATTERNS = R.NAN_FREE + R.WITH_NAN


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ks(n, ks):
    return sorted({k for k in ks if 1 <= k <= n})


ONE_LEVEL_256 = [(n, _ks(n, (1, min(30, n)) + ((n,) if n <= 257 else ()))) for n in (1, 63, 64, 65, 256, 257, 1025, 4096)]
ONE_LEVEL_1024 = [(n, [1, 30, 65]) for n in (4097, 8192)]
TWO_LEVEL = [(n, [1, 2, 30, 64, 65, 256]) for n in (8193, 12287, 12288, 12289)]
FALLBACKS = [(8193, [257]), (65537, [256])]


def _check_topk(n, ks, two_level):
    dev = _gpu()
    lib = _lib.load()
    for k in ks:
        assert (lib.cone_topk_windows_workspace(3, n, k) > 0) == (n > 2 * R.TK_CH)
        runs_two_level = n > 2 * R.TK_CH and k <= 256 and -(-n // R.TK_CH) * k <= 4096
        assert runs_two_level == two_level, (n, k)
        rows = [R.topk_rows(n, k, seed) for seed in range(3)]
        for name in PATTERNS:
            x = torch.stack([r[name] for r in rows])                         # nq = 3, another row per query
            want_i, want_v = zip(*[R.topk_reference(x[q], k) for q in range(3)])
            want_i, want_v = torch.stack(want_i), torch.stack(want_v)
            xd = x.to(dev).contiguous()
            idx, val = ops.topk_windows(xd, k)
            assert torch.equal(idx.cpu(), want_i), (name, n, k)
            assert torch.equal(_bits(val), _bits(want_v)), (name, n, k)
            # every row of a launch is independent: the same row alone
            i1, v1 = ops.topk_windows(xd[1:2].contiguous(), k)
            assert torch.equal(i1[0], idx[1]) and torch.equal(_bits(v1[0]), _bits(val[1])), (name, n, k, "nq = 1")
            if two_level:       # the one-level form on the same buffer
                i2 = torch.empty_like(idx)
                v2 = torch.empty_like(val)
                _lib.check(lib.cone_topk_windows(_lib.ptr(xd, torch.float32), 3, n, k, _lib.ptr(i2), _lib.ptr(v2), _lib.stream()))
                assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val)), (name, n, k, "forms differ")


@pytest.mark.parametrize("n,ks", ONE_LEVEL_256 + ONE_LEVEL_1024, ids=lambda v: str(v) if isinstance(v, int) else "k")
def test_topk_one_level_forms(n, ks):
    """topk_kernel<256> (n <= 4096) and topk_kernel<1024> (4097 .. 8192): idx and val are the reference's, bit for bit, on every
    pattern -- ties, +-inf, signed zeros, NaN (never selected; (-1, -inf) once the numbers run out)."""
    _check_topk(n, ks, two_level=False)


@pytest.mark.parametrize("n,ks", TWO_LEVEL, ids=lambda v: str(v) if isinstance(v, int) else "k")
def test_topk_two_level_form(n, ks):
    """topk_chunk_kernel + topk_merge_kernel: a last chunk of 1 (8193, 12289) or 4095 / 4096 windows, chunk lists padded with
    empty slots (a chunk with fewer numbers than k), the threshold selection (k <= 64) with its overflow, the pass-based
    selection (k > 64); bit-equal to the reference and to the one-level form on the same buffer."""
    _check_topk(n, ks, two_level=True)


@pytest.mark.parametrize("n,ks", FALLBACKS, ids=lambda v: str(v) if isinstance(v, int) else "k")
def test_topk_two_level_fallbacks(n, ks):
    """Rows long enough for the two-level form that cone_topk_windows_ws hands to the one-level kernel: k > 256, and more than
    4096 candidates (17 chunks x 256)."""
    _check_topk(n, ks, two_level=False)


def test_topk_seg_kernel_both_branches():
    """topk_seg_kernel through ops.prefilter_batched on a hand-built split: videos of 2, 22, 1024 (the last counting-rank size)
    and 1025 windows (the first pass-branch size), W = 90, k = 30.  The clip rows repeat with period 135 = 3 S, so window
    scores tie exactly in both branches; a run of NaN clip rows makes whole windows of one 1025-window video score -inf.  The
    returned list is topk_reference of the RETURNED window scores, and ops.topk_windows on that row, bit for bit."""
    dev = _gpu()
    W, S, dv, k = 90, 45, 256, 30
    ctx = [45, 945, 1023 * S, 1024 * S, 1024 * S]
    nws = [-(-c // S) + 1 for c in ctx]
    assert nws == [2, 22, 1024, 1025, 1025]
    g = torch.Generator().manual_seed(5)
    base = torch.nn.functional.normalize(torch.randn(135, dv, generator=g), dim=1)
    row0 = np.concatenate([[0], np.cumsum(ctx)]).astype(np.int64)
    arena = torch.cat([base[torch.arange(c) % 135] for c in ctx]).contiguous()
    nan_lo, nan_hi = int(row0[3]) + 5000, int(row0[3]) + 5300             # windows 113 .. 116 of video 3 hold NaN frames only
    arena[nan_lo:nan_hi] = float("nan")
    q_vid = [0, 1, 2, 3, 3, 4]
    nq = len(q_vid)
    cls = torch.nn.functional.normalize(torch.randn(nq, dv, generator=g), dim=1)
    groups = [(0, [0]), (1, [1]), (2, [2]), (3, [3, 4]), (4, [5])]
    q_ctx = np.array([ctx[v] for v in q_vid], np.int64)
    q_nw = np.array([nws[v] for v in q_vid], np.int64)
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)
    plan = dict(g_row0=t([row0[v] for v, _ in groups], torch.int64), g_ctx_l=t([ctx[v] for v, _ in groups], torch.int32),
                g_q=t([qs + [-1] * (4 - len(qs)) for _, qs in groups], torch.int32).contiguous(), ng=len(groups),
                max_ctx_l=max(ctx), q_fs_off=t(np.concatenate([[0], np.cumsum(q_ctx)[:-1]]), torch.int64),
                q_win_off=t(np.concatenate([[0], np.cumsum(q_nw)[:-1]]), torch.int64), q_ctx_l=t(q_ctx, torch.int32),
                fs_total=int(q_ctx.sum()), win_total=int(q_nw.sum()))
    idx, fs, ws = ops.prefilter_batched(arena.to(dev), cls.to(dev), plan, W, k)
    assert not torch.isnan(ws).any()                                         # window scores of the library are never NaN
    off = np.concatenate([[0], np.cumsum(q_nw)])
    for q in range(nq):
        row = ws[off[q]:off[q + 1]]
        want_i, _ = R.topk_reference(row, k)
        assert idx[q].cpu().tolist() == want_i.tolist(), q
        kk = min(k, int(q_nw[q]))
        i1, _ = ops.topk_windows(row[None].contiguous(), kk)
        assert idx[q, :kk].cpu().tolist() == i1[0].cpu().tolist() and (idx[q, kk:] == -1).all(), q
        r = row.cpu()
        if q_nw[q] > 100:       # exact ties between windows three apart, decided by the index
            assert torch.equal(r[10:40], r[13:43]) and len(set(r[10:13].tolist())) >= 2
            top = idx[q].cpu().tolist()
            assert any(float(r[a]) == float(r[b]) and a < b for a, b in zip(top, top[1:]))
        if q_vid[q] == 3:
            assert torch.isneginf(r[113:117]).all() and int(torch.isneginf(r).sum()) == 4
    assert idx[0].cpu().tolist()[2:] == [-1] * (k - 2)                       # the 2-window video: padded with -1


# ---- proposal pooling + cosine match ---------------------------------------------------------------------------------------
_MODELS = {}


def _model(variant):
    """The variant's model with its crafted state dict (R.matching_setup), built once."""
    from cone_amd.model import build_model
    if variant not in _MODELS:
        opt, sd, *_ = R.matching_setup(variant)
        m, _ = build_model(opt)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        _MODELS[variant] = m
    return _MODELS[variant]


def _compare(got, entries, what):
    """got (B, nq) against the float64 reference of every entry: NaN exactly where the reference has NaN, every other slot --
    the neighbours of a NaN slot included -- within TOL.  Returns the worst distance."""
    got = got.detach().cpu().double().numpy()
    worst = 0.0
    for b, en in enumerate(entries):
        ref = en["ref"]
        assert (np.isnan(got[b]) == np.isnan(ref)).all(), (what, en["vlen"], en["pad_len"], en["names"], got[b], ref)
        ok = ~np.isnan(ref)
        if ok.any():
            d = np.abs(got[b][ok] - ref[ok])
            assert d.max() <= TOL, (what, en["vlen"], en["pad_len"], [n for n, o in zip(en["names"], ok) if o], d)
            worst = max(worst, float(d.max()))
    return worst


def _gathered_inputs(rows, cls, entries, order, dev):
    """The arena entry's arguments for ``entries`` taken in ``order``: one arena (7 unrelated rows, then the clip rows) every
    window points into, per-window pad_len, and cls rows reached through cls_row (repeated and permuted)."""
    arena = torch.cat([torch.full((7, rows.shape[1]), 1e3), torch.from_numpy(rows)]).to(dev).contiguous()
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    perm = [2, 0, 1]                                                           # cls vector j lives in row perm[j]
    cls_dev = torch.from_numpy(cls)[[perm.index(r) for r in range(3)]].to(dev).contiguous()
    ens = [entries[i] for i in order]
    return dict(cls=cls_dev, cls_row=i32([perm[e["cls_j"]] for e in ens]), vid=arena, vid_row0=i32([7] * len(ens)),
                vid_len=i32([e["vlen"] for e in ens]), pad_len=i32([e["pad_len"] for e in ens]),
                spans=torch.from_numpy(np.stack([e["spans"] for e in ens])).to(dev).contiguous()), ens


@pytest.mark.parametrize("variant", [v[0] for v in R.MATCH_VARIANTS])
def test_crafted_spans_pool_the_reference_slices(variant):
    """Spans as INPUT (c and w / 2 on the 2^-7 grid: no ulp ambiguity in floor / ceil), every edge case of R.dyadic_spans on
    every window shape vlen in {1, 45, 90, 128} x pad_len in {vlen, vlen + 3, 256}, through both entries: the padded
    ``forward_clip_matching`` (pad_len = the tensor's length) and ``clip_matching_gathered`` (per-window pad_len, cls_row).
    Every case has POWER (asserted here again): a slice off by one clip, or a divisor off by one zero row, is >= 10 TOL away.

    Measured worst distance to float64: see profiles/README.md ("index kernels")."""
    dev = _gpu()
    opt, sd, rows, cls, adapter, entries = R.matching_setup(variant)
    assert R.assert_power(rows, cls, adapter, entries) >= R.POWER
    model = _model(variant)
    # arena entry: the entries in a scrambled order
    order = list(np.random.default_rng(1).permutation(len(entries)))
    args, ens = _gathered_inputs(rows, cls, entries, order, dev)
    worst_g = _compare(model.clip_matching_gathered(**args), ens, "gathered")
    # padded entry: one call per pad_len (the batch tensor's length is every window's pad_len)
    worst_p = 0.0
    for pad in sorted({e["pad_len"] for e in entries}):
        ens = [e for e in entries if e["pad_len"] == pad]
        vid = torch.zeros(len(ens), pad, rows.shape[1])
        mask = torch.zeros(len(ens), pad)
        for b, e in enumerate(ens):
            vid[b, :e["vlen"]] = torch.from_numpy(rows[:e["vlen"]])
            mask[b, :e["vlen"]] = 1
        c = torch.from_numpy(np.stack([cls[e["cls_j"]] for e in ens]))
        sp = torch.from_numpy(np.stack([e["spans"] for e in ens]))
        got = model.forward_clip_matching(c.to(dev), vid.to(dev), mask.to(dev), proposal=sp.to(dev))
        worst_p = max(worst_p, _compare(got, ens, f"padded[{pad}]"))
    # (as text: record_measured rounds floats to 6 decimals, and these are ~1e-7)
    record_measured(f"index_kernels_matching[{variant}]", worst_gathered=f"{worst_g:.3e}", worst_padded=f"{worst_p:.3e}",
                    cases=sum(len(set(e["names"])) for e in entries))


@pytest.mark.parametrize("variant", ["ego4d-linear-nq5", "ego4d-linear-nq10"])
def test_match_values_do_not_depend_on_the_batch_size(variant):
    """The adapter pair runs as the spread row GEMM (B nq <= 1024 rows), the rows chain (up to 20 480: rows_chain_supported) or
    the tiled GEMM (beyond), which the project holds bit-identical: the same windows at the head of batches of all three sizes
    give the same bits, and every later copy of a window its first copy's."""
    dev = _gpu()
    opt, sd, rows, cls, adapter, entries = R.matching_setup(variant)
    model = _model(variant)
    nq, E = opt.num_queries, len(entries)
    sizes = [E, -(-1280 // nq), 20480 // nq + 1]
    assert E * nq <= 1024 < sizes[1] * nq <= 20480 < sizes[2] * nq
    outs = []
    for B in sizes:
        args, ens = _gathered_inputs(rows, cls, entries, [i % E for i in range(B)], dev)
        outs.append(_bits(model.clip_matching_gathered(**args)))
    assert _compare(outs[0].view(torch.float32), entries, "small batch") <= TOL
    for B, o in zip(sizes[1:], outs[1:]):
        assert torch.equal(o[:E], outs[0]), B
        assert torch.equal(o, outs[0].repeat(-(-B // E), 1)[:B]), B
