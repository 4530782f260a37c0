"""The references, bounds and case families of tests/prefilter_refs.py, proved on the CPU: the two statements of the window
rule agree, the plain-fp32 / six-product restatement of every family stays inside its bound, the exact families are exact,
and every planted error of the model is caught by a named family -- with each family's blind spots listed and asserted."""
import numpy as np
import pytest
import torch

import prefilter_bf16_ref as R
import prefilter_refs as F
import row_refs as RR

POWER = dict(W=45, n=113, dv=256, nq=4)                 # S = 22 (a full and a partial tile), nh = 6, the last half window: 3 frames
POWER_Q0 = dict(W=45, n=113, dv=768, nq=40)             # dv > 512: 32 queries per launch, a second pass with q0 = 32


@pytest.mark.parametrize("W", [2, 3, 7, 90, 125])
@pytest.mark.parametrize("n", [1, 2, 44, 45, 46, 125, 313])
def test_the_two_statements_of_the_window_rule_agree(n, W):
    """Frame ranges (window_reduce) == half-window maxima + the odd-W first-frame term (window_scores_by_halves) == the model
    in either form, on every (n, W); and a NaN frame is skipped, a window without a number scores -inf."""
    c = F.unit(n, 256, 3, seed=n)
    sc = F.model_scores(c)                                   # over the poisoned arena
    fs = sc[:, F.PAD:F.PAD + n].clone()
    want = F.window_ref(fs, W)
    assert torch.equal(want, R.window_scores_by_halves(fs, W)) and want.shape[1] == F.n_half(n, W) + 1
    for form in ("stream", "tile"):
        fsb, win = F.model_run(sc.numpy(), n, W, form)
        assert torch.equal(win, want) and F.guards_intact(fsb, 3 * n)
        assert torch.equal(fsb[F.GUARD:F.GUARD + 3 * n].view(3, n), fs)
    fs[:, :] = float("nan")
    assert bool((F.window_ref(fs, W) == -np.inf).all())


def _shape(dv):
    return dict(W=45, n=max(113, dv + 3), dv=dv, nq=5)


@pytest.mark.parametrize("dv", F.DVS)
@pytest.mark.parametrize("family", F.FAMILIES)
def test_the_cpu_restatement_of_every_family_stays_inside_its_bound(family, dv):
    """Plain fp32 (torch's summation order) under the fp32 bound, the six kept products under the three-piece bound, through
    the model of either form: no failure of any check, the exact families included."""
    s = _shape(dv)
    for c in F.family_cases(family, s["n"], dv, s["nq"], s["W"]):
        for form in ("stream", "tile"):
            fails, worst = F.model_verdict(c, s["W"], form)
            assert not fails and worst <= 1.0, (family, dv, form, fails)
        fails, worst = F.model_verdict(c, s["W"], "tile", split=True)
        assert not fails and worst <= 1.0, (family, dv, "split", fails)


@pytest.mark.parametrize("dv", F.DVS)
def test_onehot_reaches_every_channel_and_the_six_products_reproduce_it(dv):
    """dv frames (queries, in the mirror case: as many as the GPU suite's largest query count allows) visit every channel;
    h + m + l == x exactly and the other three products are exact zeros, so the split form owes the exact value too."""
    n = dv
    assert {F.onehot_channel(f, dv) for f in range(n)} == set(range(dv))
    c = F.onehot(n, dv, 9)
    assert torch.equal(F.scores_split(c.ctx, c.cls), c.exact) and torch.equal(F.scores_f32(c.ctx, c.cls), c.exact)
    m = F.onehot_mirror(40, dv, dv)
    assert set(int(m.cls[q].argmax()) for q in range(dv)) == set(range(dv))
    assert torch.equal(F.scores_split(m.ctx, m.cls), m.exact) and torch.equal(F.scores_f32(m.ctx, m.cls), m.exact)
    h, mm, l = RR.split3(c.cls)
    assert torch.equal((l + mm) + h, c.cls)


@pytest.mark.parametrize("dv", F.DVS)
def test_pow2_scaling_is_exact_where_row_refs_says_it_is_safe(dv):
    """Rows x 2^20, queries x 2^-20 on the quantised base case: pow2_is_safe holds for both operands (no piece subnormal), and
    both restatements give the base case's bits."""
    base, sc = F.pow2_base(200, dv, 9), F.pow2(200, dv, 9)
    assert F.pow2_safe(base)
    assert torch.equal(F.scores_f32(sc.ctx, sc.cls), F.scores_f32(base.ctx, base.cls))
    assert torch.equal(F.scores_split(sc.ctx, sc.cls), F.scores_split(base.ctx, base.cls))
    # ... and the quantised products are exact in any order: the fp32 sum IS the float64 reference
    assert torch.equal(F.scores_f32(base.ctx, base.cls).double(), F.frame_ref(base.ctx, base.cls)[0])
    tiny = F.pow2_base(8, dv, 2)
    tiny.ctx = tiny.ctx * 2.0 ** -100                       # the proof refuses what would go subnormal
    assert not F.pow2_safe(F._case("x", tiny.ctx * 2.0 ** -20, tiny.cls))


def test_structural_frames_name_every_seam():
    """W = 45, n = 113: S = 22, half windows of a full and a 6-lane tile, a last half window of 3 frames."""
    s = F.structural_frames(113, 45)
    assert s["frame0"] == 0 and s["last"] == 112 and s["h1.first"] == 22 and s["h1.last"] == 43 and s["h1.second"] == 23
    assert s["h1.tile1.lane15"] == 37 and s["h1.tile1.lane0"] == 38 and s["h5.first"] == 110 and s["h5.last"] == 112
    assert {s[f"h1.end-{k}"] for k in range(1, 5)} == {39, 40, 41, 42}
    assert F.structural_frames(1, 90) == {"frame0": 0, "last": 0, "h0.first": 0, "h0.last": 0}
    rounds = F.peak_rounds(113, 45, 4)
    assert sorted(f for r in rounds for f in r) == sorted(set(s.values()))
    # odd W: the peak at (i+1) S is reported by window i (and i+1, i+2), not by window i-1
    c = F.peaks(113, 256, 4, [44, 44, 44, 44])
    win = F.window_ref(F.frame_ref(c.ctx, c.cls)[0], 45)
    assert [i for i in range(win.shape[1]) if win[0, i] > 0.5] == [1, 2, 3]
    assert F.edge_ctx_ls(90, 3) == [91, 92, 93, 94, 95, 134, 135] and F.MQ_W == (3, 7, 31, 32, 35, 63, 64, 67, 91, 124)


# Which family catches which planted error, per form: the table is computed, then held against what the structure of each
# family predicts (CATCHES lists at least these; BLIND lists exactly the families that can never see the error).
STRUCT = ("unit", "raw", "offset", "pow2", "onehot", "onehot2", "onehot_mirror", "peaks", "nanrows")
CATCHES = {
    # the term f[nh] is read from behind the plane: the next query's first score, or what lies behind the last query's row
    ("combine_le", "stream"): {"unit", "raw", "peaks", "onehot", "nanrows"},
    ("combine_le", "tile"): {"unit", "raw", "peaks", "onehot", "nanrows"},
    # only a window whose maximum IS frame (i+1) S changes: the peaks family puts one there on purpose
    ("odd_dropped", "stream"): {"peaks"},
    ("odd_dropped", "tile"): {"peaks"},
    ("fr_second", "stream"): {"peaks"},
    ("fr_second", "tile"): {"peaks"},
    # the spare lanes' scores are stored: into the next half window's frames and, behind the last query's row, into the guard
    ("valid_dropped", "tile"): set(STRUCT),
    # a unit that strides keeps the maximum of its previous half window: any family with nh > stride
    ("hm_not_reset", "stream"): {"unit", "raw", "peaks", "onehot", "nanrows"},
    ("hm_not_reset", "tile"): {"unit", "raw", "peaks", "onehot", "nanrows"},
    ("kslot_swap", "tile"): {"unit", "raw", "onehot", "onehot_mirror", "pow2"},
    ("kslot_swap", "split"): {"unit", "raw", "onehot", "onehot_mirror", "pow2"},
    ("q0_from_zero", "tile"): {"unit", "raw", "onehot", "peaks", "pow2"},
    # am fm is below the general three-piece bound: only a one-hot frame of two pieces (one product, bound 16 u) shows it
    ("drop_product", "split"): {"onehot2"},
}
BLIND = {
    # the spare ROWS stay masked by j0 + r < n: whichever row they read, no output changes.  The error is a read past the half
    # window -- past the video, at its end -- and nothing else; the poison surround is what keeps that read inside the buffer.
    ("row_clamp_S", "stream"): set(STRUCT),
    ("drop_product", "split"): {"onehot", "onehot_mirror", "pow2"},      # am or fm is zero in every product
    ("kslot_swap", "tile"): {"offset"},             # rows of one common value: a permutation of the channels changes nothing
    ("kslot_swap", "split"): {"offset"},            # beyond 0.03 N(0,1) x the query, far inside dv u 300 sum|q|
}


def _power_cases(family, s):
    return F.family_cases(family, s["n"], s["dv"], s["nq"], s["W"])


@pytest.mark.parametrize("fault,form", sorted(set(CATCHES) | {("row_clamp_S", "stream")}))
def test_every_planted_error_is_caught_by_a_named_family(fault, form):
    s = POWER_Q0 if fault == "q0_from_zero" else POWER
    split = form == "split"
    got = set()
    for family in STRUCT:
        hit = False
        for c in _power_cases(family, s):
            mform = "tile" if split else form
            clean, worst = F.model_verdict(c, s["W"], mform, None, split)
            assert not clean and worst <= 1.0, (family, clean)              # no case fails without a planted error
            hit |= F.caught(*F.model_verdict(c, s["W"], mform, fault, split))
        if hit:
            got.add(family)
    print(f"[power] {fault}/{form}: caught by {sorted(got)}")
    assert CATCHES.get((fault, form), set()) <= got, (fault, form, sorted(got))
    for family in BLIND.get((fault, form), ()):
        assert family not in got, (fault, form, family)
    if (fault, form) != ("row_clamp_S", "stream"):
        assert got, (fault, form)


def test_blind_spots_of_the_shapes():
    """hm_not_reset shows only where a unit takes a second half window (the grid-stride shapes); valid_dropped never shows in
    a window score, only in the stored frame scores and the guard; q0_from_zero needs more than 32 queries; a dropped odd-W
    term needs odd W."""
    s = POWER
    c = F.unit(s["n"], s["dv"], s["nq"])
    assert not F.caught(*F.model_verdict(c, s["W"], "tile", "hm_not_reset", stride=8))             # nh = 6 <= 8 units
    assert F.caught(*F.model_verdict(c, s["W"], "tile", "hm_not_reset", stride=4))
    sc = F.model_scores(c)
    _, win = F.model_run(sc.numpy(), c.n, s["W"], "tile", "valid_dropped")
    assert torch.equal(win, F.model_run(sc.numpy(), c.n, s["W"], "tile")[1])
    c32 = F.unit(s["n"], 768, 32)
    assert not F.caught(*F.model_verdict(c32, s["W"], "tile", "q0_from_zero"))
    p = F.family_cases("peaks", s["n"], s["dv"], s["nq"], 44)
    assert not any(F.caught(*F.model_verdict(x, 44, "stream", "odd_dropped")) for x in p)
    # the poison has power: a last half window taken as full (n = S) reads the rows behind the video
    arena, pad = F.poisoned(c.ctx)
    long = F._case("unit", arena[pad:pad + 6 * 22], c.cls)
    fails, _ = F.verdict(c, s["W"], None, F.window_ref(F.scores_f32(long.ctx, long.cls), s["W"])[:, :7])
    assert "win: a score of poison size" in fails


def test_suite_shapes_reach_every_launch_form():
    """The shape lists of the GPU suite against the launchers' thresholds (prefilter.hip): WPH = 4 with and without a
    grid-stride, WPH = 1 with and without; 16 / 32 / 64-query passes and q0 = 32 / 64 passes; the grouped grid-stride."""
    wide = [nh for nh in F.STREAM_NH if nh < 4096]
    assert any(nh <= 2048 for nh in wide) and any(nh > 2048 for nh in wide)                 # the barrier inside the stride loop
    long = [nh for nh in F.STREAM_NH if nh >= 4096]
    assert any((nh + 3) // 4 <= 2048 for nh in long) and any((nh + 3) // 4 > 2048 for nh in long)
    assert all(nh in F.STREAM_NH for nh in F.WIDE_NH)
    for dv, nqs in F.MQ_NQ.items():
        qpl = 64 if dv <= 512 else 32
        passes = set()
        for nq in nqs:
            q0 = 0
            while q0 < nq:
                rem = nq - q0
                wide_ = qpl == 64 and rem > 32
                passes.add((q0 > 0, 4 if wide_ else (1 if rem <= 16 else 2)))
                q0 += 64 if wide_ else 32
        want = {(False, 1), (False, 2), (True, 1), (True, 2)} | ({(False, 4), (True, 4)} if qpl == 64 else set())
        assert want <= passes, (dv, passes)
    assert F.GROUP_STRIDE_CLIPS > 2048 * 16 and max(F.EDGE_W) // 2 <= F.PAD
    assert {W // 2 for W in F.MQ_W} == {1, 3, 15, 16, 17, 31, 32, 33, 45, 62}
    assert {W // 2 for W in F.EDGE_W} == {45, 62} and {W // 2 for W in F.STREAM_W} == {1, 3}
