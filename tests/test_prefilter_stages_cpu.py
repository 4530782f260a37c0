"""tests/prefilter_stage_refs.py held against itself and against the older restatements, on the CPU: the vectorised window
rule, the families' exactness claims under torch's own fp32 / bf16 arithmetic, the stage model against
prefilter_certified_ref and a brute-force float64 top-k, and -- for every planted error of the issue -- which named case of
the model changes its answer and which families cannot see it."""
import numpy as np
import pytest
import torch

import prefilter_bf16_ref as R
import prefilter_certified_ref as C
import prefilter_refs as F
import prefilter_stage_refs as G


def _nan_to_neg(x):
    return torch.where(torch.isnan(x), torch.full_like(x, G.NEG), x)


# ------------------------------------------------------------------------------------------------ the window rule
@pytest.mark.parametrize("n,W", [(1, 2), (1, 90), (2, 3), (5, 2), (7, 3), (100, 7), (101, 90), (44, 91), (17, 35), (129, 64),
                                 (130, 65)])
def test_windows_of_is_the_window_rule(n, W):
    fs = torch.randn(3, n, generator=F._g(n, W)).double()
    fs[0, n // 2] = G.NAN
    fs[1] = G.NAN                                                   # no number at all: every window -inf
    got = G.windows_of(fs, W)
    assert torch.equal(got, R.window_reduce(_nan_to_neg(fs), W))
    assert torch.equal(got, R.window_scores_by_halves(_nan_to_neg(fs), W))
    assert torch.equal(got, C.window_scores(_nan_to_neg(fs), W))
    assert bool((got[1] == G.NEG).all()) and got.shape[1] == G.n_windows(n, W) == R.num_windows(n, W)


# ------------------------------------------------------------------------------------------------ A: the families
@pytest.mark.parametrize("dv", [32, 96, 288, 544, 1024])
def test_quantum_is_exact_in_every_summation_order(dv):
    """fp32 running sums over five random channel orders (and the ascending one) equal the float64 value bit for bit, and
    the scaled family has the same bits: the premise of `the float64 value, whatever the form`."""
    n, nq = 23, 5
    base, up = G.quantum(n, dv, nq, seed=dv), G.quantum_up(n, dv, nq, seed=dv)
    ref, ab = R.frame_scores(base.ctx, base.cls)
    assert torch.equal(base.ctx.bfloat16().float(), base.ctx) and torch.equal(up.ctx.bfloat16().float(), up.ctx)
    assert torch.equal(up.cls.bfloat16().float(), up.cls)
    assert float(ab.max()) <= 1024 and float((ref * 4096).frac().abs().max()) == 0.0        # sums on 2^-12, below 2^10
    g = F._g(77, dv)
    for order in [None] + [torch.randperm(dv, generator=g) for _ in range(5)]:
        assert torch.equal(G.model_scores16(base, order=order).double(), ref)
        assert torch.equal(G.model_scores16(up, order=order).double(), ref)
    assert torch.equal(R.frame_scores(up.ctx, up.cls)[0], ref)


@pytest.mark.parametrize("W", [2, 3, 7, 35, 90])
def test_dictated_rows_yield_the_chosen_scores(W):
    """Under torch's fp32 arithmetic on the bf16-rounded operands the frame score is s_q c_f exactly (NaN where c_f is),
    and the family holds what it claims: an all-negative half window, -0.0 beside +0.0, -inf, a NaN among numbers, a window
    of NaN only."""
    n = 40 * (W // 2) - 1
    c = G.dictated(n, 96, 6, W, seed=W)
    got = G.model_scores16(c).double()
    assert F.same(got, c.exact_fs)
    v = c.values
    assert bool(torch.isnan(v).any()) and bool((v == G.NEG).any()) and bool((v < 0).any())
    assert bool(((v == 0) & torch.signbit(v)).any()) and bool(((v == 0) & ~torch.signbit(v)).any())
    w = G.windows_of(c.exact_fs, W)
    assert bool((w == G.NEG).any()) and not bool(torch.isnan(w).any())
    assert bool((w[0] < 0).any()) and bool((w[1] > 0).any())
    nan_only = [i for i in range(w.shape[1]) if bool(torch.isnan(v[max((i - 1) * (W // 2), 0):(i - 1) * (W // 2) + W]).all())]
    assert nan_only and all(float(w[0, i]) == G.NEG for i in nan_only)


def test_a_sum_of_products_cannot_be_negative_zero():
    """Why the `+ 0.f` of pf_key cannot be seen through the public entries: every form starts its sum at +0.0 (an accumulator
    of zeros, `float s = 0.f`), and +0 + (-0) = +0 under round to nearest.  A row of -0.0 scores +0.0, so no coarse window
    score is ever -0.0; the model is told about -0.0 directly (zeros_mixed) and DOES change its answer without the + 0."""
    c = G._case("dictated", torch.full((4, 32), -0.0), torch.ones(1, 32))
    s = G.model_scores16(c)
    assert bool((s == 0).all()) and not bool(torch.signbit(s).any())
    assert G.pf_key(np.float32(-0.0)) == G.pf_key(np.float32(0.0)) == 0x80000000
    assert G.pf_key(np.float32(-0.0), plus_zero=False) == 0x7fffffff


def test_pf_key_orders_like_the_floats():
    v = np.array([G.NEG, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, float("inf")], dtype=np.float32)
    k = G.pf_key(v).astype(np.int64)
    assert (np.diff(k) >= 0).all() and (np.diff(k) == 0).sum() == 1 and k.min() > 0


# ------------------------------------------------------------------------------------------------ B: the index rows
def test_index_rows_hold_what_they_claim():
    x = G.index_rows(5, 256, "midpoints")
    h = x.bfloat16().float()
    half_ulp = (torch.nextafter(h.abs().bfloat16(), torch.tensor(float("inf")).bfloat16()).float() - h.abs()) / 2
    d = x - h
    assert bool((d != 0).all()) and bool((d > 0).any()) and bool((d < 0).any())          # rounded down AND up
    lo_bits = x.view(torch.int32) & 0xffff
    assert bool((lo_bits == 0x8000).all())
    assert bool(((h.view(torch.int32) >> 16) & 1 == 0).all())                            # ... always to the even neighbour
    assert bool((d.abs() <= half_ulp).all())
    s = G.index_rows(4, 256, "subnormal")
    assert bool((s[1::2].abs() < 2.0 ** -126).all()) and bool((s[1::2] != 0).all()) and bool((s[::2].abs() >= 2.0 ** -126).all())
    m = G.index_rows(5, 8, "f32max")
    assert bool(torch.isinf(m.bfloat16().float()).any()) and bool(torch.isfinite(m).all())
    z = G.index_rows(3, 16, "negzero")
    assert bool(torch.signbit(z[:, 0]).all())
    nrow = G.index_rows(65537, 4, "nan")
    assert int(torch.isnan(nrow).any(dim=1).sum()) == 1 and not bool(torch.isnan(nrow[-1]).any())
    assert float(nrow[-1].norm()) > float(torch.nan_to_num(nrow[:-1], nan=0.0).norm(dim=1).max())
    assert G.INDEX_INFLATE > C.INFLATE


# ------------------------------------------------------------------------------------------------ C: the stage model
@pytest.mark.parametrize("seed", range(6))
def test_stage_model_on_honest_inputs(seed):
    """Honest arenas: whatever the proof says, the list is the brute-force float64 top-k of the exact windows; where the
    float64 margin of prefilter_certified_ref is far from E the flag is the one it predicts; both flags occur."""
    W, k, n_cand, dv = 4, 2, 4, 256
    vid, cls = F._unit(2000, dv, 1, seed), F._unit(4, dv, 2, seed)
    case = G.honest_case(vid, cls, W, k, n_cand)
    idx, val, cert, _ = G.stage_model(case)
    ew = G.windows_of(case.exact_fs, W)
    for q in range(4):
        want = G.brute_topk(ew[q], k)
        m, E = C.margin(vid, cls[q], W, k, n_cand)
        if abs(m - E) > 0.02 * E:
            assert int(cert[q]) == int(m > E), (seed, q, m, E)
        if int(cert[q]):                    # the theorem: a certified list IS the exact top-k
            assert idx[q].tolist() == want
        assert idx[q].tolist() == want and val[q].tolist() == ew[q][want].tolist()
        assert abs(G.bound_E(case, q) - E) <= 1e-12 * E


def test_stage_model_certifies_some_and_refuses_some_honest_queries():
    flags = []
    for seed in range(6):
        case = G.honest_case(F._unit(2000, 256, 1, seed), F._unit(4, 256, 2, seed), 4, 2, 4)
        flags += G.stage_model(case)[2].tolist()
    assert 0 < sum(flags) < len(flags), flags


def test_solve_R0_inverts_the_header_formula():
    for dv, a in ((256, 1.0), (1024, 1.0), (256, 1 + 2.0 ** -12), (1024, 1 + 2.0 ** -12)):
        case = G.comparison_case(dv=dv, a=a)
        assert case.g > 0.1 and float(np.float64(case.g)) == case.g
        R0 = G.solve_R0(case, 0, case.g)
        assert R0 > 0 and abs(G.bound_E(case, 0, R=R0) - case.g) <= 1e-13 * case.g
        below, above = float(np.float32(R0 * (1 - 2.0 ** -20))), float(np.float32(R0 * (1 + 2.0 ** -20)))
        assert below < R0 < above                                   # fp32's spacing of R (2^-24 relative) keeps the sides
        assert G.stage_model(case, R=below)[2].tolist() == [1] and G.stage_model(case, R=above)[2].tolist() == [0]
    assert G.bound_E(G.threshold_case(1.0), 0) == 2.0 ** -113


def test_dictated_arenas_give_the_chosen_scores_in_torch_arithmetic():
    for case in G.cpu_named_cases():
        v32, v16 = G.dictated_arenas(case)
        assert F.same(v32 @ case.cls.t(), case.exact_fs.t())
        assert F.same(v16.float() @ case.cls.bfloat16().float().t(), case.coarse_fs.t())


def test_rescore_model_le_reads_the_clamped_row_again():
    """`f0 + r <= hi`: the extra slot's row index is clamped to the window's last frame, which the max already holds."""
    fs = torch.randn(301, generator=F._g(5)).tolist()
    fs[7] = G.NAN
    for W in (2, 3, 5, 63, 64, 65, 129):
        w = G.windows_of(torch.tensor([fs], dtype=torch.float64), W)[0].tolist()
        for i in range(G.n_windows(301, W)):
            assert G.rescore_model(fs, i, W) == G.rescore_model(fs, i, W, le=True) == w[i]


# ------------------------------------------------------------------------------------------------ the planted errors
BLIND_STAGE = {
    "tie_bit29": "the index bisection loses bit 30 only: it needs a tie at a window index >= 2^30, a 4 GiB score row",
    "rescore_le": "the extra row slot is clamped to the window's last frame, already in the max (rescore_model)",
}
BLIND_SCORER = {
    "mq_nnxt_long": "the k-steps loaded past the row are never multiplied (`kb + s < nks` guards the MFMA loop); they stay "
                    "inside the poisoned buffer",
}


def _answer(case, fault=None):
    idx, val, cert, _ = G.stage_model(case, fault)
    return idx.tolist(), val.tolist(), cert.tolist()


def test_every_planted_stage_error_changes_a_named_case():
    cases = G.cpu_named_cases()
    base = {c.name: _answer(c) for c in cases}
    kinds = sorted({c.name.split("/")[0] + "/" + c.name.split("/")[1] if c.name.startswith("visible") else c.name.split("/")[0]
                    for c in cases})
    for fault in G.STAGE_FAULTS:
        seen = [c.name for c in cases if _answer(c, fault) != base[c.name]]
        seen_kinds = {k for k in kinds if any(s.startswith(k) for s in seen)}
        print(f"[stage faults] {fault}: {len(seen)} of {len(cases)} cases change; blind: {sorted(set(kinds) - seen_kinds)}")
        if fault in BLIND_STAGE:
            print(f"[stage faults] {fault}: no case can see it -- {BLIND_STAGE[fault]}")
            assert not seen, (fault, seen)
        else:
            assert seen, fault
    # the named witnesses
    see = lambda fault, name: _answer(next(c for c in cases if c.name == name), fault) != base[name]
    assert see("key_no_plus_zero", "visible/zeros_mixed/nw700/nc64")
    assert see("tie_lt", "visible/tie_at_ncand/nw700/nc64") and see("tie_lt", "visible/all_equal/nw700/nc64")
    assert not see("tie_lt", "visible/distinct/nw65/nc64")          # (its one tie pair lies away from the boundary)
    assert see("certify_ge", "threshold/gap==E") and not see("certify_ge", "threshold/t==c_last")
    assert see("cmin_from_exact", "visible/distinct/nw700/nc64") and see("cmin_from_exact", "mixed/10/nw700/k8/W2")


def test_every_planted_scorer_error_and_who_sees_it():
    """half_block_le is seen only by non-numbers behind a row (dictated) at dv below 512 VPL; every number times the zero
    query share is 0, poison included."""
    W = 7
    for dv in (96, 544):
        for fam in G.SCORER_FAMILIES:
            c = G.scorer_case(fam, 40, dv, 3, W, seed=1 if fam != "dictated" else 0)
            good = G.windows_of(G.model_scores16(c), W)
            bad = G.windows_of(G.model_scores16(c, "half_block_le"), W)
            assert not G.scorer_verdict(c, W, good)[0], (fam, dv)
            sees = bool(G.scorer_verdict(c, W, bad)[0])
            print(f"[scorer faults] half_block_le dv={dv} family={fam}: {'seen' if sees else 'blind'}")
            assert sees == (fam == "dictated"), (fam, dv)
    c = G.dictated(40, 512, 3, W)                                      # dv = 512 VPL: no lane behind the row
    assert F.same(G.model_scores16(c, "half_block_le"), G.model_scores16(c))
    for fault, why in BLIND_SCORER.items():
        print(f"[scorer faults] {fault}: no case can see it -- {why}")
    assert set(BLIND_SCORER) | {"half_block_le"} == set(G.SCORER_FAULTS)
