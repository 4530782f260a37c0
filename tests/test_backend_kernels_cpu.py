"""The references and case families of tests/backend_refs.py earn their keep before test_backend_kernels_gpu.py trusts them:
they reproduce the oracle and the reference's recorded outputs, the fp32 arithmetic of the kernels stays inside every bound
that the GPU suite asserts, and every case family catches a NAMED planted error in a python model of the kernel's algorithm
(the mutant -> family maps below).  CPU only."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import backend_refs as R
from oracle import cone_oracle as O

SMALL = {f: R.OTHER_SIZES.get(f, (63,))[0] for f in R.STAGE_C_FAMILIES}


# ------------------------------------------------------------------------------------------------------------- stage C
@pytest.mark.parametrize("family", list(R.STAGE_C_FAMILIES))
def test_stage_c_expected_is_the_oracle_plus_first_occurrence(family):
    for n in (SMALL[family], 257):
        cand, _ = R.stage_c_case(family, n)
        rows4 = O.round4_rows(cand.tolist())
        rd = O.score_fusion(rows4)
        for thd, mb, ma in R.PARAMS:
            opt = SimpleNamespace(nms_thd=thd, max_before_nms=mb, max_after_nms=ma)
            exp = R.stage_c_expected(cand, thd, mb, ma)
            assert R.same_result(exp, R.stage_c_expected_named(family, n, None, thd, mb, ma))
            for (rows, idx, cnt), col in zip(exp, R.TYPE_COL):
                ref = O.post_processing_mr_nms(opt, rd, col)
                assert cnt == len(ref) and rows[:cnt].tolist() == ref, (family, n, thd)
                assert rows.shape == (ma, 5) and not rows[cnt:].any() and (idx[cnt:] == -1).all()
                for j in range(cnt):        # idx: the FIRST candidate with the kept row's key
                    key = [rows[j, 0], rows[j, 1]]
                    assert rows4[idx[j]][:2] == key and all(r[:2] != key for r in rows4[:idx[j]])


def test_stage_c_families_hold_what_they_claim():
    c = lambda f, n: R.stage_c_case(f, n)[0].astype(np.float64)
    d = c("dups_across_chunks", 1024)
    assert np.array_equal(d[768:, :2], d[:256, :2]) and not np.array_equal(d[768:, 2:], d[:256, 2:])
    assert np.array_equal(d[258, :2], d[256, :2]) and np.array_equal(d[259, :2], d[257, :2])          # A B A B
    assert len({tuple(r) for r in c("all_same_key", 257)[:, :2]}) == 1
    assert len({tuple(r) for r in c("two_keys", 257)[:, :2]}) == 2
    t = c("ties_across_chunks", 1024)
    assert np.array_equal(t[:256, 2:], t[768:, 2:]) and len(set(t[:256, 2])) == 256
    assert len(set(c("const_prop", 257)[:, 2])) == 1 and len(set(c("const_match", 257)[:, 3])) == 1
    t = c("touching", 257)
    assert np.array_equal(t[:-1, 1], t[1:, 0])
    z = c("zero_length", 64)
    assert np.array_equal(z[:, 0], z[:, 1]) and np.array_equal(z[0::2, 0], z[1::2, 0])
    r = c("round_ties", 257)
    assert np.all(np.abs(r[np.arange(257) % 8 < 6, :2] * 1e4 % 1) == 0.5), "st / ed: exact halves at the 4th decimal"
    assert np.all(r[:, 2] * 1e4 % 1 == 0.5) and r[:, 0].max() > 8192 and r[:, 0].min() < 0
    rounded = np.asarray(O.round4_rows(r.tolist()))
    assert (np.signbit(rounded) & (rounded == 0)).any(), "a value rounds to -0.0"
    for fam, sizes in R.OTHER_SIZES.items():
        assert sizes[0] <= 64 and sizes[1:] == (257, 1024) and fam not in R.EVERY_SIZE
    assert set(R.OTHER_SIZES) | set(R.EVERY_SIZE) == set(R.STAGE_C_FAMILIES) == set(R.OTHER_PARAMS) | set(R.EVERY_SIZE)


def test_stage_c_references_reproduce_the_recorded_outputs(golden_dir):
    with open(os.path.join(golden_dir, "stageC.json")) as f:
        fx = json.load(f)
    modelled = set()
    for case in fx["fusion_nms"]:
        rows = np.asarray(case["rows"], np.float64)
        par = (case["nms_thd"], case["max_before_nms"], case["max_after_nms"])
        exp = R.stage_c_expected(rows, *par)
        for (r, _, cnt), key in zip(exp, ("fused", "proposal", "matching")):
            assert r[:cnt].tolist() == case[key]
        if (len(rows), par) not in modelled and len(rows) <= 150:      # the model once per list length and parameter set
            modelled.add((len(rows), par))
            assert R.same_result(exp, R.stage_c_model(rows, *par))
    for case in fx["temporal_nms"][:30]:
        pred = [list(p) for p in case["pred"]]
        keep = R.temporal_nms_model(pred, case["nms_thd"], case["max_after_nms"])
        assert [pred[i] for i in keep] == case["out"] == O.temporal_nms(pred, case["nms_thd"], case["max_after_nms"])


@pytest.mark.parametrize("family", list(R.STAGE_C_FAMILIES))
def test_unmutated_model_equals_the_oracle(family):
    sizes = (SMALL[family], 257) + ((513,) if family in R.EVERY_SIZE else ())
    for n in sizes:
        cand, _ = R.stage_c_case(family, n)
        for par in (R.PARAMS if n <= 257 else R.PARAMS[3:5]):
            assert R.same_result(R.stage_c_model(cand, *par), R.stage_c_expected_named(family, n, None, *par)), (family, n, par)


# mutant -> (family, n, parameter set) that must tell it from the oracle: at a size <= 257 for every mutant, and at a size
# > 256 for the two chunk mutants (n = 257 is both: one candidate in the second chunk)
CATCHERS = {
    "first_value_wins": [("dups_across_chunks", 63, (-1, 2000, 1024))],
    "last_position": [("dups_across_chunks", 63, (-1, 2000, 1024)), ("zero_length", 64, (0.0, 200, 5))],
    "no_chunk_carry": [("all_ties", 257, (-1, 2000, 1024)), ("random", 513, (0.3, 200, 1024)),
                       ("dups_across_chunks", 511, (-1, 2000, 1024))],
    "no_wave_prefix": [("random", 255, (-1, 2000, 1024)), ("all_ties", 257, (0.5, 100, 100)), ("random", 513, (0.3, 200, 1024))],
    "rank_tie_le": [("all_ties", 64, (-1, 2000, 1024)), ("ties_across_chunks", 257, (0.3, 200, 1024))],
    "rank_tie_absent": [("all_ties", 64, (0.5, 100, 100)), ("ties_across_chunks", 64, (-1, 2000, 1024))],
    "ge_thd": [("touching", 64, (0.0, 200, 5)), ("two_keys", 63, (0.0, 200, 5))],
    "max_before_ignored": [("random", 257, (0.5, 100, 100)), ("chain", 257, (0.3, 200, 1024))],
    "round_half_away": [("round_ties", 63, (-1, 2000, 1024))],
}
# what a mutant is NOT caught by: the regimes that made the old suite blind (one chunk, no ties, no duplicates).  A LONE unique
# key in the last chunk or wave (n = 257, 65) only swaps two unique entries when the slot it should have taken reads as 0: the
# kept rows change under ties alone -- which is why all_ties runs at 257
BLIND = {
    "no_chunk_carry": [("random", 256, (-1, 2000, 1024)), ("dups_across_chunks", 255, (0.3, 200, 1024)),
                       ("random", 257, (-1, 2000, 1024))],
    "no_wave_prefix": [("random", 64, (-1, 2000, 1024)), ("random", 65, (-1, 2000, 1024))],
    "rank_tie_absent": [("chain", 64, (0.3, 200, 1024))],
    "first_value_wins": [("chain", 64, (-1, 2000, 1024))],
    "round_half_away": [("chain", 64, (-1, 2000, 1024))],
}


@pytest.mark.parametrize("mutant", list(CATCHERS))
def test_every_planted_error_is_caught_by_a_named_family(mutant):
    for family, n, par in CATCHERS[mutant]:
        cand, _ = R.stage_c_case(family, n)
        assert not R.same_result(R.stage_c_model(cand, *par, mut=(mutant,)), R.stage_c_expected_named(family, n, None, *par)), \
            (mutant, family, n, par)
    for family, n, par in BLIND.get(mutant, ()):
        cand, _ = R.stage_c_case(family, n)
        assert R.same_result(R.stage_c_model(cand, *par, mut=(mutant,)), R.stage_c_expected_named(family, n, None, *par)), \
            (mutant, family, n, par, "expected to be invisible here")
    assert set(CATCHERS) | {"uni_unguarded"} == set(R.STAGE_C_MUTATIONS)


def test_unguarded_zero_union_shows_only_without_the_dict():
    """Equal keys collapse in the dict, so fuse_nms never meets uni == 0; temporal_nms takes duplicate zero-length spans as
    they come, and with a negative threshold IoU 0 > thd suppresses where 0 / 0 = nan > thd does not."""
    cand, _ = R.stage_c_case("zero_length", 64)
    for par in R.PARAMS:
        assert R.same_result(R.stage_c_model(cand, *par, mut=("uni_unguarded",)), R.stage_c_expected_named("zero_length", 64, None, *par))
    pred = R.nms_list("zero_length", 64)
    want = O.temporal_nms(pred, -1, 100)
    assert [pred[i] for i in R.temporal_nms_model(pred, -1, 100)] == want
    assert [pred[i] for i in R.temporal_nms_model(pred, -1, 100, mut=("uni_unguarded",))] != want


@pytest.mark.parametrize("family", ["chain", "nested", "all_ties", "random", "zero_length"])
def test_temporal_nms_model_equals_the_oracle(family):
    for n in (2, 255, 257):
        pred = R.nms_list(family, n)
        for thd, ma in ((0.5, 5), (0.0, n + 7), (0.1, 100)):
            assert [pred[i] for i in R.temporal_nms_model(pred, thd, ma)] == O.temporal_nms(pred, thd, ma)


# ------------------------------------------------------------------------------------------------------------- criterion
def _shapes():
    return [(nq, t) for nq in range(1, 9) for t in range(1, 9) if nq * t <= 30]


def test_assign_optimum64_equals_brute_force_on_every_small_shape():
    costs = (R.HYPER["set_cost_span"], R.HYPER["set_cost_giou"], R.HYPER["set_cost_class"])
    rng = np.random.default_rng(5)
    for nq, t in _shapes():
        lg = torch.tensor(rng.standard_normal((2, nq, 2)), dtype=torch.float32)
        sp = torch.tensor(np.stack([rng.uniform(.1, .9, (2, nq)), rng.uniform(.02, .6, (2, nq))], -1), dtype=torch.float32)
        tg = [torch.tensor(np.stack([rng.uniform(.1, .9, t), rng.uniform(.02, .6, t)], -1), dtype=torch.float32) for _ in range(2)]
        ref = O.hungarian_indices(costs, lg, sp, tg)
        for b in range(2):
            C = R.cost_matrix64(lg[b], sp[b], tg[b])
            a, cost = R.assign_optimum64(C)
            want = np.full(nq, -1)
            want[ref[b][0]] = ref[b][1]
            assert a.tolist() == want.tolist(), (nq, t)
            allc, alla = R.all_assignment_costs64(C)
            k = int(allc.argmin())
            assert abs(allc[k] - cost) < 1e-12 and alla[k].tolist() == a.tolist()
            assert abs(R.assignment_cost64(C, a) - cost) < 1e-12


def test_float64_criterion_reproduces_the_recorded_outputs(golden_dir):
    with open(os.path.join(golden_dir, "criterion.json")) as f:
        fx = json.load(f)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    tgt = [t(x).reshape(-1, 2) for x in fx["tgt"]]
    neg, sal = fx["neg"], t(fx["saliency"])
    for layer, ikey, suffix in ((1, "idx", ""), (0, "idx_aux", "_0")):
        lg, sp = t(fx["layers"][layer]["pred_logits"]), t(fx["layers"][layer]["pred_spans"])
        assign = np.full(lg.shape[:2], -1)
        for b in range(lg.shape[0]):
            a, _ = R.assign_optimum64(R.cost_matrix64(lg[b], sp[b], tgt[b]))
            assign[b] = a
            got = [[n for n in range(len(a)) if a[n] >= 0], [int(j) for j in a if j >= 0]]
            assert got == fx[ikey][b]
        for key, with_neg in (("losses_with_neg", True), ("losses_without_neg", False)):
            kw = dict(neg_logits=t(neg["pred_logits"])) if with_neg else {}
            if layer == 1:
                kw.update(saliency=sal, pos_idx=np.asarray(fx["pos_idx"]), neg_idx=np.asarray(fx["neg_idx"]))
                if with_neg:
                    kw["neg_saliency"] = t(neg["saliency_scores"])
            got = R.losses64(fx["hyper"], lg, sp, tgt, assign, **kw)
            for k, v in got.items():
                assert R.within(fx[key][k + suffix], v)[0], (key, k + suffix, v, fx[key][k + suffix])
    want = fx["loss_adapter"]["loss_adapter"]
    ref = R.adapter_nce64(t(fx["sim"]), fx["hyper"]["temperature"])
    assert abs(want - ref) <= R.nce_bound(t(fx["sim"]), fx["hyper"]["temperature"], ref)


def _dp_check(c, assign):
    """The GPU suite's assignment assertions on one case; returns the worst excess / bound and how many windows were unique."""
    worst, unique = 0.0, 0
    for b in range(c.B):
        T = c.tgt[b].shape[0]
        assert R.is_partial_permutation(assign[b], T), (b, assign[b], T)
        if T == 0:
            continue
        C = R.cost_matrix64(c.logits[b], c.spans[b], c.tgt[b])
        a, opt = R.assign_optimum64(C)
        bound = R.assign_bound(C, c.Nq)
        excess = R.assignment_cost64(C, assign[b]) - opt
        assert excess <= bound, (b, excess, bound)
        worst = max(worst, excess / bound)
        allc = np.sort(R.all_assignment_costs64(C)[0])
        if len(allc) == 1 or allc[1] - allc[0] > 2 * bound:
            unique += 1
            assert assign[b].tolist() == a.tolist(), b
    return worst, unique


@pytest.mark.parametrize("family", R.CRIT_FAMILIES)
def test_fp32_dp_stays_inside_the_assignment_bound_and_fp32_losses_inside_the_tolerance(family):
    c = R.crit_case(family, 33)
    assign = R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt)
    worst, unique = _dp_check(c, assign)
    assert worst <= 1.0
    if family not in ("twin_slots", "twin_targets"):
        assert unique >= c.B // 2, "most windows of this family have a unique optimum"
    else:
        assert unique < c.B, "this family has tied optima"
    # plain fp32 (the oracle's torch arithmetic) at ITS assignment against float64 at the same assignment
    keep = [b for b in range(c.B) if c.tgt[b].shape[0] > 0][:3]          # (the oracle's assignment is brute force: 8! sums)
    lg, sp, tg, ng = c.logits[keep], c.spans[keep], [c.tgt[b] for b in keep], c.neg_logits[keep]
    for neg in (None, ng):
        ref32, idx = O.criterion_layer(R.HYPER, lg, sp, tg, neg_logits=neg)
        a = np.full(lg.shape[:2], -1)
        for b, (i, j) in enumerate(idx):
            a[b, list(i)] = list(j)
        ref64 = R.losses64(R.HYPER, lg, sp, tg, a, neg_logits=neg)
        for k, v in ref64.items():
            assert R.within(ref32[k], v)[0], (family, k, float(ref32[k]), v)


def test_criterion_planted_errors_are_caught_by_named_families():
    # the DP walks the larger side: no assignment of min(Nq, T) pairs comes out on rectangular windows
    for family in ("wide", "tall"):
        c = R.crit_case(family, 64)
        bad = R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt, mut=("dp_walks_larger_side",))
        assert sum(not R.is_partial_permutation(bad[b], c.tgt[b].shape[0]) for b in range(c.B)) >= c.B // 2, family
    c = R.crit_case("square8", 1)       # ... and a square window cannot see it
    assert np.array_equal(R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt, mut=("dp_walks_larger_side",)),
                          R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt))
    # background weight on the matched slots: loss_label moves past its tolerance
    for family in ("random", "sharp_logits"):
        c = R.crit_case(family, 64)
        a = R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt)
        ref = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a)
        bad = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a, planted=("bg_weight_on_matched",))
        assert R.within(bad["loss_label"], ref["loss_label"])[1] > 10, family
    # l0 >= l1 made strict: class_error moves where a matched slot has l0 == l1
    for family in ("twin_slots", "sharp_logits"):
        c = R.crit_case(family, 64)
        a = R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt)
        ref = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a)
        bad = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a, planted=("tie_strict",))
        assert R.within(bad["class_error"], ref["class_error"])[1] > 10, family
    c = R.crit_case("random", 64)
    a = R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt)
    assert R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a, planted=("tie_strict",)) == R.losses64(R.HYPER, c.logits, c.spans, c.tgt, a)


@pytest.mark.parametrize("mutant", ["from_not_reset", "k_gt_ns_not_skipped"])
def test_two_dp_lines_are_not_observable_on_finite_costs(mutant):
    """``from[mask] = 0`` and ``if (k > ns) continue`` cannot change an assignment while every cost is finite: a state with
    k <= ns items is written by its first finite candidate before the backtrack reads it, and states with k > ns are never
    read (the final scan takes popcount == ns only).  No family can catch them -- shown here rather than assumed; a NaN cost
    (the zero-width pair excluded in DESIGN.md) is where ``from[mask] = 0`` matters."""
    for family in R.CRIT_FAMILIES:
        c = R.crit_case(family, 33)
        assert np.array_equal(R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt, mut=(mutant,)),
                              R.criterion_dp_model(R.HYPER, c.logits, c.spans, c.tgt)), family


def test_crit_families_hold_what_they_claim():
    for B in R.CRIT_BATCHES:
        c = R.crit_case("empty_mixed", B)
        assert c.tgt[0].shape[0] > 0 and (B < 2 or c.tgt[1].shape == (0, 2))
    c = R.crit_case("disjoint", 64)
    assert all((R.giou64(c.spans[b], c.tgt[b]) < 0).all() for b in range(64))
    c = R.crit_case("out_of_unit", 64)
    assert float(c.spans[..., 0].min()) < 0 and float(c.spans[..., 0].max()) > 1
    c = R.crit_case("sharp_logits", 64)
    d = (c.logits[..., 0] - c.logits[..., 1]).abs()
    assert set(d.unique().tolist()) == {0.0, 60.0} and float(c.logits.abs().max()) > 9e3
    c = R.crit_case("square8", 64)
    assert c.Nq == 8 and all(t.shape[0] == 8 for t in c.tgt)
    assert R.crit_case("single_slot", 64).Nq == 1 and R.crit_case("tall", 64).Nq == 2


# ------------------------------------------------------------------------------------------------------------- adapter NCE
@pytest.mark.parametrize("n", R.NCE_SIZES)
def test_fp32_adapter_nce_stays_inside_its_bound_and_a_maxless_softmax_does_not(n):
    sim = R.nce_case(n)
    for T in R.NCE_TEMPS:
        ref = R.adapter_nce64(sim, T)
        bound = R.nce_bound(sim, T, ref)
        assert abs(R.adapter_nce_f32(sim, T) - ref) <= bound, (n, T)
        assert abs(float(O.adapter_nce(sim, T)) - ref) <= bound, (n, T)
    if n > 1:       # exp(100) overflows fp32: the planted error is infinitely far outside at the sharp temperature
        ref = R.adapter_nce64(sim, 0.01)
        err = abs(R.adapter_nce_f32(sim, 0.01, use_max=False) - ref)
        assert not err <= 10 * R.nce_bound(sim, 0.01, ref)


# ------------------------------------------------------------------------------------------------------------- matcher cost
@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("Nq", [1, 5, 8])
def test_matcher_cases_keep_the_small_gap_windows_under_the_cap(B, Nq):
    lg, sp, tg = R.matcher_case(B, Nq)
    C, best, gap = R.matcher_reference64(lg, sp, tg)
    assert (gap <= R.MATCHER_GAP).mean() <= 0.02
    ref32 = O.matcher_cost((10.0, 1.0, 4.0), lg, sp, tg).view(B, Nq, B)
    ref32 = ref32[torch.arange(B), :, torch.arange(B)].numpy()
    assert np.abs(ref32 - C).max() < 1e-5
    if Nq > 1:
        assert B < 51 or (gap[50] == 0 and best[50] == (1 if Nq > 2 else 0)), "an exact tie at the minimum, lower index first"


# ------------------------------------------------------------------------------------------------------------- metrics
def test_crafted_metric_spans_sit_on_the_thresholds():
    preds, gts, notes = R.metric_crafted_lists()
    ov = [O.iou_f64(p, g) for p, g in zip(preds, gts)]
    assert ov[0][0] == 0.3 and ov[1][0] == 0.5 and ov[2][0] == 0.5 and ov[2][1] > 0.5
    assert np.isnan(ov[6][0]) and ov[4][0] == 0.0 and ov[9].tolist() == [0.0, 0.0]
    f32 = [O.iou_f32(torch.tensor(p, dtype=torch.float64)[:, :2], torch.tensor(g, dtype=torch.float64)) for p, g in zip(preds, gts)]
    assert float(f32[0][0]) == float(np.float32(0.3)) and float(f32[1][0]) == 0.5 and torch.isnan(f32[6][0])


@pytest.mark.parametrize("clip_length", [0.535, 0.2, 1.0])
def test_window_cases_hit_and_miss_where_they_say(clip_length):
    ranks, gtl = R.window_cases(clip_length)
    got = O.windows_selection(ranks, gtl, [1, 2, 3, 5, 10], clip_length, 90)
    n = len(gtl)
    # per target: rank-3 hit, rank-5 hit, a miss (hi itself), a miss (lo - 1; or no such window when lo = 0)
    assert got.tolist() == [0.0, 0.0, 0.25, 0.5, 0.5], got
    assert n == 32
