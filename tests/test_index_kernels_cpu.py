"""The references of tests/index_refs.py, validated before the GPU tests (test_index_kernels_gpu.py) trust them: the stable
top-k against torch.sort, the float64 pooling + match against the reference's own fixtures and the oracle's slices, and the
POWER of every crafted matching case -- a slice moved by one clip must move the float64 value by at least 10 TOL.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import index_refs as R
import inputs as gi
from cone_amd import synth
from cone_amd.config import make_opt
from oracle import cone_oracle as O

SIZES = [(1, 1), (65, 30), (257, 257), (4097, 65), (8193, 30), (12289, 256)]


@pytest.mark.parametrize("n,k", SIZES)
def test_topk_reference_is_the_stable_sort_on_nan_free_rows(n, k):
    for seed in range(3):
        rows = R.topk_rows(n, k, seed)
        assert set(rows) == set(R.NAN_FREE) | set(R.WITH_NAN)
        for name in R.NAN_FREE:
            x = rows[name]
            assert x.shape == (n,) and not torch.isnan(x).any(), name
            assert not ((x != 0) & (x.abs() < 2.0 ** -126)).any(), (name, "denormals stay out")
            sv, si = torch.sort(x, descending=True, stable=True)
            idx, val = R.topk_reference(x, k)
            assert torch.equal(idx.long(), si[:k]), (name, n, k, seed)
            assert torch.equal(val.view(torch.int32), sv[:k].view(torch.int32)), (name, n, k, seed)     # bits: the zero's sign too


def test_topk_rows_differ_between_seeds_and_hold_what_they_claim():
    a, b = R.topk_rows(12289, 30, 0), R.topk_rows(12289, 30, 1)
    for name in a:
        if name != "all_nan":
            assert not torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
    z = a["signed_zero"]
    assert (z.view(torch.int32) == -2 ** 31).any() and (z.view(torch.int32) == 0).any()      # -0.0 and +0.0
    assert int(torch.isposinf(a["pos_inf"]).sum()) >= 3 and torch.isneginf(a["neg_inf"]).any()
    # one_lane: the 16 largest values sit in one thread's slots of one chunk; one_wave: the 96 largest in wave 0 of one chunk
    top = torch.sort(a["one_lane"], descending=True, stable=True)[1][:16]
    assert len({int(i) % 256 for i in top}) == 1 and len({int(i) // R.TK_CH for i in top}) == 1
    top = torch.sort(a["one_wave"], descending=True, stable=True)[1][:96]
    assert all(int(i) % 256 < 64 for i in top) and len({int(i) // R.TK_CH for i in top}) == 1


@pytest.mark.parametrize("n,k", SIZES)
def test_topk_reference_nan_rule(n, k):
    """A NaN is never selected; the numbers keep their stable order; what is left over is (-1, -inf)."""
    for seed in range(3):
        rows = R.topk_rows(n, k, seed)
        for name in R.WITH_NAN:
            x = rows[name]
            idx, val = R.topk_reference(x, k)
            numbers = [i for i in range(n) if not torch.isnan(x[i])]
            want = sorted(numbers, key=lambda i: (-float(x[i]), i))[:k]        # Python's sort is stable; (-0.0 == 0.0)
            m = len(want)
            assert idx[:m].tolist() == want and torch.equal(val[:m], x[want]), (name, n, k)
            assert (idx[m:] == -1).all() and torch.isneginf(val[m:]).all(), (name, n, k)
            assert not torch.isnan(val).any()
        assert torch.isnan(rows["nan_sprinkled"]).any() or n < 8
        assert int((~torch.isnan(rows["nan_few_left"])).sum()) < k and torch.isnan(rows["all_nan"]).all()


def test_threshold_selection_overflows_on_one_wave_and_not_on_noise():
    """Which branch of the two-level form a row reaches, from the selection's own rule (R.fast_select_survivors): the chunk
    that holds the planted values of ``one_wave`` has a wave with more than 64 survivors at k = 30 and 64 (the pass-based
    fallback runs there), a ``randn`` chunk has none at k = 30 (the threshold selection itself answers)."""
    for n in (8193, 12289):
        for k in (30, 64):
            x = R.topk_rows(n, k, 0)["one_wave"]
            chunk = int(torch.argmax(x)) // R.TK_CH
            assert max(R.fast_select_survivors(x[chunk * R.TK_CH:(chunk + 1) * R.TK_CH], k)) > 64, (n, k)
        x = R.topk_rows(n, 30, 0)["randn"]
        assert max(R.fast_select_survivors(x[:R.TK_CH], 30)) <= 64
        last = (n - 1) // R.TK_CH * R.TK_CH
        assert R.fast_select_survivors(x[last:], 30)[0] == n - last == 1            # a last chunk shorter than k: all survive


def _fixture_case(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    if "meta" in fx.files:
        meta = json.loads(str(fx["meta"]))
        opt = make_opt(meta["preset"], **meta["opt"])
    else:
        opt = make_opt(str(fx["preset"]))
    sd = synth.make_state_dict(opt, int(fx["weight_seed"]))
    assert synth.state_dict_checksum(sd) == str(fx["weight_checksum"])
    lens_v = fx["lens_v"].tolist()
    inp = gi.stage_b_inputs(opt, int(fx["input_seed"]), lens_v, fx["lens_q"].tolist())
    assert gi.checksum(inp["src_vid"], inp["src_txt"], inp["src_cls_txt"]) == str(fx["input_checksum"])
    return fx, opt, sd, inp, lens_v


@pytest.mark.parametrize("name", ["stageB_ego4d", "stageB_mad", "stageB_shape_128x4_prenorm"])
def test_pooled_match_reference_reproduces_the_reference_fixtures(golden_dir, name):
    """The ``matching`` column the reference wrote, from the fixture's own ``pred_spans``, within TOL -- every proposal whose
    boundaries stay 1e-3 away from an integer (there the reference's fp32 products decide, not the exact ones)."""
    fx, opt, sd, inp, lens_v = _fixture_case(golden_dir, name)
    adapter = R.adapter_of(sd) if opt.adapter_module == "linear" else None
    pad = max(lens_v)
    n_chk, worst = 0, 0.0
    for b, vlen in enumerate(lens_v):
        spans = fx["pred_spans"][b]
        got, s, e = R.pooled_match_reference(inp["src_vid"][b], vlen, pad, spans, inp["src_cls_txt"][b], adapter)
        for n in range(spans.shape[0]):
            c, w = float(spans[n, 0]), float(spans[n, 1])
            x1, x2 = (c - w / 2) * vlen, (c + w / 2) * vlen
            if abs(x1 - round(x1)) < 1e-3 or abs(x2 - round(x2)) < 1e-3:
                continue
            want = float(fx["matching"][b, n])
            assert np.isnan(got[n]) == np.isnan(want), (b, n)
            if not np.isnan(want):
                worst = max(worst, abs(got[n] - want))
            n_chk += 1
    assert n_chk >= 0.9 * fx["matching"].size and worst < R.TOL, (n_chk, worst)


@pytest.mark.parametrize("vlen,pad", R.WINDOW_SHAPES)
def test_dyadic_spans_give_the_oracles_slices(vlen, pad):
    """(s, e) of the exact arithmetic = the oracle's fp32 O.proposal_slices on every span of the 2^-7 grid the tests use, and
    each named case is what its name says."""
    cases = R.dyadic_spans(vlen, pad)
    spans = torch.tensor([[c, w] for _, c, w, _ in cases], dtype=torch.float32)
    assert torch.equal(spans.double() * 128, (spans.double() * 128).round())            # c and w / 2 on the grid (w = 2 hw)
    mask = torch.zeros(1, pad)
    mask[0, :vlen] = 1
    start, end, prop = O.proposal_slices(spans[None], mask)
    for i, (name, c, w, in_range) in enumerate(cases):
        s, e = R.exact_slice(c, w, vlen)
        assert (int(start[0, i]), int(end[0, i])) == (s, e), name
        assert in_range == (0 <= c <= 1 and 0 <= w <= 1) and e >= 1, name
        assert in_range or name in ("empty_s_eq_end", "empty_s_gt_pad"), name
        n_pool = min(e, pad) - s
        if name.startswith("len_"):
            assert n_pool == int(name[4:]) and e <= vlen
        if name.startswith("empty") or name == "w0_on_integer":
            assert n_pool <= 0
        if name == "empty_s_gt_pad":
            assert s > pad
        if name == "empty_s_eq_end":
            assert s == min(e, pad) and w > 0
        if name == "zero_rows":
            assert vlen < e <= pad and s < vlen
        if name == "clamped":
            assert e > pad
        if name == "negative_x1":
            assert c - w / 2 < 0 and s == 0
        if name == "w0_off_integer":
            assert w == 0 and n_pool == 1
        if name == "both_integral":
            assert float(prop[0, i, 0]).is_integer() and float(prop[0, i, 1]).is_integer() and n_pool >= 2
        if name == "full_window":
            assert (s, e) == (0, vlen)
    # the case list as a whole: everything the kernel distinguishes is reached on some shape
    everywhere = {n for v, p in R.WINDOW_SHAPES for n, *_ in R.dyadic_spans(v, p)}
    assert everywhere == {"both_integral", "negative_x1", "len_1", "len_7", "len_8", "len_9", "len_16", "len_17", "zero_rows",
                          "clamped", "empty_s_eq_end", "empty_s_gt_pad", "w0_on_integer", "w0_off_integer", "full_window"}


@pytest.mark.parametrize("variant", [v[0] for v in R.MATCH_VARIANTS])
def test_crafted_matching_cases_have_power_and_match_the_oracle(variant):
    """Every crafted case the GPU test feeds: (1) a neighbouring slice that is another answer lies >= 10 TOL away in float64 (no
    case exempt); (2) the float64 value is the oracle's fp32 O.clip_matching on the same zero-padded window within TOL, NaN
    where it has NaN; (3) the slices are the oracle's."""
    opt, sd, rows, cls, adapter, entries = R.matching_setup(variant)
    assert R.assert_power(rows, cls, adapter, entries) >= R.POWER
    assert {(e["vlen"], e["pad_len"]) for e in entries} == set(R.WINDOW_SHAPES)
    tsd = O.as_torch_sd(sd)
    worst = 0.0
    for en in entries:
        vid = torch.zeros(1, en["pad_len"], rows.shape[1])
        vid[0, :en["vlen"]] = torch.from_numpy(rows[:en["vlen"]])
        mask = torch.zeros(1, en["pad_len"])
        mask[0, :en["vlen"]] = 1
        sp = torch.from_numpy(en["spans"])[None]
        start, end, _ = O.proposal_slices(sp, mask)
        assert start[0].tolist() == en["s"].tolist() and end[0].tolist() == en["e"].tolist()
        want = O.clip_matching(tsd, opt, torch.from_numpy(cls[en["cls_j"]])[None], vid, mask, sp)[0].double().numpy()
        assert (np.isnan(want) == np.isnan(en["ref"])).all(), en["names"]
        ok = ~np.isnan(want)
        worst = max(worst, float(np.abs(want[ok] - en["ref"][ok]).max()) if ok.any() else 0.0)
    assert worst < R.TOL, worst
