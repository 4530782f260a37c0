"""The kernels that turn numbers into what a user reads, pinned at their edge cases against the references of
tests/backend_refs.py (validated on the CPU by test_backend_kernels_cpu.py): stage C bit for bit at every chunk and wave edge of
fuse_nms_kernel -- counts, kept rows, first-occurrence index and the fill -- in both entry types and both launch forms; the
criterion's assignment against scipy's optimum within a derived bound and its losses against float64 at the kernel's own
assignment; adapter NCE, matcher cost, compose_rows and both metric kernels at their workgroup edges.  Needs an MI355X.

Which path a stage C list runs (postproc.hip, kMaxCand = 1024, 256 threads = 4 waves):
  n <= 64          one wave of one chunk: no prefix over s_cnt, no carry
  64 < n <= 256    one chunk: the wave prefix over s_cnt[0..wave)[0], nu_acc = 0
  n > 256          ceil(n / 256) chunks: the nu_acc carry, first / last found across chunks, s_cnt[.][1..3]
  nq <= 128        gridDim.y = 3, a workgroup per (query, score type); nq > 128: one workgroup walks the three types
criterion_window_kernel: 64-thread workgroups, one thread per window (B = 63 / 64 / 65 / 129); matcher_cost_kernel,
compose_rows_kernel, eval_recall_kernel, eval_window_recall_kernel: 256-thread workgroups, one thread per window / query."""
import numpy as np
import pytest
import torch

import backend_refs as R
from cone_amd import _lib, ops
from cone_amd.config import make_opt
from oracle import cone_oracle as O
from test_gpu_parity import record_measured

pytestmark = pytest.mark.gpu


def _gpu():
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------- stage C
def _padded(lists, n_max=None, dtype=np.float32):
    n_max = n_max or max(1, max(len(c) for c in lists))
    cand = np.zeros((len(lists), n_max, 4), dtype)
    for q, c in enumerate(lists):
        cand[q, :len(c)] = c
    return cand, np.asarray([len(c) for c in lists], np.int32)


def _fuse(cand, nv, par, **kw):
    dev = _gpu()
    rows, n, idx = ops.fuse_nms(torch.from_numpy(np.ascontiguousarray(cand)).to(dev), torch.from_numpy(nv).to(dev), *par, **kw)
    return rows.cpu().numpy(), n.cpu().numpy(), idx.cpu().numpy()


def _assert_expected(out, q, exp, what):
    rows, n, idx = out
    for t, (erows, eidx, ecnt) in enumerate(exp):
        assert int(n[t, q]) == ecnt, (what, t, int(n[t, q]), ecnt)
        assert np.array_equal(R.bits(rows[t, q]), R.bits(erows)), (what, t, "kept rows / zero fill")
        assert np.array_equal(idx[t, q], eidx), (what, t, "first-occurrence index / -1 fill")


SIZE_PARTS = (tuple(n for n in R.SIZES if n <= 513), (1023,), (1024,))      # the oracle takes ~2 s on a list of 1024 that keeps all


@pytest.mark.parametrize("part", range(len(SIZE_PARTS)))
@pytest.mark.parametrize("family", R.EVERY_SIZE)
@pytest.mark.parametrize("p", range(len(R.PARAMS)))
def test_stage_c_every_size_is_bit_exact(p, family, part):
    """One launch, one query per size 1 .. 1024: counts, kept rows, idx and the fill up to max_after against the oracle (each
    case checks its part of the 13 queries, so that the python reference stays within a few seconds per case)."""
    par = R.PARAMS[p]
    out = _fuse(*_padded([R.stage_c_case(family, n)[0] for n in R.SIZES], R.K_MAX_CAND), par)
    for q, n in enumerate(R.SIZES):
        if n in SIZE_PARTS[part]:
            _assert_expected(out, q, R.stage_c_expected_named(family, n, None, *par), (family, n, par))


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("p", range(len(R.PARAMS)))
def test_stage_c_named_families_are_bit_exact(p, part):
    par = R.PARAMS[p]
    queries = R.other_family_queries(p)
    assert 8 <= len(queries) <= 24
    out = _fuse(*_padded([R.stage_c_case(f, n)[0] for f, n in queries]), par)
    for q, (f, n) in list(enumerate(queries))[part::2]:          # (two lists of 1024 that keep all: one in each half)
        _assert_expected(out, q, R.stage_c_expected_named(f, n, None, *par), (f, n, par))


FORM_LISTS = [("dups_across_chunks", n) for n in R.SIZES] + [("all_ties", 257), ("round_ties", 63), ("chain", 64)]


@pytest.mark.parametrize("par", [(0.3, 200, 1024), (-1, 2000, 1024), (0.7, 300, 1)])
def test_stage_c_entry_and_launch_forms_are_bit_identical(par):
    """fp32 rows / pre-rounded fp64 rows, padded / cand_off, gridDim.y = 3 (nq = 16, 128) / 1 (nq = 129): the same lists give
    the same rows, counts and idx, element for element."""
    dev = _gpu()
    lists = [R.stage_c_case(f, n)[0] for f, n in FORM_LISTS]
    nq = len(lists)
    assert nq == 16
    cand, nv = _padded(lists)
    base = _fuse(cand, nv, par)
    for q, (f, n) in enumerate(FORM_LISTS):
        _assert_expected(base, q, R.stage_c_expected_named(f, n, None, *par), (f, n, par))
    same = lambda a, b: all(np.array_equal(R.bits(x) if x.dtype == np.float64 else x, R.bits(y) if y.dtype == np.float64 else y)
                            for x, y in zip(a, b))
    # cone_fuse_nms_f64 on the rows rounded by the reference's own float(f"{e:.4f}")
    c64, _ = _padded([np.asarray(O.round4_rows(c.tolist()), np.float64) for c in lists], dtype=np.float64)
    assert same(_fuse(c64, nv, par), base), "fp64 entry"
    # cand_off: one flat matrix, the lists in shuffled order, the gaps between them filled with rows that would win if read
    rng = np.random.default_rng(3)
    order = rng.permutation(nq)
    winner = np.asarray([1e4, 1e4 + 1, 9.0, 9.0])
    for dtype, src in ((np.float32, lists), (np.float64, [c64[q, :len(lists[q])] for q in range(nq)])):
        flat, off = [], np.zeros(nq, np.int64)
        for q in order:
            flat.append(np.tile(winner + q, (int(rng.integers(1, 6)), 1)).astype(dtype))
            off[q] = sum(len(f) for f in flat)
            flat.append(np.asarray(src[q], dtype))
        flat.append(np.tile(winner, (3, 1)).astype(dtype))
        got = _fuse(np.concatenate(flat), nv, par, cand_off=torch.from_numpy(off).to(dev), n_max=R.K_MAX_CAND)
        assert same(got, base), ("cand_off", dtype)
    # nq = 128 (a workgroup per score type) and nq = 129 (one workgroup per query): the lists tiled
    for reps, extra in ((8, 0), (8, 1)):
        ct = np.concatenate([np.tile(cand, (reps, 1, 1)), cand[:extra]])
        nt = np.concatenate([np.tile(nv, reps), nv[:extra]])
        assert len(nt) == 128 + extra
        got = _fuse(ct, nt, par)
        for r in range(reps):
            assert same([g[:, r * nq:(r + 1) * nq] for g in got], base), (len(nt), r)
        if extra:
            assert same([g[:, reps * nq:] for g in got], [b[:, :extra] for b in base]), "query 128"


def test_stage_c_n_valid_edges_and_padding_independence():
    """n_valid = 0, 1, > n_max in one batch; rows past n_valid[q] poisoned (NaN, and spans / scores that would rank first) give
    what the zero-padded batch gives."""
    n_max = 300
    lists = [np.zeros((0, 4), np.float32), R.stage_c_case("random", 1)[0], R.stage_c_case("random", 300)[0],
             R.stage_c_case("dups_across_chunks", 257)[0], R.stage_c_case("all_ties", 64)[0], np.zeros((0, 4), np.float32)]
    cand, nv = _padded(lists, n_max)
    said = nv.copy()
    said[2] = 500                                         # n_valid[q] > n_max behaves as n_max
    poisoned = cand.copy()
    for q, c in enumerate(lists):
        pad = poisoned[q, len(c):]
        pad[0::2] = np.nan
        pad[1::2] = (2e4, 2e4 + 5, 7.0, 7.0)
    for par in ((0.5, 100, 100), (-1, 200, 5), (0.0, 200, 301)):
        zero = _fuse(cand, said, par)
        for q, c in enumerate(lists):
            _assert_expected(zero, q, R.stage_c_expected(c, *par), (q, len(c), par))
        for t in range(3):
            assert zero[1][t, 0] == 0 and not zero[0][t, 0].any() and (zero[2][t, 0] == -1).all(), "n_valid = 0"
        pois = _fuse(poisoned, said, par)
        for z, p_ in zip(zero, pois):
            assert np.array_equal(z.view(np.int64) if z.dtype == np.float64 else z, p_.view(np.int64) if p_.dtype == np.float64 else p_)


@pytest.mark.parametrize("family", ["chain", "nested", "all_ties", "random", "zero_length"])
def test_temporal_nms_matches_the_oracle(family):
    for n in (2, 255, 256, 257, 1024):
        pred = R.nms_list(family, n)
        thds = (-1,) if family == "zero_length" else ((0.1,) if n == 1024 else (0.1, 0.5))      # zero_length: uni == 0, IoU 0 > -1
        for thd in thds:
            for ma in (5, n + 7) if n > 5 else (1, n + 7):       # max_after below and above n
                assert ops.temporal_nms([list(p) for p in pred], thd, ma) == O.temporal_nms(pred, thd, ma), (family, n, thd, ma)


def test_stage_c_refusals_name_the_limit():
    dev = _gpu()
    nv = torch.tensor([1], dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ConeHipError, match=r"n_max=1025 not in \[1,1024\]"):
        ops.fuse_nms(torch.zeros(1, 1025, 4, device=dev), nv, 0.5, 200, 5)
    with pytest.raises(_lib.ConeHipError, match="fuse_nms: bad limits"):
        ops.fuse_nms(torch.zeros(1, 8, 4, device=dev), nv, 0.5, 200, 1025)
    with pytest.raises(_lib.ConeHipError, match="fuse_nms: bad limits"):
        ops.fuse_nms(torch.zeros(1, 8, 4, device=dev), nv, 0.5, 0, 5)
    with pytest.raises(_lib.ConeHipError, match=r"temporal_nms: n=1025 not in \[1,1024\]"):
        ops.temporal_nms([[float(i), i + 1.5, 0.5] for i in range(1025)], 0.5, 5)


# ------------------------------------------------------------------------------------------------------------- compose_rows
@pytest.mark.parametrize("Nq", [1, 5, 16])
def test_compose_rows_at_the_workgroup_edges_with_tied_scores(Nq):
    from types import SimpleNamespace
    dev = _gpu()
    worst = 0.0
    for B in (1, 255, 256, 257):
        logits, spans, match, dur, vs = R.compose_case(B, Nq)
        for clip_len in (0.535, 0.2):
            for sort in (True, False):
                opt = SimpleNamespace(clip_length=clip_len, no_sort_results=not sort)
                ref = torch.tensor(O.compose_rows(opt, logits, spans, match, dur.tolist(), vs.tolist()), dtype=torch.float64)
                got = ops.compose_rows(logits.to(dev), spans.to(dev), match.to(dev), dur.to(dev), vs.to(dev), clip_len, sort)
                got = got.cpu().double()
                assert torch.equal(got[..., :2], ref[..., :2]), (B, Nq, clip_len, sort)     # st / ed: the stable order shows here
                assert torch.equal(got[..., 3], ref[..., 3])
                err = float((got[..., 2] - ref[..., 2]).abs().max())
                assert err < 1e-6
                worst = max(worst, err)
        if Nq > 1:
            assert bool((ref[:, 1:, 2] == ref[:, :-1, 2]).any()), "the case holds exact score ties"
    record_measured("backend.compose_rows", Nq=Nq, worst_over_tol=worst / 1e-6)


def test_compose_rows_refuses_17_slots():
    dev = _gpu()
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(_lib.ConeHipError, match=r"compose_rows: Nq=17 not in \[1,16\]"):
        ops.compose_rows(z(2, 17, 2), z(2, 17, 2), z(2, 17), torch.ones(2, dtype=torch.int32, device=dev),
                         torch.zeros(2, dtype=torch.int32, device=dev), 0.5)


# ------------------------------------------------------------------------------------------------------------- criterion
def _criterion(Nq, **kw):
    from cone_amd.criterion import build_criterion
    return build_criterion(make_opt("ego4d", num_queries=Nq, **{**R.HYPER, **kw}))


def _run_layer(crit, c, dev, neg, sal=None):
    from cone_amd.criterion import _layer_losses
    outputs = dict(pred_logits=c.logits.to(dev), pred_spans=c.spans.to(dev))
    targets = dict(span_labels=[dict(spans=t) for t in c.tgt])
    neg_out = dict(pred_logits=c.neg_logits.to(dev)) if neg else None
    if sal is not None:
        s, pos, ng, nsal = sal
        outputs["saliency_scores"] = s.to(dev)
        targets.update(saliency_pos_labels=pos, saliency_neg_labels=ng)
        if neg:
            neg_out["saliency_scores"] = nsal.to(dev)
    vals, assign = _layer_losses(crit.matcher, crit, outputs, targets, neg_out, want_saliency=sal is not None)
    names = ("loss_span", "loss_giou", "loss_label", "class_error", "loss_saliency")
    return dict(zip(names, vals.cpu().tolist())), assign.cpu().numpy(), (outputs, targets, neg_out)


def _check_assignment(c, assign):
    """Partial permutation of exactly min(Nq, T) pairs; float64 cost within the bound of scipy's optimum; equal to scipy's
    where the optimum is unique by more than twice the bound.  -> (worst excess / bound, windows with a unique optimum)."""
    worst, unique = 0.0, 0
    for b in range(c.B):
        T = c.tgt[b].shape[0]
        assert R.is_partial_permutation(assign[b], T), (b, assign[b].tolist(), T)
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
            assert assign[b].tolist() == a.tolist(), (b, assign[b].tolist(), a.tolist())
    return worst, unique


@pytest.mark.parametrize("family", R.CRIT_FAMILIES)
def test_criterion_assignment_and_losses(family):
    dev = _gpu()
    worst_a, worst_l = 0.0, {}
    for B in R.CRIT_BATCHES:
        c = R.crit_case(family, B)
        crit = _criterion(c.Nq)
        for neg in (False, True):
            got, assign, _ = _run_layer(crit, c, dev, neg)
            if not neg:
                wa, unique = _check_assignment(c, assign)
                worst_a = max(worst_a, wa)
            ref = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, assign, neg_logits=c.neg_logits if neg else None)
            for k, v in ref.items():
                ok, ratio = R.within(got[k], v)
                print(f"[backend] criterion {family} B={B} neg={neg} {k}: got {got[k]!r} ref {v!r} err/tol {ratio:.3f}")
                worst_l[k] = max(worst_l.get(k, 0.0), ratio)
                assert ok, (family, B, neg, k, got[k], v)
    record_measured("backend.criterion", family=family, assign_excess_over_bound=worst_a,
                    **{k + "_over_tol": v for k, v in worst_l.items()})


def test_criterion_public_entry_equals_the_layer_call_and_all_windows_empty():
    dev = _gpu()
    c = R.crit_case("empty_mixed", 65)
    crit = _criterion(c.Nq)
    got, assign, (outputs, targets, _) = _run_layer(crit, c, dev, False)
    pub = crit(outputs, targets)
    assert {k: float(v) for k, v in pub.items()} == {k: got[k] for k in pub} and "loss_saliency" in pub
    pairs = crit.matcher(outputs, targets)
    for b, (i, j) in enumerate(pairs):
        assert i.tolist() == [n for n in range(c.Nq) if assign[b, n] >= 0] and j.tolist() == [int(x) for x in assign[b] if x >= 0]
    # every window empty: the means of nothing are NaN as in the reference, loss_label is finite
    for B in (1, 65):
        c = R.crit_case("random", B)
        c = type(c)(**{**vars(c), "tgt": [torch.zeros(0, 2) for _ in range(B)]})
        for neg in (False, True):
            got, assign, _ = _run_layer(_criterion(c.Nq), c, dev, neg)
            assert (assign == -1).all()
            assert all(np.isnan(got[k]) for k in ("loss_span", "loss_giou", "class_error")), got
            ref = R.losses64(R.HYPER, c.logits, c.spans, c.tgt, assign, neg_logits=c.neg_logits if neg else None)
            assert np.isfinite(got["loss_label"]) and R.within(got["loss_label"], ref["loss_label"])[0]


@pytest.mark.parametrize("L,P,L2", [(1, 1, 3), (75, 2, 90), (128, 2, 75), (128, 1, 1)])
def test_criterion_saliency_and_negative_window(L, P, L2):
    dev = _gpu()
    worst = 0.0
    for B in (1, 65):
        c = R.crit_case("random", B)
        sal = R.saliency_case(B, L, P, L2)
        assert B == 1 or L == 1 or bool((sal[1] < 0).any()), "negative label indices: the host wraps them"
        for margin in (0.0, 0.2):
            hyper = {**R.HYPER, "saliency_margin": margin}
            crit = _criterion(c.Nq, saliency_margin=margin)
            for neg in (False, True):
                got, assign, _ = _run_layer(crit, c, dev, neg, sal)
                ref = R.losses64(hyper, c.logits, c.spans, c.tgt, assign, neg_logits=c.neg_logits if neg else None,
                                 saliency=sal[0], pos_idx=sal[1].numpy(), neg_idx=sal[2].numpy(), neg_saliency=sal[3] if neg else None)
                for k, v in ref.items():
                    ok, ratio = R.within(got[k], v)
                    assert ok, (L, P, L2, B, margin, neg, k, got[k], v)
                    worst = max(worst, ratio)
    record_measured("backend.criterion_saliency", L=L, P=P, L2=L2, worst_over_tol=worst)


def test_criterion_refuses_more_than_8_slots_or_targets():
    dev = _gpu()
    c = R.crit_case("random", 1)
    crit = _criterion(c.Nq)
    targets = dict(span_labels=[dict(spans=torch.rand(9, 2))])
    with pytest.raises(NotImplementedError, match="more than 8 target spans"):      # on the host: the kernel trusts tgt_off
        crit(dict(pred_logits=c.logits.to(dev), pred_spans=c.spans.to(dev)), targets)
    with pytest.raises(_lib.ConeHipError, match="criterion: bad sizes B=1 Nq=9"):
        crit(dict(pred_logits=torch.zeros(1, 9, 2, device=dev), pred_spans=torch.rand(1, 9, 2, device=dev)),
             dict(span_labels=[dict(spans=torch.rand(2, 2))]))


@pytest.mark.parametrize("n", R.NCE_SIZES)
def test_adapter_nce_within_the_derived_bound(n):
    dev = _gpu()
    sim = R.nce_case(n)
    worst = 0.0
    for T in R.NCE_TEMPS:
        got = float(_criterion(5, temperature=T).loss_adapter(dict(logits_per_video=sim.to(dev)))["loss_adapter"])
        ref = R.adapter_nce64(sim, T)
        bound = R.nce_bound(sim, T, ref)
        print(f"[backend] adapter_nce n={n} T={T}: got {got!r} ref {ref!r} err {abs(got - ref):.3e} bound {bound:.3e}")
        assert abs(got - ref) <= bound, (n, T, got, ref, bound)
        worst = max(worst, abs(got - ref) / bound)
    record_measured("backend.adapter_nce", n=n, worst_over_bound=worst)


@pytest.mark.parametrize("Nq", [1, 5, 8])
def test_matcher_cost_at_the_workgroup_edges(Nq):
    dev = _gpu()
    worst = 0.0
    for B in (1, 255, 256, 257):
        lg, sp, tg = R.matcher_case(B, Nq)
        C, best, gap = R.matcher_reference64(lg, sp, tg)
        cost, got = ops.matcher_cost(lg.to(dev), sp.to(dev), tg.to(dev))
        err = float(np.abs(cost.cpu().numpy() - C).max())
        assert err < 1e-5, (B, Nq, err)
        worst = max(worst, err / 1e-5)
        got = got.cpu().numpy()
        clear = gap > R.MATCHER_GAP
        assert clear.mean() >= 0.98 and np.array_equal(got[clear], best[clear]), (B, Nq)
        ties = gap == 0
        assert np.array_equal(got[ties], best[ties]), "an exact tie returns the lower index"
        assert Nq == 1 or B < 51 or ties[50]
    record_measured("backend.matcher_cost", Nq=Nq, worst_over_tol=worst)


# ------------------------------------------------------------------------------------------------------------- metrics
def _rows_tensor(preds, gts, A, poison, dev):
    """(nq, A, 5) rows; past a query's own list: zeros, or alternately a copy of its target (an IoU-1 hit) and NaN."""
    rows = torch.zeros(len(preds), A, 5, dtype=torch.float64)
    for q, p in enumerate(preds):
        rows[q, :len(p)] = torch.tensor(p, dtype=torch.float64)
        if poison:
            rows[q, len(p)::2, 0], rows[q, len(p)::2, 1] = gts[q][0], gts[q][1]
            rows[q, len(p) + 1::2] = float("nan")
    return rows.to(dev)


def _check_recall(preds, gts, rows, n, thr, ks, dev):
    from cone_amd import metrics as M
    gt = torch.tensor(gts, dtype=torch.float64, device=dev)
    sub = [{"query_id": f"q{q}", "predicted_times": p} for q, p in enumerate(preds)]
    gtl = [{"query_id": f"q{q}", "timestamps": g} for q, g in enumerate(gts)]
    with np.errstate(all="ignore"):
        assert torch.equal(M.evaluate_nlq_performance_mad(rows, n, gt, thr, ks), O.evaluate_nlq_performance_mad(sub, gtl, thr, ks))
    ov = [O.iou_f64(p, g) for p, g in zip(preds, gts)]
    hits, top1 = M.recall_counts(rows, n, gt, thr, ks, 0)
    assert np.array_equal(top1.cpu().numpy(), np.array([o[0] for o in ov]), equal_nan=True)
    want = [[sum(bool((o > th)[:k].any()) for o in ov) for k in ks] for th in thr]
    assert hits.cpu().tolist() == want
    _, top1f = M.recall_counts(rows, n, gt, thr, ks, 1)
    f32 = [float(O.iou_f32(torch.tensor(p, dtype=torch.float64)[:, :2], torch.tensor(g, dtype=torch.float64))[0]) for p, g in zip(preds, gts)]
    assert np.array_equal(top1f.cpu().numpy(), np.array(f32), equal_nan=True)


@pytest.mark.parametrize("nq", [1, 255, 256, 257])
def test_recall_kernels_do_not_read_past_a_querys_count(nq):
    dev = _gpu()
    preds, gts = R.metric_random_lists(nq)
    n = torch.tensor([len(p) for p in preds], dtype=torch.int32, device=dev)
    A = 12 + 4
    thr, ks = [0.1, 0.3, 0.5], [1, 5, 10, 50]
    _check_recall(preds, gts, _rows_tensor(preds, gts, A, True, dev), n, thr, ks, dev)
    # n[q] > A is clamped: no room past the longest list, and the full-length queries claim 5 rows more than there are
    A = max(len(p) for p in preds)
    over = torch.tensor([len(p) + (5 if len(p) == A else 0) for p in preds], dtype=torch.int32, device=dev)
    _check_recall(preds, gts, _rows_tensor(preds, gts, A, True, dev), over, thr, ks, dev)


def test_recall_on_crafted_spans_and_capacity_limits():
    from cone_amd import metrics as M
    dev = _gpu()
    preds, gts, _ = R.metric_crafted_lists()
    n = torch.tensor([len(p) for p in preds], dtype=torch.int32, device=dev)
    rows = _rows_tensor(preds, gts, 5, True, dev)
    _check_recall(preds, gts, rows, n, [0.3, 0.5, 0.7, 0.01], [1, 2, 5], dev)
    thr8 = [0.05, 0.1, 0.3, 0.5, 0.7, 0.9, 0.95, 0.99]
    k16 = list(range(1, 16)) + [1000]                      # 8 thresholds x 16 K values; one K far beyond A
    _check_recall(preds, gts, rows, n, thr8, k16, dev)
    gt = torch.tensor(gts, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.ConeHipError, match=r"at most 8 thresholds and 16 K values \(got 9, 16\)"):
        M.recall_counts(rows, n, gt, thr8 + [0.999], k16, 0)
    with pytest.raises(_lib.ConeHipError, match=r"at most 8 thresholds and 16 K values \(got 8, 17\)"):
        M.recall_counts(rows, n, gt, thr8, k16 + [2000], 1)
    wi = torch.zeros(len(preds), 4, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.ConeHipError, match=r"at most 8 thresholds and 16 K values \(got 0, 17\)"):
        M.windows_selection(wi, gt, k16 + [2000], 0.535, 90)


@pytest.mark.parametrize("clip_length", [0.535, 0.2, 1.0])
def test_window_recall_on_boundary_targets_and_terminated_lists(clip_length):
    from cone_amd import metrics as M
    dev = _gpu()
    ranks, gtl = R.window_cases(clip_length)
    nq = len(gtl)
    gt = torch.tensor([g["timestamps"] for g in gtl], dtype=torch.float64, device=dev)
    for topK, K in (([1, 2, 3, 5, 10], 12), ([1, 3, 50], 7)):          # K below max(topK): the table ends before it
        wi = torch.full((nq, K), -1, dtype=torch.int32)
        for q in range(nq):
            r = ranks[f"q{q}"][:K]
            wi[q, :len(r)] = torch.tensor(r, dtype=torch.int32)
        want = O.windows_selection(ranks, gtl, topK, clip_length, 90)
        assert torch.equal(M.windows_selection(wi.to(dev), gt, topK, clip_length, 90), want)
        assert 0 < float(want[-1]) < 1
    # a -1 terminator followed by a hitting index: the list ended, the hit must not count
    short = {q: r[:1] for q, r in ranks.items()}
    wi = torch.full((nq, 6), -1, dtype=torch.int32)
    for q in range(nq):
        lo = int(np.floor(float(gt[q, 0]) / clip_length / 45))
        wi[q, 0], wi[q, 2] = short[f"q{q}"][0], lo
    want = O.windows_selection(short, gtl, [1, 5], clip_length, 90)
    assert torch.equal(M.windows_selection(wi.to(dev), gt, [1, 5], clip_length, 90), want) and float(want[1]) == 0.0
