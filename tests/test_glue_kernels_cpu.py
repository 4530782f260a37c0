"""The references of tests/glue_refs.py deserve trust, and the case families of tests/test_glue_kernels_gpu.py see every
planted error: no GPU here.

  * sine_rows64 against the oracle's sine_position on masks of every length, window_table_ref against the oracle's
    window_bounds in build_batch's row order and against inference.window_table's torch index arithmetic, txt_pos64 / saliency64 / rowdot64
    against torch in float64;
  * one planted error per family in a Python model of each kernel: a float family has to move by >= 10 bounds, an integer
    family has to change an integer; where a case of a family CANNOT see an error it is named and asserted blind;
  * the inputs of the sine bound: the CPU's own fp32 sin / cos error on the table's arguments, the smallest planted distance,
    and their ratio."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import glue_refs as G
import row_refs as R
from oracle import cone_oracle as O


# ------------------------------------------------------------------------------------------------ the references
def test_sine_rows_match_the_oracle_on_masks_of_every_length():
    lvs = G.SINE_LVS
    L = max(lvs)
    worst = 0.0
    for lv in lvs:
        mask = torch.zeros(1, L)
        mask[0, :lv] = 1
        ref = O.sine_position(mask, 256)[0, :lv].double().numpy()
        worst = max(worst, float(np.abs(ref - G.sine_rows64(lv, 256)).max()))
    # the oracle is fp32 end to end: the same argument bit for bit, then the CPU's fp32 sin / cos
    assert worst <= 2 * G.U, worst
    assert worst == pytest.approx(G.sine_cpu_error(), rel=1e-6)


@pytest.mark.parametrize("d", [64, 128, 320, 512])
def test_sine_rows_match_the_oracle_at_other_widths(d):
    for lv in (1, 2, 64, 255, 1023):
        mask = torch.ones(1, lv)
        ref = O.sine_position(mask, d)[0].double().numpy()
        assert float(np.abs(ref - G.sine_rows64(lv, d)).max()) <= 2 * G.U


def test_dim_t_is_the_formula():
    """dim_t32 is fp32: the exponent e <= 1 is rounded once (U / 2 relative), which pow turns into ln(10000) e U / 2 <= 4.7 U, and
    pow rounds once more; 8 U covers both."""
    for d in (64, 128, 256, 320, 512):
        i = np.arange(d)
        exact = 10000.0 ** (2 * (i // 2) / d)
        assert float(np.abs(G.dim_t32(d) / exact - 1).max()) <= 8 * G.U
        from cone_amd.model import _dim_t_table
        assert G.same_bits(G.dim_t32(d), _dim_t_table(d))       # what the model hands the library


def test_table_layout():
    t = G.table_rows64(7, 64)
    assert t.shape == (G.table_row_count(7), 64) and not t[-1].any()
    for lv in range(1, 8):
        assert np.array_equal(t[lv * (lv - 1) // 2: lv * (lv - 1) // 2 + lv], G.sine_rows64(lv, 64))
    assert np.array_equal(G.table_rows64(3, 64)[:-1], t[:6])            # a shorter bound is a prefix


def _oracle_table(c, q_base):
    """The oracle's build_batch loop over (query, selected window) -- its window_bounds per row, duration = e - s, video_start =
    s -- on the crafted metadata alone (no features), with the reference batch of every row; the caller applies the collate's
    rule (pad_sequences_1d: a batch is padded to its longest window)."""
    rows = {k: [] for k in ("vid_len", "video_start", "cls_row", "bid")}
    for q in range(c.nq):
        own = min(c.K, int(c.nwin[q])) if c.row_q is not None else c.K
        for s in range(own):
            st, ed = O.window_bounds(int(c.win_idx[q, s]), int(c.q_ctx_l[q]), c.W)
            rows["vid_len"].append(ed - st)
            rows["video_start"].append(st)
            rows["cls_row"].append(q)
            rows["bid"].append((q + q_base) // c.eval_bsz)
    return {k: np.asarray(v) for k, v in rows.items()}


def _torch_table(c, q_base, batch_pad):
    """inference.window_table's torch index arithmetic on a stand-in store that holds the crafted metadata."""
    from cone_amd import inference as inf
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int64)
    # one video per query: ctx_l indexed by q_vid = the query itself.  The row list comes from the store's Selection, which
    # gives a query min(K, windows of its video) rows: the DENSE family (K rows for every query, windows repeated where the
    # video owns fewer) is stated to it through videos that are long enough -- the geometry reads q_ctx_l below, not this
    sel_ctx = c.q_ctx_l.astype(np.int64) if c.row_q is not None else np.full(c.nq, 10 ** 6, np.int64)
    store = SimpleNamespace(ctx_l=sel_ctx, q_vid=np.arange(c.nq), q_base=q_base, nq_split=q_base + c.nq)
    tens = dict(q_ctx_l=t64(c.q_ctx_l), q_vid_off=t64(c.q_vid_off), tok_off=t64(c.tok_off), tok_len=t64(c.tok_len))
    store.index_tensors = lambda: tens
    opt = SimpleNamespace(max_v_l=c.W, topk_window=c.K, eval_bsz=c.eval_bsz, window_table_torch=True)
    return inf.window_table(store, opt, torch.as_tensor(c.win_idx), batch_pad=t64(batch_pad))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("eval_bsz,K", G.WT_BATCHING)
@pytest.mark.parametrize("W", G.WT_WS)
def test_window_table_ref_matches_the_oracle_and_the_torch_arithmetic(W, eval_bsz, K, sparse):
    c = G.wt_case(W, eval_bsz, K, sparse=sparse)
    if sparse:
        own = np.minimum(K, c.nwin)
        assert (own < K).any() and (own == K).any() or K == 1     # videos with fewer than K windows next to videos with K
    # selections include window 0, the last window and the one before it
    flat = [(q, int(w)) for q in range(c.nq) for w in c.win_idx[q] if w >= 0]
    assert any(w == 0 for _, w in flat) and any(w == c.nwin[q] - 1 for q, w in flat)
    assert any(w == c.nwin[q] - 2 for q, w in flat) or K == 1
    for q_base in G.wt_q_bases(eval_bsz):
        nb, kw = G.wt_view(c, q_base)
        ref = G.window_table_ref(**kw)
        o = _oracle_table(c, q_base)
        for k in ("vid_len", "video_start", "cls_row"):
            assert np.array_equal(ref[k], o[k]), (k, q_base)
        # the collate pads a batch to its longest window
        for bid in range(nb):
            sel = o["bid"] == bid
            assert ref["batch_pad"][bid] == (o["vid_len"][sel].max() if sel.any() else 0)
            assert (ref["pad_len"][sel] == ref["batch_pad"][bid]).all()
        t = _torch_table(c, q_base, ref["batch_pad"])
        for k in ("vid_row0", "vid_len", "video_start", "pad_len", "txt_row0", "txt_len", "cls_row"):
            assert np.array_equal(ref[k], t[k].numpy()), (k, q_base)
        # a table handed in comes back unchanged and is what pad_len reads
        given = ref["batch_pad"] + 3
        again = G.window_table_ref(**kw, batch_pad=given)
        assert np.array_equal(again["batch_pad"], given) and np.array_equal(again["pad_len"], ref["pad_len"] + 3)


def test_window_lengths_cover_the_family():
    for W in G.WT_WS:
        S = int(W / 2)
        c = G.wt_case(W, 4, 4)
        assert set(c.q_ctx_l.tolist()) == {1, S - 1, S, S + 1, W - 1, W, W + 1, 3 * S + 1, 19 * S + 1}
        assert W != 125 or W % 2 == 1


@pytest.mark.parametrize("d", [128, 256, 512])
def test_float_references_match_torch_float64(d):
    c = G.txt_case(d, 257)
    _, j = G.txt_index(c.tok, None, 1, c.n_emb, c.n)
    assert j.min() == 0 and j.max() == c.n_emb - 1
    want = torch.nn.functional.layer_norm(c.x.double() + c.E.double()[torch.as_tensor(j)], (d,), c.g.double(), c.b.double(), 1e-5)
    assert float((torch.as_tensor(G.txt_pos64(c.x.numpy(), c.E.numpy(), j, c.g.numpy(), c.b.numpy())) - want).abs().max()) < 1e-12
    ref, bound, info = G.txt_ref_bound(c, j)
    assert float((ref - want).abs().max()) < 1e-12
    assert bool(torch.isfinite(bound).all()) and info["first"] <= R.LN_VALID, info       # every row has a first-order bound
    s = G.sal_case(d)
    sal = G.saliency64(s.MEM, s.off, s.vlen, s.w, s.bias, s.lv_max + 3)
    for b in range(s.B):
        lv = int(s.vlen[b])
        want = torch.as_tensor(s.MEM[s.off[b]:s.off[b] + lv]).double() @ torch.as_tensor(s.w).double().t() + float(s.bias[0])
        assert np.allclose(sal[b, :lv], want.numpy().reshape(-1), rtol=0, atol=1e-12) and not sal[b, lv:].any()
    h = G.head_case(d, 5, 2)
    for act in (0, 1):
        want = torch.as_tensor(h.x).double() @ torch.as_tensor(h.W).double().t() + torch.as_tensor(h.b).double()
        want = torch.sigmoid(want) if act else want
        assert float((torch.as_tensor(G.rowdot64(h.x, h.W, h.b, act)[0]) - want).abs().max()) < 1e-12


def test_head_case_holds_the_saturating_logits():
    h = G.head_case(256, 1025, 2)
    s = G.rowdot64(h.x, h.W, h.b, 0)[0]
    assert [t for _, t in h.sat] == list(G.SAT_LOGITS)
    for r, t in h.sat:
        assert abs(s[r, 0] - t) < 1e-3 and abs(s[r - 1, 0]) < 10 and abs(s[r + 1, 0]) < 10
    assert len(G.head_case(256, 3, 1).sat) == 1 and not G.head_case(256, 1, 1).sat


def test_integer_references_on_hand_cases():
    assert G.scan_ref([3, 0, 2], [1, 1, 0]).tolist() == [0, 4, 5, 7]
    assert G.scan_ref([3, 0, 2]).tolist() == [0, 3, 3, 5]
    voff, toff, vidx, tidx = G.compact_ref([2, 0, 1], [1, 2, 0], 4, 2)
    assert vidx.tolist() == [0, 1, 8] and tidx.tolist() == [0, 2, 3] and voff.tolist() == [0, 2, 2, 3] and toff.tolist() == [0, 1, 3, 3]
    assert G.row_index_ref([10, 0], [2, 0], [5, 7], [1, 2]).tolist() == [10, 11, ~5, ~7, ~8]
    assert G.tile_ref(np.arange(6).reshape(3, 2), 5).tolist() == [[0, 1], [2, 3], [4, 5], [0, 1], [2, 3]]
    assert G.mask_lengths_ref(G.mask_case(5, 65, "ones")).tolist() == [65] * 5
    p = G.poison(4, 3)
    assert bool(torch.isnan(p).all()) and G.untouched(p)
    p[1, 2] = 0.0
    m = np.zeros((4, 3), bool)
    assert not G.untouched(p, m)
    m[1, 2] = True
    assert G.untouched(p, m)
    pi = G.poison(5, dtype=torch.int32)
    assert pi.dtype == torch.int32 and G.untouched(pi) and int(pi[0]) == G.POISON_BITS


# ------------------------------------------------------------------------------------------------ discrimination
def test_the_sine_bound_and_the_planted_sine_errors():
    """The inputs of the sine bound and the condition it is held to: the smallest planted distance is >= 10 bounds."""
    cpu_err = G.sine_cpu_error()
    bound = G.sine_bound()
    assert bound == G.SINE_FACTOR * cpu_err
    assert 0.25 * G.U <= cpu_err <= 1.0 * G.U, cpu_err            # under one ulp of 1.0 (measured here: 3.6e-8 = 0.6 U)
    d_lv = d_p = float("inf")
    for lv in G.SINE_LVS:
        ref = G.sine_rows64(lv, 256)
        # per ROW (every row of the table has to tell): the largest channel distance
        d_lv = min(d_lv, float(np.abs(G.sine_rows64(lv, 256, lv_shift=-1) - ref).max(1).min()))
        d_p = min(d_p, float(np.abs(G.sine_rows64(lv, 256, p_shift=-1) - ref).max(1).min()))
    print(f"[glue] cpu fp32 sin/cos error {cpu_err:.3g}, bound {bound:.3g}, smallest distance lv-1: {d_lv:.3g}, p for p+1: {d_p:.3g}")
    assert d_lv >= 10 * bound and d_p >= 10 * bound, (d_lv, d_p, bound)
    assert 4e-6 <= d_lv <= 8e-6 and 3e-3 <= d_p <= 6e-3           # 6.0e-6 (lv 1022 against 1023, p = 0) and 4.4e-3


def test_a_garbage_zero_row_is_seen():
    t = G.table_rows64(5, 64).copy()
    assert not t[-1].any()
    t[-1] = G.poison(64).numpy()
    assert not np.array_equal(t[-1], np.zeros(64))                 # the GPU test compares the row's BITS with +0.0


@pytest.mark.parametrize("B", G.SCAN_BS)
def test_scan_model_and_the_planted_wave_base(B):
    for kind in G.SCAN_KINDS:
        v, q = G.scan_case(B, kind)
        for ql in (q, None):
            assert np.array_equal(G.scan_model(v, ql), G.scan_ref(v, ql))
    v, q = G.scan_case(B, "max")
    # (wave 15 writes the total from ITS base, so even B = 1 tells)
    assert not np.array_equal(G.scan_model(v, q, mut="base_block"), G.scan_ref(v, q)), B
    v, q = G.scan_case(B, "zero")
    assert np.array_equal(G.scan_model(v, q, mut="base_block"), G.scan_ref(v, q))     # all-zero lengths: blind by construction


def _bids(c, q_base):
    _, kw = G.wt_view(c, q_base)
    ref = G.window_table_ref(**kw)
    return ref, ((ref["cls_row"].astype(np.int64) + q_base) // c.eval_bsz).tolist()


@pytest.mark.parametrize("eval_bsz,K", G.WT_BATCHING)
def test_batch_maximum_model_and_the_dropped_second_batch(eval_bsz, K):
    seen = False
    for sparse in (False, True):
        c = G.wt_case(90, eval_bsz, K, sparse=sparse)
        for q_base in G.wt_q_bases(eval_bsz):
            nb, _ = G.wt_view(c, q_base)
            ref, bid = _bids(c, q_base)
            assert np.array_equal(G.batch_max_model(ref["vid_len"].tolist(), bid, nb), ref["batch_pad"])
            moved = not np.array_equal(G.batch_max_model(ref["vid_len"].tolist(), bid, nb, mut="drop_second"), ref["batch_pad"])
            # a ballot loop that clears only its leader's bit repeats work and changes nothing: proved here, since no GPU
            # case can fail on it
            assert np.array_equal(G.batch_max_model(ref["vid_len"].tolist(), bid, nb, mut="clear_lowest"), ref["batch_pad"])
            two_in_a_wave = any(len(set(bid[w:w + 64])) > 1 for w in range(0, len(bid), 64))
            if not two_in_a_wave:
                assert not moved            # (100, 20) at q_base 0: one batch, no wave holds a second one -- blind
            seen |= moved
    if (eval_bsz, K) == (100, 20):
        c = G.wt_case(90, eval_bsz, K)
        assert len(set(_bids(c, 0)[1])) == 1 and c.n_rows == 1400             # one batch across six workgroups
    if (eval_bsz, K) == (1, 1):
        assert len(set(_bids(G.wt_case(90, 1, 1), 0)[1][:64])) == 64         # a wave of 64 one-row batches
    # (100, 20): a batch is 2000 rows, so wherever a wave holds a second batch the waves after it hold that batch FIRST and
    # restore its maximum (every batch of 100 queries has a full window outside the wave of its boundary): the family is blind
    # to this error and says so; the three families with several batches per wave all see it
    assert seen == ((eval_bsz, K) != (100, 20)), "which batching families see a dropped second batch has changed"


@pytest.mark.parametrize("n", G.TXT_NS)
def test_text_index_planted_errors_change_an_integer(n):
    c = G.txt_case(256, n)
    for mod in G.TXT_MODS:
        cnt, j = G.txt_index(None, c.src_row, mod, c.n_emb, n)
        _, jd = G.txt_index(None, c.src_row, mod, c.n_emb, n, mut="div_for_mod")
        # row 0 comes from source row 0, where 0 % mod == 0 / mod: n = 1 cannot tell the two apart
        assert (not np.array_equal(j, jd)) == (n > 1), (n, mod)
    _, j = G.txt_index(c.tok, None, 1, c.n_emb, n)
    _, jn = G.txt_index(c.tok, None, 1, c.n_emb, n, mut="no_clamp")
    assert j.min() >= 0 and j.max() < c.n_emb
    assert (not np.array_equal(j, jn)) == (n >= 3)                 # the first index past the table sits in row 6 % n
    for n_dev in (0, n - 1, n, n + 5):
        cnt, _ = G.txt_index(c.tok, None, 1, c.n_emb, n, n_dev)
        cnt_i, _ = G.txt_index(c.tok, None, 1, c.n_emb, n, n_dev, mut="n_dev_ignored")
        assert cnt == min(n_dev, n) and (cnt != cnt_i) == (n_dev < n)


@pytest.mark.parametrize("d", [128, 256])
def test_a_wrong_text_index_moves_the_value_by_ten_bounds(d):
    c = G.txt_case(d, 257)
    _, j = G.txt_index(None, c.src_row, 7, c.n_emb, c.n)
    _, jd = G.txt_index(None, c.src_row, 7, c.n_emb, c.n, mut="div_for_mod")
    ref, bound, _ = G.txt_ref_bound(c, j)
    wrong = torch.as_tensor(G.txt_pos64(c.x.numpy(), c.E.numpy(), jd, c.g.numpy(), c.b.numpy()))
    assert float(((wrong - ref).abs() / bound).max()) >= 10


@pytest.mark.parametrize("d", [128, 256])
def test_shifted_text_half_of_the_memory_tap_is_seen(d):
    s = G.sal_case(d)
    good = G.mem_tap_ref(s.MEM, s.off, s.vlen, s.qlen, s.lv_max, s.lq_max)
    bad = G.mem_tap_ref(s.MEM, s.off, s.vlen, s.qlen, s.lv_max, s.lq_max, mut="txt_shift")
    for b in range(s.B):
        blind = s.vlen[b] == 0 or s.qlen[b] == 0           # no clips: nothing to shift by; no tokens: nothing to shift
        assert G.same_bits(good[b], bad[b]) == bool(blind), b
    assert not G.same_bits(good, bad)


@pytest.mark.parametrize("d", [128, 256, 512])
def test_sigmoid_on_the_class_head_moves_by_ten_bounds(d):
    h = G.head_case(d, 1025, 2)
    for act in (0, 1):
        ref = G.rowdot64(h.x, h.W, h.b, act)[0]
        wrong = G.rowdot64(h.x, h.W, h.b, 1 - act)[0]
        assert float((np.abs(wrong - ref) / G.rowdot_bound(h.x, h.W, h.b, act)).max()) >= 10


def test_dropped_padding_guard_of_the_saliency_head_is_seen():
    """A saliency kernel without its p < lv guard writes <some row, w> + bias into the padding: not +0.0 for any window shorter
    than Lv_out (the bias alone is 0.37)."""
    s = G.sal_case(256)
    assert (s.vlen < s.lv_max).any() and float(s.bias[0]) != 0.0


def test_families_hold_the_edges_the_gpu_suite_promises():
    c = G.pack_case(256)
    L = (c.vlen + c.qlen).tolist()
    assert c.Lmax == G.PACK_LMAX == max(L) and (1, 1) in G.PACK_WINDOWS and (0, 0) in G.PACK_WINDOWS
    assert {3, 4, 5} <= set(L) and {255, 256, 257} <= set(L)
    assert any(v == 0 and q > 0 for v, q in G.PACK_WINDOWS) and any(q == 0 and v > 0 for v, q in G.PACK_WINDOWS)
    assert G.same_bits(G.row_index_ref(c.vrow0, c.vlen, c.trow0, c.qlen), np.where(c.kind, c.src, ~c.src).astype(np.int32))
    for B in (3, 1025):
        for Lv, Lq in G.COMPACT_PADS:
            v, q = G.compact_case(B, Lv, Lq)
            assert v.max() == Lv and q.max() == Lq and v.min() == 0 and q.min() == 0
