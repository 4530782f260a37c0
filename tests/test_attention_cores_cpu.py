"""The references and cases of tests/attention_refs.py, validated before the GPU tests (test_attention_cores_gpu.py) trust
them: enc_rows against a direct torch evaluation of nn.MultiheadAttention's arithmetic, the saturated construction against
what it claims, and the POWER of every window of every batch the GPU file runs -- the float64 output of a kernel that is off
by one key (the padded copy of the last key leaking through the mask, the last key dropped) or by one table row (the rows of
lv - 1 / lv + 1 clips, of clip p - 1 / p + 1, the zero row for a text token's own) is at least 10 TOL away.  CPU only.

Cases that cannot differ by construction are EXEMPT by name (``exempt`` below), never silently passed:
  * one key: softmax over a single key is 1 whatever its score, so the output is v -- dropping it leaves no key at all, the
    duplicate is the same v at weights 1/2 + 1/2, and no table row can show;
  * lv = 0: a window without clips reads no clip row of the table, whatever clip count is assumed;
  * lv = 1 with clip p - 1 or with lv - 1: the window owns table row 0, there is no row before it, and a window "with no
    clips" adds none -- the same rows;
  * no text token with the text-position row replaced by the zero row.
An exempt case is asserted to be EXACTLY equal to the reference, so a case cannot hide behind the word."""
import math

import pytest
import torch

import attention_refs as R

POWER = 10 * R.TOL


def far(a, b):
    return float((a - b).abs().max())


def exempt(L, lv=None, kind=""):
    if L == 1:
        return "one key: the output is v whatever the scores"
    if lv == 0:
        return "no clip: no clip row of the table is read"
    if lv == 1 and kind in ("p-1", "lv-1"):
        return "a one-clip window owns table row 0: there is no row before it, and no clips have none either"
    if kind == "text" and lv is None:
        return "no text token: no text position row is read"
    return None


def _assert_far(ref, wrong, what, seen):
    d = far(ref, wrong)
    seen.append(d)
    assert d >= POWER, (what, d)


def _enc_power(c, modes, rows_of):
    """Every window of case c: key-count wrong versions in every mode, table wrong versions in the table modes."""
    seen, n_exempt = [], 0
    for mode in modes:
        rows = rows_of(mode, c)
        wrong_rows = {}
        if mode & 3:
            wrong_rows = {"lv-1": R.enc_rows(mode, c, lv_table=[max(v - 1, 0) for v in c.vl]),
                          "lv+1": R.enc_rows(mode, c, lv_table=[v + 1 for v in c.vl]),
                          "p-1": R.enc_rows(mode, c, p_shift=-1), "p+1": R.enc_rows(mode, c, p_shift=1)}
        if mode & 4:
            wrong_rows["text"] = R.enc_rows(mode & 3, c)
        for b in range(c.B):
            sl = slice(int(c.off[b]), int(c.off[b + 1]))
            ref = R.enc_window64(rows[sl])
            for name, e in (("last key duplicated", 1), ("last key dropped", -1)):
                if exempt(c.L[b]):
                    n_exempt += 1
                    continue
                _assert_far(ref, R.enc_window64(rows[sl], e), (mode, b, c.L[b], name), seen)
            for name, wr in wrong_rows.items():
                why = exempt(c.L[b], c.vl[b], name) if name != "text" else exempt(c.L[b], 1 if c.tl[b] else None, name)
                if why:
                    n_exempt += 1
                    assert far(ref, R.enc_window64(wr[sl])) == 0, (why, mode, b)        # exempt means: it cannot differ
                    continue
                _assert_far(ref, R.enc_window64(wr[sl]), (mode, b, c.vl[b], c.tl[b], name), seen)
    return seen, n_exempt


@pytest.mark.parametrize("n", list(range(6, 17)))
def test_encoder_batches_have_off_by_one_power(n):
    c = R.enc_case(n)
    assert c.Lmax == 16 * n and c.zrow == c.pos.shape[0] - 1 and not c.pos[c.zrow].any()
    assert sorted(c.vrow0) != c.vrow0 and min(c.vrow0) > 0 and min(c.trow0) > 0
    assert any(v and t and v % 4 for v, t in zip(c.vl, c.tl)), "a clip / text boundary inside a key quad"
    assert any(v == 0 for v in c.vl) and any(t == 0 and v > 1 for v, t in zip(c.vl, c.tl))
    seen, n_exempt = _enc_power(c, R.MODES, R.enc_rows)
    print(f"encoder batch n={n}: smallest wrong-version distance {min(seen):.3g} over {len(seen)} (exempt {n_exempt})")


def test_short_batch_is_all_one_key_windows():
    """Lmax = 1 on the 6-wave build: every window is a one-key window -- the whole batch is exempt from the power check, by
    name; what the GPU test pins there is the spare waves' exit and the store of v."""
    c = R.enc_case(6, short=True)
    assert c.Lmax == 1 and all(exempt(l) for l in c.L)
    for mode in R.MODES:
        rows = R.enc_rows(mode, c)
        assert far(R.enc_ref64(rows, c.off), rows[:, 512:]) == 0


@pytest.mark.parametrize("lv,lt", R.SAT_WINDOWS)
def test_saturated_construction(lv, lt):
    c = R.enc_saturated_case(lv, lt)
    n = lv + lt
    for mode in (0, 2):
        rows = R.saturated_rows(mode, c)
        for b in (0, c.B - 1):
            r = rows[b * n:(b + 1) * n]
            for h in range(R.HEADS):
                s = R.scores64(r[:, :256], r[:, 256:512], h)
                assert s.max() > 50 and s.min() < -50
                assert bool((s.argmax(dim=1) == n - 1).all())
    seen, n_exempt = _enc_power(c, (0,), R.saturated_rows)
    assert n_exempt == 0
    print(f"saturated {n}: smallest wrong-version distance {min(seen):.3g}")


@pytest.mark.parametrize("Lmax", [110, 128, 129, 150, 192, 193, 241, 256])
@pytest.mark.parametrize("shared", [False, True])
def test_decoder_cross_batches_have_off_by_one_power(Lmax, shared):
    c = R.dec_case(Lmax, 5, shared)
    assert c.Lmax == Lmax and set(x for x in (1, 16, 17, 128, 129, 143, 144, 145, 240, 241) if x <= Lmax) <= set(c.L)
    seen, n_exempt = [], 0
    for b in range(c.B):
        ref, ref_xp = R.dec_window64(c, b), R.dec_window64(c, b, use_xp=True)
        if exempt(c.L[b]):
            n_exempt += 1
        else:
            for e in (1, -1):
                _assert_far(ref, R.dec_window64(c, b, extra_last=e), (b, c.L[b], e), seen)
                _assert_far(ref_xp, R.dec_window64(c, b, use_xp=True, extra_last=e), (b, c.L[b], e, "XP"), seen)
            _assert_far(ref, ref_xp, (b, "XP read as memory + table row"), seen)
        for kind, lvw in (("lv-1", c.vl[b] - 1), ("lv+1", c.vl[b] + 1)):
            if exempt(c.L[b], c.vl[b], kind):
                n_exempt += 1
                continue
            _assert_far(ref, R.dec_window64(c, b, lv_table=lvw), (b, c.vl[b], lvw), seen)
    print(f"decoder cross Lmax={Lmax}: smallest wrong-version distance {min(seen):.3g} (exempt {n_exempt})")


@pytest.mark.parametrize("nq", [1, 5, 8, 9, 16])
def test_small_cross_batches_have_off_by_one_power(nq):
    c = R.small_cross_case(nq)
    assert tuple(c.L) == R.SMALL_KEYS
    for b in range(c.B):
        if exempt(c.L[b]):
            continue
        ref = R.small_cross_window64(c, b)
        for e in (1, -1):
            assert far(ref, R.small_cross_window64(c, b, e)) >= POWER, (nq, b, e)
        # the first layer's slice of the strided K / V buffers in place of the second's
        wrong = R.mha64(c.Q[b * nq:(b + 1) * nq], c.KD[c.off[b]:c.off[b + 1], :R.D], c.VD[c.off[b]:c.off[b + 1], :R.D])
        assert far(ref, wrong) >= POWER


@pytest.mark.parametrize("nq", list(range(1, 17)))
def test_small_self_batches_have_off_by_one_power(nq):
    qkv = R.small_self_case(nq)
    for b in range(max(R.SMALL_SELF_B)):
        if exempt(nq):
            continue
        ref = R.small_self_window64(qkv, nq, b)
        for e in (1, -1):
            assert far(ref, R.small_self_window64(qkv, nq, b, e)) >= POWER, (nq, b, e)
        if b:       # the neighbouring window's slots as keys
            r = qkv[b * nq:(b + 1) * nq].double()
            o = qkv[(b - 1) * nq:b * nq].double()
            assert far(ref, R.mha64(r[:, :256], o[:, 256:512], o[:, 512:])) >= POWER


@pytest.mark.parametrize("mode", R.MODES)
def test_enc_rows_match_multihead_attention_arithmetic(mode):
    """One small window per mode through nn.MultiheadAttention's own arithmetic (cone/transformer.py:233-240: q = k = src + pos,
    value = src, in_proj, per-head softmax(q k^T / sqrt(head_dim)) v) in float64: the module's in_proj applied to src + pos
    must give what enc_rows assembles from the projected rows and the projected position rows."""
    g = torch.Generator().manual_seed(40 + mode)
    lv, lt = 7, 3
    L = lv + lt
    mha = torch.nn.MultiheadAttention(R.D, R.HEADS, bias=True).double()
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / (16 if p.dim() > 1 else 1))
        mha.out_proj.weight.copy_(torch.eye(R.D, dtype=torch.float64))
        mha.out_proj.bias.zero_()
    W, bias = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
    src = torch.randn(L, R.D, generator=g, dtype=torch.float64)
    pos = torch.zeros(L, R.D, dtype=torch.float64)
    pos[:lv] = torch.randn(lv, R.D, generator=g, dtype=torch.float64)     # (mode 0: carried by the packed rows themselves)
    if mode & 4:
        pos[lv:] = torch.randn(lt, R.D, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = mha((src + pos)[:, None], (src + pos)[:, None], src[:, None], need_weights=False)[0][:, 0]
    # the case enc_rows reads: projected rows (x W^T + b) and projected position rows (pos W_qk^T), float32 storage
    c = R._enc_case_from([lv], [lt], torch.Generator().manual_seed(1))
    proj = (src @ W.t() + bias).float()
    pos_qk = (pos @ W[:512].t()).float()
    if mode == 0:
        proj[:, :512] = ((src + pos) @ W[:512].t() + bias[:512]).float()
    c.QKV = proj
    c.qkv_vid = torch.zeros_like(c.qkv_vid)
    c.qkv_txt = torch.zeros_like(c.qkv_txt)
    c.qkv_vid[c.vrow0[0]:c.vrow0[0] + lv] = proj[:lv]
    c.qkv_txt[c.trow0[0]:c.trow0[0] + lt] = proj[lv:]
    c.pos[R.pos_base(lv):R.pos_base(lv) + lv] = pos_qk[:lv]
    c.txt_pos = torch.zeros_like(c.txt_pos)
    c.txt_pos[c.trow0[0]:c.trow0[0] + lt] = pos_qk[lv:]
    got = R.enc_ref64(R.enc_rows(mode, c), c.off)
    assert far(got, want) < 1e-5       # float32 storage of the projected rows: ~1e-7 relative per element, not a kernel bound
    assert math.isfinite(far(got, want))
    if mode & 3:    # and the position term is not decorative
        c.pos.zero_()
        assert far(R.enc_ref64(R.enc_rows(mode, c), c.off), want) >= POWER
