"""Video sessions on the GPU: everything a session returns is compared with ``==`` against ``CONELocalizator.predict_moment``
on the same video and query -- no tolerances.  (A session re-sequences the launchers ``predict_moment`` calls; it computes
nothing new.)"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import session_refs as R
from cone_amd import synth
from cone_amd.config import make_opt

pytestmark = pytest.mark.gpu

STEPS = ("python", "c")
POISON = 0x7EADBEEF


# ------------------------------------------------------------------------------------------------ fixtures
_LOCS, _REFS = {}, {}


def _localizer(kind="default", **extra):
    """One localizer per checkpoint kind for the whole module (weights from synth.make_state_dict)."""
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        kw = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4),
                  long=dict(max_v_l=300, topk_window=5))[kind]
        sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
        _LOCS[key] = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}, **kw, **extra)
    return _LOCS[key]


def _video(ctx_l, seed=0):
    return torch.randn(ctx_l, 256, generator=torch.Generator().manual_seed(1000 + seed + ctx_l)) * 2


def _queries(lens, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return [(torch.randn(n, 768, generator=g), torch.randn(256, generator=g)) for n in lens]


def _mixed_lens(Q):
    return [(1, 7, 20, 12, 3)[i % 5] for i in range(Q)]


def _reference(loc, tag, vid, queries):
    """predict_moment per query, computed once per (localizer, video, queries) tag and never changed."""
    key = (id(loc), tag)
    if key not in _REFS:
        _REFS[key] = [loc.predict_moment(vid, q) for q in queries]
        assert all(len(r) >= 1 for r in _REFS[key])
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ single calls
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("ctx_l", [1, 45, 46, 90, 91, 333, 900, 6000])
def test_single_call_equals_predict_moment(ctx_l, step):
    loc = _localizer()
    vid = _video(ctx_l)
    queries = _queries([1, 7, 20], seed=ctx_l)
    want = _reference(loc, ("single", ctx_l), vid, queries)
    with loc.open_video(vid, step=step) as s:                   # host video, host queries
        assert s.nbytes > 0
        for q, w in zip(queries, want):
            assert s.predict_moment(q) == w, (ctx_l, step, q[0].shape)
    s = loc.open_video(vid.cuda(), step=step)                   # resident video, resident queries
    for (tok, cls), w in zip(queries, want):
        assert s.predict_moment((tok.cuda(), cls.cuda())) == w, (ctx_l, step, tok.shape)
    s.close()
    assert s.nbytes == 0
    with pytest.raises(RuntimeError, match="closed"):
        s.predict_moment(queries[0])


def test_resident_bytes_per_clip():
    loc = _localizer()
    vid = _video(900)
    sizes = {step: loc.open_video(vid, step=step).nbytes for step in STEPS}
    assert sizes["python"] == 900 * (256 + 256 + 256 + 768) * 4             # normalised, adapted, projected, q | k | v
    assert sizes["python"] <= sizes["c"] <= sizes["python"] + 4 * 256       # the arena aligns its four regions
    cert = loc.open_video(vid, certified=True).nbytes
    assert cert == sizes["python"] + 900 * 256 * 2 + 8                      # + the bf16 shadow and its two measures


@pytest.mark.parametrize("step", STEPS)
def test_golden_cases_through_a_session(golden_dir, step):
    """tests/golden/localizer.json (the reference's own run_on_video output) under the bounds of
    test_localizer_matches_reference_golden."""
    from cone_amd.localizator import CONELocalizator
    with open(os.path.join(golden_dir, "localizer.json")) as f:
        fx = json.load(f)
    opt = make_opt("ego4d", clip_length=fx["clip_length"], topk_window=fx["topk_window"])
    sd = synth.make_state_dict(opt, fx["weight_seed"])
    loc = CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()})
    rng = np.random.default_rng(fx["input_seed"])
    for case in fx["cases"]:
        vid = rng.standard_normal((case["ctx_l"], 256), dtype=np.float32) * 3
        tok = rng.standard_normal((case["lq"], 768), dtype=np.float32)
        cls = rng.standard_normal((256,), dtype=np.float32)
        with loc.open_video(torch.from_numpy(vid), step=step) as s:
            got = s.predict_moment((torch.from_numpy(tok), torch.from_numpy(cls)))
        ref = np.array(case["out"])
        assert len(got) == len(ref)
        got = np.array(got)
        assert np.abs(got[:, :2] - ref[:, :2]).max() <= 1e-4 * 90 * fx["clip_length"] + 1e-4
        assert np.abs(got[:, 2] - ref[:, 2]).max() < 2e-3


# ------------------------------------------------------------------------------------------------ batches
BATCH_Q = (1, 2, 4, 5, 7, 9, 17, 65)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("kind", ["default", "txt_pos", "pre_norm"])
def test_batches_equal_the_single_calls(kind, step):
    """Ragged batches of every size around the pre-filter's form switch (5) and the C entry's limit (64): each query's
    moments == its own predict_moment call.  65 queries go through the wrapper's split."""
    loc = _localizer(kind)
    vid = _video(900, seed=3)
    queries = _queries(_mixed_lens(65), seed=11)
    want = _reference(loc, ("batch", 900), vid, queries)
    with loc.open_video(vid, step=step) as s:
        for Q in BATCH_Q:
            got = s.predict_moments(queries[:Q])
            assert len(got) == Q
            for i in range(Q):
                assert got[i] == want[i], (kind, step, Q, i)
        assert s.predict_moments([]) == []


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("kind,ctx_l", [("general", 900), ("long", 1000)])
def test_batch_on_general_path_handles(kind, ctx_l, step):
    """A 128 / 4 handle (general path, row caches built and unused) and a long-window handle (max_v_l + max_q_l > 256: no
    row caches at all)."""
    loc = _localizer(kind)
    vid = _video(ctx_l, seed=4)
    queries = _queries(_mixed_lens(7), seed=13)
    want = _reference(loc, ("batch", ctx_l), vid, queries)
    with loc.open_video(vid, step=step) as s:
        if step == "python":
            assert (s.qkv_vid is None) == (kind == "long")
        else:
            assert (not s._cs.qkv_vid) == (kind == "long")
        assert s.predict_moments(queries) == want
        assert s.predict_moment(queries[2]) == want[2]


@pytest.mark.parametrize("step", STEPS)
def test_prefilter_bf16_localizer_session_equals_its_own_predict_moment(step):
    loc = _localizer(prefilter_bf16=True)
    vid = _video(400, seed=5)
    queries = _queries(_mixed_lens(6), seed=17)
    vid[130:133] = queries[0][1]
    want = _reference(loc, ("bf16", 400), vid, queries)
    with loc.open_video(vid, step=step) as s:
        assert s.predict_moment(queries[0]) == want[0]
        assert s.predict_moments(queries) == want
    with pytest.raises(ValueError, match="prefilter_bf16"):
        loc.open_video(vid, certified=True, step=step)


# ------------------------------------------------------------------------------------------------ certified stage A
def _planted(ctx_l, cls, n_peaks=30, seed=9):
    """Random clips with n_peaks clips pointing along cls, each a little less than the one before: separable window scores."""
    vid = _video(ctx_l, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for i in range(n_peaks):
        at = 60 + i * ((ctx_l - 120) // n_peaks)
        vid[at] = cls * (1.0 - 0.02 * i) + torch.randn(256, generator=g) * (0.2 + 0.1 * i)
    return vid


@pytest.mark.parametrize("step", STEPS)
def test_certified_session_on_more_windows_than_candidates(step):
    """6000 clips = 135 windows, the default candidate count is 128: the proof has to cover windows it never rescored."""
    loc = _localizer()
    queries = _queries([9], seed=19)
    vid = _planted(6000, queries[0][1])
    with loc.open_video(vid, step=step) as plain, loc.open_video(vid, certified=True, step=step) as cert:
        want = plain.predict_moments(queries)
        assert want == [loc.predict_moment(vid, queries[0])]
        assert cert.predict_moments(queries) == want
        assert cert.last_certified.tolist() == [1]
        assert plain.last_certified is None


@pytest.mark.parametrize("step", STEPS)
def test_certified_session_with_one_window_outside_the_candidates(step):
    """900 clips = 21 windows, n_cand = 20."""
    loc = _localizer()
    vid = _video(900, seed=3)
    queries = _queries(_mixed_lens(3), seed=11)
    want = _reference(loc, ("batch", 900), vid, _queries(_mixed_lens(65), seed=11))[:3]
    with loc.open_video(vid, certified=True, n_cand=20, step=step) as s:
        assert s.predict_moments(queries) == want
        assert s.last_certified.shape == (3,) and set(s.last_certified.tolist()) <= {0, 1}


@pytest.mark.parametrize("step", STEPS)
def test_identical_rows_never_certify_and_still_answer(step):
    """Every window ties: nothing separates the top-k from the rest, the query falls back to the full fp32 scan."""
    loc = _localizer()
    row = torch.randn(256, generator=torch.Generator().manual_seed(21))
    vid = row.repeat(6000, 1)
    queries = _queries([8], seed=23)
    want = [loc.predict_moment(vid, queries[0])]
    with loc.open_video(vid, certified=True, step=step) as s:
        assert s.predict_moments(queries) == want
        assert s.last_certified.tolist() == [0]


@pytest.mark.parametrize("step", STEPS)
def test_certified_batch_mixes_a_separable_and_a_tied_query(step):
    """3000 clips with peaks along query A, then 6000 copies of one row that query B points along (201 windows, 128
    candidates).  B's best windows are the ~133 of the repeated row and all tie: more than the candidates hold, so the k-th
    exact score equals the best score left outside and the strict inequality of the proof fails -- never certified.  (Ties
    INSIDE the candidate set would not matter: they are rescored exactly.)  A's 20 best windows are peaks that stand clear of
    the repeated row's score, which is what the windows outside its candidates carry -- certified."""
    loc = _localizer()
    qa, qb = _queries([6, 15], seed=29)
    row = qb[1].clone()
    vid = torch.cat([_planted(3000, qa[1]), row.repeat(6000, 1)])
    queries = [qa, qb]
    want = [loc.predict_moment(vid, q) for q in queries]
    with loc.open_video(vid, certified=True, step=step) as s:
        assert s.predict_moments(queries) == want
        assert s.last_certified.tolist() == [1, 0]
    with loc.open_video(vid, step=step) as s:
        assert s.predict_moments(queries) == want


# ------------------------------------------------------------------------------------------------ the layout kernel
def _guarded(n, guard=64):
    buf = torch.full((n + 2 * guard,), POISON, dtype=torch.int32, device="cuda")
    return buf, buf[guard:guard + n]


@pytest.mark.parametrize("case", range(len(R.LAYOUT_CASES)))
def test_query_layout_kernel_matches_the_model_inside_guarded_buffers(case):
    from cone_amd import _lib
    lib = _lib.load()
    lens, ctx_l, K = R.LAYOUT_CASES[case]
    want = R.layout_model(lens, ctx_l, K)
    bufs = {k: _guarded(len(want[k])) for k in R.OUTPUTS}
    arr = (C.c_int32 * len(lens))(*lens)
    _lib.check(lib.cone_session_query_layout(arr, len(lens), R.MAX_Q_L, ctx_l, K, R.NUM_QUERIES, R.MAX_V_L,
                                             *(C.c_void_p(bufs[k][1].data_ptr()) for k in R.OUTPUTS), _lib.stream()))
    torch.cuda.synchronize()
    for k in R.OUTPUTS:
        whole, inner = bufs[k]
        assert np.array_equal(inner.cpu().numpy(), want[k]), (k, lens)
        assert bool((whole[:64] == POISON).all()) and bool((whole[64 + len(want[k]):] == POISON).all()), (k, lens)


def test_query_layout_refuses_by_name():
    from cone_amd import _lib
    lib = _lib.load()
    outs = [_guarded(64 * 20)[1] for _ in R.OUTPUTS]

    def refused(lens):
        arr = (C.c_int32 * max(len(lens), 1))(*lens)
        rc = lib.cone_session_query_layout(arr, len(lens), 20, 900, 20, 5, 90, *(C.c_void_p(o.data_ptr()) for o in outs),
                                           _lib.stream())
        assert rc == -1
        return lib.cone_last_error().decode()
    assert "session_query_layout: nq=0 not in [1, 64]" in refused([])
    assert "session_query_layout: nq=65 not in [1, 64]" in refused([3] * 65)
    assert "tok_len[0]=0 not in [1, max_q_l=20]" in refused([0, 4])
    assert "tok_len[1]=21 not in [1, max_q_l=20]" in refused([4, 21])
    torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs)         # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ handle changes
def test_stale_handle_is_refused_and_a_new_session_works():
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    opt = SimpleNamespace(**LOCALIZER_OPT)
    sds = [{k: torch.from_numpy(v) for k, v in synth.make_state_dict(opt, seed).items()} for seed in (5, 6)]
    loc = CONELocalizator(state_dict=sds[0])
    vid = _video(333)
    q = _queries([7], seed=31)[0]
    for i, step in enumerate(STEPS):
        s = loc.open_video(vid, step=step)
        before = s.predict_moment(q)
        assert before == loc.predict_moment(vid, q)
        loc.localizator.load_state_dict(sds[(i + 1) % 2])
        with pytest.raises(RuntimeError, match="load_state_dict replaced the model handle"):
            s.predict_moment(q)
        with pytest.raises(RuntimeError, match="load_state_dict replaced the model handle"):
            s.predict_moments([q, q])
        with loc.open_video(vid, step=step) as s2:
            after = s2.predict_moment(q)
        assert after == loc.predict_moment(vid, q) and after != before


# ------------------------------------------------------------------------------------------------ the C entries themselves
def _c_session(loc, vid_d, flags=0, arena=None, ws=None):
    from cone_amd import _lib
    lib, h = _lib.load(), loc.localizator._h()
    ctx_l = vid_d.shape[0]
    n_arena, n_ws = lib.cone_session_arena_bytes(h, ctx_l, flags), lib.cone_session_workspace(h, ctx_l, flags)
    arena = torch.empty(n_arena, dtype=torch.uint8, device="cuda") if arena is None else arena
    ws = torch.empty(n_ws, dtype=torch.uint8, device="cuda") if ws is None else ws
    ses = _lib.Session()
    rc = lib.cone_session_index(h, _lib.ptr(vid_d), ctx_l, flags, _lib.ptr(arena), arena.numel(), _lib.ptr(ws), ws.numel(),
                                C.byref(ses), _lib.stream())
    return rc, ses, arena, (n_arena, n_ws)


def _params(loc):
    from cone_amd import _lib
    a = loc.args
    return _lib.SessionParams(a.max_v_l, a.max_q_l, a.clip_length, 0.5, 100, 5)


def _margined(nbytes, margin=4096):
    whole = torch.full((nbytes + 2 * margin,), 0xA5, dtype=torch.uint8, device="cuda")
    inner = whole[margin:margin + nbytes]
    assert inner.data_ptr() % 256 == 0
    return whole, inner, margin


def test_arena_and_workspace_edges():
    """The arena and both workspaces are slices of larger poisoned buffers: the calls stay inside them, the moments equal
    predict_moment's, and a buffer one byte short is refused by name."""
    from cone_amd import _lib
    from cone_amd.session import VideoSession
    lib, loc = _lib.load(), _localizer()
    h = loc.localizator._h()
    vid = _video(333)
    queries = _queries([7, 20, 1], seed=37)
    want = [loc.predict_moment(vid, q) for q in queries]
    vid_d = vid.cuda()
    n_arena, n_ws = lib.cone_session_arena_bytes(h, 333, 0), lib.cone_session_workspace(h, 333, 0)
    assert n_arena >= 333 * (256 * 3 + 768) * 4 and n_ws > 0
    a_whole, a_in, m = _margined(n_arena)
    w_whole, w_in, _ = _margined(n_ws)
    rc, ses, _, _ = _c_session(loc, vid_d, arena=a_in, ws=w_in)
    assert rc == 0, lib.cone_last_error()
    for short_arena, short_ws, name in ((1, 0, "arena too small"), (0, 1, "workspace too small")):
        rc2, _, _, _ = _c_session(loc, vid_d, arena=a_in[:n_arena - short_arena], ws=w_in[:n_ws - short_ws])
        assert rc2 == -3 and f"session_index: {name}" in lib.cone_last_error().decode()
    lens = [int(t.shape[0]) for t, _ in queries]
    nq, K = len(lens), min(20, 333 // 45 + 2)
    arr, p = (C.c_int32 * nq)(*lens), _params(loc)
    n_loc = lib.cone_session_localize_workspace(h, C.byref(ses), arr, nq, K, 0, C.byref(p))
    assert n_loc > 0
    l_whole, l_in, _ = _margined(n_loc)
    tok = torch.cat([t for t, _ in queries]).cuda()
    cls = torch.stack([c for _, c in queries]).cuda()
    k_whole, k_in, _ = _margined(3 * nq * 5 * 5 * 8 + 3 * nq * 4)
    R8 = 3 * nq * 5 * 5 * 8
    call = lambda ws_t: lib.cone_session_localize(h, C.byref(ses), _lib.ptr(tok), arr, nq, _lib.ptr(cls), K, 0, C.byref(p),
                                                  C.c_void_p(k_in.data_ptr()), C.c_void_p(k_in.data_ptr() + R8), None,
                                                  _lib.ptr(ws_t), ws_t.numel(), _lib.stream())
    assert call(l_in[:n_loc - 1]) == -3
    assert "session_localize: workspace too small" in lib.cone_last_error().decode()
    torch.cuda.synchronize()
    assert bool((k_in == 0xA5).all())                           # the refused call wrote nothing
    assert call(l_in) == 0, lib.cone_last_error()
    torch.cuda.synchronize()
    assert VideoSession.read_kept(k_in.cpu(), nq) == want
    for whole, n in ((a_whole, n_arena), (w_whole, n_ws), (l_whole, n_loc), (k_whole, k_in.numel())):
        assert bool((whole[:m] == 0xA5).all()) and bool((whole[m + n:] == 0xA5).all())
    # another handle than the one the session was indexed with is refused by name
    other = _localizer("pre_norm").localizator._h()
    assert lib.cone_session_localize(other, C.byref(ses), _lib.ptr(tok), arr, nq, _lib.ptr(cls), K, 0, C.byref(p),
                                     C.c_void_p(k_in.data_ptr()), C.c_void_p(k_in.data_ptr() + R8), None, _lib.ptr(l_in),
                                     l_in.numel(), _lib.stream()) == -1
    assert "indexed with another handle" in lib.cone_last_error().decode()


def test_localize_can_be_captured_and_replayed_on_new_inputs():
    """cone_session_localize on one stream, captured once; the token and cls buffers are overwritten and the graph replayed:
    the moments of the NEW queries, == the eager calls."""
    from cone_amd.session import VideoSession
    loc = _localizer()
    vid = _video(900, seed=3)
    lens = [7, 12]
    first, second = _queries(lens, seed=41), _queries(lens, seed=43)
    s = loc.open_video(vid, step="c")
    tok_d = torch.cat([t for t, _ in first]).cuda()
    cls_d = torch.stack([c for _, c in first]).cuda()
    eager_first = VideoSession.read_kept(s.enqueue(tok_d, lens, cls_d).cpu(), 2)         # (sizes the workspace)
    assert eager_first == [loc.predict_moment(vid, q) for q in first]
    ws = s._ws.buf                                              # what the captured launches point at
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = s.enqueue(tok_d, lens, cls_d)
    assert s._ws.buf is ws
    tok_d.copy_(torch.cat([t for t, _ in second]))
    cls_d.copy_(torch.stack([c for _, c in second]))
    graph.replay()
    torch.cuda.synchronize()
    assert VideoSession.read_kept(out.cpu(), 2) == [loc.predict_moment(vid, q) for q in second]
    tok_d.copy_(torch.cat([t for t, _ in first]))
    cls_d.copy_(torch.stack([c for _, c in first]))
    graph.replay()
    torch.cuda.synchronize()
    assert VideoSession.read_kept(out.cpu(), 2) == eager_first
    s.close()
