"""Standing queries on the GPU.

The pin the feature stands on: the candidate rows of a (window, query) do not depend on the call they are computed in --
``cone_library_localize_candidates`` on dictated lists, window ``wi`` alone, as the only window of several pairs, and among all K
windows of 64 pairs, equal as words.

Kernel level: ``cone_watch_plan`` / ``cone_watch_store`` on dictated lists and stamps (tests/watch_refs.py), every buffer inside a
poisoned, guarded buffer, against the numpy models bit for bit.

End to end: ``lib.watch(...).poll()`` ``==`` a fresh ``predict_moment`` on the concatenated features after every kind of change
to the library, ``windows_run ==`` the model's count on the scan's lists, two read-backs a poll."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_library_budget_gpu as T
import watch_refs as R

pytestmark = pytest.mark.gpu

POISON = 0x7EADBEEF
GUARD = 64


def _guarded(n, dtype, fill=None):
    """``n`` elements of ``dtype`` between two guards of 64 words; the inside poisoned too unless ``fill`` (numpy) is given."""
    words = n * (2 if dtype == torch.int64 else 1)
    whole = torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda")
    inner = whole[GUARD:GUARD + words].view(dtype)
    if fill is not None:
        inner.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).cuda().view(dtype))
    return whole, inner


def _guards_hold(whole, inner):
    n = inner.view(torch.int32).numel()
    return bool((whole[:GUARD] == POISON).all()) and bool((whole[GUARD + n:] == POISON).all())


def _words(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype != np.int64 else a


# ------------------------------------------------------------------------------------------------ the two kernels
def _plan(widx, wval, stamp, ctx_l, W, Nq):
    from cone_amd import _lib
    lib = _lib.load()
    nq, K = widx.shape
    n_win = stamp.shape[1]
    ins = [_guarded(nq * K, torch.int32, widx), _guarded(nq * K, torch.float32, wval), _guarded(nq * n_win, torch.int32, stamp)]
    outs = [_guarded(nq * K, torch.int32), _guarded(nq * K, torch.float32), _guarded(nq, torch.int32), _guarded(nq + 1, torch.int32),
            _guarded(nq * K, torch.int64), _guarded(nq * K, torch.int32), _guarded(nq * K, torch.int32)]
    p = lambda b: C.c_void_p(b[1].data_ptr())
    rc = lib.cone_watch_plan(p(ins[0]), p(ins[1]), nq, K, p(ins[2]), n_win, ctx_l, W, Nq, *(p(o) for o in outs), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.cone_last_error()
    for b in ins + outs:
        assert _guards_hold(*b)
    assert np.array_equal(ins[2][1].cpu().numpy().reshape(stamp.shape), stamp)              # the plan writes no stamp
    mw, mv, n, off, cand, sn, tag = (o[1].cpu().numpy() for o in outs)
    return mw.reshape(nq, K), mv.reshape(nq, K), n, off, cand, sn, tag


def _store(cand, miss_widx, n_miss, ctx_l, Nq, cache, stamp):
    from cone_amd import _lib
    lib = _lib.load()
    nq, K = miss_widx.shape
    n_win = stamp.shape[1]
    bufs = [_guarded(cand.size, torch.float32, cand), _guarded(nq * K, torch.int32, miss_widx), _guarded(nq, torch.int32, n_miss),
            _guarded(cache.size, torch.float32, cache), _guarded(stamp.size, torch.int32, stamp)]
    p = lambda b: C.c_void_p(b[1].data_ptr())
    rc = lib.cone_watch_store(p(bufs[0]), p(bufs[1]), p(bufs[2]), nq, K, n_win, ctx_l, Nq, p(bufs[3]), p(bufs[4]), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.cone_last_error()
    for b in bufs:
        assert _guards_hold(*b)
    return bufs[3][1].cpu().numpy().reshape(cache.shape), bufs[4][1].cpu().numpy().reshape(stamp.shape)


def _poisoned_cache(nq, n_win, Nq):
    return np.full((nq, n_win, Nq, 4), POISON, np.int32).view(np.float32)


@pytest.mark.parametrize("K", R.KS)
def test_plan_and_store_equal_the_models_bit_for_bit(K):
    """Every pattern and query count at this K (the compaction's wave edges); the slot count rotates through 3, 5, 10 so that every
    (K, Nq) and every (pattern, Nq) meets.  The store runs on the plan's own outputs and a cache of poison: rows and stamps it
    does not name keep their words."""
    for a, nq in enumerate(R.N_QUERIES):
        for b, pattern in enumerate(R.PATTERNS):
            Nq = R.SLOTS[(a + b + R.KS.index(K)) % 3]
            widx, wval, stamp, ctx_l = R.dictated(nq, K, pattern)
            want = R.plan_ref(widx, wval, stamp, ctx_l, R.W_DICTATED, Nq)
            got = _plan(widx, wval, stamp, ctx_l, R.W_DICTATED, Nq)
            for name, g, w in zip(("miss_widx", "miss_wval", "n_miss", "seg_off", "seg_cand", "seg_n", "seg_tag"), got, want):
                assert np.array_equal(_words(g), _words(w)), (name, nq, pattern, Nq)
            cand, cache = R.cand_rows(want[2], K, Nq), _poisoned_cache(nq, stamp.shape[1], Nq)
            want_cache, want_stamp = R.store_ref(cand, want[0], want[2], ctx_l, Nq, cache, stamp)
            got_cache, got_stamp = _store(cand, got[0], got[2], ctx_l, Nq, cache, stamp)
            assert np.array_equal(_words(got_cache), _words(want_cache)), (nq, pattern, Nq)
            assert np.array_equal(got_stamp, want_stamp), (nq, pattern, Nq)
            # the entries just stored are valid: a second plan at the same ctx_l runs nothing
            assert not _plan(widx, wval, got_stamp, ctx_l, R.W_DICTATED, Nq)[2].any()


def test_the_store_clamps_hostile_counts_and_skips_indices_outside_the_cache():
    K, Nq, n_win, ctx_l = 5, 3, 9, 300
    miss = np.asarray([[1, 2, 3, 4, 5], [0, 9, -1, 7, 8], [6, 5, 4, 3, 2], [8, -3, 1 << 30, 0, 1], [2, 3, 4, 5, 6]], np.int32)
    n_miss = np.asarray([-3, 4, 0, 9, 2], np.int32)                             # below 0, inside, none, above K, inside
    cand = R.cand_rows(n_miss, K, Nq)
    assert cand.shape[0] == (0 + 4 + 0 + 5 + 2) * Nq
    cache, stamp = _poisoned_cache(5, n_win, Nq), np.full((5, n_win), 7, np.int32)
    want = R.store_ref(cand, miss, n_miss, ctx_l, Nq, cache, stamp)
    got = _store(cand, miss, n_miss, ctx_l, Nq, cache, stamp)
    assert np.array_equal(_words(got[0]), _words(want[0])) and np.array_equal(got[1], want[1])
    assert (got[1][0] == 7).all() and (got[1][2] == 7).all() and got[1][1].tolist() == [300, 7, 7, 7, 7, 7, 7, 300, 7]
    assert got[0][3, 8, 0].tolist() == cand[4 * Nq].tolist() and got[0][4, 2, 0].tolist() == cand[9 * Nq].tolist()


# ------------------------------------------------------------------------------------------------ the pin: rows do not depend on the call
def _candidates(lib, vid, queries, rows):
    """``cone_library_localize_candidates`` on dictated lists: ``rows`` = [(query index, [window, ...]), ...], one pair each;
    returns per pair the (windows, Nq, 4) rows as int32 words."""
    loc = lib._loc
    K, Nq = int(loc.args.topk_window), int(loc.args.num_queries)
    widx = torch.full((len(rows), 1, K), -1, dtype=torch.int32)
    for p, (_, ws) in enumerate(rows):
        widx[p, 0, :len(ws)] = torch.tensor(ws, dtype=torch.int32)
    wval = torch.where(widx >= 0, 0.5, float("-inf")).to(torch.float32)
    ks = [len(ws) for _, ws in rows]
    cand = torch.full((sum(ks) * Nq, 4), float("nan"), dtype=torch.float32, device="cuda")
    place = lib._videos[vid][:2]
    lib._enqueue_ragged([(place, queries[q], p, 0) for p, (q, _) in enumerate(rows)], ks,
                        (0, [None] * len(rows), widx.cuda().reshape(-1), wval.cuda().reshape(-1)), 1, cand=cand)
    words = cand.cpu().view(torch.int32).numpy().reshape(-1, Nq, 4)
    out, at = [], 0
    for k in ks:
        out.append(words[at:at + k])
        at += k
    return out


@pytest.mark.parametrize("kind", ("default", "general", "long"))
def test_a_windows_candidate_rows_do_not_depend_on_the_call(kind):
    loc = T._localizer(kind)
    K, W = int(loc.args.topk_window), int(loc.args.max_v_l)
    queries = T._queries(T._mixed_lens(64), seed=5)
    with loc.open_library(2000) as lib:
        lib.add(T._video(57, seed=3))                                           # the video does not start at row 0
        n = (K + 1) * (W // 2) - 7                                              # K + 2 windows, the last one short
        vid = lib.add(T._video(n, seed=4))
        n_win = R.num_windows(n, W)
        assert n_win == K + 2
        # all K windows of 64 pairs: pair q lists windows q, q + 1, ... (mod n_win): every window at every position
        full = _candidates(lib, vid, queries, [(q, [(q + j) % n_win for j in range(K)]) for q in range(64)])
        for wi in (0, 1, n_win // 2, n_win - 2, n_win - 1):
            several = _candidates(lib, vid, queries, [(q, [wi]) for q in range(5)])
            for q in range(5):
                alone = _candidates(lib, vid, queries, [(q, [wi])])[0][0]
                assert not np.array_equal(alone, np.full_like(alone, 0x7FC00000))
                assert np.array_equal(alone, several[q][0]), (kind, wi, q)
                j = (wi - q) % n_win
                if j < K:
                    assert np.array_equal(alone, full[q][j]), (kind, wi, q, j)
        # and with the rest of the library's pairs around it: two windows of pair 3 inside a ragged call of other counts
        mixed = _candidates(lib, vid, queries, [(0, [2, 1, 0]), (3, [n_win - 1, 0]), (9, [1])])
        assert np.array_equal(mixed[1][0], _candidates(lib, vid, queries, [(3, [n_win - 1])])[0][0])
        assert np.array_equal(mixed[1][1], _candidates(lib, vid, queries, [(3, [0])])[0][0])


# ------------------------------------------------------------------------------------------------ end to end
class _Model:
    """The host's mirror of a watcher's stamps: which listed windows the next poll must run, from the scan's own lists."""

    def __init__(self, lib, vid, queries):
        self.lib, self.vid, self.queries = lib, vid, queries
        self.stamp = [dict() for _ in queries]

    def reset(self):
        self.stamp = [dict() for _ in self.queries]

    def poll(self):
        lib, W = self.lib, int(self.lib._loc.args.max_v_l)
        ctx_l = lib._videos[self.vid][1]
        table = lib._table([self.vid], [self.vid])
        run, listed = [], []
        for g in range(0, len(self.queries), 64):
            chunk = self.queries[g:g + 64]
            widx = lib._scan(table, chunk, 1)[0].cpu().view(len(chunk), -1).tolist()
            for q, row in enumerate(widx):
                live = [wi for wi in row if wi >= 0]
                miss = [wi for wi in live if not R.valid_rule(wi, self.stamp[g + q].get(wi, 0), ctx_l, W)]
                for wi in miss:
                    self.stamp[g + q][wi] = ctx_l
                run.append(len(miss))
                listed.append(len(live))
        return run, listed


def _same(got, want):
    """``==`` on moment lists, except that a NaN equals a NaN (``predict_moment`` itself answers NaN scores on NaN frames)."""
    return len(got) == len(want) and all(len(g) == len(w) and all(len(a) == len(b) and all(x == y or (x != x and y != y)
                                                                                           for x, y in zip(a, b))
                                                                  for a, b in zip(g, w)) for g, w in zip(got, want))


def _check(w, model, loc, feats, queries, monkeypatch, tag, nan_ok=False):
    want_run, want_listed = model.poll()
    calls = T._count_readbacks(monkeypatch)
    got = w.poll()
    n_calls = len(calls)
    monkeypatch.undo()
    assert n_calls == 2, tag
    assert w.windows_run == want_run and w.windows_listed == want_listed, (tag, w.windows_run, want_run)
    want = [loc.predict_moment(feats, q) for q in queries]
    assert all(len(m) >= 1 for m in want)
    assert _same(got, want) if nan_ok else got == want, tag
    return want_run


@pytest.mark.parametrize("n_queries", (3, 65))
def test_poll_is_predict_moment_after_every_kind_of_change(n_queries, monkeypatch):
    loc = T._localizer(topk_window=4)
    W = int(loc.args.max_v_l)
    S = W // 2
    queries = T._queries(T._mixed_lens(n_queries), seed=21)
    feats = T._video(300, seed=9)
    more = T._video(400, seed=10)
    with loc.open_library(1500) as lib:
        vid = lib.add(feats)
        with lib.watch(vid, queries) as w:
            Nq = int(loc.args.num_queries)
            assert w.nbytes == n_queries * 8 * (Nq * 16 + 4) and w.windows_run == [0] * n_queries
            model = _Model(lib, vid, queries)
            cold = _check(w, model, loc, feats, queries, monkeypatch, "cold")
            assert cold == [4] * n_queries                                      # every listed window runs once
            # nothing changed: no window runs and the query half is not called at all
            half = []
            real = lib._enqueue_ragged
            monkeypatch.setattr(lib, "_enqueue_ragged", lambda *a, **k: (half.append(1), real(*a, **k))[1])
            again = w.poll()
            assert again == [loc.predict_moment(feats, q) for q in queries] and w.windows_run == [0] * n_queries and not half
            monkeypatch.undo()
            at = 0
            for m in (1, S - 1, S, S + 1, W):                                   # in place: the rows behind the video are free
                row0 = lib._videos[vid][0]
                lib.extend(vid, more[at:at + m])
                assert lib._videos[vid][0] == row0
                feats, at = torch.cat([feats, more[at:at + m]]), at + m
                ran = _check(w, model, loc, feats, queries, monkeypatch, ("extend", m))
                assert max(ran) <= 4 and sum(ran) < 4 * n_queries                # some listed window is answered from the cache
            assert w._n_win > 8 and w.nbytes == n_queries * w._n_win * (Nq * 16 + 4)     # the video outgrew the first cache
            blocker = lib.add(T._video(50, seed=11))                            # right behind the video: the next extend relocates
            ran = _check(w, model, loc, feats, queries, monkeypatch, "add")
            assert ran == [0] * n_queries
            row0 = lib._videos[vid][0]
            lib.extend(vid, more[at:at + 10])
            assert lib._videos[vid][0] != row0
            feats, at = torch.cat([feats, more[at:at + 10]]), at + 10
            _check(w, model, loc, feats, queries, monkeypatch, "relocating extend")
            assert lib.compact() > 0
            assert _check(w, model, loc, feats, queries, monkeypatch, "compact") == [0] * n_queries
            lib.resize(1200)
            assert _check(w, model, loc, feats, queries, monkeypatch, "resize") == [0] * n_queries
            for n_front in (2 * S, 7):                                          # a multiple of S and none: both reset the watcher
                lib.trim(vid, n_front)
                feats = feats[n_front:]
                model.reset()
                ran = _check(w, model, loc, feats, queries, monkeypatch, ("trim", n_front))
                assert ran == [4] * n_queries
            lib.remove(blocker)
            other = lib.add(T._video(120, seed=12))
            assert _check(w, model, loc, feats, queries, monkeypatch, "remove / add") == [0] * n_queries
            lib.extend(vid, more[at:at + 3])
            feats = torch.cat([feats, more[at:at + 3]])
            _check(w, model, loc, feats, queries, monkeypatch, "extend after trim")
            assert lib.predict_moment(other, queries[0]) == loc.predict_moment(T._video(120, seed=12), queries[0])


def test_clips_of_nan_frames_answer_like_predict_moment(monkeypatch):
    """The library's -inf window case: the new clips are NaN frames, every window that holds one ranks last.  ``predict_moment``
    itself answers NaN scores there (a NaN is not ``==`` itself: the lists are compared with NaN equal to NaN, all else ``==``)."""
    loc = T._localizer(topk_window=4)
    queries = T._queries(T._mixed_lens(3), seed=22)
    feats = T._video(300, seed=13)
    with loc.open_library(1000) as lib:
        vid = lib.add(feats)
        with lib.watch(vid, queries) as w:
            model = _Model(lib, vid, queries)
            _check(w, model, loc, feats, queries, monkeypatch, "before")
            for m in (20, 50):
                nan = torch.full((m, 256), float("nan"))
                lib.extend(vid, nan)
                feats = torch.cat([feats, nan])
                _check(w, model, loc, feats, queries, monkeypatch, ("nan", m), nan_ok=True)


def test_lifetime_and_a_general_checkpoint(monkeypatch):
    loc = T._localizer("general", topk_window=4)
    queries = T._queries(T._mixed_lens(3), seed=23)
    feats, more = T._video(300, seed=14), T._video(60, seed=15)
    with loc.open_library(1000) as lib:
        vid = lib.add(feats)
        w = lib.watch(vid, queries)
        model = _Model(lib, vid, queries)
        _check(w, model, loc, feats, queries, monkeypatch, "general cold")
        lib.extend(vid, more)
        _check(w, model, loc, torch.cat([feats, more]), queries, monkeypatch, "general extend")
        w2 = lib.watch(vid, queries[:1])
        w2.close()
        with pytest.raises(RuntimeError, match="the watcher is closed"):
            w2.poll()
        lib.remove(vid)
        with pytest.raises(ValueError, match="unknown or removed video id"):
            w.poll()
        with pytest.raises(ValueError, match="unknown or removed video id"):
            lib.watch(vid, queries)
        vid2 = lib.add(feats)
        w3 = lib.watch(vid2, queries)
    with pytest.raises(RuntimeError, match="the library is closed"):
        w3.poll()
