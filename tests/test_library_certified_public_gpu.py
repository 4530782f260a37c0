"""Certified library budgets through the public interface: a certified and a plain library receive the same videos and go through
the same operations; after each, ``search_windows`` and ``search_moments`` are ``==`` between the two -- whatever
``last_certified`` says --, and everything else on the certified library is the plain library's.  The localizer's synthetic
checkpoint.  On the parent ``open_library(..., certified=True)`` does not exist: every test here fails there."""
import ctypes as C

import pytest
import torch

import test_library_budget_gpu as T            # its localizers, videos and queries: built once per session

pytestmark = pytest.mark.gpu

LENGTHS = (1, 45, 46, 90, 200, 900, 333, 91, 500, 2, 700, 150)
CAPACITY = 6000


def _planted(ctx_l, seed, queries):
    """A video of noise with a few clips that point along the queries' cls vectors: a peak per query, its place and height differ from
    video to video."""
    v = T._video(ctx_l, seed)
    g = torch.Generator().manual_seed(31 * seed + ctx_l)
    for i, (_, cls) in enumerate(queries[:5]):
        at = int(torch.randint(0, ctx_l, (1,), generator=g))
        v[at] = cls * (3.0 + 0.5 * ((seed + i) % 7))
    return v


_STATE = {}


def _queries():
    if "q" not in _STATE:
        _STATE["q"] = T._queries(T._mixed_lens(65), seed=3)
    return _STATE["q"]


def _pair(**kw):
    loc = T._localizer()
    return loc.open_library(CAPACITY, certified=True, **kw), loc.open_library(CAPACITY)


def _same(cert, plain, queries, n_windows=20, videos=None, want_flags=None):
    a = cert.search_windows(queries, n_windows, videos=videos)
    flags = list(cert.last_certified)
    assert a == plain.search_windows(queries, n_windows, videos=videos)
    assert len(flags) == len(queries) and set(flags) <= {0, 1}
    b = cert.search_moments(queries, n_windows, videos=videos)
    assert b == plain.search_moments(queries, n_windows, videos=videos)
    assert list(cert.last_certified) == flags                       # the same scans: the same proofs
    assert any(len(row) for row in a) and any(len(row) for row in b)
    if want_flags is not None:
        assert flags == want_flags, flags
    return flags


def _both(cert, plain, call, *args, **kw):
    got = getattr(cert, call)(*args, **kw), getattr(plain, call)(*args, **kw)
    assert got[0] == got[1], call
    return got[0]


def test_the_two_libraries_agree_after_every_operation():
    queries = _queries()[:5]
    vids = [_planted(n, i, queries) for i, n in enumerate(LENGTHS)]
    cert, plain = _pair()
    assert cert.certified and cert.n_cand == 0 and not plain.certified and plain.last_certified is None
    from cone_amd import _lib
    assert cert.nbytes - plain.nbytes == _lib.load().cone_library_shadow_bytes(C.byref(cert._cl)) == cert._shadow.numel()
    ids = _both(cert, plain, "add_many", vids[:10])
    flags = _same(cert, plain, queries)
    assert flags == [1] * 5                                         # planted peaks, the default n_cand: every proof holds
    for v in ids[::3]:
        cert.remove(v), plain.remove(v)
    live = [v for v in ids if v not in ids[::3]]
    _same(cert, plain, queries, want_flags=[1] * 5)
    ids += [_both(cert, plain, "add", vids[10])]                    # into the first hole that fits
    _same(cert, plain, queries)
    last = max(cert._videos, key=lambda v: cert._videos[v][0])
    more = T._video(60, 77)
    row0 = cert._videos[last][0]
    assert _both(cert, plain, "extend", last, more) == cert._videos[last][1] and cert._videos[last][0] == row0     # in place
    _same(cert, plain, queries)
    first = min(cert._videos, key=lambda v: cert._videos[v][0] if cert._videos[v][1] > 40 else 10 ** 9)
    row0 = cert._videos[first][0]
    _both(cert, plain, "extend", first, _planted(50, 5, queries))
    assert cert._videos[first][0] != row0                           # a neighbour lies behind it: relocated, the shadow rows with it
    _same(cert, plain, queries)
    _both(cert, plain, "trim", first, 30)
    _same(cert, plain, queries)
    assert _both(cert, plain, "compact") > 0
    _same(cert, plain, queries)
    _same(cert, plain, queries, videos=live[1::2])
    cert.resize(7000), plain.resize(7000)
    assert cert.nbytes - plain.nbytes == _lib.load().cone_library_shadow_bytes(C.byref(cert._cl))
    _same(cert, plain, queries)
    ids += [_both(cert, plain, "add", vids[11])]                    # the new arena's shadow follows new rows too
    _same(cert, plain, queries, want_flags=[1] * 5)
    # everything else runs the fp32 path on the same rows
    pairs = [(v, queries[i % 5]) for i, v in enumerate(list(cert._videos)[:6])]
    _both(cert, plain, "predict_moments", pairs)
    _both(cert, plain, "rank_videos", queries)
    _both(cert, plain, "search", queries[:2], 3)
    wc, wp = cert.watch_moments(queries[:3], 20, 5), plain.watch_moments(queries[:3], 20, 5)
    assert wc.poll() == wp.poll() == cert.search_moments(queries[:3], 20, 5)
    assert cert.search_windows([], 20) == [] and cert.last_certified == []           # nothing searched: the old flags do not linger
    cert.search_windows(queries[:2], 20)
    assert cert.search_moments(queries[:2], 20, videos=[]) == [[], []] and cert.last_certified == []
    cert.close(), plain.close()
    assert cert.nbytes == 0


@pytest.fixture(scope="module")
def libraries():
    queries = _queries()
    cert, plain = _pair()
    vids = [_planted(n, 20 + i, queries) for i, n in enumerate(LENGTHS)]
    ids = _both(cert, plain, "add_many", vids)
    yield cert, plain, ids
    cert.close(), plain.close()


@pytest.mark.parametrize("n_windows", [1, 20, 60])
@pytest.mark.parametrize("nq", [1, 5, 65])
def test_query_counts_and_budgets(libraries, nq, n_windows):
    cert, plain, ids = libraries
    flags = _same(cert, plain, _queries()[:nq], n_windows)
    assert len(flags) == nq
    if n_windows == 20:
        _same(cert, plain, _queries()[:nq], n_windows, videos=ids[2::3])


def test_the_fallback_a_twin_video_at_n_cand_w_plus_2(monkeypatch):
    """The library holds one flat video twice: its 16 windows tie exactly, in the shadow and in fp32.  A budget of 10 windows with 12
    candidates ends inside that tie -- t and c_last are scores of the same rows, so t - c_last <= E: not proved --, the chunk runs the
    fp32 scan again (a second small read-back) and the answer is the plain library's."""
    queries = _queries()[:3]
    flat = (queries[0][1] * 4.0).repeat(300, 1)
    cert, plain = _pair(n_cand=12)
    assert cert.n_cand == 12
    for lib in (cert, plain):
        lib.add_many([flat, T._video(400, 9), flat.clone()])
    calls = T._count_readbacks(monkeypatch)
    a = cert.search_windows(queries[:1], 10)
    assert cert.last_certified == [0] and len(calls) == 3           # budget + flags, the fallback's budget, the kept rows
    del calls[:]
    assert a == plain.search_windows(queries[:1], 10) and len(calls) == 2
    assert [row[2] for row in a[0]][:2] == [8, 2]                   # the first twin's eight windows, then the second's first two
    flags = _same(cert, plain, queries, 10)
    assert flags[0] == 0
    cert.close(), plain.close()


def test_certified_with_prefilter_bf16_is_open_videos_refusal():
    loc = T._localizer(prefilter_bf16=True)
    with pytest.raises(ValueError) as lib_err:
        loc.open_library(100, certified=True)
    with pytest.raises(ValueError) as vid_err:
        loc.open_video(T._video(50), certified=True)
    assert str(lib_err.value) == str(vid_err.value)
    loc.open_library(100).close()                                   # a plain bf16 library opens as before
