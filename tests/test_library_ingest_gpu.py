"""Library ingest on the GPU.  First the contract everything else rests on: a clip's rows in every plane of the arena do not
depend on the launch it was indexed in -- neither on the launch's row count (pinned on either side of every form threshold of
the chain's GEMMs) nor on the row's place inside a tile.  Then ``add_many`` against sequential ``add`` calls (the whole arena,
bit for bit), and ``extend`` / ``trim`` against ``CONELocalizator.predict_moment`` on the raw clips, ``==``: no tolerance
appears anywhere."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import ingest_refs as R
from cone_amd import synth

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000            # the arenas' fill: a quiet NaN in every fp32, one in every pair of bf16
KINDS = dict(default={}, txt_pos=dict(use_txt_pos=True), pre_norm=dict(pre_norm=True), general=dict(hidden_dim=128, nheads=4),
             long=dict(max_v_l=300, topk_window=5))


# ------------------------------------------------------------------------------------------------ fixtures
_LOCS, _REFS = {}, {}


def _new_localizer(kind="default", **extra):
    from cone_amd.localizator import CONELocalizator, LOCALIZER_OPT
    kw = KINDS[kind]
    sd = synth.make_state_dict(SimpleNamespace(**dict(LOCALIZER_OPT, **kw)), 5)
    return CONELocalizator(state_dict={k: torch.from_numpy(v) for k, v in sd.items()}, **kw, **extra)


def _localizer(kind="default", **extra):
    """One localizer per checkpoint kind for the whole module (tests/test_library_gpu.py's kinds)."""
    key = (kind, tuple(sorted(extra.items())))
    if key not in _LOCS:
        _LOCS[key] = _new_localizer(kind, **extra)
    return _LOCS[key]


def _kind(kind):
    return _localizer(prefilter_bf16=True) if kind == "prefilter_bf16" else _localizer(kind)


def _video(ctx_l, seed=0):
    return torch.randn(ctx_l, 256, generator=torch.Generator().manual_seed(1000 + seed + ctx_l)) * 2


def _queries(lens, seed=0):
    g = torch.Generator().manual_seed(277 + seed)
    return [(torch.randn(n, 768, generator=g), torch.randn(256, generator=g)) for n in lens]


def _mixed_lens(Q):
    return [(1, 7, 20, 12, 3)[i % 5] for i in range(Q)]


def _want(loc, tag, video, query):
    """``predict_moment`` on raw clips, computed once per tag and never changed."""
    key = (id(loc), tag)
    if key not in _REFS:
        _REFS[key] = loc.predict_moment(video, query)
        assert len(_REFS[key]) >= 1
    return _REFS[key]


def _regions(lib):
    """(int32 view of the plane, int32 words per row) of every plane of the arena: vid_norm, adapted or adapted_bf16, vproj,
    qkv_vid where the handle keeps it."""
    base, words = lib._arena.data_ptr(), lib._arena.view(torch.int32)
    cl, cap = lib._cl, lib._rows.capacity
    out = []
    for ptr, row_bytes in ((cl.vid_norm, cl.v_dim * 4), (cl.adapted, cl.v_dim * 4), (cl.adapted_bf16, cl.v_dim * 2),
                           (cl.vproj, cl.hidden_dim * 4), (cl.qkv_vid, cl.hidden_dim * 12)):
        if ptr:
            at = (ptr - base) // 4
            out.append((words[at:at + cap * row_bytes // 4], row_bytes // 4))
    return out


def _fill(lib, pattern=QNAN):
    lib._arena.view(torch.int32).fill_(pattern)


def _fill_free_rows(lib, pattern=QNAN):
    for words, w in _regions(lib):
        for start, n in lib._rows.holes:
            words[start * w:(start + n) * w] = pattern


def _rows_outside(lib, lo, hi):
    """A copy of every plane's rows outside [lo, hi)."""
    torch.cuda.synchronize()
    return [torch.cat([words[:lo * w], words[hi * w:]]).clone() for words, w in _regions(lib)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. row-count independence
BIG = 20497                  # one launch past the small form's end at N = 256, and 7 rows more for the shifted slices


def _c_add(loc, lib, row0, raw):
    """One ``cone_library_add``: the rows of ``raw`` (a contiguous device view) into arena rows [row0, row0 + n)."""
    from cone_amd import _lib
    clib, h, n = _lib.load(), loc.localizator._h(), int(raw.shape[0])
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == torch.float32 and raw.shape[1] == 256
    assert 0 <= row0 and row0 + n <= lib._rows.capacity
    n_ws = clib.cone_library_add_workspace(h, n)
    ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device="cuda")
    _lib.check(clib.cone_library_add(h, C.byref(lib._cl), row0, C.c_void_p(raw.data_ptr()), n, _lib.ptr(ws), n_ws, _lib.stream()))


def _pin(loc, raw, counts, planes):
    """``raw`` indexed as ONE launch against ``raw[:n]`` and ``raw[7:7 + n]`` as launches of their own, for every n: every plane's
    rows equal bit for bit, and the slice launches touch no other row."""
    total, shift, gap = int(raw.shape[0]), 7, 5
    assert max(counts) + shift <= total
    with loc.open_library(total) as big, loc.open_library(2 * max(counts) + 3 * gap) as small:
        _fill(big)
        _c_add(loc, big, 0, raw)
        big_planes = _regions(big)
        assert len(big_planes) == planes
        torch.cuda.synchronize()
        for words, w in big_planes:
            assert bool((words[:total * w] != QNAN).all())                  # the big launch wrote every row
        cap = small._rows.capacity
        for n in counts:
            _fill(small)
            a0, b0 = gap, 2 * gap + n
            _c_add(loc, small, a0, raw[:n])
            _c_add(loc, small, b0, raw[shift:shift + n])
            torch.cuda.synchronize()
            for p, ((bw, w), (sw, w2)) in enumerate(zip(big_planes, _regions(small))):
                assert w == w2
                assert torch.equal(sw[a0 * w:(a0 + n) * w], bw[:n * w]), (n, p, "rows [0, n)")
                assert torch.equal(sw[b0 * w:(b0 + n) * w], bw[shift * w:(shift + n) * w]), (n, p, "rows [7, 7 + n)")
                for lo, hi in ((0, a0), (a0 + n, b0), (b0 + n, cap)):
                    assert bool((sw[lo * w:hi * w] == QNAN).all()), (n, p, lo, hi)


@pytest.mark.parametrize("kind", ["default", "pre_norm", "txt_pos", "prefilter_bf16", "long", "general"])
def test_a_rows_bits_do_not_depend_on_its_launchs_row_count(kind):
    """The tile edges and either side of every form threshold of the chain's GEMMs (spread form / small form / row tile at
    N = 768 and N = 256; tests/ingest_refs.py derives the counts from csrc/gemm.hip's constants) on the default handle, the
    reduced list on the others: bf16 ``adapted`` rows, no ``qkv_vid`` plane (long windows), the 128 / 4 handle's other GEMMs."""
    loc = _kind(kind)
    counts = R.pin_row_counts() if kind == "default" else R.reduced_row_counts()
    assert max(counts) + 7 <= BIG
    raw = _video(BIG).cuda()
    _pin(loc, raw, counts, planes=3 if kind == "long" else 4)


def test_a_rows_bits_do_not_depend_on_the_tall_form():
    """The tall form of the N = 768 projection (built-in threshold: 262 144 rows) reached through the handle option
    ``gemm_tall_min_rows`` = 4096 on a localizer of this test's own: 4095 rows run below it, 4096 / 4097 and the 8192-row launch
    they are compared with on it."""
    loc = _new_localizer()
    loc.localizator.set_option("gemm_tall_min_rows", 4096)
    raw = _video(BIG).cuda()[:8192].contiguous()
    _pin(loc, raw, [4095, 4096, 4097], planes=4)
    # ... and the same rows on a handle with the built-in threshold: no launch of these sizes is tall there
    plain = _localizer()
    with loc.open_library(8192) as a, plain.open_library(8192) as b:
        _fill(a)
        _fill(b)
        _c_add(loc, a, 0, raw)
        _c_add(plain, b, 0, raw)
        torch.cuda.synchronize()
        assert torch.equal(a._arena.view(torch.int32), b._arena.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. add_many
MIXED_CLIPS = (1, 45, 46, 91, 333, 900, 6000)
FRAGMENTED = (100, 60, 333, 50, 150)


def _mixed_case(loc):
    videos = [_video(n) for n in MIXED_CLIPS]
    queries = _queries(_mixed_lens(21), seed=3)
    pairs = [(i % 7, q) for i, q in enumerate(queries)]
    want = [_want(loc, ("mixed", i), videos[v], q) for i, (v, q) in enumerate(pairs)]
    return videos, pairs, want


def _open(loc, capacity, fragmented):
    """A NaN-filled library; ``fragmented``: the five videos of tests/test_library_gpu.py's isolation test, the second and
    fourth removed and their rows NaN-filled again."""
    lib = loc.open_library(capacity)
    _fill(lib)
    if fragmented:
        ids = [lib.add(_video(n, seed=8)) for n in FRAGMENTED]
        for i in (1, 3):
            lib.remove(ids[i])
        _fill_free_rows(lib)
        assert lib._rows.holes == [(100, 60), (493, 50), (693, 37 + capacity - 730)]
    return lib


def _count_uploads(monkeypatch):
    calls = []
    real_to, real_cuda = torch.Tensor.to, torch.Tensor.cuda

    def to(t, *a, **k):
        out = real_to(t, *a, **k)
        if out.is_cuda and not t.is_cuda:
            calls.append(tuple(t.shape))
        return out

    def cuda(t, *a, **k):
        calls.append(tuple(t.shape))
        return real_cuda(t, *a, **k)
    monkeypatch.setattr(torch.Tensor, "to", to)
    monkeypatch.setattr(torch.Tensor, "cuda", cuda)
    return calls


@pytest.mark.parametrize("fragmented", [False, True])
def test_add_many_leaves_the_state_of_sequential_adds(fragmented, monkeypatch):
    """Fresh: one run, one launch of 7416 rows.  Fragmented: 1 + 45 clips share the first hole, 46 go into the second, the rest
    behind the last video: three runs.  Ids, ``(row0, n, K)``, holes and the WHOLE arena as int32 words equal those of the
    sequential adds; so do they with the runs cut every 1000 rows."""
    from cone_amd.library import plan_runs
    loc = _localizer()
    videos, pairs, want = _mixed_case(loc)
    capacity = sum(MIXED_CLIPS) + (730 if fragmented else 10)
    with _open(loc, capacity, fragmented) as seq, _open(loc, capacity, fragmented) as many, _open(loc, capacity, fragmented) as cut:
        ids = [seq.add(v) for v in videos]
        uploads = _count_uploads(monkeypatch)
        assert many.add_many(videos) == ids
        assert uploads == [(sum(MIXED_CLIPS), 256)]                                             # the call's one upload
        monkeypatch.undo()
        assert cut.add_many(videos, chunk_clips=1000) == ids
        assert [many._videos[i][2] for i in ids] == [2, 2, 3, 4, 9, 20, 20]
        runs = plan_runs([many._videos[i][:2] for i in ids])
        assert [r[:2] for r in runs] == ([(100, 46), (493, 46), (693, 7324)] if fragmented else [(0, 7416)])
        torch.cuda.synchronize()
        for lib in (many, cut):
            assert lib._videos == seq._videos and lib._rows.holes == seq._rows.holes and lib._next_id == seq._next_id
            assert torch.equal(lib._arena.view(torch.int32), seq._arena.view(torch.int32))
        got = many.predict_moments([(ids[v], q) for v, q in pairs])
        for i in range(21):
            assert got[i] == want[i], (i, MIXED_CLIPS[pairs[i][0]])
        assert many.add_many([]) == []


def test_add_many_with_compact_places_behind_the_compacted_videos():
    loc = _localizer()
    late = [_video(60, seed=9), _video(61, seed=9)]
    q = _queries([7], seed=5)[0]
    with _open(loc, 730, True) as lib:
        kept = list(lib._videos)
        before = lib.predict_moments([(v, q) for v in kept])
        with pytest.raises(ValueError, match="add_many: video 1: no free range of 61 clips: the largest free hole has 50"):
            lib.add_many(late)
        assert lib._rows.holes == [(100, 60), (493, 50), (693, 37)]
        ids = lib.add_many(late, compact=True)
        assert [lib._videos[i][:2] for i in ids] == [(583, 60), (643, 61)] and lib._rows.holes == [(704, 26)]
        assert lib.predict_moments([(v, q) for v in kept]) == before
        for i, v in zip(ids, late):
            assert lib.predict_moment(i, q) == loc.predict_moment(v, q)


# ------------------------------------------------------------------------------------------------ 4. extend
CHAIN = (1, 2, 44, 45, 46, 90, 91, 333)
EXTEND_KINDS = ("default", "prefilter_bf16", "long", "general")


def _chain_case(loc, kind):
    full = _video(333, seed=2)
    queries = _queries([1, 7, 20], seed=7)
    want = {n: [_want(loc, ("chain", n, j), full[:n], q) for j, q in enumerate(queries)] for n in CHAIN}
    return full, queries, want


@pytest.mark.parametrize("kind", EXTEND_KINDS)
def test_a_video_grows_in_place_when_the_rows_behind_it_are_free(kind):
    """1 -> 2 -> 44 -> 45 -> 46 -> 90 -> 91 -> 333 clips on one id: half-block and window seams (max_v_l = 90: K goes 2 -> 9).  The
    video lies behind another one, with free rows behind it: it never moves and no row outside its own is written."""
    loc = _kind(kind)
    full, queries, want = _chain_case(loc, kind)
    front = _video(50, seed=3)
    with loc.open_library(400) as lib:
        _fill(lib)
        f = lib.add(front)
        v = lib.add(full[:1])
        assert lib._videos[v][:2] == (50, 1)
        ks = [lib._videos[v][2]]
        for n, grown in zip(CHAIN[:-1], CHAIN[1:]):
            outside = _rows_outside(lib, 50, 50 + grown)
            assert lib.extend(v, full[n:grown]) == grown
            assert lib._videos[v][:2] == (50, grown) and lib._rows.holes == [(50 + grown, 350 - grown)]
            assert _same(_rows_outside(lib, 50, 50 + grown), outside)
            ks.append(lib._videos[v][2])
            for j, q in enumerate(queries):
                assert lib.predict_moment(v, q) == want[grown][j], (grown, j)
        if kind != "long":
            assert ks == [2, 2, 2, 2, 3, 3, 4, 9]
        assert lib.predict_moment(f, queries[1]) == loc.predict_moment(front, queries[1])
        for words, w in _regions(lib):
            assert bool((words[383 * w:] == QNAN).all())


@pytest.mark.parametrize("kind", EXTEND_KINDS)
def test_a_video_relocates_when_a_neighbour_lies_directly_behind(kind):
    """The same chain; before every step a 400-clip neighbour is added, which only fits behind the video (the holes the video
    leaves are smaller and lie between neighbours): every step moves the resident rows into the tail hole, leaves the old range
    as a hole, and changes neither the neighbour's rows nor its answers."""
    loc = _kind(kind)
    full, queries, want = _chain_case(loc, kind)
    neighbour = _video(400, seed=4)
    want_nb = _want(loc, "chain-neighbour", neighbour, queries[1])
    with loc.open_library(sum(CHAIN) + 7 * 400 + 20) as lib:
        _fill(lib)
        v = lib.add(full[:1])
        for n, grown in zip(CHAIN[:-1], CHAIN[1:]):
            row0 = lib._videos[v][0]
            nb = lib.add(neighbour)
            nb_row0 = lib._videos[nb][0]
            assert nb_row0 == row0 + n                                                          # directly behind
            torch.cuda.synchronize()
            nb_rows = [words[nb_row0 * w:(nb_row0 + 400) * w].clone() for words, w in _regions(lib)]
            assert lib.extend(v, full[n:grown]) == grown
            assert lib._videos[v][:2] == (nb_row0 + 400, grown) and (row0, n) in lib._rows.holes
            torch.cuda.synchronize()
            assert _same([words[nb_row0 * w:(nb_row0 + 400) * w] for words, w in _regions(lib)], nb_rows)
            for j, q in enumerate(queries):
                assert lib.predict_moment(v, q) == want[grown][j], (grown, j)
            assert lib.predict_moment(nb, queries[1]) == want_nb
        _fill_free_rows(lib)                                                # (the old ranges keep stale rows: nobody may need them)
        assert lib.predict_moment(v, queries[2]) == want[333][2]


def test_extend_with_compact_where_the_free_clips_suffice_but_no_hole_does():
    loc = _localizer()
    clips = (40, 10, 30, 100)
    videos = [_video(n, seed=6) for n in clips]
    more = _video(45, seed=7)
    queries = _queries([7, 20], seed=9)
    with loc.open_library(250) as lib:
        _fill(lib)
        a, filler, b, c = (lib.add(v) for v in videos)
        lib.remove(filler)
        _fill_free_rows(lib)
        assert lib._rows.holes == [(40, 10), (180, 70)] and lib.free_clips == 80
        others = lib.predict_moments([(a, queries[0]), (c, queries[1])])
        with pytest.raises(ValueError, match="extend: the 45 rows behind video 3 are not free and no free range of 75 clips: the largest "
                                             "free hole has 70"):
            lib.extend(b, more)
        assert lib._rows.holes == [(40, 10), (180, 70)] and lib._videos[b] == (50, 30, 2)
        assert lib.extend(b, more, compact=True) == 75
        assert lib._videos == {a: (0, 40, 2), b: (170, 75, 3), c: (70, 100, 4)} and lib._rows.holes == [(40, 30), (245, 5)]
        _fill_free_rows(lib)
        whole = torch.cat([videos[2], more])
        for q in queries:
            assert lib.predict_moment(b, q) == loc.predict_moment(whole, q)
        assert lib.predict_moments([(a, queries[0]), (c, queries[1])]) == others


# ------------------------------------------------------------------------------------------------ search after ingest
def test_search_after_ingest_equals_a_fresh_library_in_the_same_arena_order():
    """``add_many`` three videos, grow the last in place, grow the first (it relocates behind the others: arena order 2, 3, 1).
    Rankings and searches equal those of a library that ``add``ed the whole videos in that order, score bits included; two of
    the videos are twins, so the tie order is the arena order in both."""
    loc = _localizer()
    v1, v2, v3 = _video(200, seed=11), _video(333, seed=12), _video(200, seed=11)
    assert torch.equal(v1, v3)
    queries = _queries(_mixed_lens(5), seed=13)
    with loc.open_library(1200) as lib, loc.open_library(1200) as fresh:
        _fill(lib)
        _fill(fresh)
        a, b, c = lib.add_many([v1[:120], v2, v3[:150]])
        lib.rank_videos(queries[:1])                                        # (a scan table of the old layout exists)
        assert lib._scan_cache is not None
        assert lib.extend(c, v3[150:]) == 200 and lib._videos[c][:2] == (453, 200)
        assert lib._scan_cache is None
        assert lib.extend(a, v1[120:]) == 200 and lib._videos[a][:2] == (653, 200)
        _fill_free_rows(lib)
        fb, fc, fa = (fresh.add(v) for v in (v2, v3, v1))
        to_fresh = {a: fa, b: fb, c: fc}
        ranked = lib.rank_videos(queries)
        assert [[(to_fresh[v], s) for v, s in row] for row in ranked] == fresh.rank_videos(queries)
        for row in ranked:
            order = [v for v, _ in row]
            assert order.index(c) + 1 == order.index(a) and dict(row)[a] == dict(row)[c]        # twins: the one in front first
        found = lib.search(queries, n_videos=2)
        assert [[(to_fresh[v], s, m) for v, s, m in row] for row in found] == fresh.search(queries, n_videos=2)
        assert all(len(row) == 2 for row in found)


# ------------------------------------------------------------------------------------------------ 5. trim
@pytest.mark.parametrize("t", [1, 45, 46])
def test_trim_answers_like_the_video_without_its_first_clips(t):
    loc = _localizer()
    full = _video(333, seed=2)
    queries = _queries([1, 7, 20], seed=7)
    with loc.open_library(340) as lib:
        _fill(lib)
        v = lib.add(full)
        torch.cuda.synchronize()
        before = lib._arena.clone()
        assert lib.trim(v, t) == 333 - t
        assert lib._videos[v] == (t, 333 - t, min(20, R.L.num_windows(333 - t))) and lib._rows.holes == [(0, t), (333, 7)]
        for j, q in enumerate(queries):
            assert lib.predict_moment(v, q) == _want(loc, ("trim", t, j), full[t:], q)
        torch.cuda.synchronize()
        assert torch.equal(lib._arena.view(torch.int32), before.view(torch.int32))              # nothing was written
        with pytest.raises(ValueError, match="trim: n_front=%d not in" % (333 - t)):
            lib.trim(v, 333 - t)


def test_extend_and_trim_alternate_as_a_sliding_window():
    """Six rounds on a 300-row arena, seams crossed in both directions; in round five neither the rows behind the video nor any
    hole hold the new clips, and ``compact=True`` slides the video to the front first."""
    loc = _localizer()
    source = _video(600, seed=14)
    queries = _queries([7, 20], seed=15)
    with loc.open_library(300) as lib:
        _fill(lib)
        lo, hi = 0, 200
        v = lib.add(source[lo:hi])
        rows = []
        for r, (more, drop) in enumerate(((8, 8), (45, 1), (1, 45), (37, 46), (90, 90), (3, 7))):
            assert lib.extend(v, source[hi:hi + more], compact=True) == hi + more - lo
            hi += more
            assert lib.predict_moment(v, queries[0]) == _want(loc, ("slide", lo, hi, 0), source[lo:hi], queries[0]), (r, "extend")
            assert lib.trim(v, drop) == hi - lo - drop
            lo += drop
            assert lib.predict_moment(v, queries[1]) == _want(loc, ("slide", lo, hi, 1), source[lo:hi], queries[1]), (r, "trim")
            rows.append(lib._videos[v][:2])
        assert rows == [(8, 200), (9, 244), (54, 200), (100, 191), (90, 191), (97, 187)]
