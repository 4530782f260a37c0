"""Library ingest, the part that needs no GPU: ``RowRanges.take_at`` against the row model, ``plan_runs`` / ``plan_extend`` and the
placement of ``add_many`` / ``extend`` / ``trim`` against first-principles models on a library object without a handle or an
arena (its launches are recorded, not run), and every refusal before any GPU work."""
import numpy as np
import pytest
import torch

import ingest_refs as R


def _feats(n, dim=256):
    return torch.zeros(n, dim)


# ------------------------------------------------------------------------------------------------ take_at
def test_take_at_follows_the_model_on_the_scripted_sequence():
    from cone_amd.library import RowRanges
    rows, model, owned = RowRanges(R.TAKE_AT_CAPACITY), R.RowModel(R.TAKE_AT_CAPACITY), {}
    seen = set()
    for op, arg, n in R.TAKE_AT_SCRIPT:
        if op == "take":
            owned[arg] = (rows.take(n), n)
            assert model.take(n) == owned[arg][0]
        elif op == "release":
            rows.release(*owned[arg])
            model.release(*owned.pop(arg))
        elif op == "take_at":
            assert model.take_at(arg, n) == arg, (op, arg, n)
            assert rows.take_at(arg, n) == arg
        else:
            assert model.take_at(arg, n) is None, (op, arg, n)
            before = list(rows.holes)
            with pytest.raises(ValueError):
                rows.take_at(arg, n)
            assert rows.holes == before
        assert rows.holes == model.holes(), (op, arg, n)
        assert rows.free == int((~model.used).sum())
        seen.add(op)
    assert seen == {"take", "release", "take_at", "refuse_at"}
    assert rows.holes == []                                                 # the script ends on a full arena
    with pytest.raises(ValueError, match=r"rows \[3, 5\) do not lie inside one free hole"):
        rows.take_at(3, 2)


def test_take_keeps_its_message():
    from cone_amd.library import RowRanges
    rows = RowRanges(10)
    rows.take_at(4, 2)
    with pytest.raises(ValueError, match=r"no free range of 5 clips: the largest free hole has 4 \(8 of 10 clips are free; a library "
                                         r"does not compact\)"):
        rows.take(5)


def test_take_take_at_and_release_follow_the_model_on_random_traffic():
    from cone_amd.library import RowRanges
    exact = refused = 0
    for seq in range(240):
        rng = np.random.default_rng(1000 + seq)
        cap = int(rng.integers(20, 200))
        rows, model, owned = RowRanges(cap), R.RowModel(cap), []
        for _ in range(60):
            p = rng.random()
            if owned and p < 0.35:
                r = owned.pop(int(rng.integers(len(owned))))
                rows.release(*r)
                model.release(*r)
            elif p < 0.65:
                n = int(rng.integers(1, 40))
                want = model.take(n)
                if want is None:
                    with pytest.raises(ValueError, match=f"no free range of {n} clips"):
                        rows.take(n)
                else:
                    assert rows.take(n) == want
                    owned.append((want, n))
            else:
                # half of the exact claims aim at a hole (start, inside, end), half anywhere
                holes = model.holes()
                n = int(rng.integers(1, 25))
                if holes and rng.random() < 0.5:
                    h0, length = holes[int(rng.integers(len(holes)))]
                    start = h0 + int(rng.integers(0, max(1, length - n + 2)))
                else:
                    start = int(rng.integers(0, cap))
                want = model.take_at(start, n)
                if want is None:
                    with pytest.raises(ValueError, match="do not lie inside one free hole"):
                        rows.take_at(start, n)
                    refused += 1
                else:
                    assert rows.take_at(start, n) == start
                    owned.append((start, n))
                    exact += 1
            assert rows.holes == model.holes(), seq
    assert exact > 1000 and refused > 1000


# ------------------------------------------------------------------------------------------------ plan_runs
def test_plan_runs_merges_adjacent_ascending_ranges_only():
    from cone_amd.library import plan_runs
    assert plan_runs([]) == []
    assert plan_runs([(0, 5)]) == [(0, 5, 0, 1)]
    assert plan_runs([(0, 5), (5, 7), (12, 1)]) == [(0, 13, 0, 3)]                              # a fresh arena: one run
    assert plan_runs([(5, 7), (0, 5)]) == [(5, 7, 0, 1), (0, 5, 1, 2)]                          # adjacent but descending
    assert plan_runs([(0, 5), (6, 7)]) == [(0, 5, 0, 1), (6, 7, 1, 2)]                          # a gap of one row
    assert plan_runs([(100, 1), (101, 45), (493, 46), (160, 91)]) == [(100, 46, 0, 2), (493, 46, 2, 3), (160, 91, 3, 4)]
    with pytest.raises(ValueError):
        plan_runs([(0, 0)])
    rng = np.random.default_rng(8)
    for _ in range(200):
        rows, videos = __import__("move_refs").history(rng)
        lens = [int(n) for n in rng.integers(1, 50, int(rng.integers(1, 8)))]
        placed, _ = R.sequential_add(rows.capacity, videos, lens)
        if isinstance(placed, int):
            continue
        runs = plan_runs(placed)
        assert runs == R.runs_model(placed)
        assert sum(r[1] for r in runs) == sum(lens) and [r[2] for r in runs][1:] == [r[3] for r in runs][:-1]


# ------------------------------------------------------------------------------------------------ add_many
FRAGMENTED = [(0, 100), (160, 333), (543, 150)]            # holes [(100, 60), (493, 50), (693, 37)] of 730 rows
COMPACT_HELPS = [(0, 40), (50, 30), (80, 100)]             # holes [(40, 10), (180, 70)] of 250 rows


def _launch_rows(launched):
    """(arena row, raw row, rows) of every recorded index launch."""
    return [l for kind, *rest in launched if kind == "index" for l in rest[1]]


@pytest.mark.parametrize("capacity,owned,lens", [
    (7436, [], (1, 45, 46, 91, 333, 900, 6000)),                            # fresh: one run
    (730 + 7416, FRAGMENTED, (1, 45, 46, 91, 333, 900, 6000)),              # fragmented: 1 + 45 | 46 | 91, 333, 900, 6000
    (730, FRAGMENTED, (60, 50, 37)),                                        # fills every hole exactly: a full arena
    (730, FRAGMENTED, (37, 37, 37, 23)),                                    # 37 + 23 share the first hole with a video between them
    (300, [(0, 100), (100, 200)], ()),                                      # a full arena, nothing to add
])
def test_add_many_places_like_sequential_adds(capacity, owned, lens):
    from cone_amd.library import plan_runs
    lib = R.stub_library(capacity, owned)
    want, holes = R.sequential_add(capacity, owned, lens)
    first_id = lib._next_id
    ids = lib.add_many([_feats(n) for n in lens])
    assert ids == list(range(first_id, first_id + len(lens))) and lib._next_id == first_id + len(lens)
    assert [lib._videos[i][:2] for i in ids] == want and lib._rows.holes == holes
    assert [lib._videos[i][2] for i in ids] == [min(20, R.L.num_windows(n)) for n in lens]
    if not lens:
        assert lib.launched == [] and lib._scan_cache == "stale"
        return
    assert lib._scan_cache is None
    assert len(lib.launched) == 1 and lib.launched[0][1] == (sum(lens), 256)                     # one concatenation, one _index
    runs = plan_runs(want)
    assert _launch_rows(lib.launched) == [(r[0], sum(lens[:r[2]]), r[1]) for r in runs]         # one launch per run
    if not owned:
        assert len(runs) == 1
    # every video's rows come from its own rows of the concatenation
    at = np.cumsum([0] + list(lens))
    for i, (row0, n) in enumerate(want):
        hit = [(a, r, k) for a, r, k in _launch_rows(lib.launched) if a <= row0 and row0 + n <= a + k]
        assert len(hit) == 1 and hit[0][1] + (row0 - hit[0][0]) == at[i]


def test_add_many_on_random_arenas_equals_the_sequential_model():
    import move_refs
    rng = np.random.default_rng(21)
    fitted = refused = 0
    for _ in range(300):
        rows, videos = move_refs.history(rng)
        lens = [int(n) for n in rng.integers(1, 70, int(rng.integers(1, 7)))]
        lib = R.stub_library(rows.capacity, videos)
        assert lib._rows.holes == rows.holes
        before = R.state(lib)
        want, holes = R.sequential_add(rows.capacity, videos, lens)
        if isinstance(want, int):
            with pytest.raises(ValueError, match=f"add_many: video {want}: no free range of {lens[want]} clips"):
                lib.add_many([_feats(n) for n in lens])
            assert R.state(lib) == before and lib.launched == []
            refused += 1
        else:
            ids = lib.add_many([_feats(n) for n in lens])
            assert [lib._videos[i][:2] for i in ids] == want and lib._rows.holes == holes
            fitted += 1
    assert fitted > 50 and refused > 50


def test_add_many_cuts_runs_at_chunk_clips():
    lib = R.stub_library(730 + 3000, FRAGMENTED)
    lib.add_many([_feats(n) for n in (40, 20, 50, 2500)], chunk_clips=1000)
    # runs: [100, 160) (two videos), [493, 543), [693, 3193): the last is cut into 1000 + 1000 + 500
    assert _launch_rows(lib.launched) == [(100, 0, 60), (493, 60, 50), (693, 110, 1000), (1693, 1110, 1000), (2693, 2110, 500)]
    lib = R.stub_library(100, [])
    lib.add_many([_feats(30), _feats(30)], chunk_clips=30)                                      # a cut on a video seam
    assert _launch_rows(lib.launched) == [(0, 0, 30), (30, 30, 30)]
    lib = R.stub_library(100, [])
    lib.add_many([_feats(30), _feats(31)], chunk_clips=60)                                      # a last chunk of one row
    assert _launch_rows(lib.launched) == [(0, 0, 60), (60, 60, 1)]


def test_a_failing_add_many_rolls_back_and_names_the_video():
    lib = R.stub_library(730, FRAGMENTED)
    before = R.state(lib)
    with pytest.raises(ValueError, match=r"add_many: video 2: no free range of 51 clips: the largest free hole has 37 "
                                         r"\(37 of 730 clips are free; a library does not compact\)"):
        lib.add_many([_feats(60), _feats(50), _feats(51)])                  # two ranges were taken when the third fails
    assert R.state(lib) == before and lib.launched == [] and lib._scan_cache == "stale"
    ids = lib.add_many([_feats(60), _feats(50)])                             # ids were not burnt by the failure
    assert ids == [4, 5]


def test_add_many_with_compact_in_three_situations():
    # it suffices without: nothing is compacted
    lib = R.stub_library(730, FRAGMENTED)
    lib.add_many([_feats(60), _feats(37)], compact=True)
    assert [k for k, *_ in lib.launched] == ["index"] and lib._rows.holes == [(530, 13), (693, 37)]     # first fit
    # it is needed: first-fit fails on the second video, the free clips hold both
    lib = R.stub_library(730, FRAGMENTED)
    ids = lib.add_many([_feats(60), _feats(61)], compact=True)
    assert [k for k, *_ in lib.launched] == ["compact", "index"]
    assert [lib._videos[v][:2] for v in (1, 2, 3)] == [(0, 100), (100, 333), (433, 150)]
    assert [lib._videos[v][:2] for v in ids] == [(583, 60), (643, 61)] and lib._rows.holes == [(704, 26)]
    assert _launch_rows(lib.launched) == [(583, 0, 121)]                                        # behind the resident videos: one run
    # it is not enough: more than is free in total -- nothing is compacted, nothing changes
    lib = R.stub_library(730, FRAGMENTED)
    before = R.state(lib)
    with pytest.raises(ValueError, match="add_many: video 1: no free range of 88 clips: the largest free hole has 50"):
        lib.add_many([_feats(60), _feats(88)], compact=True)
    assert R.state(lib) == before and lib.launched == []
    with pytest.raises(ValueError, match="add_many: video 0: no free range of 61 clips: the largest free hole has 60"):
        lib.add_many([_feats(61)])                                          # the default never compacts
    assert R.state(lib) == before and lib.launched == []


def _forbid_live_check(lib):
    def boom():
        raise AssertionError("_check_live ran before the refusal")
    lib._check_live = boom
    return lib


def test_add_many_checks_every_video_before_it_takes_a_row():
    lib = _forbid_live_check(R.stub_library(730, FRAGMENTED))
    before = R.state(lib)
    for videos, want in (([_feats(5), torch.zeros(5)], r"add_many: video 1: video_feats must be \(clips >= 1, dim\), got \(5,\)"),
                         ([_feats(5), _feats(0)], r"add_many: video 1: .*got \(0, 256\)"),
                         ([_feats(5), _feats(5), _feats(5, 128)], "add_many: video 2: appearance clip features: feature dim 128, the "
                                                                   "model was built for 256"),
                         ([None], "add_many: video 0")):
        with pytest.raises(ValueError, match=want):
            lib.add_many(videos)
    with pytest.raises(ValueError, match="chunk_clips=0 < 1"):
        lib.add_many([_feats(5)], chunk_clips=0)
    assert lib.add_many([]) == []                                           # nothing to do: not even the live check
    assert R.state(lib) == before and lib.launched == []
    closed = R.stub_library(100, [])
    closed._open = False
    with pytest.raises(RuntimeError, match="closed"):
        closed.add_many([_feats(5)])
    assert closed._rows.holes == [(0, 100)] and closed.launched == []


# ------------------------------------------------------------------------------------------------ extend
def test_plan_extend_in_place_relocation_and_no_room():
    from cone_amd.library import RowRanges, plan_extend
    rows = RowRanges(730)
    for row0, n in FRAGMENTED:
        rows.take_at(row0, n)
    assert plan_extend(rows, 0, 100, 60) == ("in_place", 0)                 # the hole behind it, exactly
    assert plan_extend(rows, 0, 100, 1) == ("in_place", 0)
    assert plan_extend(rows, 543, 150, 37) == ("in_place", 543)             # up to the capacity
    assert plan_extend(rows, 543, 150, 38) == ("no_room", None)
    assert plan_extend(rows, 0, 100, 61) == ("no_room", None)               # 161 rows: no hole
    rows.release(160, 333)                                                  # [100, 543) is one hole now
    assert plan_extend(rows, 543, 150, 38) == ("relocate", 100)             # behind it only 37: into the first hole that holds 188
    assert plan_extend(rows, 543, 150, 293) == ("relocate", 100) and plan_extend(rows, 543, 150, 294) == ("no_room", None)
    assert plan_extend(rows, 0, 100, 443) == ("in_place", 0) and plan_extend(rows, 0, 100, 444) == ("no_room", None)
    assert rows.holes == [(100, 443), (693, 37)]                            # a plan changes nothing
    with pytest.raises(ValueError):
        plan_extend(rows, 0, 100, 0)
    rng = np.random.default_rng(33)
    import move_refs
    kinds = set()
    for _ in range(300):
        rr, videos = move_refs.history(rng)
        if not videos:
            continue
        row0, n = videos[int(rng.integers(len(videos)))]
        m = int(rng.integers(1, 80))
        got = plan_extend(rr, row0, n, m)
        assert got == R.extend_model(rr.capacity, videos, row0, n, m)
        kinds.add(got[0])
    assert kinds == {"in_place", "relocate", "no_room"}


def test_extend_in_place_takes_only_the_rows_behind_the_video():
    lib = R.stub_library(730, FRAGMENTED, max_v_l=90)
    assert lib.extend(1, _feats(45)) == 145
    assert lib._videos[1] == (0, 145, 5) and lib._rows.holes == [(145, 15), (493, 50), (693, 37)]
    assert lib.launched == [("index", (45, 256), [(100, 0, 45)])] and lib._scan_cache is None
    assert lib.extend(1, _feats(15)) == 160 and lib._rows.holes == [(493, 50), (693, 37)]
    assert lib._videos[2] == (160, 333, 9) and lib._videos[3] == (543, 150, 5)


def test_extend_relocates_when_a_neighbour_lies_behind():
    lib = R.stub_library(1000, [(0, 100), (100, 40), (140, 60)])
    assert lib.extend(2, _feats(5)) == 45                                   # rows [140, ...) belong to video 3
    assert lib._videos[2] == (200, 45, 2) and lib._rows.holes == [(100, 40), (245, 755)]
    assert lib.launched == [("move", [(100, 200, 40)], [(0, 40, False)]), ("index", (5, 256), [(240, 0, 5)])]
    assert lib._videos[1] == (0, 100, 4) and lib._videos[3] == (140, 60, 3)
    # first fit: a hole in FRONT of the video is taken when it holds all of it
    lib = R.stub_library(300, [(100, 50), (150, 150)])
    lib.extend(1, _feats(50))
    assert lib._videos[1] == (0, 100, 4) and lib._rows.holes == [(100, 50)]
    assert lib.launched[0] == ("move", [(100, 0, 50)], [(0, 50, False)])


def test_extend_with_no_room_changes_nothing_and_compact_helps_where_it_can():
    lib = R.stub_library(730, FRAGMENTED)
    before = R.state(lib)
    with pytest.raises(ValueError, match=r"extend: the 61 rows behind video 1 are not free and no free range of 161 clips: the "
                                         r"largest free hole has 60 \(147 of 730 clips are free"):
        lib.extend(1, _feats(61))
    assert R.state(lib) == before and lib.launched == [] and lib._scan_cache == "stale"
    # compact=True: video 1 is not the last one, 100 + 61 > 147 free clips: still no room, nothing is compacted
    with pytest.raises(ValueError, match="extend: the 61 rows behind video 1 are not free"):
        lib.extend(1, _feats(61), compact=True)
    assert R.state(lib) == before and lib.launched == []
    # free clips suffice, no hole does: 80 clips are free in holes of 10 and 70, the grown video takes 75
    lib = R.stub_library(250, COMPACT_HELPS)
    assert lib._rows.holes == [(40, 10), (180, 70)]
    with pytest.raises(ValueError, match="extend: the 45 rows behind video 2 are not free and no free range of 75 clips"):
        lib.extend(2, _feats(45))
    assert lib.extend(2, _feats(45), compact=True) == 75
    assert lib.launched == [("compact",), ("move", [(40, 170, 30)], [(0, 30, False)]), ("index", (45, 256), [(200, 0, 45)])]
    assert lib._videos == {1: (0, 40, 2), 2: (170, 75, 3), 3: (70, 100, 4)} and lib._rows.holes == [(40, 30), (245, 5)]
    # the LAST video needs only the new rows: it grows in place behind the compacted arena
    lib = R.stub_library(730, FRAGMENTED)
    assert lib.extend(3, _feats(147), compact=True) == 297
    assert [k for k, *_ in lib.launched] == ["compact", "index"]
    assert lib._videos[3] == (433, 297, 8) and lib._rows.holes == []
    assert lib.launched[1] == ("index", (147, 256), [(583, 0, 147)])
    lib = R.stub_library(730, FRAGMENTED)
    with pytest.raises(ValueError, match="extend: the 148 rows behind video 3 are not free"):
        lib.extend(3, _feats(148), compact=True)
    assert lib.launched == []
    # compact=True where a hole fits anyway: nothing is compacted
    lib = R.stub_library(730, FRAGMENTED)
    lib.extend(1, _feats(60), compact=True)
    assert [k for k, *_ in lib.launched] == ["index"]


def test_extend_refuses_before_any_gpu_work():
    lib = _forbid_live_check(R.stub_library(730, FRAGMENTED))
    before = R.state(lib)
    with pytest.raises(ValueError, match="unknown or removed video id 9"):
        lib.extend(9, _feats(5))
    with pytest.raises(ValueError, match=r"extend: video_feats must be \(clips >= 1, dim\), got \(0, 256\)"):
        lib.extend(1, _feats(0))
    with pytest.raises(ValueError, match="extend: video_feats must be"):
        lib.extend(1, torch.zeros(256))
    with pytest.raises(ValueError, match="appearance clip features: feature dim 128, the model was built for 256"):
        lib.extend(1, _feats(5, 128))
    assert R.state(lib) == before and lib.launched == []
    closed = R.stub_library(730, FRAGMENTED)
    closed._open = False
    with pytest.raises(RuntimeError, match="closed"):
        closed.extend(1, _feats(5))
    assert R.state(closed) == before and closed.launched == []


# ------------------------------------------------------------------------------------------------ trim
def test_trim_frees_the_front_rows_and_launches_nothing():
    lib = R.stub_library(730, FRAGMENTED)
    assert lib.trim(2, 0) == 333 and lib._scan_cache == "stale" and lib._videos[2] == (160, 333, 9)      # a no-op
    assert lib.trim(2, 45) == 288
    assert lib._videos[2] == (205, 288, 8) and lib._rows.holes == [(100, 105), (493, 50), (693, 37)]     # coalesced with the hole in front
    assert lib._scan_cache is None and lib.launched == []
    assert lib.trim(2, 287) == 1 and lib._videos[2] == (492, 1, 2) and lib._rows.holes == [(100, 392), (493, 50), (693, 37)]
    before = R.state(lib)
    for bad, want in ((1, r"trim: n_front=1 not in \[0, 1\) for video 2"), (-1, "trim: n_front=-1 not in"),
                      (1.0, "trim: n_front must be an integer")):
        with pytest.raises(ValueError, match=want):
            lib.trim(2, bad)
    with pytest.raises(ValueError, match=r"trim: n_front=150 not in \[0, 150\) for video 3 \(remove drops a whole video\)"):
        lib.trim(3, 150)
    with pytest.raises(ValueError, match="unknown or removed video id 7"):
        lib.trim(7, 1)
    assert R.state(lib) == before and lib.launched == []
    lib.remove(2)
    assert lib._rows.holes == [(100, 443), (693, 37)]


def test_extend_and_trim_slide_a_window_along_the_arena():
    """A live recording: 8 clips in, 8 clips out.  It walks up the arena in place; at the end of the arena the 40 free rows lie
    in front of it and cannot hold it, so ``compact=True`` slides it back to row 0 and it grows in place again."""
    lib = R.stub_library(130, [(0, 90)])
    where = []
    for _ in range(7):
        lib.extend(1, _feats(8), compact=True)
        lib.trim(1, 8)
        where.append(lib._videos[1][:2])
        assert lib._videos[1][1] == 90 and lib._rows.free == 40
    assert where == [(8, 90), (16, 90), (24, 90), (32, 90), (40, 90), (8, 90), (16, 90)]
    kinds = [k for k, *_ in lib.launched]
    assert kinds.count("compact") == 1 and kinds.count("move") == 0 and kinds.count("index") == 7
    # with room for two copies the video relocates to the front instead
    lib = R.stub_library(200, [(110, 90)])
    lib.extend(1, _feats(8))
    assert lib._videos[1][:2] == (0, 98) and lib.launched[0] == ("move", [(110, 0, 90)], [(0, 90, False)])


# ------------------------------------------------------------------------------------------------ the thresholds the GPU pins use
def test_the_pinned_row_counts_follow_the_gemm_constants():
    c = R.gemm_constants()
    assert c == dict(RSP_MAX_GROUPS=64, RSP_MAX_TILES=1024, RS_MAX_WGS=1280, TALL_MIN_ROWS=262144)
    assert R.threshold_rows(c) == dict(spread_768=336, spread_256=1024, small_768=6816, small_256=20480)
    assert R.pin_row_counts(c) == [1, 15, 16, 17, 127, 128, 129, 336, 337, 1024, 1025, 6816, 6817, 20480, 20481]
    assert R.reduced_row_counts(c) == [1, 17, 337, 1025, 6817]
