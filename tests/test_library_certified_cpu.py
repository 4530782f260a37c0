"""Certified library budgets without a GPU: the header, the exports and the binding; every refusal from host values with null
pointers; ``certified_table`` against brute force; the bound on CPU fp32 scores; the prefix argument by brute force on the model
(tests/certified_library_refs.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import budget_refs as B
import certified_library_refs as R
import prefilter_certified_ref as PC
import prefilter_stage_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ header, exports, binding
def test_the_header_declares_the_entries_and_the_binding_mirrors_them():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    at = hdr.index("certified library budgets")
    assert hdr.index("standing queries over a library") < at < hdr.index("metrics on the device")
    section = hdr[at:hdr.index("metrics on the device")]
    for name in R.NEW_SYMBOLS:
        assert name + "(" in section
    assert section.count("cone/inference.py:276-299") >= 3 and section.count("run_on_video/cone_localizator.py:83-100") >= 2
    for word in ("CONTRACT", "bit for bit", "EVERY element written", "library_shadow: ", "library_scan_certified: ", "strictly",
                 "nothing allocated", "no host read-back", "} cone_library_shadow;"):
        assert word in section, word
    for name, n in R.N_ARGS.items():
        assert len(_lib._SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == n, name
    body = re.search(r"typedef struct \{([^}]*)\} cone_library_shadow;", hdr).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.LibraryShadow._fields_]


# ------------------------------------------------------------------------------------------------ refusals, host values only
def _handle(capacity=1000, flags=0, v_dim=256):
    from cone_amd import _lib
    return _lib.Library(FAKE, capacity, flags, v_dim, 256, None, None, None, None, None)


def _err():
    from cone_amd import _lib
    return _lib.load().cone_last_error().decode()


@pytest.mark.parametrize("kw,word", [(dict(flags=1), "flags=1"), (dict(flags=2), "flags=2"), (dict(capacity=0), "capacity=0"),
                                     (dict(capacity=1 << 31), "capacity="), (dict(v_dim=128), "feature dim 128"),
                                     (dict(v_dim=1280), "feature dim 1280")])
def test_the_shadow_refuses_by_name_before_any_pointer(kw, word):
    from cone_amd import _lib
    lib, h = _lib.load(), _handle(**kw)
    assert lib.cone_library_shadow_bytes(C.byref(h)) == 0 and _err().startswith("library_shadow: ") and word in _err()
    assert lib.cone_library_shadow_open(C.byref(h), None, 0, None) != 0 and word in _err()
    assert lib.cone_library_shadow_index(None, C.byref(h), None, 0, 1, None) != 0 and word in _err()


def test_the_shadow_layout_and_its_argument_refusals():
    from cone_amd import _lib
    lib, h, sh = _lib.load(), _handle(capacity=1001, v_dim=768), _lib.LibraryShadow()
    n = lib.cone_library_shadow_bytes(C.byref(h))
    rows = -(-1001 * 768 * 2 // 256) * 256
    assert n == rows + -(-1001 * 8 // 256) * 256
    assert lib.cone_library_shadow_bytes(None) == 0 and "null argument" in _err()
    assert lib.cone_library_shadow_open(C.byref(h), None, n, C.byref(sh)) != 0 and "null argument" in _err()
    assert lib.cone_library_shadow_open(C.byref(h), C.c_void_p(0x10080), n, C.byref(sh)) != 0 and "256-B aligned" in _err()
    assert lib.cone_library_shadow_open(C.byref(h), C.c_void_p(0x10000), n - 1, C.byref(sh)) != 0 and "arena too small" in _err()
    assert lib.cone_library_shadow_open(C.byref(h), C.c_void_p(0x10000), n, C.byref(sh)) == 0          # layout only: nothing is touched
    assert (sh.model, sh.capacity, sh.v_dim, sh.rows_bf16, sh.err) == (FAKE, 1001, 768, 0x10000, 0x10000 + rows)
    for row0, n_rows in ((-1, 1), (0, 0), (1001, 1), (1000, 2), (0, 1002)):
        assert lib.cone_library_shadow_index(None, C.byref(h), None, row0, n_rows, None) != 0 and "leave the arena" in _err()
    assert lib.cone_library_shadow_index(None, C.byref(h), C.byref(sh), 0, 1, None) != 0 and "null argument" in _err()
    assert lib.cone_library_shadow_index(C.c_void_p(0x2000), C.byref(h), C.byref(sh), 0, 1, None) != 0 and "another handle" in _err()
    for other in (_lib.LibraryShadow(0x2000, 1001, 768, 1, 1), _lib.LibraryShadow(FAKE, 1000, 768, 1, 1),
                  _lib.LibraryShadow(FAKE, 1001, 256, 1, 1), _lib.LibraryShadow(FAKE, 1001, 768, None, 1)):
        assert lib.cone_library_shadow_index(C.c_void_p(FAKE), C.byref(h), C.byref(other), 0, 1, None) != 0
        assert "the shadow belongs to another library" in _err()


GOOD = dict(n_videos=10, total_hb=50, total_win=60, nq=4, K=20, W=20, n_cand=0, max_v_l=90)


@pytest.mark.parametrize("kw,word", [
    (dict(nq=0), "nq=0"), (dict(nq=65), "nq=65"), (dict(n_videos=0), "n_videos=0"), (dict(total_hb=9, total_win=19), "total_hb=9"),
    (dict(total_hb=1001, total_win=1011), "total_hb=1001"), (dict(K=0), "K=0"), (dict(K=257), "K=257"), (dict(max_v_l=1), "max_v_l=1"),
    (dict(flags=2), "CONE_SESSION_CERTIFIED"), (dict(flags=1), "CONE_SESSION_BF16"), (dict(W=0), "W=0"), (dict(W=257), "W=257"),
    (dict(total_win=59), "total_win=59"), (dict(total_win=61), "total_win=61"), (dict(n_cand=19), "n_cand=19"),
    (dict(n_cand=61), "n_cand=61"), (dict(n_cand=-1), "n_cand=-1"),
    (dict(n_videos=100, total_hb=900, total_win=1000, W=256, n_cand=255), "n_cand=255"),
    (dict(capacity=10000, n_videos=100, total_hb=9000, total_win=9100, n_cand=4097), "n_cand=4097")])
def test_the_certified_scan_refuses_from_host_values_with_null_pointers(kw, word):
    from cone_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **{k: v for k, v in kw.items() if k in GOOD})
    h = _handle(capacity=kw.get("capacity", 1000), flags=kw.get("flags", 0))
    p = _lib.SessionParams(a["max_v_l"], 20, 0.5333, 0.5, 100, 5)
    rc = lib.cone_library_scan_certified(None, C.byref(h), None, None, None, None, None, a["n_videos"], a["total_hb"], a["total_win"],
                                         None, a["nq"], a["K"], a["W"], a["n_cand"], C.byref(p), None, None, None, None, 0, None)
    assert rc != 0 and _err().startswith("library_scan_certified: ") and word in _err(), _err()
    if "max_v_l" not in kw:
        assert lib.cone_library_scan_certified_workspace(C.byref(h), a["n_videos"], a["total_hb"], a["total_win"], a["nq"], a["K"],
                                                         a["W"], a["n_cand"]) == 0 and word in _err()


def test_good_host_values_pass_on_to_the_pointer_checks():
    from cone_amd import _lib
    lib, h = _lib.load(), _handle()
    p = _lib.SessionParams(90, 20, 0.5333, 0.5, 100, 5)
    a = GOOD
    args = (a["n_videos"], a["total_hb"], a["total_win"])
    tail = (a["nq"], a["K"], a["W"], a["n_cand"], C.byref(p), None, None, None, None, 0, None)
    assert lib.cone_library_scan_certified(None, C.byref(h), None, None, None, None, None, *args, None, *tail) != 0
    assert _err() == "library_scan_certified: null argument"
    n = lib.cone_library_scan_certified_workspace(C.byref(h), *args, a["nq"], a["K"], a["W"], a["n_cand"])
    assert n > 0 and n % 256 == 0
    # the planes, the window row and the default candidate count's lists all fit
    assert n >= 4 * (2 * 4 * 50 + 4 * 60) + 5 * 4 * 4 * 60
    for n_cand in (20, 60):
        assert lib.cone_library_scan_certified_workspace(C.byref(h), *args, a["nq"], a["K"], a["W"], n_cand) > 0, _err()


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("max_v_l", [4, 5, 90, 125])
def test_certified_table_against_brute_force(max_v_l):
    from cone_amd.library import certified_table, scan_table
    S = max_v_l // 2
    lengths = [1, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 7 * S + 3]
    lengths = [n for n in lengths if n >= 1]
    videos, _ = R.stacked(lengths, gaps=[(3 * i) % 5 for i in range(len(lengths))])
    videos = videos[::-1]                                          # any order in, slots by row0 out
    order, row0, ctx, hb_off, win_off = certified_table(videos, S, max_v_l)
    want = R.table_brute(videos, max_v_l)
    assert list(order) == want[0] and row0.tolist() == want[1] and ctx.tolist() == want[2]
    assert hb_off.tolist() == want[3] and win_off.tolist() == want[4]
    assert win_off.dtype == np.int64 and int(win_off[-1]) == int(hb_off[-1]) + len(videos)
    from cone_amd import _lib
    lib = _lib.load()
    assert np.diff(win_off).tolist() == [lib.cone_num_windows(int(n), max_v_l) for n in ctx]
    plain = scan_table(videos, S)                                   # scan_table's arrays, unchanged
    assert list(plain[0]) == list(order) and all(np.array_equal(a, b) for a, b in zip(plain[1:], (row0, ctx, hb_off)))
    with pytest.raises(ValueError, match="certified_table: S="):
        certified_table(videos, S + 1, max_v_l)


# ------------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("kind", ["unit", "midpoints", "subnormal"])
@pytest.mark.parametrize("dv", [256, 768])
def test_the_bound_holds_on_cpu_fp32_scores_with_the_per_row_measures(kind, dv):
    """|coarse - exact| <= E for every frame, hence for every window: coarse = fp32 sums of bf16 x bf16 products, exact = fp32
    sums of the fp32 rows (torch's CPU kernels: some summation order -- the bound holds in any), R and N the maxima of the model's
    per-row measures."""
    rows = P.index_rows(300, dv, kind, seed=dv)
    g = torch.Generator().manual_seed(5 + dv)
    cls = torch.randn(9, dv, generator=g)
    cls = cls / cls.norm(dim=1, keepdim=True)
    if kind == "subnormal":
        cls[0] = 0.0
        cls[0, 3] = 1.0
    err = R.row_measures(rows)
    Rm, Nm = R.table_measures(err, [(0, 300)])
    assert Rm >= PC.index_norms(rows)[0] and Nm >= PC.index_norms(rows)[1]
    exact = cls @ rows.t()
    coarse = cls.bfloat16().float() @ rows.bfloat16().float().t()
    for q in range(cls.shape[0]):
        E = PC.device_bound(cls[q], Rm, Nm, dv)
        gap = float((coarse[q].double() - exact[q].double()).abs().max())
        assert gap <= E, (kind, q, gap, E)
    if kind == "midpoints":                                         # the rounding error is as large as it gets: the bound is not idle
        assert float((coarse.double() - exact.double()).abs().max()) > 1e-3 * PC.device_bound(cls[1], Rm, Nm, dv)


# ------------------------------------------------------------------------------------------------ the prefix argument
def _proved_case(seed, lengths, W, K, nq, Wb, n_cand, E):
    """Random exact window scores; coarse = exact + noise inside (-E, E) -- so the bound holds -- both as fp32."""
    rng = np.random.default_rng(seed)
    win_off = np.concatenate([[0], np.cumsum([R.num_windows(n, W) for n in lengths])])
    total = int(win_off[-1])
    exact = rng.choice(np.arange(-4000, 4000), size=(nq, total)).astype(np.float32) / 16     # ties occur
    coarse = (exact + rng.uniform(-0.99 * E, 0.99 * E, size=exact.shape)).astype(np.float32)
    return win_off, coarse, exact


PROVED_SHAPES = ((1, 1, 3, 0.25), (3, 20, 8, 0.25), (20, 20, 0, 0.25), (20, 20, 22, 1.5), (20, 1, 0, 0.25), (20, 3, 0, 0.25), (60, 3, 0, 0.25),
                 (256, 20, 400, 0.25), (256, 1, 300, 0.25), (256, 1, 200, 0.25))           # (W, K, n_cand, E)


def test_budget_on_the_emitted_lists_equals_budget_on_the_full_lists_where_the_proof_holds():
    """For every query the model certifies, ``budget_ref`` on the emitted lists == ``budget_ref`` on the scan's full lists, and the
    chosen slots' prefixes are the scan's.  W > K with the cap binding is among the shapes -- (20, 1), (20, 3) and (60, 3): a slot gives at
    most K, so the walk goes far down the candidates --; both outcomes occur, and every shape but the last certifies somewhere
    ((256, 1): 30 slots cannot give 256 windows -- certified with all 243 windows as candidates, never with 200 of them)."""
    W = 4
    lengths = [1, 2, 3, 5, 40, 37, 30, 2, 2, 15] * 3
    outcomes = {}
    for Wb, K, n_cand, E in PROVED_SHAPES:
        seen = outcomes.setdefault((Wb, K, n_cand), set())
        for seed in range(4):
            win_off, coarse, exact = _proved_case(seed, lengths, W, K, 8, Wb, n_cand, E)
            widx, wval, flags, margin = R.certified_model(coarse, exact, win_off, K, Wb, n_cand, E)
            full = R.full_lists(exact, win_off, K)
            want = B.budget_ref(full[1], Wb)
            got = B.budget_ref(wval, Wb)
            for q in range(len(flags)):
                seen.add(int(flags[q]))
                if flags[q]:
                    for a, b in zip(got, want):
                        assert np.array_equal(a[q].view(np.int32), b[q].view(np.int32)), (Wb, K, n_cand, seed, q)
                    assert R.chosen_prefixes_equal(want[0], want[1], want[2], (widx, wval), full, q), (Wb, K, n_cand, seed, q)
                    if (Wb, K) == (20, 1):                                  # the cap binds: 20 windows from 20 slots, where the
                        assert int(want[0][q]) == 20                        # uncapped top 20 lie in fewer
                        top = np.argsort(-exact[q].astype(np.float64), kind="stable")[:20]
                        assert len(set(np.searchsorted(win_off, top, side="right"))) < 20
                lists = np.where(np.isfinite(wval[q]), wval[q], -1e30).astype(np.float64)
                assert (np.diff(lists, axis=1) <= 0).all()                  # well-formed either way: descending, padded
    assert all(1 in seen for key, seen in outcomes.items() if key != (256, 1, 200)), outcomes
    assert outcomes[(256, 1, 300)] == {1} and outcomes[(256, 1, 200)] == {0} and outcomes[(20, 20, 22)] == {0, 1}, outcomes


def test_the_cap_binds_and_an_exact_tie_across_slots_is_not_certified():
    """Two slots with the same scores, n_cand so small that the twin of the W-th window is no candidate: t == the twin's exact
    score, so the margin cannot exceed E > 0 ... and with every window a candidate the query certifies, the lower slot first."""
    W = 4
    win_off = np.asarray([0, 6, 12])
    exact = np.asarray([[9, 7, 5, 3, 2, 1, 9, 7, 5, 3, 2, 1]], dtype=np.float32)
    coarse = exact.copy()
    widx, wval, flags, margin = R.certified_model(coarse, exact, win_off, K=2, W=3, n_cand=3, E=0.5)
    assert flags.tolist() == [0]                                    # candidates 0, 6, 1: t = 7 = c_last
    widx, wval, flags, _ = R.certified_model(coarse, exact, win_off, K=2, W=3, n_cand=12, E=0.5)
    assert flags.tolist() == [1] and widx[0].tolist() == [[0, 1], [0, -1]] and wval[0, 1].tolist() == [9.0, float("-inf")]
    widx, wval, flags, _ = R.certified_model(coarse, exact, win_off, K=1, W=3, n_cand=12, E=0.5)     # the cap binds: W is not reached
    assert widx[0].tolist() == [[0], [0]] and flags.tolist() == [1]
    widx, wval, flags, margin = R.certified_model(coarse, exact, win_off, K=1, W=3, n_cand=11, E=0.5)
    assert flags.tolist() == [0] and np.isnan(margin[0])            # two taken, W = 3 asked, a window is no candidate: not proved


# ------------------------------------------------------------------------------------------------ the fallback's splice
def test_splice_budgets_replaces_exactly_the_rerun_chunks_words():
    from cone_amd.library import decode_budget, splice_budgets
    W, nqs = 3, [64, 64, 2]
    size = lambda nq: nq * (1 + 3 * W)
    host = []
    for c, nq in enumerate(nqs):
        host += [1] * nq + [100 * c + i for i in range(3 * nq * W)]                 # n_pairs = 1 everywhere, distinct words behind
    before = list(host)
    again = [[2] * nq + [-(100 * c + i) - 1 for i in range(3 * nq * W)] for c, nq in enumerate(nqs)]
    splice_budgets(host, nqs, W, [0, 2], again[0] + again[2])
    assert host[:size(64)] == again[0] and host[size(64):2 * size(64)] == before[size(64):2 * size(64)] and host[2 * size(64):] == again[2]
    at = 0
    for c, nq in enumerate(nqs):                                                    # the decoder walks the spliced words chunk by chunk
        pairs, at = decode_budget(host, at, nq, W)
        assert all(len(row) == (1 if c == 1 else 2) for row in pairs)
    assert at == len(host)
    with pytest.raises(ValueError, match="splice_budgets"):
        splice_budgets(host, nqs, W, [1], again[0] + again[2])


# ------------------------------------------------------------------------------------------------ planted errors
def test_every_planted_error_is_caught_by_a_named_case():
    """``catches()`` runs every dictated case on the model with one planted error at a time: the table of which case tells which
    error is computed, equals the declared one, and leaves no error uncaught.  The GPU file runs the same cases on the device."""
    got = R.catches()
    assert got == R.CATCHES, got
    assert set(got) == set(R.FAULTS) and all(got[f] for f in R.FAULTS)
    flags = {name: R.run_case(case)[2].tolist() for name, case in R.DICTATED.items()}
    assert flags == dict(threshold_eq=[0], threshold_above=[1], tie_at_5=[0], tie_at_6=[0], tie_at_7=[1], cap_all_candidates=[1],
                         cap_short=[0], cap_counts=[1], nan_measure=[0])
    assert R.unit_query_bound(2.0 ** -6, 0.0, 256) == R.E_EXACT          # the threshold cases' E, to the bit


def test_merge_ranges_joins_the_destinations_of_a_compaction():
    from cone_amd.library import compaction_moves, merge_ranges
    moves = compaction_moves([(5, 10), (40, 3), (100, 900), (2000, 1)])
    assert merge_ranges([(d, n) for s, d, n in moves if s != d]) == [(0, 914)]
    assert merge_ranges([(30, 5), (0, 10), (10, 2), (40, 1), (33, 4)]) == [(0, 12), (30, 7), (40, 1)]
    assert merge_ranges([]) == []
    with pytest.raises(ValueError, match="merge_ranges"):
        merge_ranges([(0, 0)])
