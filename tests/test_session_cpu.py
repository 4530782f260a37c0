"""Video sessions, the part that needs no GPU: the C ABI's declarations and binding, the host model of a call's index
metadata, and the refusals that fire before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import session_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cone_hip.h")) as f:
        return f.read()


def test_header_declares_the_session_entries_and_stays_abi_8():
    from cone_amd import _lib
    hdr = _header()
    assert re.search(r"#define\s+CONE_HIP_ABI_VERSION\s+8\b", hdr)
    declared = set(re.findall(r"\b(cone_[a-z0-9_]+)\s*\(", hdr))
    for name in R.NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS, name
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    # every entry cites the reference site it replaces and states the contract
    section = hdr[hdr.index("video sessions (additive in ABI 8)"):hdr.index("metrics on the device")]
    assert section.count("run_on_video/cone_localizator.py:121-221") >= 3
    assert "the bits" in section and "predict_moment" in section
    assert "typedef struct" in section and "} cone_session;" in section


def test_binding_mirrors_the_declared_structs_and_signatures():
    from cone_amd import _lib
    hdr = _header()
    assert len(_lib._SIGNATURES["cone_session_localize"][1]) == 15
    assert len(_lib._SIGNATURES["cone_session_query_layout"][1]) == 16
    assert len(_lib._SIGNATURES["cone_session_index"][1]) == 10
    for name in ("cone_session_arena_bytes", "cone_session_workspace", "cone_session_localize_workspace"):
        assert _lib._SIGNATURES[name][0] is ctypes.c_size_t
    # field order of the host structs as the header declares them
    body = re.search(r"typedef struct \{([^}]*)\} cone_session;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in _lib.Session._fields_]
    assert [n for n, _ in _lib.SessionParams._fields_] == ["max_v_l", "max_q_l", "clip_length", "nms_thd", "max_before", "max_after"]
    assert (int(re.search(r"#define\s+CONE_SESSION_MAX_QUERIES\s+(\d+)", hdr).group(1)) == _lib.SESSION_MAX_QUERIES == 64)
    assert ctypes.sizeof(_lib.Session) == 80 and ctypes.sizeof(_lib.SessionParams) == 32 and ctypes.sizeof(_lib.ModelDims) == 32


def test_library_exports_the_session_entries():
    from cone_amd import _lib
    lib = _lib.load()
    for name in R.NEW_SYMBOLS:
        assert hasattr(lib, name), name
    # the layout entry refuses by name on the host, before it looks at an output pointer or launches anything
    def refused(lens, nq=None):
        arr = (ctypes.c_int32 * max(len(lens), 1))(*lens)
        rc = lib.cone_session_query_layout(arr, len(lens) if nq is None else nq, 20, 900, 20, 5, 90, *([None] * 8), None)
        assert rc == -1
        return lib.cone_last_error().decode()
    assert "nq=0 not in [1, 64]" in refused([])
    assert "nq=65 not in [1, 64]" in refused([1] * 65)
    assert "tok_len[1]=0 not in [1, max_q_l=20]" in refused([5, 0])
    assert "tok_len[2]=21 not in [1, max_q_l=20]" in refused([5, 20, 21])


@pytest.mark.parametrize("case", range(len(R.LAYOUT_CASES)))
def test_host_query_layout_matches_the_numpy_model(case):
    from cone_amd import session
    lens, ctx_l, K = R.LAYOUT_CASES[case]
    got = session.query_layout(lens, R.MAX_Q_L, ctx_l, K, R.NUM_QUERIES, R.MAX_V_L)
    want = R.layout_model(lens, ctx_l, K)
    assert tuple(got) == R.OUTPUTS == session.LAYOUT_NAMES
    for k in R.OUTPUTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (k, lens)
    assert got["tok_off"][-1] == sum(lens) == len(got["tok_idx"])


def test_layout_cases_cover_what_the_issue_names():
    sums = {sum(c[0]) for c in R.LAYOUT_CASES}
    assert {255, 256, 257} <= sums
    assert {len(c[0]) for c in R.LAYOUT_CASES} >= {1, 2, 64}
    assert any(set(c[0]) == {1} for c in R.LAYOUT_CASES) and any(set(c[0]) == {20} for c in R.LAYOUT_CASES)


def test_host_layout_refuses_bad_lengths():
    from cone_amd import session
    with pytest.raises(ValueError, match="21 tokens > max_q_l=20"):
        session.query_layout([3, 21], 20, 900, 20, 5, 90)
    with pytest.raises(ValueError, match="0 tokens"):
        session.query_layout([0], 20, 900, 20, 5, 90)


def test_certified_with_prefilter_bf16_is_refused_before_any_gpu_work():
    from cone_amd.localizator import CONELocalizator
    loc = object.__new__(CONELocalizator)       # no handle, no GPU: the refusal comes first
    loc.prefilter_bf16 = True
    with pytest.raises(ValueError) as e:
        loc.open_video(torch.zeros(100, 256), certified=True)
    assert "certified" in str(e.value) and "prefilter_bf16" in str(e.value)
    with pytest.raises(ValueError, match="step"):
        loc.prefilter_bf16 = False
        loc.open_video(torch.zeros(100, 256), step="graph")


def test_over_long_query_is_refused_as_predict_moment_refuses_it():
    from cone_amd.session import VideoSession
    s = object.__new__(VideoSession)
    s.max_q_l = 20
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        s.predict_moments([(torch.zeros(5, 768), torch.zeros(256)), (torch.zeros(21, 768), torch.zeros(256))])
    with pytest.raises(ValueError, match="query has 21 tokens > max_q_l=20"):
        s.predict_moment((torch.zeros(21, 768), torch.zeros(256)))
    assert s.predict_moments([]) == []
