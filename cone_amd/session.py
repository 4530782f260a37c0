"""Video sessions: index one video once, answer query batches on it (``CONELocalizator.open_video``).

``CONELocalizator.predict_moment`` (run_on_video/cone_localizator.py:121-221) redoes on every call what depends on the video
alone: the clips' L2 norm, the adapter, ``input_vid_proj`` and the first encoder layer's q | k | v row of every clip.  A
``VideoSession`` does that half once and keeps it resident; a query then runs only the launches of ``_enqueue`` that read the
query.  Nothing new is computed: a session re-sequences the launchers ``_enqueue`` calls, with the same arguments, and every
result equals ``predict_moment``'s on the same video and query with ``==``.

Two steps, the same launchers in the same order:

* ``step="python"`` -- one ctypes call per launcher, index metadata cached per tuple of token lengths (the yardstick);
* ``step="c"`` -- ``cone_session_index`` / ``cone_session_localize`` (csrc/session.hip): the whole query half is ONE C call on
  one caller-owned workspace, the index metadata written on the device by ``cone_session_query_layout``.

A batch of queries shares every launch: stage A runs the streaming pre-filter in launches of at most 4 queries (the form whose
bits do not depend on the launch; ``prefilter_scores`` would switch to the matrix cores from 5 queries on), or the certified
index; then one window table, ONE ``forward_packed`` over all Q * K windows, one matching call, one ``compose_rows``, one
``fuse_nms`` with a row per query, one read-back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops

MAX_QUERIES = _lib.SESSION_MAX_QUERIES      # queries of one cone_session_localize call; the wrapper splits longer lists
NMS_THD, MAX_BEFORE, MAX_AFTER = 0.5, 100, 5      # run_on_video/cone_localizator.py:200-219


def check_queries(tok_len, max_q_l: int):
    """The refusals of ``predict_moment``: every query has 1 .. max_q_l tokens."""
    for n in tok_len:
        if n > max_q_l:
            raise ValueError(f"query has {n} tokens > max_q_l={max_q_l}")
        if n < 1:
            raise ValueError(f"query has {n} tokens: a query needs at least one")


def query_layout(tok_len, max_q_l: int, ctx_l: int, K: int, num_queries: int, max_v_l: int):
    """The index metadata of one call, on the host (int32 arrays; what ``cone_session_query_layout`` writes on the device):
    ``tok_off`` (nq + 1) / ``tok_len`` (nq) of the concatenated token rows, ``tok_idx`` = index of every token inside ITS
    query (restarts at 0: ``text_positions``), ``q_ctx_l`` / ``q_vid_off``, and ``batch_pad`` (nq) / ``full_w`` (nq * K) =
    max_v_l (every window counts as padded to max_v_l), ``n_valid`` (nq) = K * num_queries."""
    tok_len = [int(n) for n in tok_len]
    check_queries(tok_len, max_q_l)
    nq = len(tok_len)
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    off = [0]
    for n in tok_len:
        off.append(off[-1] + n)
    return dict(tok_off=i32(off), tok_len=i32(tok_len), tok_idx=i32([j for n in tok_len for j in range(n)]),
                q_ctx_l=i32([ctx_l] * nq), q_vid_off=i32([0] * nq), batch_pad=i32([max_v_l] * nq),
                full_w=i32([max_v_l] * (nq * K)), n_valid=i32([K * num_queries] * nq))


LAYOUT_NAMES = ("tok_off", "tok_len", "tok_idx", "q_ctx_l", "q_vid_off", "batch_pad", "full_w", "n_valid")


def _kept_bytes(nq: int):
    """Bytes of the kept rows (3, nq, MAX_AFTER, 5) fp64 and of the counts (3, nq) int32, back to back as ``ops.fuse_nms``
    lays them out."""
    return 3 * nq * MAX_AFTER * 5 * 8, 3 * nq * 4


def _pack_queries(queries, dev):
    """``[(text_token_feats, text_cls_feat), ...]`` -> what one call takes of them, on the device: the token rows back to back
    (sum of the lengths, t_dim) fp32, ``cls`` (n, v_dim) fp32, and the token lengths."""
    toks = [t.to(dev, torch.float32).contiguous() for t, _ in queries]
    tok_cat = toks[0] if len(toks) == 1 else torch.cat(toks)
    cls = torch.stack([c.to(dev, torch.float32).reshape(-1) for _, c in queries]).contiguous()
    return tok_cat, cls, [int(t.shape[0]) for t in toks]


# what ``open_video`` and ``open_library`` answer to certified=True on a prefilter_bf16 localizer
CERTIFIED_WITH_BF16 = ("open_video: certified=True and prefilter_bf16=True exclude each other -- the certified index "
                       "returns the exact-fp32 ranking, the bf16 pre-filter ranks on bf16 rows")


class VideoSession:
    """One resident video of a ``CONELocalizator`` (``open_video``).  ``predict_moment`` / ``predict_moments`` return what the
    localizer's ``predict_moment`` returns for the same video, ``==``."""

    def __init__(self, localizer, video_feats, certified: bool = False, n_cand=None, step: str = "python"):
        if certified and localizer.prefilter_bf16:
            raise ValueError(CERTIFIED_WITH_BF16)
        if step not in ("python", "c"):
            raise ValueError(f"open_video: step must be 'python' or 'c', got {step!r}")
        from .model import Workspace
        self._loc = localizer
        a, m = localizer.args, localizer.localizator
        self.step, self.certified, self.n_cand = step, bool(certified), int(n_cand or 0)
        self.max_q_l = int(a.max_q_l)
        self._handle_obj, self._handle_value = m._handle, m._h().value    # the handle this video is indexed with
        vid = video_feats.to(localizer.device, torch.float32).contiguous()
        if vid.dim() != 2 or vid.shape[0] < 1:
            raise ValueError(f"open_video: video_feats must be (clips >= 1, dim), got {tuple(vid.shape)}")
        m._check_dim(vid, a.v_appear_feat_dim, "appearance clip features")
        m._check_dim(vid, a.v_motion_feat_dim, "motion clip features")
        self.ctx_l = int(vid.shape[0])
        self.K = min(int(a.topk_window), ops.num_windows(self.ctx_l, a.max_v_l))
        self._ws = Workspace()          # the C step's per-call workspace (grow-only)
        self._consts = {}
        self.last_certified = None
        self.index = self._arena = self._cs = None
        if step == "c":
            self._open_c(vid)
        else:
            self.vid = ops.l2_normalize(vid, 1e-5, clamp=True)                                      # :129
            self.adapted = m.adapter_norm(self.vid, renorm=False,                                   # :135-138
                                          out_dtype=torch.bfloat16 if localizer.prefilter_bf16 else torch.float32)
            if certified:
                self.index = ops.PrefilterIndex(self.adapted)       # (keeps the fp32 rows themselves: no copy)
            self.vproj = m.project(0, self.vid)
            self.qkv_vid = None if m.long_windows else m.layer0_rows(self.vproj)
        self._open = True

    def _open_c(self, vid):
        lib, m = _lib.load(), self._loc.localizator
        h = m._h()
        flags = (_lib.SESSION_BF16 if self._loc.prefilter_bf16 else 0) | (_lib.SESSION_CERTIFIED if self.certified else 0)
        n_arena, n_ws = lib.cone_session_arena_bytes(h, self.ctx_l, flags), lib.cone_session_workspace(h, self.ctx_l, flags)
        self._arena = torch.empty(max(n_arena, 1), dtype=torch.uint8, device=vid.device)
        ws = torch.empty(max(n_ws, 1), dtype=torch.uint8, device=vid.device)
        self._cs = _lib.Session()
        _lib.check(lib.cone_session_index(h, _lib.ptr(vid), self.ctx_l, flags, _lib.ptr(self._arena), n_arena, _lib.ptr(ws),
                                          n_ws, C.byref(self._cs), _lib.stream()))
        a = self._loc.args
        self._params = _lib.SessionParams(int(a.max_v_l), int(a.max_q_l), float(a.clip_length), NMS_THD, MAX_BEFORE, MAX_AFTER)

    # ---- lifetime ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        """Bytes that stay resident for this video."""
        if not self._open:
            return 0
        if self._arena is not None:
            return int(self._arena.numel())
        ts = [self.vid, self.adapted, self.vproj, self.qkv_vid]
        if self.index is not None:
            ts += [self.index.vid16, self.index.err]
        return int(sum(t.numel() * t.element_size() for t in ts if t is not None))

    def close(self):
        self._open = False
        self.vid = self.adapted = self.vproj = self.qkv_vid = self.index = self._arena = self._cs = None
        self._consts = {}
        self._ws = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_live(self):
        if not self._open:
            raise RuntimeError("VideoSession: the session is closed")
        m = self._loc.localizator
        if m._handle is not self._handle_obj or m._handle is None or m._handle.value != self._handle_value:
            raise RuntimeError("VideoSession: load_state_dict replaced the model handle this video was indexed with; the "
                               "resident rows belong to the old weights -- open a new session")

    # ---- the query half ------------------------------------------------------------------------
    def _layout(self, lens):
        """Device copies of ``query_layout`` for one tuple of token lengths, uploaded once (the Python step uploads nothing
        per call: a pageable H2D copy waits for the stream to drain)."""
        c = self._consts.get(lens)
        if c is None:
            if len(self._consts) > 64:
                self._consts.clear()
            a = self._loc.args
            host = query_layout(lens, self.max_q_l, self.ctx_l, self.K, self._loc.localizator.num_queries, a.max_v_l)
            c = self._consts[lens] = {k: torch.from_numpy(v).to(self._loc.device) for k, v in host.items()}
        return c

    def _window_scores(self, cls):
        """Window scores (nq, num_window) in the streaming form's bits whatever nq is: launches of at most 4 queries."""
        W = self._loc.args.max_v_l
        parts = [ops.prefilter_scores(self.adapted, cls[g:g + 4], W, frame_scores=False)[1] for g in range(0, cls.shape[0], 4)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    @torch.no_grad()
    def _enqueue_python(self, tok_cat, lens, cls):
        a, m = self._loc.args, self._loc.localizator
        nq, K, W = len(lens), self.K, a.max_v_l
        c = self._layout(lens)
        tok = ops.l2_normalize(tok_cat, 1e-5, clamp=True)                                              # :133
        if self.index is not None:
            widx, _, self.last_certified = self.index.topk(cls, W, K, self.n_cand or None)
        else:
            widx, _ = ops.topk_windows(self._window_scores(cls), K)                                    # :83-100
        wt = ops.window_table_rows(widx, c["q_ctx_l"], c["q_vid_off"], c["tok_off"], c["tok_len"], 0, 1, W,
                                   batch_pad=c["batch_pad"], n_batches=nq)
        tproj = m.project(1, tok)
        l0 = None
        if self.qkv_vid is not None and not m.long_windows:
            l0 = dict(qkv_vid=self.qkv_vid, qkv_txt=m.layer0_rows(tproj), max_v_l=W)
            if m.txt_pos_tables:
                l0["txt_pos"], l0["txt_pos_qk"] = m.text_positions(tproj, c["tok_idx"])
        out = m.forward_packed(self.vproj, wt["vid_row0"], wt["vid_len"], tproj, wt["txt_row0"], wt["txt_len"], W, a.max_q_l,
                               l0=l0, saliency=False)
        match = m.clip_matching_gathered(cls, wt["cls_row"], self.vid, wt["vid_row0"], wt["vid_len"], wt["pad_len"],
                                         out["pred_spans"])
        rows = ops.compose_rows(out["pred_logits"], out["pred_spans"], match, c["full_w"], wt["video_start"], a.clip_length,
                                sort=False)                                                            # :191
        kept, _, _ = ops.fuse_nms(rows.reshape(nq, K * m.num_queries, 4), c["n_valid"], NMS_THD, MAX_BEFORE, MAX_AFTER)
        return kept.kept_buf

    @torch.no_grad()
    def _enqueue_c(self, tok_cat, lens, cls):
        lib, m = _lib.load(), self._loc.localizator
        h, nq, dev = m._h(), len(lens), tok_cat.device
        arr = (C.c_int32 * nq)(*lens)
        ws = self._ws.get(_lib.sized(lib.cone_session_localize_workspace(h, C.byref(self._cs), arr, nq, self.K, self.n_cand,
                                                                         C.byref(self._params))), dev)
        R, N = _kept_bytes(nq)
        buf = torch.empty(R + N, dtype=torch.uint8, device=dev)
        cert = torch.empty(nq, dtype=torch.int32, device=dev) if self.certified else None
        _lib.check(lib.cone_session_localize(h, C.byref(self._cs), _lib.ptr(tok_cat, torch.float32), arr, nq,
                                             _lib.ptr(cls, torch.float32), self.K, self.n_cand, C.byref(self._params),
                                             C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + R), _lib.ptr(cert),
                                             _lib.ptr(ws), ws.numel(), _lib.stream()))
        if cert is not None:
            self.last_certified = cert
        return buf

    def enqueue(self, tok_cat, lens, cls):
        """The device half of one call, no host round trip: ``tok_cat`` (sum(lens), t_dim) fp32 = the queries' raw token rows
        back to back, ``cls`` (len(lens), v_dim) fp32, both on the device; at most ``MAX_QUERIES`` queries.  Returns the kept
        rows (3, nq, 5, 5) fp64 and their counts (3, nq) int32 as one byte buffer (``ops.fuse_nms``'s layout).  On one stream:
        with ``step="c"`` it can be captured in a graph once a call of the same lengths has sized the workspace."""
        self._check_live()
        lens = tuple(int(n) for n in lens)
        check_queries(lens, self.max_q_l)
        if not 1 <= len(lens) <= MAX_QUERIES:
            raise ValueError(f"enqueue takes 1 .. {MAX_QUERIES} queries, got {len(lens)}")
        return (self._enqueue_c if self.step == "c" else self._enqueue_python)(tok_cat, lens, cls)

    @staticmethod
    def read_kept(buf_host, nq: int):
        """The moments of ``enqueue``'s buffer (on the host) as ``predict_moment`` returns them, a list per query."""
        R, N = _kept_bytes(nq)
        rows = buf_host[:R].view(torch.float64).view(3, nq, MAX_AFTER, 5)[0].tolist()
        n = buf_host[R:R + N].view(torch.int32).view(3, nq)[0].tolist()
        return [[[r[0], r[1], r[4]] for r in rows[q][:n[q]]] for q in range(nq)]

    @staticmethod
    def _read_calls(bufs, sizes):
        """The moments of the calls ``bufs`` (``enqueue``'s buffers on the device, ``sizes[i]`` queries each) after ONE
        read-back, in the calls' order."""
        host = (bufs[0] if len(bufs) == 1 else torch.cat(bufs)).cpu()
        out, at = [], 0
        for nq in sizes:
            n = sum(_kept_bytes(nq))
            out += VideoSession.read_kept(host[at:at + n].clone() if at else host, nq)      # (a view of another dtype starts aligned)
            at += n
        return out

    @torch.no_grad()
    def predict_moments(self, queries):
        """``[(text_token_feats, text_cls_feat), ...]`` -> a list of moment lists, each ``==`` the localizer's
        ``predict_moment(video_feats, query)``.  One enqueue and one read-back for any number of queries of ragged lengths
        (``cone_session_localize`` takes ``MAX_QUERIES`` a call: longer lists are split here, in either step, still one
        read-back)."""
        queries = list(queries)
        check_queries([int(t.shape[0]) for t, _ in queries], self.max_q_l)      # refused before anything else, as today
        if not queries:
            return []
        self._check_live()
        bufs, counts = [], []
        for g in range(0, len(queries), MAX_QUERIES):
            tok_cat, cls, lens = _pack_queries(queries[g:g + MAX_QUERIES], self._loc.device)
            bufs.append(self.enqueue(tok_cat, lens, cls))
            counts.append(len(lens))
        return self._read_calls(bufs, counts)                                 # the call's one read-back

    def predict_moment(self, text_feats):
        """``localizer.predict_moment(video_feats, text_feats)`` for the resident video."""
        return self.predict_moments([text_feats])[0]
