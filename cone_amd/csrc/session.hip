// Video sessions (include/cone_hip.h, "video sessions"): one resident video, indexed once, answering batches of queries.
//
// Nothing is computed here.  cone_session_index and cone_session_localize only SEQUENCE the library's own extern "C"
// launchers -- the calls cone_amd/localizator.py issues one by one through ctypes for run_on_video/cone_localizator.py:121-221
// -- and carve their operands out of the caller's arena / workspace.  The one kernel of this file writes a call's index
// metadata (what the localizer keeps per shape in _const) from lengths that travel as kernel arguments.
#include "common.h"

namespace cone {

#define RUN(x)            \
    do {                  \
        int _rc = (x);    \
        if (_rc) return _rc; \
    } while (0)

constexpr size_t SES_ALIGN = 256;

// A running offset over one caller-owned region: every take() is a region of its own, SES_ALIGN aligned, at least one
// aligned unit long (two takes never share an address, whatever their sizes).
struct Regions {
    size_t cur = 0;
    size_t take(size_t bytes) {
        const size_t at = cur;
        cur += align_up(bytes ? bytes : 1, SES_ALIGN);
        return at;
    }
};

static bool flags_ok(int flags) {
    return (flags & ~(CONE_SESSION_BF16 | CONE_SESSION_CERTIFIED)) == 0 &&
           (flags & (CONE_SESSION_BF16 | CONE_SESSION_CERTIFIED)) != (CONE_SESSION_BF16 | CONE_SESSION_CERTIFIED);
}

// ------------------------------------------------------------------------------ the video half
struct ArenaLayout {
    size_t vid_norm, adapted, adapted_bf16, err, vproj, qkv_vid, total;
    bool has_f32, has_bf16, has_err, has_qkv;
};
static ArenaLayout arena_layout(const cone_model_dims& d, int64_t n, int flags) {
    ArenaLayout L{};
    Regions r;
    L.has_f32 = !(flags & CONE_SESSION_BF16);
    L.has_bf16 = (flags & (CONE_SESSION_BF16 | CONE_SESSION_CERTIFIED)) != 0;
    L.has_err = (flags & CONE_SESSION_CERTIFIED) != 0;
    L.has_qkv = !d.long_windows;
    L.vid_norm = r.take((size_t)n * d.v_dim * 4);
    if (L.has_f32) L.adapted = r.take((size_t)n * d.v_dim * 4);
    if (L.has_bf16) L.adapted_bf16 = r.take((size_t)n * d.v_dim * 2);
    if (L.has_err) L.err = r.take(2 * sizeof(float));
    L.vproj = r.take((size_t)n * d.hidden_dim * 4);
    if (L.has_qkv) L.qkv_vid = r.take((size_t)n * 3 * d.hidden_dim * 4);
    L.total = r.cur;
    return L;
}
struct IndexWs { size_t adapter, adapter_bytes, proj, proj_bytes, l0, l0_bytes, total; };
static IndexWs index_ws(const cone_model* m, int64_t n) {
    IndexWs w{};
    Regions r;
    w.adapter_bytes = cone_adapter_norm_workspace(m, n); w.adapter = r.take(w.adapter_bytes);
    w.proj_bytes = cone_project_workspace(m, 0, n); w.proj = r.take(w.proj_bytes);
    w.l0_bytes = cone_layer0_project_workspace(m, n); w.l0 = r.take(w.l0_bytes);
    w.total = r.cur;
    return w;
}

// ------------------------------------------------------------------------------ the query half
struct QueryLens { int32_t len[CONE_SESSION_MAX_QUERIES]; };

// One workgroup.  Every output element has one writer; nothing outside the documented extents is touched:
// tok_off [0, nq], the per-query arrays [0, nq), full_w [0, nq K), tok_idx [0, sum of the lengths).
__global__ __launch_bounds__(256) void session_layout_kernel(QueryLens L, int nq, int max_q_l, int ctx_l, int K, int n_cand_rows,
                                                             int W, int* __restrict__ tok_off, int* __restrict__ tok_len,
                                                             int* __restrict__ tok_idx, int* __restrict__ q_ctx_l,
                                                             int* __restrict__ q_vid_off, int* __restrict__ batch_pad,
                                                             int* __restrict__ full_w, int* __restrict__ n_valid) {
    __shared__ int off[CONE_SESSION_MAX_QUERIES + 1];
    __shared__ int len[CONE_SESSION_MAX_QUERIES];
    const int t = threadIdx.x;
    if (t == 0) {
        int a = 0;
        for (int q = 0; q < nq; ++q) { off[q] = a; len[q] = L.len[q]; a += L.len[q]; }
        off[nq] = a;
    }
    __syncthreads();
    for (int q = t; q < nq; q += blockDim.x) {
        tok_off[q] = off[q]; tok_len[q] = len[q];
        q_ctx_l[q] = ctx_l; q_vid_off[q] = 0; batch_pad[q] = W; n_valid[q] = n_cand_rows;
    }
    if (t == 0) tok_off[nq] = off[nq];
    for (int i = t; i < nq * K; i += blockDim.x) full_w[i] = W;
    for (int i = t; i < nq * max_q_l; i += blockDim.x) {
        const int q = i / max_q_l, j = i - q * max_q_l;
        if (j < len[q]) tok_idx[off[q] + j] = j;
    }
}

static int check_queries(const char* who, const int32_t* tok_len, int nq, int max_q_l, int64_t* total) {
    CONE_REQUIRE(tok_len, "%s: null argument", who);
    CONE_REQUIRE(nq >= 1 && nq <= CONE_SESSION_MAX_QUERIES, "%s: nq=%d not in [1, %d]", who, nq, CONE_SESSION_MAX_QUERIES);
    CONE_REQUIRE(max_q_l >= 1, "%s: max_q_l=%d", who, max_q_l);
    int64_t T = 0;
    for (int q = 0; q < nq; ++q) {
        CONE_REQUIRE(tok_len[q] >= 1 && tok_len[q] <= max_q_l, "%s: tok_len[%d]=%d not in [1, max_q_l=%d]", who, q, tok_len[q],
                     max_q_l);
        T += tok_len[q];
    }
    *total = T;
    return 0;
}

// Every buffer and every launcher's scratch of one cone_session_localize call: the ONE function behind the workspace-size
// entry and the entry itself.  Each take() is a region of its own.
struct LocalizeLayout {
    size_t tok_off, tok_len, tok_idx, q_ctx_l, q_vid_off, batch_pad, full_w, n_valid;      // int32 metadata
    size_t tok_norm, scores, widx, wval, cert, wt, tproj, qkv_txt, txt_pos, txt_pos_qk, logits, spans, match, rows, nms_idx;
    size_t pf_ws, pf_bytes, topk_ws, topk_bytes, proj_ws, proj_bytes, l0_ws, l0_bytes, fwd_ws, fwd_bytes, match_ws, match_bytes;
    size_t total;
    int64_t T, nw;
    int B;
    bool use_l0, use_txt_pos;
};
static int localize_layout(const cone_model* m, const cone_model_dims& d, const cone_session* ses, const int32_t* tok_len, int nq,
                           int K, int n_cand, const cone_session_params* p, LocalizeLayout* out) {
    const char* who = "session_localize";
    CONE_REQUIRE(m && ses && p, "%s: null argument", who);
    CONE_REQUIRE(ses->model == m, "%s: the session was indexed with another handle", who);
    CONE_REQUIRE(flags_ok(ses->flags), "%s: bad session flags %d", who, ses->flags);
    CONE_REQUIRE(ses->v_dim == d.v_dim && ses->hidden_dim == d.hidden_dim, "%s: the session's row widths %d / %d are not the handle's %d / %d",
                 who, ses->v_dim, ses->hidden_dim, d.v_dim, d.hidden_dim);
    CONE_REQUIRE(p->max_v_l >= 2 && p->max_after >= 1 && p->max_before >= 1, "%s: bad params (max_v_l=%d, max_before=%d, max_after=%d)",
                 who, p->max_v_l, p->max_before, p->max_after);
    LocalizeLayout L{};
    RUN(check_queries(who, tok_len, nq, p->max_q_l, &L.T));
    CONE_REQUIRE(ses->ctx_l >= 1 && ses->ctx_l < (1ll << 31), "%s: ctx_l=%lld not in [1, 2^31)", who, (long long)ses->ctx_l);
    L.nw = cone_num_windows(ses->ctx_l, p->max_v_l);
    CONE_REQUIRE(K >= 1 && K <= L.nw && K <= 256, "%s: K=%d not in [1, min(num_window=%lld, 256)]", who, K, (long long)L.nw);
    CONE_REQUIRE(n_cand >= 0, "%s: n_cand=%d", who, n_cand);
    L.B = nq * K;
    const size_t T = (size_t)L.T, B = (size_t)L.B, Nq = (size_t)d.num_queries, dh = (size_t)d.hidden_dim;
    const bool cert = (ses->flags & CONE_SESSION_CERTIFIED) != 0;
    L.use_l0 = ses->qkv_vid != nullptr && !d.long_windows;
    L.use_txt_pos = L.use_l0 && d.txt_pos;
    Regions r;
    L.tok_off = r.take((nq + 1) * 4); L.tok_len = r.take(nq * 4); L.tok_idx = r.take(T * 4);
    L.q_ctx_l = r.take(nq * 4); L.q_vid_off = r.take(nq * 4); L.batch_pad = r.take(nq * 4);
    L.full_w = r.take(B * 4); L.n_valid = r.take(nq * 4);
    L.tok_norm = r.take(T * d.t_dim * 4);
    if (!cert) L.scores = r.take((size_t)nq * L.nw * 4);
    L.widx = r.take(B * 4); L.wval = r.take(B * 4); L.cert = r.take(nq * 4);
    L.wt = r.take(7 * align_up(B * 4, SES_ALIGN));
    L.tproj = r.take(T * dh * 4);
    if (L.use_l0) L.qkv_txt = r.take(T * 3 * dh * 4);
    if (L.use_txt_pos) { L.txt_pos = r.take(T * dh * 4); L.txt_pos_qk = r.take((size_t)d.enc_layers * T * 2 * dh * 4); }
    L.logits = r.take(B * Nq * 2 * 4); L.spans = r.take(B * Nq * 2 * 4);
    L.match = r.take(B * Nq * 4); L.rows = r.take(B * Nq * 4 * 4);
    L.nms_idx = r.take((size_t)3 * nq * p->max_after * 4);
    if (cert) {
        L.pf_bytes = cone_prefilter_topk_certified_workspace(ses->ctx_l, nq, p->max_v_l, K, n_cand);
        CONE_REQUIRE(L.pf_bytes, "%s: n_cand=%d is not a candidate count the certified pre-filter takes for %lld windows and K=%d", who,
                     n_cand, (long long)L.nw, K);
    } else {
        L.pf_bytes = ses->flags & CONE_SESSION_BF16 ? cone_prefilter_scores_bf16_workspace(ses->ctx_l, nq < 4 ? nq : 4, p->max_v_l)
                                                    : cone_prefilter_scores_workspace(ses->ctx_l, nq < 4 ? nq : 4, p->max_v_l);
        L.topk_bytes = cone_topk_windows_workspace(nq, L.nw, K);
    }
    L.pf_ws = r.take(L.pf_bytes); L.topk_ws = r.take(L.topk_bytes);
    L.proj_bytes = cone_project_workspace(m, 1, L.T); L.proj_ws = r.take(L.proj_bytes);
    L.l0_bytes = L.use_l0 ? cone_layer0_project_workspace(m, L.T) : 0; L.l0_ws = r.take(L.l0_bytes);
    // the forward's workspace depends on WHICH caches the call brings, never on where they live: placeholders stand in
    cone_layer0 probe{};
    static const float placeholder = 0.f;
    if (L.use_l0) { probe.qkv_vid = probe.qkv_txt = &placeholder; probe.max_v_l = p->max_v_l; }
    if (L.use_txt_pos) { probe.txt_pos = probe.txt_pos_qk = &placeholder; probe.n_txt = L.T; }
    L.fwd_bytes = cone_forward_packed_workspace(m, L.B, p->max_v_l, p->max_q_l, L.use_l0 ? &probe : nullptr);
    L.fwd_ws = r.take(L.fwd_bytes);
    L.match_bytes = cone_clip_matching_workspace(m, L.B); L.match_ws = r.take(L.match_bytes);
    L.total = r.cur;
    *out = L;
    return 0;
}

}  // namespace cone

using namespace cone;

extern "C" size_t cone_session_arena_bytes(const cone_model* m, int64_t ctx_l, int flags) {
    cone_model_dims d;
    if (ctx_l <= 0 || !flags_ok(flags) || cone_model_get_dims(m, &d)) return 0;
    return arena_layout(d, ctx_l, flags).total;
}
extern "C" size_t cone_session_workspace(const cone_model* m, int64_t ctx_l, int flags) {
    if (!m || ctx_l <= 0 || !flags_ok(flags)) return 0;
    return index_ws(m, ctx_l).total;
}

extern "C" int cone_session_index(const cone_model* m, const float* raw_vid, int64_t ctx_l, int flags, void* arena,
                                  size_t arena_bytes, void* ws, size_t ws_bytes, cone_session* session, void* stream) {
    CONE_REQUIRE(m && raw_vid && arena && ws && session, "session_index: null argument");
    CONE_REQUIRE(ctx_l >= 1 && ctx_l < (1ll << 31), "session_index: ctx_l=%lld not in [1, 2^31)", (long long)ctx_l);
    CONE_REQUIRE(flags_ok(flags), "session_index: flags=%d (CONE_SESSION_BF16 and CONE_SESSION_CERTIFIED exclude each other)", flags);
    CONE_REQUIRE(((uintptr_t)arena & (SES_ALIGN - 1)) == 0 && ((uintptr_t)ws & (SES_ALIGN - 1)) == 0,
                 "session_index: arena and workspace must be 256-B aligned");
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    CONE_REQUIRE(d.v_dim == d.v_motion_dim, "session_index: the localizer feeds one clip feature to both sides, v_dim=%d != v_motion_dim=%d",
                 d.v_dim, d.v_motion_dim);
    const ArenaLayout A = arena_layout(d, ctx_l, flags);
    const IndexWs w = index_ws(m, ctx_l);
    if (arena_bytes < A.total) { set_error("session_index: arena too small (%zu < %zu)", arena_bytes, A.total); return CONE_E_WORKSPACE; }
    if (ws_bytes < w.total) { set_error("session_index: workspace too small (%zu < %zu)", ws_bytes, w.total); return CONE_E_WORKSPACE; }
    char* a = (char*)arena;
    char* s = (char*)ws;
    float* vid_norm = (float*)(a + A.vid_norm);
    float* adapted = A.has_f32 ? (float*)(a + A.adapted) : nullptr;
    uint16_t* adapted16 = A.has_bf16 ? (uint16_t*)(a + A.adapted_bf16) : nullptr;
    float* err = A.has_err ? (float*)(a + A.err) : nullptr;
    float* vproj = (float*)(a + A.vproj);
    float* qkv_vid = A.has_qkv ? (float*)(a + A.qkv_vid) : nullptr;
    RUN(cone_l2_normalize_rows(raw_vid, ctx_l, d.v_dim, 1e-5f, 1, vid_norm, stream));                       // :129
    if (flags & CONE_SESSION_BF16)                                                                           // :135-138
        RUN(cone_adapter_norm_bf16(m, vid_norm, ctx_l, adapted16, 0, s + w.adapter, w.adapter_bytes, stream));
    else
        RUN(cone_adapter_norm(m, vid_norm, ctx_l, adapted, 0, s + w.adapter, w.adapter_bytes, stream));
    if (flags & CONE_SESSION_CERTIFIED) RUN(cone_prefilter_index_bf16(adapted, ctx_l, d.v_dim, adapted16, err, stream));
    RUN(cone_project_tokens(m, 0, vid_norm, ctx_l, vproj, s + w.proj, w.proj_bytes, stream));
    if (qkv_vid) RUN(cone_layer0_project(m, vproj, ctx_l, qkv_vid, w.l0_bytes ? s + w.l0 : nullptr, w.l0_bytes, stream));
    *session = cone_session{m, ctx_l, flags, d.v_dim, d.hidden_dim, vid_norm, adapted, adapted16, err, vproj, qkv_vid};
    return 0;
}

extern "C" int cone_session_query_layout(const int32_t* tok_len, int nq, int max_q_l, int64_t ctx_l, int K, int Nq, int max_v_l,
                                         int32_t* tok_off, int32_t* tok_len_dev, int32_t* tok_idx, int32_t* q_ctx_l,
                                         int32_t* q_vid_off, int32_t* batch_pad, int32_t* full_w, int32_t* n_valid, void* stream) {
    const char* who = "session_query_layout";
    int64_t T = 0;
    RUN(check_queries(who, tok_len, nq, max_q_l, &T));
    CONE_REQUIRE(tok_off && tok_len_dev && tok_idx && q_ctx_l && q_vid_off && batch_pad && full_w && n_valid, "%s: null argument", who);
    CONE_REQUIRE(ctx_l >= 1 && ctx_l < (1ll << 31), "%s: ctx_l=%lld not in [1, 2^31)", who, (long long)ctx_l);
    CONE_REQUIRE(K >= 1 && K <= 256 && Nq >= 1 && Nq <= 16 && max_v_l >= 2 && max_q_l <= 1024, "%s: bad sizes K=%d Nq=%d max_v_l=%d max_q_l=%d",
                 who, K, Nq, max_v_l, max_q_l);
    QueryLens L{};
    for (int q = 0; q < nq; ++q) L.len[q] = tok_len[q];
    hipLaunchKernelGGL(session_layout_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, L, nq, max_q_l, (int)ctx_l, K, K * Nq,
                       max_v_l, tok_off, tok_len_dev, tok_idx, q_ctx_l, q_vid_off, batch_pad, full_w, n_valid);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t cone_session_localize_workspace(const cone_model* m, const cone_session* session, const int32_t* tok_len, int nq,
                                                  int K, int n_cand, const cone_session_params* params) {
    cone_model_dims d;
    LocalizeLayout L;
    if (!m || cone_model_get_dims(m, &d) || localize_layout(m, d, session, tok_len, nq, K, n_cand, params, &L)) return 0;
    return L.total;
}

extern "C" int cone_session_localize(const cone_model* m, const cone_session* session, const float* tok, const int32_t* tok_len,
                                     int nq, const float* cls, int K, int n_cand, const cone_session_params* params, double* kept,
                                     int32_t* n_kept, int32_t* certified, void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && session && tok && tok_len && cls && params && kept && n_kept && ws, "session_localize: null argument");
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "session_localize: the workspace must be 256-B aligned");
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    LocalizeLayout L;
    RUN(localize_layout(m, d, session, tok_len, nq, K, n_cand, params, &L));
    if (ws_bytes < L.total) { set_error("session_localize: workspace too small (%zu < %zu)", ws_bytes, L.total); return CONE_E_WORKSPACE; }
    const cone_session& S = *session;
    const cone_session_params& P = *params;
    char* w = (char*)ws;
    auto I = [&](size_t at) { return (int32_t*)(w + at); };
    auto F = [&](size_t at) { return (float*)(w + at); };
    auto scratch = [&](size_t at, size_t bytes) { return bytes ? (void*)(w + at) : nullptr; };
    const int W = P.max_v_l, Sl = P.max_v_l / 2, B = L.B, Nq = d.num_queries, dv = d.v_dim;
    const size_t col = align_up((size_t)B * 4, SES_ALIGN);
    int32_t *vid_row0 = I(L.wt), *vid_len = I(L.wt + col), *video_start = I(L.wt + 2 * col), *pad_len = I(L.wt + 3 * col),
            *txt_row0 = I(L.wt + 4 * col), *txt_len = I(L.wt + 5 * col), *cls_row = I(L.wt + 6 * col);

    RUN(cone_session_query_layout(tok_len, nq, P.max_q_l, S.ctx_l, K, Nq, W, I(L.tok_off), I(L.tok_len), I(L.tok_idx), I(L.q_ctx_l),
                                  I(L.q_vid_off), I(L.batch_pad), I(L.full_w), I(L.n_valid), stream));
    RUN(cone_l2_normalize_rows(tok, L.T, d.t_dim, 1e-5f, 1, F(L.tok_norm), stream));                          // :133
    // stage A (:83-100, stable tie order): the raw cls vectors against the adapted rows
    if (S.flags & CONE_SESSION_CERTIFIED) {
        RUN(cone_prefilter_topk_certified(S.adapted, S.adapted_bf16, S.ctx_l, dv, cls, nq, W, Sl, K, n_cand, S.err, I(L.widx),
                                          F(L.wval), certified ? certified : I(L.cert), w + L.pf_ws, L.pf_bytes, stream));
    } else {
        for (int q0 = 0; q0 < nq; q0 += 4) {        // at most 4 queries a launch: the streaming form, whatever nq is
            const int n = nq - q0 < 4 ? nq - q0 : 4;
            float* sc = F(L.scores) + (size_t)q0 * L.nw;
            if (S.flags & CONE_SESSION_BF16)
                RUN(cone_prefilter_scores_bf16(S.adapted_bf16, S.ctx_l, dv, cls + (size_t)q0 * dv, n, W, Sl, sc, w + L.pf_ws,
                                               L.pf_bytes, stream));
            else
                RUN(cone_prefilter_scores(S.adapted, S.ctx_l, dv, cls + (size_t)q0 * dv, n, W, Sl, nullptr, sc, w + L.pf_ws,
                                          L.pf_bytes, stream));
        }
        RUN(cone_topk_windows_ws(F(L.scores), nq, L.nw, K, I(L.widx), F(L.wval), w + L.topk_ws, L.topk_bytes, stream));
    }
    // every window counts as padded to max_v_l (:150-170): one reference batch per query, its padding max_v_l
    RUN(cone_window_table(I(L.widx), nq, K, nullptr, nullptr, B, I(L.q_ctx_l), I(L.q_vid_off), I(L.tok_off), I(L.tok_len), 0, 1, W,
                          I(L.batch_pad), 0, nq, vid_row0, vid_len, video_start, pad_len, txt_row0, txt_len, cls_row, stream));
    RUN(cone_project_tokens(m, 1, F(L.tok_norm), L.T, F(L.tproj), w + L.proj_ws, L.proj_bytes, stream));
    cone_layer0 l0{};
    if (L.use_l0) {
        RUN(cone_layer0_project(m, F(L.tproj), L.T, F(L.qkv_txt), scratch(L.l0_ws, L.l0_bytes), L.l0_bytes, stream));
        l0.qkv_vid = S.qkv_vid; l0.qkv_txt = F(L.qkv_txt); l0.max_v_l = W;
        if (L.use_txt_pos) {
            RUN(cone_layer0_text_positions(m, F(L.tproj), I(L.tok_idx), L.T, F(L.txt_pos), F(L.txt_pos_qk), stream));
            l0.txt_pos = F(L.txt_pos); l0.txt_pos_qk = F(L.txt_pos_qk); l0.n_txt = L.T;
        }
    }
    RUN(cone_forward_packed(m, S.vproj, vid_row0, vid_len, F(L.tproj), txt_row0, txt_len, B, W, P.max_q_l, F(L.logits), F(L.spans),
                            nullptr, nullptr, L.use_l0 ? &l0 : nullptr, w + L.fwd_ws, L.fwd_bytes, stream));
    RUN(cone_clip_matching_gathered(m, cls, cls_row, S.vid_norm, vid_row0, vid_len, pad_len, F(L.spans), B, F(L.match),
                                    w + L.match_ws, L.match_bytes, stream));
    RUN(cone_compose_rows(F(L.logits), F(L.spans), F(L.match), I(L.full_w), video_start, P.clip_length, 0, B, Nq, F(L.rows),
                          stream));                                                                           // :191
    return cone_fuse_nms(F(L.rows), nullptr, I(L.n_valid), nq, K * Nq, P.nms_thd, P.max_before, P.max_after, kept, n_kept,
                         I(L.nms_idx), stream);                                                               // :200-219
}
