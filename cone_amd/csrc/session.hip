// Video sessions (include/cone_hip.h, "video sessions"): one resident video, indexed once, answering batches of queries.
// Video libraries ("video libraries"): many videos in the rows of one arena, one call for queries on any mix of them.
// Library search ("library search"): the query half on the window lists of a cone_library_scan (csrc/prefilter.hip).
// Library window budgets ("library window budgets"): the query half with a window count per pair (cone_library_localize_ragged;
// its own layout kernel and a gather of every pair's prefix -- the budget itself is csrc/library_budget.hip).
// Library moment search ("library moment search"): the ragged call that ends at its candidate rows
// (cone_library_localize_candidates; the pooled stage C is csrc/library_corpus.hip).
//
// Nothing is computed here.  cone_session_index / cone_library_add and cone_session_localize / cone_library_localize only
// SEQUENCE the library's own extern "C" launchers -- the calls cone_amd/localizator.py issues one by one through ctypes for
// run_on_video/cone_localizator.py:121-221 -- and carve their operands out of the caller's arena / workspace.  The layout kernels
// of this file write a call's index metadata (what the localizer keeps per shape in _const) from lengths, row
// offsets and clip counts that travel as kernel arguments.
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

// The video half on n rows: the ONE launcher chain behind cone_session_index (the whole arena, row 0) and cone_library_add
// (rows [row0, row0 + n) of a library's arena: the caller passes the regions already offset).  Every launcher works row by
// row: a row's bits depend neither on where the rows live nor on the launch's n (every form launch_gemm picks by the row
// bound runs the same chains per row; tests/test_library_ingest_gpu.py pins it at the forms' thresholds).
struct IndexRows { float* vid_norm; float* adapted; uint16_t* adapted_bf16; float* err; float* vproj; float* qkv_vid; };
static int index_rows(const cone_model* m, const cone_model_dims& d, int flags, const float* raw, int64_t n, const IndexRows& o,
                      char* s, const IndexWs& w, void* stream) {
    RUN(cone_l2_normalize_rows(raw, n, d.v_dim, 1e-5f, 1, o.vid_norm, stream));                              // :129
    if (flags & CONE_SESSION_BF16)                                                                           // :135-138
        RUN(cone_adapter_norm_bf16(m, o.vid_norm, n, o.adapted_bf16, 0, s + w.adapter, w.adapter_bytes, stream));
    else
        RUN(cone_adapter_norm(m, o.vid_norm, n, o.adapted, 0, s + w.adapter, w.adapter_bytes, stream));
    if (flags & CONE_SESSION_CERTIFIED) RUN(cone_prefilter_index_bf16(o.adapted, n, d.v_dim, o.adapted_bf16, o.err, stream));
    RUN(cone_project_tokens(m, 0, o.vid_norm, n, o.vproj, s + w.proj, w.proj_bytes, stream));
    if (o.qkv_vid) RUN(cone_layer0_project(m, o.vproj, n, o.qkv_vid, w.l0_bytes ? s + w.l0 : nullptr, w.l0_bytes, stream));
    return 0;
}

// What the query half reads of the resident rows: a session's one video, or a library's arena of many.
struct Resident {
    const cone_model* model;
    int32_t flags, v_dim, hidden_dim;
    const float *vid_norm, *adapted;
    const uint16_t* adapted_bf16;
    const float *err, *vproj, *qkv_vid;
};
static Resident resident_of(const cone_session& S) {
    return {S.model, S.flags, S.v_dim, S.hidden_dim, S.vid_norm, S.adapted, S.adapted_bf16, S.err, S.vproj, S.qkv_vid};
}
static Resident resident_of(const cone_library& B) {
    return {B.model, B.flags, B.v_dim, B.hidden_dim, B.vid_norm, B.adapted, B.adapted_bf16, nullptr, B.vproj, B.qkv_vid};
}

// ------------------------------------------------------------------------------ the query half
struct QueryLens { int32_t len[CONE_SESSION_MAX_QUERIES]; };

struct QueryPairs { int32_t len[CONE_SESSION_MAX_QUERIES], row0[CONE_SESSION_MAX_QUERIES], ctx_l[CONE_SESSION_MAX_QUERIES]; };

// One workgroup.  Every output element has one writer; nothing outside the documented extents is touched:
// tok_off [0, nq], the per-query arrays [0, nq), full_w [0, nq K), tok_idx [0, sum of the lengths).
// in_len: the token lengths (kernel arguments); ctx_of / off_of: query -> clips of its video / first arena row of its video.
template <class CtxOf, class OffOf>
__device__ __forceinline__ void layout_body(const int32_t* in_len, CtxOf ctx_of, OffOf off_of, int nq, int max_q_l, int K,
                                            int n_cand_rows, int W, int* __restrict__ tok_off, int* __restrict__ tok_len,
                                            int* __restrict__ tok_idx, int* __restrict__ q_ctx_l, int* __restrict__ q_vid_off,
                                            int* __restrict__ batch_pad, int* __restrict__ full_w, int* __restrict__ n_valid) {
    __shared__ int off[CONE_SESSION_MAX_QUERIES + 1];
    __shared__ int len[CONE_SESSION_MAX_QUERIES];
    const int t = threadIdx.x;
    if (t == 0) {
        int a = 0;
        for (int q = 0; q < nq; ++q) { off[q] = a; len[q] = in_len[q]; a += in_len[q]; }
        off[nq] = a;
    }
    __syncthreads();
    for (int q = t; q < nq; q += blockDim.x) {
        tok_off[q] = off[q]; tok_len[q] = len[q];
        q_ctx_l[q] = ctx_of(q); q_vid_off[q] = off_of(q); batch_pad[q] = W; n_valid[q] = n_cand_rows;
    }
    if (t == 0) tok_off[nq] = off[nq];
    for (int i = t; i < nq * K; i += blockDim.x) full_w[i] = W;
    for (int i = t; i < nq * max_q_l; i += blockDim.x) {
        const int q = i / max_q_l, j = i - q * max_q_l;
        if (j < len[q]) tok_idx[off[q] + j] = j;
    }
}

__global__ __launch_bounds__(256) void session_layout_kernel(QueryLens L, int nq, int max_q_l, int ctx_l, int K, int n_cand_rows,
                                                             int W, int* __restrict__ tok_off, int* __restrict__ tok_len,
                                                             int* __restrict__ tok_idx, int* __restrict__ q_ctx_l,
                                                             int* __restrict__ q_vid_off, int* __restrict__ batch_pad,
                                                             int* __restrict__ full_w, int* __restrict__ n_valid) {
    layout_body(L.len, [=](int) { return ctx_l; }, [](int) { return 0; }, nq, max_q_l, K, n_cand_rows, W, tok_off, tok_len, tok_idx,
                q_ctx_l, q_vid_off, batch_pad, full_w, n_valid);
}

// The library's form: every query brings the clips and the first arena row of ITS video.
__global__ __launch_bounds__(256) void library_layout_kernel(QueryPairs P, int nq, int max_q_l, int K, int n_cand_rows, int W,
                                                             int* __restrict__ tok_off, int* __restrict__ tok_len,
                                                             int* __restrict__ tok_idx, int* __restrict__ q_ctx_l,
                                                             int* __restrict__ q_vid_off, int* __restrict__ batch_pad,
                                                             int* __restrict__ full_w, int* __restrict__ n_valid) {
    const int32_t *ctx = P.ctx_l, *row0 = P.row0;
    layout_body(P.len, [=](int q) { return ctx[q]; }, [=](int q) { return row0[q]; }, nq, max_q_l, K, n_cand_rows, W, tok_off,
                tok_len, tok_idx, q_ctx_l, q_vid_off, batch_pad, full_w, n_valid);
}

// The ragged form (cone_library_localize_ragged): pair q brings its own window count k[q] <= Kmax.  What library_layout_kernel
// writes, except that the window rows are the concatenation of the pairs' k[q] rows: row_q / row_slot / full_w [0, sum k),
// n_valid[q] = k[q] Nq, cand_off[q] = (rows before pair q) Nq.  One workgroup, one writer per element.
struct RaggedK { int32_t k[CONE_SESSION_MAX_QUERIES]; };
__global__ __launch_bounds__(256) void library_ragged_layout_kernel(QueryPairs P, RaggedK R, int nq, int max_q_l, int Kmax, int Nq,
                                                                    int W, int* __restrict__ tok_off, int* __restrict__ tok_len,
                                                                    int* __restrict__ tok_idx, int* __restrict__ q_ctx_l,
                                                                    int* __restrict__ q_vid_off, int* __restrict__ batch_pad,
                                                                    int* __restrict__ full_w, int* __restrict__ n_valid,
                                                                    int* __restrict__ row_q, int* __restrict__ row_slot,
                                                                    int64_t* __restrict__ cand_off) {
    __shared__ int off[CONE_SESSION_MAX_QUERIES + 1];       // exclusive prefix sums of the token lengths
    __shared__ int woff[CONE_SESSION_MAX_QUERIES + 1];      // ... of the window counts
    __shared__ int len[CONE_SESSION_MAX_QUERIES];
    __shared__ int kq[CONE_SESSION_MAX_QUERIES];
    const int t = threadIdx.x;
    if (t == 0) {
        int a = 0, b = 0;
        for (int q = 0; q < nq; ++q) {
            off[q] = a; woff[q] = b; len[q] = P.len[q]; kq[q] = R.k[q];
            a += P.len[q]; b += R.k[q];
        }
        off[nq] = a; woff[nq] = b;
    }
    __syncthreads();
    for (int q = t; q < nq; q += blockDim.x) {
        tok_off[q] = off[q]; tok_len[q] = len[q];
        q_ctx_l[q] = P.ctx_l[q]; q_vid_off[q] = P.row0[q]; batch_pad[q] = W;
        n_valid[q] = kq[q] * Nq; cand_off[q] = (int64_t)woff[q] * Nq;
    }
    if (t == 0) tok_off[nq] = off[nq];
    for (int i = t; i < nq * Kmax; i += blockDim.x) {
        const int q = i / Kmax, j = i - q * Kmax;
        if (j < kq[q]) { const int b = woff[q] + j; row_q[b] = q; row_slot[b] = j; full_w[b] = W; }
    }
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

// The (video, query) pairs of a library call, on the host, before any pointer into the device is read: every query's video
// lies inside [0, rows) (rows < 0: only inside the int32 row range) and has at least K windows.
static int check_pairs(const char* who, const int32_t* q_row0, const int32_t* q_ctx_l, int nq, int64_t rows, int K, int max_v_l) {
    CONE_REQUIRE(q_row0 && q_ctx_l, "%s: null argument", who);
    CONE_REQUIRE(max_v_l >= 2, "%s: max_v_l=%d", who, max_v_l);
    for (int q = 0; q < nq; ++q) {
        CONE_REQUIRE(q_ctx_l[q] >= 1, "%s: q_ctx_l[%d]=%d < 1", who, q, q_ctx_l[q]);
        CONE_REQUIRE(q_row0[q] >= 0, "%s: q_row0[%d]=%d < 0", who, q, q_row0[q]);
        const int64_t end = (int64_t)q_row0[q] + q_ctx_l[q];
        if (rows >= 0)
            CONE_REQUIRE(end <= rows, "%s: q_row0[%d] + q_ctx_l[%d] = %lld > capacity=%lld", who, q, q, (long long)end, (long long)rows);
        else
            CONE_REQUIRE(end < (1ll << 31), "%s: q_row0[%d] + q_ctx_l[%d] = %lld not below 2^31", who, q, q, (long long)end);
        const int64_t nw = cone_num_windows(q_ctx_l[q], max_v_l);
        CONE_REQUIRE(K >= 1 && K <= nw && K <= 256, "%s: K=%d not in [1, min(num_window=%lld, 256)] for query %d", who, K, (long long)nw, q);
    }
    return 0;
}

// The window counts of a ragged call (after check_pairs): pair p has at least pair_k[p] windows.  Kmax = their maximum.
static int check_ragged(const char* who, const int32_t* pair_k, const int32_t* q_ctx_l, int nq, int max_v_l, int* Kmax) {
    CONE_REQUIRE(pair_k, "%s: null argument", who);
    int m = 0;
    for (int p = 0; p < nq; ++p) {
        const int64_t nw = cone_num_windows(q_ctx_l[p], max_v_l);
        CONE_REQUIRE(pair_k[p] >= 1 && pair_k[p] <= nw && pair_k[p] <= 256, "%s: pair_k[%d]=%d not in [1, min(num_window=%lld, 256)]", who, p,
                     pair_k[p], (long long)nw);
        m = pair_k[p] > m ? pair_k[p] : m;
    }
    *Kmax = m;
    return 0;
}

// Consecutive queries of one video: one stage A.  A session is one run.
struct Run { int q0, n; int64_t row0, ctx_l, nw; size_t score_off; int k; size_t st_off; };     // (k, st_off: a ragged call's)

// Every buffer and every launcher's scratch of one cone_session_localize / cone_library_localize call: the ONE function
// behind the workspace-size entries and the entries themselves.  Each take() is a region of its own.
struct LocalizeLayout {
    Run runs[CONE_SESSION_MAX_QUERIES];
    int n_runs;
    size_t tok_off, tok_len, tok_idx, q_ctx_l, q_vid_off, batch_pad, full_w, n_valid;      // int32 metadata
    size_t tok_norm, scores, widx, wval, cert, wt, tproj, qkv_txt, txt_pos, txt_pos_qk, logits, spans, match, rows, nms_idx;
    size_t row_q, row_slot, cand_off, st_idx, st_val;       // a ragged call's: the row maps, the row offsets, the runs' own lists
    size_t pf_ws, pf_bytes, topk_ws, topk_bytes, proj_ws, proj_bytes, l0_ws, l0_bytes, fwd_ws, fwd_bytes, match_ws, match_bytes;
    size_t total;
    int64_t T, nw;
    int B;
    bool use_l0, use_txt_pos;
};
// rows: the session's ctx_l, or the library's capacity; q_row0 / q_ctx_l: NULL for a session (one run over all of its rows).
static int localize_layout(const char* who, const char* what, const cone_model* m, const cone_model_dims& d, const Resident* ses,
                           int64_t rows, const int32_t* q_row0, const int32_t* q_ctx_l, const int32_t* tok_len, int nq, int K,
                           int n_cand, const cone_session_params* p, LocalizeLayout* out, bool ranked = false,
                           const int32_t* pair_k = nullptr) {      // pair_k: a ragged call (K = their maximum, check_ragged's)
    CONE_REQUIRE(m && ses && p, "%s: null argument", who);
    CONE_REQUIRE(ses->model == m, "%s: the %s was indexed with another handle", who, what);
    CONE_REQUIRE(flags_ok(ses->flags), "%s: bad %s flags %d", who, what, ses->flags);
    CONE_REQUIRE(ses->v_dim == d.v_dim && ses->hidden_dim == d.hidden_dim, "%s: the %s's row widths %d / %d are not the handle's %d / %d",
                 who, what, ses->v_dim, ses->hidden_dim, d.v_dim, d.hidden_dim);
    CONE_REQUIRE(p->max_v_l >= 2 && p->max_after >= 1 && p->max_before >= 1, "%s: bad params (max_v_l=%d, max_before=%d, max_after=%d)",
                 who, p->max_v_l, p->max_before, p->max_after);
    LocalizeLayout L{};
    RUN(check_queries(who, tok_len, nq, p->max_q_l, &L.T));
    const bool cert = (ses->flags & CONE_SESSION_CERTIFIED) != 0;
    size_t n_scores = 0;
    if (q_row0) {       // (library_precheck has vetted the pairs, K and the capacity)
        for (int q = 0; q < nq; ++q) {
            if (q == 0 || q_row0[q] != q_row0[q - 1] || q_ctx_l[q] != q_ctx_l[q - 1])
                L.runs[L.n_runs++] = Run{q, 0, q_row0[q], q_ctx_l[q], cone_num_windows(q_ctx_l[q], p->max_v_l), n_scores, 0, 0};
            Run& r = L.runs[L.n_runs - 1];
            r.n += 1;
            n_scores += (size_t)r.nw;
        }
    } else {
        CONE_REQUIRE(rows >= 1 && rows < (1ll << 31), "%s: ctx_l=%lld not in [1, 2^31)", who, (long long)rows);
        L.nw = cone_num_windows(rows, p->max_v_l);
        CONE_REQUIRE(K >= 1 && K <= L.nw && K <= 256, "%s: K=%d not in [1, min(num_window=%lld, 256)]", who, K, (long long)L.nw);
        L.runs[L.n_runs++] = Run{0, nq, 0, rows, L.nw, 0, 0, 0};
        n_scores = (size_t)nq * L.nw;
    }
    CONE_REQUIRE(n_cand >= 0, "%s: n_cand=%d", who, n_cand);
    L.B = nq * K;
    if (pair_k) {
        L.B = 0;
        for (int q = 0; q < nq; ++q) L.B += pair_k[q];
    }
    const size_t T = (size_t)L.T, B = (size_t)L.B, Nq = (size_t)d.num_queries, dh = (size_t)d.hidden_dim;
    L.use_l0 = ses->qkv_vid != nullptr && !d.long_windows;
    L.use_txt_pos = L.use_l0 && d.txt_pos;
    Regions r;
    L.tok_off = r.take((nq + 1) * 4); L.tok_len = r.take(nq * 4); L.tok_idx = r.take(T * 4);
    L.q_ctx_l = r.take(nq * 4); L.q_vid_off = r.take(nq * 4); L.batch_pad = r.take(nq * 4);
    L.full_w = r.take(B * 4); L.n_valid = r.take(nq * 4);
    if (pair_k) { L.row_q = r.take(B * 4); L.row_slot = r.take(B * 4); L.cand_off = r.take(nq * 8); }
    L.tok_norm = r.take(T * d.t_dim * 4);
    if (!cert && !ranked) L.scores = r.take(n_scores * 4);        // (ranked: the lists come from a scan -- no stage A here)
    const size_t n_list = pair_k ? (size_t)nq * K : B;            // the call's (nq, K) window list
    L.widx = r.take(n_list * 4); L.wval = r.take(n_list * 4); L.cert = r.take(nq * 4);
    if (pair_k && !ranked) {        // every run ranks its video at the largest count among its pairs; the pairs take prefixes
        size_t at = 0;
        for (int i = 0; i < L.n_runs; ++i) {
            Run& u = L.runs[i];
            for (int q = u.q0; q < u.q0 + u.n; ++q) u.k = pair_k[q] > u.k ? pair_k[q] : u.k;
            u.st_off = at;
            at += (size_t)u.n * u.k;
        }
        L.st_idx = r.take(at * 4); L.st_val = r.take(at * 4);
    }
    L.wt = r.take(7 * align_up(B * 4, SES_ALIGN));
    L.tproj = r.take(T * dh * 4);
    if (L.use_l0) L.qkv_txt = r.take(T * 3 * dh * 4);
    if (L.use_txt_pos) { L.txt_pos = r.take(T * dh * 4); L.txt_pos_qk = r.take((size_t)d.enc_layers * T * 2 * dh * 4); }
    L.logits = r.take(B * Nq * 2 * 4); L.spans = r.take(B * Nq * 2 * 4);
    L.match = r.take(B * Nq * 4); L.rows = r.take(B * Nq * 4 * 4);
    L.nms_idx = r.take((size_t)3 * nq * p->max_after * 4);
    if (cert) {
        L.pf_bytes = cone_prefilter_topk_certified_workspace(rows, nq, p->max_v_l, K, n_cand);
        CONE_REQUIRE(L.pf_bytes, "%s: n_cand=%d is not a candidate count the certified pre-filter takes for %lld windows and K=%d", who,
                     n_cand, (long long)L.nw, K);
    } else if (!ranked) {
        for (int i = 0; i < L.n_runs; ++i) {        // the runs follow each other on one stream: they share the largest scratch
            const Run& u = L.runs[i];
            const int n = u.n < 4 ? u.n : 4;
            const size_t pf = ses->flags & CONE_SESSION_BF16 ? cone_prefilter_scores_bf16_workspace(u.ctx_l, n, p->max_v_l)
                                                             : cone_prefilter_scores_workspace(u.ctx_l, n, p->max_v_l);
            const size_t tk = cone_topk_windows_workspace(u.n, u.nw, pair_k ? u.k : K);
            L.pf_bytes = pf > L.pf_bytes ? pf : L.pf_bytes;
            L.topk_bytes = tk > L.topk_bytes ? tk : L.topk_bytes;
        }
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
    RUN(index_rows(m, d, flags, raw_vid, ctx_l, IndexRows{vid_norm, adapted, adapted16, err, vproj, qkv_vid}, s, w, stream));
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

extern "C" int cone_library_query_layout(const int32_t* tok_len, const int32_t* q_row0, const int32_t* q_ctx_l, int nq, int max_q_l,
                                         int K, int Nq, int max_v_l, int32_t* tok_off, int32_t* tok_len_dev, int32_t* tok_idx,
                                         int32_t* q_ctx_l_dev, int32_t* q_vid_off, int32_t* batch_pad, int32_t* full_w,
                                         int32_t* n_valid, void* stream) {
    const char* who = "library_query_layout";
    int64_t T = 0;
    RUN(check_queries(who, tok_len, nq, max_q_l, &T));
    RUN(check_pairs(who, q_row0, q_ctx_l, nq, -1, K, max_v_l));
    CONE_REQUIRE(tok_off && tok_len_dev && tok_idx && q_ctx_l_dev && q_vid_off && batch_pad && full_w && n_valid, "%s: null argument", who);
    CONE_REQUIRE(Nq >= 1 && Nq <= 16 && max_q_l <= 1024, "%s: bad sizes Nq=%d max_q_l=%d", who, Nq, max_q_l);
    QueryPairs P{};
    for (int q = 0; q < nq; ++q) { P.len[q] = tok_len[q]; P.row0[q] = q_row0[q]; P.ctx_l[q] = q_ctx_l[q]; }
    hipLaunchKernelGGL(library_layout_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, P, nq, max_q_l, K, K * Nq, max_v_l, tok_off,
                       tok_len_dev, tok_idx, q_ctx_l_dev, q_vid_off, batch_pad, full_w, n_valid);
    CONE_LAUNCH_CHECK();
    return 0;
}

namespace cone {

// "The lists are here": the window lists of a cone_library_scan -- (scan_nq, n_videos, scan_K) on the device -- and, per pair of
// this call, the scan's query index and table slot (host values: kernel arguments, nothing is uploaded).
struct RankedPairs { int32_t query[CONE_SESSION_MAX_QUERIES], slot[CONE_SESSION_MAX_QUERIES]; };
struct RankedLists {
    const int32_t* widx;
    const float* wval;
    int64_t n_videos;
    int scan_K;
    RankedPairs pairs;
};
// pair p's first K entries of the list of (query[p], slot[p]) -> the call's window list; one writer per element
__global__ __launch_bounds__(256) void library_gather_lists_kernel(RankedPairs P, int nq, int K, int64_t n_videos, int scan_K,
                                                                   const int32_t* __restrict__ scan_widx,
                                                                   const float* __restrict__ scan_wval, int32_t* __restrict__ widx,
                                                                   float* __restrict__ wval) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq * K) return;
    const int p = i / K, j = i - p * K;
    const size_t src = ((size_t)P.query[p] * n_videos + P.slot[p]) * scan_K + j;
    widx[i] = scan_widx[src];
    wval[i] = scan_wval[src];
}

// A ragged call's lists: pair p's first k[p] entries of the list that starts at element off[p] of (src_idx, src_val) -- a scan's
// lists, or the lists the call's own runs ranked -- -> row p of the call's (nq, Kmax) window list; the rest of the row is
// (-1, -inf) and never read.  One writer per element, every element written.
struct RaggedSrc { int64_t off[CONE_SESSION_MAX_QUERIES]; int32_t k[CONE_SESSION_MAX_QUERIES]; };
__global__ __launch_bounds__(256) void library_gather_ragged_kernel(RaggedSrc R, int nq, int Kmax, const int32_t* __restrict__ src_idx,
                                                                    const float* __restrict__ src_val, int32_t* __restrict__ widx,
                                                                    float* __restrict__ wval) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq * Kmax) return;
    const int p = i / Kmax, j = i - p * Kmax;
    const bool in = j < R.k[p];
    widx[i] = in ? src_idx[R.off[p] + j] : -1;
    wval[i] = in ? src_val[R.off[p] + j] : -INFINITY;
}

// The query half for both kinds of resident rows: q_row0 / q_ctx_l == NULL is a session (one video at row 0, `rows` clips),
// otherwise a library call (every query names its video's rows inside an arena of `rows`).  Nothing differs after stage A.
// pair_k != NULL is a ragged library call (K = the largest count): pair q owns pair_k[q] window rows, not K -- its own layout
// kernel, a gather of every pair's prefix, then the row form of cone_window_table and the offset form of cone_fuse_nms.  The
// uniform calls run the launches they always ran.  cand != NULL (cone_library_localize_candidates): the call ends at its
// candidate rows, composed straight into `cand`; kept / n_kept are not touched.
static int localize(const char* who, const cone_model* m, const cone_model_dims& d, const Resident& S, int64_t rows,
                    const LocalizeLayout& L, const int32_t* q_row0, const int32_t* q_ctx_l, const float* tok, const int32_t* tok_len,
                    int nq, const float* cls, int K, int n_cand, const cone_session_params& P, double* kept, int32_t* n_kept,
                    int32_t* certified, char* w, void* stream, const RankedLists* lists = nullptr,
                    const int32_t* pair_k = nullptr, float* cand = nullptr) {
    auto I = [&](size_t at) { return (int32_t*)(w + at); };
    auto F = [&](size_t at) { return (float*)(w + at); };
    auto scratch = [&](size_t at, size_t bytes) { return bytes ? (void*)(w + at) : nullptr; };
    const int W = P.max_v_l, Sl = P.max_v_l / 2, B = L.B, Nq = d.num_queries, dv = d.v_dim;
    const size_t col = align_up((size_t)B * 4, SES_ALIGN);
    int32_t *vid_row0 = I(L.wt), *vid_len = I(L.wt + col), *video_start = I(L.wt + 2 * col), *pad_len = I(L.wt + 3 * col),
            *txt_row0 = I(L.wt + 4 * col), *txt_len = I(L.wt + 5 * col), *cls_row = I(L.wt + 6 * col);

    if (pair_k) {
        QueryPairs Q{};
        RaggedK R{};
        for (int q = 0; q < nq; ++q) { Q.len[q] = tok_len[q]; Q.row0[q] = q_row0[q]; Q.ctx_l[q] = q_ctx_l[q]; R.k[q] = pair_k[q]; }
        hipLaunchKernelGGL(library_ragged_layout_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, Q, R, nq, P.max_q_l, K, Nq, W,
                           I(L.tok_off), I(L.tok_len), I(L.tok_idx), I(L.q_ctx_l), I(L.q_vid_off), I(L.batch_pad), I(L.full_w),
                           I(L.n_valid), I(L.row_q), I(L.row_slot), (int64_t*)(w + L.cand_off));
        CONE_LAUNCH_CHECK();
    } else if (q_row0)
        RUN(cone_library_query_layout(tok_len, q_row0, q_ctx_l, nq, P.max_q_l, K, Nq, W, I(L.tok_off), I(L.tok_len), I(L.tok_idx),
                                      I(L.q_ctx_l), I(L.q_vid_off), I(L.batch_pad), I(L.full_w), I(L.n_valid), stream));
    else
        RUN(cone_session_query_layout(tok_len, nq, P.max_q_l, rows, K, Nq, W, I(L.tok_off), I(L.tok_len), I(L.tok_idx), I(L.q_ctx_l),
                                      I(L.q_vid_off), I(L.batch_pad), I(L.full_w), I(L.n_valid), stream));
    RUN(cone_l2_normalize_rows(tok, L.T, d.t_dim, 1e-5f, 1, F(L.tok_norm), stream));                          // :133
    // stage A (:83-100, stable tie order): the raw cls vectors against the adapted rows
    if (lists && !pair_k) {     // a scan has ranked the windows (cone_library_scan: the same lists, bit for bit): copy each pair's
        hipLaunchKernelGGL(library_gather_lists_kernel, dim3((unsigned)((nq * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           lists->pairs, nq, K, lists->n_videos, lists->scan_K, lists->widx, lists->wval, I(L.widx), F(L.wval));
        CONE_LAUNCH_CHECK();
    } else if (S.flags & CONE_SESSION_CERTIFIED) {
        RUN(cone_prefilter_topk_certified(S.adapted, S.adapted_bf16, rows, dv, cls, nq, W, Sl, K, n_cand, S.err, I(L.widx),
                                          F(L.wval), certified ? certified : I(L.cert), w + L.pf_ws, L.pf_bytes, stream));
    } else if (!lists) {
        for (int i = 0; i < L.n_runs; ++i) {        // one video a run, in the form and with the arguments of a session on it
            const Run& u = L.runs[i];
            float* scores = F(L.scores) + u.score_off;
            for (int q0 = 0; q0 < u.n; q0 += 4) {   // at most 4 queries a launch: the streaming form, whatever the run's length
                const int n = u.n - q0 < 4 ? u.n - q0 : 4;
                float* sc = scores + (size_t)q0 * u.nw;
                const float* c = cls + (size_t)(u.q0 + q0) * dv;
                if (S.flags & CONE_SESSION_BF16)
                    RUN(cone_prefilter_scores_bf16(S.adapted_bf16 + (size_t)u.row0 * dv, u.ctx_l, dv, c, n, W, Sl, sc, w + L.pf_ws,
                                                   L.pf_bytes, stream));
                else
                    RUN(cone_prefilter_scores(S.adapted + (size_t)u.row0 * dv, u.ctx_l, dv, c, n, W, Sl, nullptr, sc, w + L.pf_ws,
                                              L.pf_bytes, stream));
            }
            if (pair_k)     // a ragged call: the run's lists at the largest count among its pairs (a video may have fewer than K windows)
                RUN(cone_topk_windows_ws(scores, u.n, u.nw, u.k, I(L.st_idx) + u.st_off, F(L.st_val) + u.st_off, w + L.topk_ws,
                                         L.topk_bytes, stream));
            else
                RUN(cone_topk_windows_ws(scores, u.n, u.nw, K, I(L.widx) + (size_t)u.q0 * K, F(L.wval) + (size_t)u.q0 * K, w + L.topk_ws,
                                         L.topk_bytes, stream));
        }
    }
    if (pair_k) {       // every pair takes the prefix it asked for: of a scan's list of (query, slot), or of its run's list
        RaggedSrc R{};
        for (int q = 0; q < nq; ++q) R.k[q] = pair_k[q];
        if (lists)
            for (int q = 0; q < nq; ++q)
                R.off[q] = ((int64_t)lists->pairs.query[q] * lists->n_videos + lists->pairs.slot[q]) * lists->scan_K;
        else
            for (int i = 0; i < L.n_runs; ++i)
                for (int q = 0; q < L.runs[i].n; ++q)
                    R.off[L.runs[i].q0 + q] = (int64_t)(L.runs[i].st_off + (size_t)q * L.runs[i].k);
        hipLaunchKernelGGL(library_gather_ragged_kernel, dim3((unsigned)((nq * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R, nq,
                           K, lists ? lists->widx : I(L.st_idx), lists ? lists->wval : F(L.st_val), I(L.widx), F(L.wval));
        CONE_LAUNCH_CHECK();
    }
    // every window counts as padded to max_v_l (:150-170): one reference batch per query, its padding max_v_l
    RUN(cone_window_table(I(L.widx), nq, K, pair_k ? I(L.row_q) : nullptr, pair_k ? I(L.row_slot) : nullptr, B, I(L.q_ctx_l),
                          I(L.q_vid_off), I(L.tok_off), I(L.tok_len), 0, 1, W, I(L.batch_pad), 0, nq, vid_row0, vid_len, video_start, pad_len, txt_row0, txt_len, cls_row, stream));
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
    RUN(cone_compose_rows(F(L.logits), F(L.spans), F(L.match), I(L.full_w), video_start, P.clip_length, 0, B, Nq,
                          cand ? cand : F(L.rows), stream));                                                  // :191
    if (cand) return 0;     // the caller pools the candidates of many calls (cone_corpus_fuse_nms): the B * Nq rows, no stage C
    return cone_fuse_nms(F(L.rows), pair_k ? (const int64_t*)(w + L.cand_off) : nullptr, I(L.n_valid), nq, K * Nq, P.nms_thd, P.max_before, P.max_after, kept, n_kept,
                         I(L.nms_idx), stream);                                                               // :200-219
}

}  // namespace cone

extern "C" size_t cone_session_localize_workspace(const cone_model* m, const cone_session* session, const int32_t* tok_len, int nq,
                                                  int K, int n_cand, const cone_session_params* params) {
    cone_model_dims d;
    LocalizeLayout L;
    if (!m || cone_model_get_dims(m, &d)) return 0;
    const Resident S = session ? resident_of(*session) : Resident{};
    if (localize_layout("session_localize", "session", m, d, session ? &S : nullptr, session ? session->ctx_l : 0, nullptr, nullptr,
                        tok_len, nq, K, n_cand, params, &L))
        return 0;
    return L.total;
}

extern "C" int cone_session_localize(const cone_model* m, const cone_session* session, const float* tok, const int32_t* tok_len,
                                     int nq, const float* cls, int K, int n_cand, const cone_session_params* params, double* kept,
                                     int32_t* n_kept, int32_t* certified, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "session_localize";
    CONE_REQUIRE(m && session && tok && tok_len && cls && params && kept && n_kept && ws, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    const Resident S = resident_of(*session);
    LocalizeLayout L;
    RUN(localize_layout(who, "session", m, d, &S, session->ctx_l, nullptr, nullptr, tok_len, nq, K, n_cand, params, &L));
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    return localize(who, m, d, S, session->ctx_l, L, nullptr, nullptr, tok, tok_len, nq, cls, K, n_cand, *params, kept, n_kept,
                    certified, (char*)ws, stream);
}

// ------------------------------------------------------------------------------ video libraries
namespace cone {

static bool library_flags_ok(int flags) { return flags == 0 || flags == CONE_SESSION_BF16; }

// The refusals a library call makes from host values alone, in this order, before the handle is looked at.
static int library_precheck(const char* who, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                            const int32_t* tok_len, int nq, int K, const cone_session_params* p) {
    CONE_REQUIRE(lib && q_row0 && q_ctx_l && tok_len && p, "%s: null argument", who);
    CONE_REQUIRE(!(lib->flags & CONE_SESSION_CERTIFIED), "%s: CONE_SESSION_CERTIFIED libraries are not supported", who);
    CONE_REQUIRE(lib->capacity >= 1 && lib->capacity < (1ll << 31), "%s: capacity=%lld not in [1, 2^31)", who, (long long)lib->capacity);
    int64_t T = 0;
    RUN(check_queries(who, tok_len, nq, p->max_q_l, &T));
    return check_pairs(who, q_row0, q_ctx_l, nq, lib->capacity, K, p->max_v_l);
}
static int library_handle(const char* who, const cone_model* m, const cone_library* lib) {
    CONE_REQUIRE(m, "%s: null argument", who);
    CONE_REQUIRE(lib->model == m, "%s: the library was opened with another handle", who);
    return 0;
}

}  // namespace cone

extern "C" size_t cone_library_arena_bytes(const cone_model* m, int64_t capacity, int flags) {
    cone_model_dims d;
    if (flags & CONE_SESSION_CERTIFIED) { set_error("library_arena_bytes: CONE_SESSION_CERTIFIED libraries are not supported"); return 0; }
    if (capacity <= 0 || capacity >= (1ll << 31) || !library_flags_ok(flags) || cone_model_get_dims(m, &d)) return 0;
    return arena_layout(d, capacity, flags).total;
}

extern "C" int cone_library_open(const cone_model* m, int64_t capacity, int flags, void* arena, size_t arena_bytes, cone_library* out) {
    const char* who = "library_open";
    CONE_REQUIRE(m && arena && out, "%s: null argument", who);
    CONE_REQUIRE(!(flags & CONE_SESSION_CERTIFIED), "%s: CONE_SESSION_CERTIFIED libraries are not supported", who);
    CONE_REQUIRE(library_flags_ok(flags), "%s: flags=%d (0 or CONE_SESSION_BF16)", who, flags);
    CONE_REQUIRE(capacity >= 1 && capacity < (1ll << 31), "%s: capacity=%lld not in [1, 2^31)", who, (long long)capacity);
    CONE_REQUIRE(((uintptr_t)arena & (SES_ALIGN - 1)) == 0, "%s: the arena must be 256-B aligned", who);
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    CONE_REQUIRE(d.v_dim == d.v_motion_dim, "%s: the localizer feeds one clip feature to both sides, v_dim=%d != v_motion_dim=%d", who,
                 d.v_dim, d.v_motion_dim);
    const ArenaLayout A = arena_layout(d, capacity, flags);
    if (arena_bytes < A.total) { set_error("%s: arena too small (%zu < %zu)", who, arena_bytes, A.total); return CONE_E_WORKSPACE; }
    char* a = (char*)arena;
    *out = cone_library{m, capacity, flags, d.v_dim, d.hidden_dim, (float*)(a + A.vid_norm), A.has_f32 ? (float*)(a + A.adapted) : nullptr,
                        A.has_bf16 ? (uint16_t*)(a + A.adapted_bf16) : nullptr, (float*)(a + A.vproj),
                        A.has_qkv ? (float*)(a + A.qkv_vid) : nullptr};
    return 0;
}

extern "C" size_t cone_library_add_workspace(const cone_model* m, int64_t n_rows) {
    if (!m || n_rows <= 0) return 0;
    return index_ws(m, n_rows).total;
}

extern "C" int cone_library_add(const cone_model* m, const cone_library* lib, int64_t row0, const float* raw_clips, int64_t n_rows,
                                void* ws, size_t ws_bytes, void* stream) {
    const char* who = "library_add";
    CONE_REQUIRE(m && lib && raw_clips && ws, "%s: null argument", who);
    RUN(library_handle(who, m, lib));
    CONE_REQUIRE(library_flags_ok(lib->flags), "%s: bad library flags %d", who, lib->flags);
    CONE_REQUIRE(row0 >= 0 && n_rows >= 1 && row0 + n_rows <= lib->capacity, "%s: rows [%lld, %lld + %lld) are not inside [0, capacity=%lld)",
                 who, (long long)row0, (long long)row0, (long long)n_rows, (long long)lib->capacity);
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    CONE_REQUIRE(lib->v_dim == d.v_dim && lib->hidden_dim == d.hidden_dim, "%s: the library's row widths %d / %d are not the handle's %d / %d",
                 who, lib->v_dim, lib->hidden_dim, d.v_dim, d.hidden_dim);
    CONE_REQUIRE(lib->vid_norm && lib->vproj && (lib->flags & CONE_SESSION_BF16 ? lib->adapted_bf16 != nullptr : lib->adapted != nullptr),
                 "%s: the library handle misses a region (not one cone_library_open filled)", who);
    const IndexWs w = index_ws(m, n_rows);
    if (ws_bytes < w.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total); return CONE_E_WORKSPACE; }
    const size_t r = (size_t)row0, dv = (size_t)d.v_dim, dh = (size_t)d.hidden_dim;
    const IndexRows o{lib->vid_norm + r * dv, lib->adapted ? lib->adapted + r * dv : nullptr,
                      lib->adapted_bf16 ? lib->adapted_bf16 + r * dv : nullptr, nullptr, lib->vproj + r * dh,
                      lib->qkv_vid ? lib->qkv_vid + r * 3 * dh : nullptr};
    return index_rows(m, d, lib->flags, raw_clips, n_rows, o, (char*)ws, w, stream);
}

extern "C" size_t cone_library_localize_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                  const int32_t* q_ctx_l, const int32_t* tok_len, int nq, int K,
                                                  const cone_session_params* params) {
    const char* who = "library_localize";
    cone_model_dims d;
    LocalizeLayout L;
    if (library_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, K, params)) return 0;
    if (library_handle(who, m, lib) || cone_model_get_dims(m, &d)) return 0;
    const Resident S = resident_of(*lib);
    if (localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, K, 0, params, &L)) return 0;
    return L.total;
}

extern "C" int cone_library_localize(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                     const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                                     const cone_session_params* params, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes,
                                     void* stream) {
    const char* who = "library_localize";
    CONE_REQUIRE(m && lib && q_row0 && q_ctx_l && tok && tok_len && cls && params && kept && n_kept && ws, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    RUN(library_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, K, params));
    RUN(library_handle(who, m, lib));
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    const Resident S = resident_of(*lib);
    LocalizeLayout L;
    RUN(localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, K, 0, params, &L));
    CONE_REQUIRE(S.vid_norm && S.vproj && (S.flags & CONE_SESSION_BF16 ? S.adapted_bf16 != nullptr : S.adapted != nullptr),
                 "%s: the library handle misses a region (not one cone_library_open filled)", who);
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    return localize(who, m, d, S, lib->capacity, L, q_row0, q_ctx_l, tok, tok_len, nq, cls, K, 0, *params, kept, n_kept, nullptr,
                    (char*)ws, stream);
}


// ------------------------------------------------------------------------------ library search: the query half on scanned lists
namespace cone {

static int ranked_precheck(const char* who, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                           const int32_t* tok_len, int nq, int K, const cone_session_params* p) {
    RUN(library_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, K, p));
    CONE_REQUIRE(!(lib->flags & CONE_SESSION_BF16), "%s: CONE_SESSION_BF16 libraries are not supported", who);
    return 0;
}

}  // namespace cone

extern "C" size_t cone_library_localize_ranked_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                         const int32_t* q_ctx_l, const int32_t* tok_len, int nq, int K,
                                                         const cone_session_params* params) {
    const char* who = "library_localize_ranked";
    cone_model_dims d;
    LocalizeLayout L;
    if (ranked_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, K, params)) return 0;
    if (library_handle(who, m, lib) || cone_model_get_dims(m, &d)) return 0;
    const Resident S = resident_of(*lib);
    if (localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, K, 0, params, &L, true)) return 0;
    return L.total;
}

extern "C" int cone_library_localize_ranked(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                            const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                                            const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                            const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos,
                                            int scan_K, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "library_localize_ranked";
    RUN(ranked_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, K, params));
    CONE_REQUIRE(pair_query && pair_slot, "%s: null argument", who);
    CONE_REQUIRE(scan_nq >= 1 && scan_n_videos >= 1 && scan_K >= 1 && K <= scan_K, "%s: K=%d not in [1, scan_K=%d] (scan_nq=%d, scan_n_videos=%lld)",
                 who, K, scan_K, scan_nq, (long long)scan_n_videos);
    RankedLists lists{scan_widx, scan_wval, scan_n_videos, scan_K, {}};
    for (int q = 0; q < nq; ++q) {
        CONE_REQUIRE(pair_query[q] >= 0 && pair_query[q] < scan_nq, "%s: pair_query[%d]=%d not in [0, scan_nq=%d)", who, q, pair_query[q],
                     scan_nq);
        CONE_REQUIRE(pair_slot[q] >= 0 && pair_slot[q] < scan_n_videos, "%s: pair_slot[%d]=%d not in [0, scan_n_videos=%lld)", who, q,
                     pair_slot[q], (long long)scan_n_videos);
        lists.pairs.query[q] = pair_query[q];
        lists.pairs.slot[q] = pair_slot[q];
    }
    CONE_REQUIRE(m && tok && cls && scan_widx && scan_wval && kept && n_kept && ws, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    RUN(library_handle(who, m, lib));
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    const Resident S = resident_of(*lib);
    LocalizeLayout L;
    RUN(localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, K, 0, params, &L, true));
    CONE_REQUIRE(S.vid_norm && S.vproj && S.adapted, "%s: the library handle misses a region (not one cone_library_open filled)", who);
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    return localize(who, m, d, S, lib->capacity, L, q_row0, q_ctx_l, tok, tok_len, nq, cls, K, 0, *params, kept, n_kept, nullptr,
                    (char*)ws, stream, &lists);
}


// ------------------------------------------------------------------------------ library window budgets: a window count per pair
namespace cone {

// The refusals of a ragged call from host values alone, in this order: the library call's with K = 1 (every video has a window),
// then the counts; with lists, then what the ranked entry refuses.  *Kmax = the largest count.
static int ragged_precheck(const char* who, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                           const int32_t* tok_len, int nq, const int32_t* pair_k, const cone_session_params* p, bool ranked, int* Kmax) {
    RUN(library_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, 1, p));
    RUN(check_ragged(who, pair_k, q_ctx_l, nq, p->max_v_l, Kmax));
    CONE_REQUIRE(!ranked || !(lib->flags & CONE_SESSION_BF16), "%s: CONE_SESSION_BF16 libraries are not supported with a scan's lists", who);
    return 0;
}

}  // namespace cone

namespace cone {

static size_t ragged_workspace(const char* who, const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                               const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const int32_t* pair_k,
                               const cone_session_params* params, int ranked) {
    cone_model_dims d;
    LocalizeLayout L;
    int Kmax = 0;
    if (ragged_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, pair_k, params, ranked != 0, &Kmax)) return 0;
    if (library_handle(who, m, lib) || cone_model_get_dims(m, &d)) return 0;
    const Resident S = resident_of(*lib);
    if (localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, Kmax, 0, params, &L, ranked != 0, pair_k))
        return 0;
    return L.total;
}

// cone_library_localize_ragged (cand == NULL: kept / n_kept are the outputs) and cone_library_localize_candidates (cand is):
// the same refusals in the same order, the same launches up to cone_compose_rows.
static int ragged_call(const char* who, const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                       const float* tok, const int32_t* tok_len, int nq, const float* cls, const int32_t* pair_k,
                       const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                       const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K,
                       double* kept, int32_t* n_kept, float* cand, bool to_cand, void* ws, size_t ws_bytes, void* stream) {
    const bool ranked = pair_query || pair_slot || scan_widx || scan_wval;      // the lists come as a block: all of it or none
    int Kmax = 0;
    RUN(ragged_precheck(who, lib, q_row0, q_ctx_l, tok_len, nq, pair_k, params, ranked, &Kmax));
    RankedLists lists{scan_widx, scan_wval, scan_n_videos, scan_K, {}};
    if (ranked) {
        CONE_REQUIRE(pair_query && pair_slot, "%s: null argument", who);
        CONE_REQUIRE(scan_nq >= 1 && scan_n_videos >= 1 && scan_K >= 1 && Kmax <= scan_K,
                     "%s: max pair_k=%d not in [1, scan_K=%d] (scan_nq=%d, scan_n_videos=%lld)", who, Kmax, scan_K, scan_nq,
                     (long long)scan_n_videos);
        for (int q = 0; q < nq; ++q) {
            CONE_REQUIRE(pair_query[q] >= 0 && pair_query[q] < scan_nq, "%s: pair_query[%d]=%d not in [0, scan_nq=%d)", who, q,
                         pair_query[q], scan_nq);
            CONE_REQUIRE(pair_slot[q] >= 0 && pair_slot[q] < scan_n_videos, "%s: pair_slot[%d]=%d not in [0, scan_n_videos=%lld)", who, q,
                         pair_slot[q], (long long)scan_n_videos);
            lists.pairs.query[q] = pair_query[q];
            lists.pairs.slot[q] = pair_slot[q];
        }
        CONE_REQUIRE(scan_widx && scan_wval, "%s: null argument", who);
    }
    CONE_REQUIRE(m && tok && cls && (to_cand ? cand != nullptr : kept && n_kept) && ws, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    RUN(library_handle(who, m, lib));
    cone_model_dims d;
    RUN(cone_model_get_dims(m, &d));
    const Resident S = resident_of(*lib);
    LocalizeLayout L;
    RUN(localize_layout(who, "library", m, d, &S, lib->capacity, q_row0, q_ctx_l, tok_len, nq, Kmax, 0, params, &L, ranked, pair_k));
    CONE_REQUIRE(S.vid_norm && S.vproj && (S.flags & CONE_SESSION_BF16 ? S.adapted_bf16 != nullptr : S.adapted != nullptr),
                 "%s: the library handle misses a region (not one cone_library_open filled)", who);
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    return localize(who, m, d, S, lib->capacity, L, q_row0, q_ctx_l, tok, tok_len, nq, cls, Kmax, 0, *params, kept, n_kept, nullptr,
                    (char*)ws, stream, ranked ? &lists : nullptr, pair_k, to_cand ? cand : nullptr);
}

}  // namespace cone

extern "C" size_t cone_library_localize_ragged_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                         const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const int32_t* pair_k,
                                                         const cone_session_params* params, int ranked) {
    return cone::ragged_workspace("library_localize_ragged", m, lib, q_row0, q_ctx_l, tok_len, nq, pair_k, params, ranked);
}

extern "C" int cone_library_localize_ragged(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                            const float* tok, const int32_t* tok_len, int nq, const float* cls, const int32_t* pair_k,
                                            const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                            const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos,
                                            int scan_K, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream) {
    return cone::ragged_call("library_localize_ragged", m, lib, q_row0, q_ctx_l, tok, tok_len, nq, cls, pair_k, params, pair_query,
                             pair_slot, scan_widx, scan_wval, scan_nq, scan_n_videos, scan_K, kept, n_kept, nullptr, false, ws, ws_bytes,
                             stream);
}

// ------------------------------------------------------------------------------ library moment search: the call that ends at its candidates
extern "C" size_t cone_library_localize_candidates_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                             const int32_t* q_ctx_l, const int32_t* tok_len, int nq,
                                                             const int32_t* pair_k, const cone_session_params* params, int ranked) {
    return cone::ragged_workspace("library_localize_candidates", m, lib, q_row0, q_ctx_l, tok_len, nq, pair_k, params, ranked);
}

extern "C" int cone_library_localize_candidates(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                const int32_t* q_ctx_l, const float* tok, const int32_t* tok_len, int nq,
                                                const float* cls, const int32_t* pair_k, const cone_session_params* params,
                                                const int32_t* pair_query, const int32_t* pair_slot, const int32_t* scan_widx,
                                                const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K, float* cand,
                                                void* ws, size_t ws_bytes, void* stream) {
    return cone::ragged_call("library_localize_candidates", m, lib, q_row0, q_ctx_l, tok, tok_len, nq, cls, pair_k, params, pair_query,
                             pair_slot, scan_widx, scan_wval, scan_nq, scan_n_videos, scan_K, nullptr, nullptr, cand, true, ws, ws_bytes,
                             stream);
}
