// Video sessions (include/cone_hip.h, "video sessions"): one resident video, indexed once, answering batches of queries.
// Video libraries ("video libraries"): many videos in the rows of one arena, one call for queries on any mix of them.
// Library search ("library search"): the query half on the window lists of a cone_library_scan (csrc/prefilter.hip).
// Library window budgets ("library window budgets"): the query half with a window count per pair (cone_library_localize_ragged;
// the budget itself is csrc/library_budget.hip).
// Library moment search ("library moment search"): the ragged call that ends at its candidate rows
// (cone_library_localize_candidates; the pooled stage C is csrc/library_corpus.hip).
//
// Nothing is computed here.  cone_session_index / cone_library_add and the localize entries only SEQUENCE the library's own
// extern "C" launchers -- the calls cone_amd/localizator.py issues one by one through ctypes for
// run_on_video/cone_localizator.py:121-221 -- and carve their operands out of the caller's arena / workspace.
//
// The query half is ONE path.  Every size / run entry fills a QueryCall -- the descriptor that names everything such a call can
// carry -- and walks the same named steps in its own order: a precheck on host values (library_precheck, ranked_precheck,
// ragged_precheck), check_lists where a scan's lists come along, resolve (handle, dims, localize_layout, "misses a region",
// "workspace too small"), and for a run entry localize.  A _workspace twin is the same steps stopping after the layout.
// ONE layout kernel writes a call's index metadata (what the localizer keeps per shape in _const) from each query's
// (len, row0, ctx_l, k), which travel as kernel arguments: a session is row0 = 0 and one ctx_l, a uniform call is k = K.
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

// ------------------------------------------------------------------------------ the query half: the layout kernel
// Per query, as kernel arguments: token length, first arena row and clips of its video, window count.
struct QueryShape {
    int32_t len[CONE_SESSION_MAX_QUERIES], row0[CONE_SESSION_MAX_QUERIES], ctx_l[CONE_SESSION_MAX_QUERIES], k[CONE_SESSION_MAX_QUERIES];
};
// ctx_l: every query's clips where q_ctx_l is NULL (a session); K: every query's windows where pair_k is NULL (a uniform call)
static QueryShape shape_of(const int32_t* tok_len, const int32_t* q_row0, const int32_t* q_ctx_l, const int32_t* pair_k, int nq,
                           int64_t ctx_l, int K) {
    QueryShape P{};
    for (int q = 0; q < nq; ++q) {
        P.len[q] = tok_len[q];
        P.row0[q] = q_row0 ? q_row0[q] : 0;
        P.ctx_l[q] = q_ctx_l ? q_ctx_l[q] : (int32_t)ctx_l;
        P.k[q] = pair_k ? pair_k[q] : K;
    }
    return P;
}
// The arrays the kernel writes.  row_q / row_slot / cand_off: only a ragged call passes them (NULL: not written).
struct LayoutOut {
    int32_t *tok_off, *tok_len, *tok_idx, *q_ctx_l, *q_vid_off, *batch_pad, *full_w, *n_valid, *row_q, *row_slot;
    int64_t* cand_off;
};

// One workgroup.  Every output element has one writer; nothing outside the documented extents is touched:
// tok_off [0, nq], the per-query arrays [0, nq), tok_idx [0, sum of the lengths), and over the window rows -- the concatenation
// of the queries' k[q] rows, nq K of them in a uniform call -- full_w / row_q / row_slot [0, sum k).
// n_valid[q] = k[q] Nq, cand_off[q] = (rows before query q) Nq.
__global__ __launch_bounds__(256) void query_layout_kernel(QueryShape P, int nq, int max_q_l, int Kmax, int Nq, int W, LayoutOut o) {
    __shared__ int off[CONE_SESSION_MAX_QUERIES + 1];       // exclusive prefix sums of the token lengths
    __shared__ int woff[CONE_SESSION_MAX_QUERIES + 1];      // ... of the window counts
    __shared__ int len[CONE_SESSION_MAX_QUERIES];
    __shared__ int kq[CONE_SESSION_MAX_QUERIES];
    const int t = threadIdx.x;
    if (t == 0) {
        int a = 0, b = 0;
        for (int q = 0; q < nq; ++q) {
            off[q] = a; woff[q] = b; len[q] = P.len[q]; kq[q] = P.k[q];
            a += P.len[q]; b += P.k[q];
        }
        off[nq] = a; woff[nq] = b;
    }
    __syncthreads();
    for (int q = t; q < nq; q += blockDim.x) {
        o.tok_off[q] = off[q]; o.tok_len[q] = len[q];
        o.q_ctx_l[q] = P.ctx_l[q]; o.q_vid_off[q] = P.row0[q]; o.batch_pad[q] = W;
        o.n_valid[q] = kq[q] * Nq;
        if (o.cand_off) o.cand_off[q] = (int64_t)woff[q] * Nq;
    }
    if (t == 0) o.tok_off[nq] = off[nq];
    for (int i = t; i < nq * Kmax; i += blockDim.x) {
        const int q = i / Kmax, j = i - q * Kmax;
        if (j < kq[q]) {
            const int b = woff[q] + j;
            o.full_w[b] = W;
            if (o.row_q) { o.row_q[b] = q; o.row_slot[b] = j; }
        }
    }
    for (int i = t; i < nq * max_q_l; i += blockDim.x) {
        const int q = i / max_q_l, j = i - q * max_q_l;
        if (j < len[q]) o.tok_idx[off[q] + j] = j;
    }
}
static int launch_layout(const QueryShape& P, int nq, int max_q_l, int Kmax, int Nq, int W, const LayoutOut& o, void* stream) {
    hipLaunchKernelGGL(query_layout_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, P, nq, max_q_l, Kmax, Nq, W, o);
    CONE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------ the query half: the descriptor
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

// Everything a query-half call can carry.  An entry fills what it has -- the rest stays zero -- and the steps below read it.
struct QueryCall {
    const char *who, *what;                     // the entry's name in its messages; "session" / "library"
    const cone_model* model;
    cone_model_dims dims;                       // (resolve fills them)
    bool resident;                              // the caller passed a session / library: res and rows are its
    Resident res;
    int64_t rows;                               // the session's ctx_l, or the library's capacity
    const int32_t *q_row0, *q_ctx_l;            // per query, its video's first arena row and clips; NULL: a session (one video at row 0)
    const float* tok;
    const int32_t* tok_len;
    int nq;
    const float* cls;
    int K, n_cand;                              // windows per query (a ragged call: the largest count, ragged_precheck's)
    const cone_session_params* params;
    const int32_t* pair_k;                      // a window count per pair; NULL: a uniform call
    bool ranked;                                // stage A is a scan's: `lists` (a size entry knows only that much)
    const int32_t *pair_query, *pair_slot;      // as the caller passed them: check_lists vets them into lists.pairs
    int scan_nq;
    RankedLists lists;
    bool to_cand;                               // the call ends at its candidate rows: `cand` is the output, kept / n_kept are not touched
    double* kept;
    int32_t *n_kept, *certified;
    float* cand;
    void* ws;
    size_t ws_bytes;
    void* stream;
};

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

// Every buffer and every launcher's scratch of one call: the ONE function behind the workspace-size entries and the entries
// themselves.  Each take() is a region of its own.
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
static int localize_layout(const QueryCall& c, LocalizeLayout* out) {
    const char* who = c.who;
    const cone_model* m = c.model;
    const cone_model_dims& d = c.dims;
    const Resident* ses = &c.res;
    const cone_session_params* p = c.params;
    const int32_t* pair_k = c.pair_k;
    const int nq = c.nq, K = c.K;
    CONE_REQUIRE(m && c.resident && p, "%s: null argument", who);
    CONE_REQUIRE(ses->model == m, "%s: the %s was indexed with another handle", who, c.what);
    CONE_REQUIRE(flags_ok(ses->flags), "%s: bad %s flags %d", who, c.what, ses->flags);
    CONE_REQUIRE(ses->v_dim == d.v_dim && ses->hidden_dim == d.hidden_dim, "%s: the %s's row widths %d / %d are not the handle's %d / %d",
                 who, c.what, ses->v_dim, ses->hidden_dim, d.v_dim, d.hidden_dim);
    CONE_REQUIRE(p->max_v_l >= 2 && p->max_after >= 1 && p->max_before >= 1, "%s: bad params (max_v_l=%d, max_before=%d, max_after=%d)",
                 who, p->max_v_l, p->max_before, p->max_after);
    LocalizeLayout L{};
    RUN(check_queries(who, c.tok_len, nq, p->max_q_l, &L.T));
    const bool cert = (ses->flags & CONE_SESSION_CERTIFIED) != 0;
    size_t n_scores = 0;
    if (c.q_row0) {     // (library_precheck has vetted the pairs, K and the capacity)
        for (int q = 0; q < nq; ++q) {
            if (q == 0 || c.q_row0[q] != c.q_row0[q - 1] || c.q_ctx_l[q] != c.q_ctx_l[q - 1])
                L.runs[L.n_runs++] = Run{q, 0, c.q_row0[q], c.q_ctx_l[q], cone_num_windows(c.q_ctx_l[q], p->max_v_l), n_scores, 0, 0};
            Run& r = L.runs[L.n_runs - 1];
            r.n += 1;
            n_scores += (size_t)r.nw;
        }
    } else {
        CONE_REQUIRE(c.rows >= 1 && c.rows < (1ll << 31), "%s: ctx_l=%lld not in [1, 2^31)", who, (long long)c.rows);
        L.nw = cone_num_windows(c.rows, p->max_v_l);
        CONE_REQUIRE(K >= 1 && K <= L.nw && K <= 256, "%s: K=%d not in [1, min(num_window=%lld, 256)]", who, K, (long long)L.nw);
        L.runs[L.n_runs++] = Run{0, nq, 0, c.rows, L.nw, 0, 0, 0};
        n_scores = (size_t)nq * L.nw;
    }
    CONE_REQUIRE(c.n_cand >= 0, "%s: n_cand=%d", who, c.n_cand);
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
    if (!cert && !c.ranked) L.scores = r.take(n_scores * 4);      // (ranked: the lists come from a scan -- no stage A here)
    const size_t n_list = pair_k ? (size_t)nq * K : B;            // the call's (nq, K) window list
    L.widx = r.take(n_list * 4); L.wval = r.take(n_list * 4); L.cert = r.take(nq * 4);
    if (pair_k && !c.ranked) {      // every run ranks its video at the largest count among its pairs; the pairs take prefixes
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
        L.pf_bytes = cone_prefilter_topk_certified_workspace(c.rows, nq, p->max_v_l, K, c.n_cand);
        CONE_REQUIRE(L.pf_bytes, "%s: n_cand=%d is not a candidate count the certified pre-filter takes for %lld windows and K=%d", who,
                     c.n_cand, (long long)L.nw, K);
    } else if (!c.ranked) {
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
    return launch_layout(shape_of(tok_len, nullptr, nullptr, nullptr, nq, ctx_l, K), nq, max_q_l, K, Nq, max_v_l,
                         LayoutOut{tok_off, tok_len_dev, tok_idx, q_ctx_l, q_vid_off, batch_pad, full_w, n_valid, nullptr, nullptr, nullptr},
                         stream);
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
    return launch_layout(shape_of(tok_len, q_row0, q_ctx_l, nullptr, nq, 0, K), nq, max_q_l, K, Nq, max_v_l,
                         LayoutOut{tok_off, tok_len_dev, tok_idx, q_ctx_l_dev, q_vid_off, batch_pad, full_w, n_valid, nullptr, nullptr, nullptr},
                         stream);
}

namespace cone {

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

// The query half for both kinds of resident rows: c.q_row0 == NULL is a session (one video at row 0, c.rows clips), otherwise a
// library call (every query names its video's rows inside an arena of c.rows).  Nothing differs after stage A.
// c.pair_k != NULL is a ragged library call (c.K = the largest count): pair q owns pair_k[q] window rows, not K -- the layout
// kernel's row maps, a gather of every pair's prefix, then the row form of cone_window_table and the offset form of
// cone_fuse_nms.  The uniform calls run the launches they always ran.  c.to_cand (cone_library_localize_candidates): the call
// ends at its candidate rows, composed straight into c.cand; kept / n_kept are not touched.
static int localize(const QueryCall& c, const LocalizeLayout& L) {
    const cone_model* m = c.model;
    const cone_model_dims& d = c.dims;
    const Resident& S = c.res;
    const cone_session_params& P = *c.params;
    const RankedLists* lists = c.ranked ? &c.lists : nullptr;
    const int32_t* pair_k = c.pair_k;
    const float* cls = c.cls;
    void* stream = c.stream;
    char* w = (char*)c.ws;
    auto I = [&](size_t at) { return (int32_t*)(w + at); };
    auto F = [&](size_t at) { return (float*)(w + at); };
    auto scratch = [&](size_t at, size_t bytes) { return bytes ? (void*)(w + at) : nullptr; };
    const int nq = c.nq, K = c.K, W = P.max_v_l, Sl = P.max_v_l / 2, B = L.B, Nq = d.num_queries, dv = d.v_dim;
    const size_t col = align_up((size_t)B * 4, SES_ALIGN);
    int32_t *vid_row0 = I(L.wt), *vid_len = I(L.wt + col), *video_start = I(L.wt + 2 * col), *pad_len = I(L.wt + 3 * col),
            *txt_row0 = I(L.wt + 4 * col), *txt_len = I(L.wt + 5 * col), *cls_row = I(L.wt + 6 * col);

    if (pair_k)
        RUN(launch_layout(shape_of(c.tok_len, c.q_row0, c.q_ctx_l, pair_k, nq, 0, K), nq, P.max_q_l, K, Nq, W,
                          LayoutOut{I(L.tok_off), I(L.tok_len), I(L.tok_idx), I(L.q_ctx_l), I(L.q_vid_off), I(L.batch_pad), I(L.full_w),
                                    I(L.n_valid), I(L.row_q), I(L.row_slot), (int64_t*)(w + L.cand_off)},
                          stream));
    else if (c.q_row0)
        RUN(cone_library_query_layout(c.tok_len, c.q_row0, c.q_ctx_l, nq, P.max_q_l, K, Nq, W, I(L.tok_off), I(L.tok_len), I(L.tok_idx),
                                      I(L.q_ctx_l), I(L.q_vid_off), I(L.batch_pad), I(L.full_w), I(L.n_valid), stream));
    else
        RUN(cone_session_query_layout(c.tok_len, nq, P.max_q_l, c.rows, K, Nq, W, I(L.tok_off), I(L.tok_len), I(L.tok_idx), I(L.q_ctx_l),
                                      I(L.q_vid_off), I(L.batch_pad), I(L.full_w), I(L.n_valid), stream));
    RUN(cone_l2_normalize_rows(c.tok, L.T, d.t_dim, 1e-5f, 1, F(L.tok_norm), stream));                        // :133
    // stage A (:83-100, stable tie order): the raw cls vectors against the adapted rows
    if (lists && !pair_k) {     // a scan has ranked the windows (cone_library_scan: the same lists, bit for bit): copy each pair's
        hipLaunchKernelGGL(library_gather_lists_kernel, dim3((unsigned)((nq * K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           lists->pairs, nq, K, lists->n_videos, lists->scan_K, lists->widx, lists->wval, I(L.widx), F(L.wval));
        CONE_LAUNCH_CHECK();
    } else if (S.flags & CONE_SESSION_CERTIFIED) {
        RUN(cone_prefilter_topk_certified(S.adapted, S.adapted_bf16, c.rows, dv, cls, nq, W, Sl, K, c.n_cand, S.err, I(L.widx),
                                          F(L.wval), c.certified ? c.certified : I(L.cert), w + L.pf_ws, L.pf_bytes, stream));
    } else if (!lists) {
        for (int i = 0; i < L.n_runs; ++i) {        // one video a run, in the form and with the arguments of a session on it
            const Run& u = L.runs[i];
            float* scores = F(L.scores) + u.score_off;
            for (int q0 = 0; q0 < u.n; q0 += 4) {   // at most 4 queries a launch: the streaming form, whatever the run's length
                const int n = u.n - q0 < 4 ? u.n - q0 : 4;
                float* sc = scores + (size_t)q0 * u.nw;
                const float* cq = cls + (size_t)(u.q0 + q0) * dv;
                if (S.flags & CONE_SESSION_BF16)
                    RUN(cone_prefilter_scores_bf16(S.adapted_bf16 + (size_t)u.row0 * dv, u.ctx_l, dv, cq, n, W, Sl, sc, w + L.pf_ws,
                                                   L.pf_bytes, stream));
                else
                    RUN(cone_prefilter_scores(S.adapted + (size_t)u.row0 * dv, u.ctx_l, dv, cq, n, W, Sl, nullptr, sc, w + L.pf_ws,
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
                          I(L.q_vid_off), I(L.tok_off), I(L.tok_len), 0, 1, W, I(L.batch_pad), 0, nq, vid_row0, vid_len, video_start,
                          pad_len, txt_row0, txt_len, cls_row, stream));
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
                          c.to_cand ? c.cand : F(L.rows), stream));                                           // :191
    if (c.to_cand) return 0;    // the caller pools the candidates of many calls (cone_corpus_fuse_nms): the B * Nq rows, no stage C
    return cone_fuse_nms(F(L.rows), pair_k ? (const int64_t*)(w + L.cand_off) : nullptr, I(L.n_valid), nq, K * Nq, P.nms_thd,
                         P.max_before, P.max_after, c.kept, c.n_kept, I(L.nms_idx), stream);                  // :200-219
}

// ------------------------------------------------------------------------------ the query half: the steps of an entry
static bool library_flags_ok(int flags) { return flags == 0 || flags == CONE_SESSION_BF16; }

static int library_handle(const char* who, const cone_model* m, const cone_model* opened_with) {
    CONE_REQUIRE(m, "%s: null argument", who);
    CONE_REQUIRE(opened_with == m, "%s: the library was opened with another handle", who);
    return 0;
}

// The refusals a library call makes from host values alone, in this order, before the handle is looked at.  K: the window
// count every pair's video must have.
static int library_precheck(const QueryCall& c, int K) {
    CONE_REQUIRE(c.resident && c.q_row0 && c.q_ctx_l && c.tok_len && c.params, "%s: null argument", c.who);
    CONE_REQUIRE(!(c.res.flags & CONE_SESSION_CERTIFIED), "%s: CONE_SESSION_CERTIFIED libraries are not supported", c.who);
    CONE_REQUIRE(c.rows >= 1 && c.rows < (1ll << 31), "%s: capacity=%lld not in [1, 2^31)", c.who, (long long)c.rows);
    int64_t T = 0;
    RUN(check_queries(c.who, c.tok_len, c.nq, c.params->max_q_l, &T));
    return check_pairs(c.who, c.q_row0, c.q_ctx_l, c.nq, c.rows, K, c.params->max_v_l);
}
static int ranked_precheck(const QueryCall& c) {
    RUN(library_precheck(c, c.K));
    CONE_REQUIRE(!(c.res.flags & CONE_SESSION_BF16), "%s: CONE_SESSION_BF16 libraries are not supported", c.who);
    return 0;
}
// A ragged call's: the library call's with K = 1 (every video has a window), then the counts; with lists, then what the ranked
// entry refuses.  c.K = the largest count.
static int ragged_precheck(QueryCall& c) {
    RUN(library_precheck(c, 1));
    RUN(check_ragged(c.who, c.pair_k, c.q_ctx_l, c.nq, c.params->max_v_l, &c.K));
    CONE_REQUIRE(!c.ranked || !(c.res.flags & CONE_SESSION_BF16), "%s: CONE_SESSION_BF16 libraries are not supported with a scan's lists",
                 c.who);
    return 0;
}

// The scan's lists of a ranked call, as the caller passed them (after the precheck: c.K is known) -> c.lists.pairs.
static int check_lists(QueryCall& c) {
    const char* who = c.who;
    CONE_REQUIRE(c.pair_query && c.pair_slot, "%s: null argument", who);
    CONE_REQUIRE(c.scan_nq >= 1 && c.lists.n_videos >= 1 && c.lists.scan_K >= 1 && c.K <= c.lists.scan_K,
                 "%s: %s=%d not in [1, scan_K=%d] (scan_nq=%d, scan_n_videos=%lld)", who, c.pair_k ? "max pair_k" : "K", c.K,
                 c.lists.scan_K, c.scan_nq, (long long)c.lists.n_videos);
    for (int q = 0; q < c.nq; ++q) {
        CONE_REQUIRE(c.pair_query[q] >= 0 && c.pair_query[q] < c.scan_nq, "%s: pair_query[%d]=%d not in [0, scan_nq=%d)", who, q,
                     c.pair_query[q], c.scan_nq);
        CONE_REQUIRE(c.pair_slot[q] >= 0 && c.pair_slot[q] < c.lists.n_videos, "%s: pair_slot[%d]=%d not in [0, scan_n_videos=%lld)", who, q,
                     c.pair_slot[q], (long long)c.lists.n_videos);
        c.lists.pairs.query[q] = c.pair_query[q];
        c.lists.pairs.slot[q] = c.pair_slot[q];
    }
    CONE_REQUIRE(c.lists.widx && c.lists.wval, "%s: null argument", who);
    return 0;
}

// What only a run entry carries: the device pointers of the call and its workspace.
static int check_run_pointers(const QueryCall& c) {
    CONE_REQUIRE(c.model && c.tok && c.cls && (c.to_cand ? c.cand != nullptr : c.kept && c.n_kept) && c.ws, "%s: null argument", c.who);
    CONE_REQUIRE(((uintptr_t)c.ws & (SES_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", c.who);
    return 0;
}

// The handle, its dims and the call's layout; for a run entry (to_run) then the resident regions and the workspace's size.
static int resolve(QueryCall& c, LocalizeLayout* L, bool to_run) {
    if (c.q_row0) RUN(library_handle(c.who, c.model, c.res.model));
    RUN(cone_model_get_dims(c.model, &c.dims));
    RUN(localize_layout(c, L));
    if (!to_run) return 0;
    if (c.q_row0)
        CONE_REQUIRE(c.res.vid_norm && c.res.vproj && (c.res.flags & CONE_SESSION_BF16 ? c.res.adapted_bf16 != nullptr : c.res.adapted != nullptr),
                     "%s: the library handle misses a region (not one cone_library_open filled)", c.who);
    if (c.ws_bytes < L->total) { set_error("%s: workspace too small (%zu < %zu)", c.who, c.ws_bytes, L->total); return CONE_E_WORKSPACE; }
    return 0;
}

// What a size entry and its run entry both fill of a library call.
static QueryCall library_query(const char* who, const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                               const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const cone_session_params* params) {
    QueryCall c{};
    c.who = who; c.what = "library"; c.model = m;
    if (lib) { c.resident = true; c.res = resident_of(*lib); c.rows = lib->capacity; }
    c.q_row0 = q_row0; c.q_ctx_l = q_ctx_l; c.tok_len = tok_len; c.nq = nq; c.params = params;
    return c;
}
static QueryCall session_query(const cone_model* m, const cone_session* session, const int32_t* tok_len, int nq, int K, int n_cand,
                               const cone_session_params* params) {
    QueryCall c{};
    c.who = "session_localize"; c.what = "session"; c.model = m;
    if (session) { c.resident = true; c.res = resident_of(*session); c.rows = session->ctx_l; }
    c.tok_len = tok_len; c.nq = nq; c.K = K; c.n_cand = n_cand; c.params = params;
    return c;
}
// ... and what only the run entry adds.
static void run_on(QueryCall& c, const float* tok, const float* cls, void* ws, size_t ws_bytes, void* stream) {
    c.tok = tok; c.cls = cls; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
}
static void scan_lists(QueryCall& c, const int32_t* pair_query, const int32_t* pair_slot, const int32_t* scan_widx,
                       const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K) {
    c.pair_query = pair_query; c.pair_slot = pair_slot; c.scan_nq = scan_nq;
    c.lists.widx = scan_widx; c.lists.wval = scan_wval; c.lists.n_videos = scan_n_videos; c.lists.scan_K = scan_K;
}
static size_t size_of(int rc, const LocalizeLayout& L) { return rc ? 0 : L.total; }

// cone_library_localize_ragged and cone_library_localize_candidates (c.to_cand): the same refusals in the same order, the same
// launches up to cone_compose_rows.
static size_t ragged_size(QueryCall& c) {
    LocalizeLayout L;
    if (ragged_precheck(c)) return 0;
    return size_of(resolve(c, &L, false), L);
}
static int ragged_run(QueryCall& c) {
    c.ranked = c.pair_query || c.pair_slot || c.lists.widx || c.lists.wval;     // the lists come as a block: all of it or none
    RUN(ragged_precheck(c));
    if (c.ranked) RUN(check_lists(c));
    RUN(check_run_pointers(c));
    LocalizeLayout L;
    RUN(resolve(c, &L, true));
    return localize(c, L);
}

}  // namespace cone

extern "C" size_t cone_session_localize_workspace(const cone_model* m, const cone_session* session, const int32_t* tok_len, int nq,
                                                  int K, int n_cand, const cone_session_params* params) {
    if (!m) return 0;
    QueryCall c = session_query(m, session, tok_len, nq, K, n_cand, params);
    LocalizeLayout L;
    return size_of(resolve(c, &L, false), L);
}

extern "C" int cone_session_localize(const cone_model* m, const cone_session* session, const float* tok, const int32_t* tok_len,
                                     int nq, const float* cls, int K, int n_cand, const cone_session_params* params, double* kept,
                                     int32_t* n_kept, int32_t* certified, void* ws, size_t ws_bytes, void* stream) {
    QueryCall c = session_query(m, session, tok_len, nq, K, n_cand, params);
    run_on(c, tok, cls, ws, ws_bytes, stream);
    c.kept = kept; c.n_kept = n_kept; c.certified = certified;
    CONE_REQUIRE(c.resident && tok_len && params, "%s: null argument", c.who);
    RUN(check_run_pointers(c));
    LocalizeLayout L;
    RUN(resolve(c, &L, true));
    return localize(c, L);
}

// ------------------------------------------------------------------------------ video libraries

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
    RUN(library_handle(who, m, lib->model));
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
    QueryCall c = library_query("library_localize", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    c.K = K;
    LocalizeLayout L;
    if (library_precheck(c, K)) return 0;
    return size_of(resolve(c, &L, false), L);
}

extern "C" int cone_library_localize(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                     const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                                     const cone_session_params* params, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes,
                                     void* stream) {
    QueryCall c = library_query("library_localize", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    run_on(c, tok, cls, ws, ws_bytes, stream);
    c.K = K; c.kept = kept; c.n_kept = n_kept;
    CONE_REQUIRE(lib && q_row0 && q_ctx_l && tok_len && params, "%s: null argument", c.who);     // (this entry: pointers first)
    RUN(check_run_pointers(c));
    RUN(library_precheck(c, K));
    LocalizeLayout L;
    RUN(resolve(c, &L, true));
    return localize(c, L);
}

// ------------------------------------------------------------------------------ library search: the query half on scanned lists
extern "C" size_t cone_library_localize_ranked_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                         const int32_t* q_ctx_l, const int32_t* tok_len, int nq, int K,
                                                         const cone_session_params* params) {
    QueryCall c = library_query("library_localize_ranked", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    c.K = K; c.ranked = true;
    LocalizeLayout L;
    if (ranked_precheck(c)) return 0;
    return size_of(resolve(c, &L, false), L);
}

extern "C" int cone_library_localize_ranked(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                            const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                                            const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                            const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos,
                                            int scan_K, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream) {
    QueryCall c = library_query("library_localize_ranked", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    run_on(c, tok, cls, ws, ws_bytes, stream);
    c.K = K; c.kept = kept; c.n_kept = n_kept;
    c.ranked = true;
    scan_lists(c, pair_query, pair_slot, scan_widx, scan_wval, scan_nq, scan_n_videos, scan_K);
    RUN(ranked_precheck(c));
    RUN(check_lists(c));
    RUN(check_run_pointers(c));
    LocalizeLayout L;
    RUN(resolve(c, &L, true));
    return localize(c, L);
}

// ------------------------------------------------------------------------------ library window budgets: a window count per pair
extern "C" size_t cone_library_localize_ragged_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                         const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const int32_t* pair_k,
                                                         const cone_session_params* params, int ranked) {
    QueryCall c = library_query("library_localize_ragged", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    c.pair_k = pair_k; c.ranked = ranked != 0;
    return ragged_size(c);
}

extern "C" int cone_library_localize_ragged(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                            const float* tok, const int32_t* tok_len, int nq, const float* cls, const int32_t* pair_k,
                                            const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                            const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos,
                                            int scan_K, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream) {
    QueryCall c = library_query("library_localize_ragged", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    run_on(c, tok, cls, ws, ws_bytes, stream);
    c.pair_k = pair_k; c.kept = kept; c.n_kept = n_kept;
    scan_lists(c, pair_query, pair_slot, scan_widx, scan_wval, scan_nq, scan_n_videos, scan_K);
    return ragged_run(c);
}

// ------------------------------------------------------------------------------ library moment search: the call that ends at its candidates
extern "C" size_t cone_library_localize_candidates_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                             const int32_t* q_ctx_l, const int32_t* tok_len, int nq,
                                                             const int32_t* pair_k, const cone_session_params* params, int ranked) {
    QueryCall c = library_query("library_localize_candidates", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    c.pair_k = pair_k; c.ranked = ranked != 0;
    return ragged_size(c);
}

extern "C" int cone_library_localize_candidates(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                const int32_t* q_ctx_l, const float* tok, const int32_t* tok_len, int nq,
                                                const float* cls, const int32_t* pair_k, const cone_session_params* params,
                                                const int32_t* pair_query, const int32_t* pair_slot, const int32_t* scan_widx,
                                                const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K, float* cand,
                                                void* ws, size_t ws_bytes, void* stream) {
    QueryCall c = library_query("library_localize_candidates", m, lib, q_row0, q_ctx_l, tok_len, nq, params);
    run_on(c, tok, cls, ws, ws_bytes, stream);
    c.pair_k = pair_k; c.to_cand = true; c.cand = cand;
    scan_lists(c, pair_query, pair_slot, scan_widx, scan_wval, scan_nq, scan_n_videos, scan_K);
    return ragged_run(c);
}
