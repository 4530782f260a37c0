/*
 * cone_hip.h -- C ABI of libcone_hip.so: the MI355X (gfx950) implementation of CONE's
 * coarse-to-fine inference hot path.
 *
 * The reference (houzhijian/CONE) has no FFI: the path is plain Python calling torch.nn.
 * Each entry point below therefore names the reference *Python* site it replaces
 * (file:line relative to the reference repository).  A maintainer binds these with
 * ctypes (cone_amd/_lib.py is that binding).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer to fp32 / int32 / fp64 memory owned by the
 *     caller (torch tensors), row-major, densely packed unless a stride is given;
 *     cone_weights pointers may be host or device (copied once at cone_model_create);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on
 *     it, nothing synchronises, nothing allocates (scratch comes in through `ws`) -- except
 *     cone_model_create / cone_model_destroy, which allocate / free the handle's weight arena
 *     (hipMalloc + blocking copies) and therefore synchronise with the device;
 *   - return value 0 = success, negative = error (CONE_E_*), text in cone_last_error();
 *     nothing throws across the ABI;
 *   - a cone_model is immutable after creation (cone_model_set_option, a parity-test hook, is the
 *     one exception and must not race with calls on the handle): one handle may be used from several
 *     streams/threads concurrently as long as each call has its own workspace.  The library keeps no
 *     other mutable state besides the opt-in launch timer (cone_prof_*).
 */
#ifndef CONE_HIP_H
#define CONE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONE_HIP_ABI_VERSION 8

#define CONE_E_INVALID (-1)  /* bad argument / unsupported shape */
#define CONE_E_HIP (-2)      /* a HIP runtime call failed        */
#define CONE_E_WORKSPACE (-3) /* workspace too small             */

#define CONE_MAX_LAYERS 8
#define CONE_MAX_PROJ 3
#define CONE_TABLE_MAX_V_L 255 /* longest window (clips) the handle's own position tables cover */
#define CONE_MAX_WINDOW_TOKENS 256 /* clips + text tokens of one window (WINDOW_LENGTH + max_q_l of the reference's scripts): the
                                    * limit of a handle as created, and of the fused kernels (position tables, layer-0 caches,
                                    * fused tails, folded cross-attention) */
#define CONE_MAX_LONG_WINDOW_TOKENS 1024 /* the limit a handle can be raised to (cone_model_set_option "max_window_tokens"): such a
                                          * handle runs every forward on the general path with the streaming attention core */

typedef struct cone_model cone_model;

/* torch.nn.Linear: weight [out][in], bias [out] */
typedef struct { const float* w; const float* b; } cone_linear_w;
/* torch.nn.LayerNorm: weight, bias (eps 1e-5) */
typedef struct { const float* g; const float* b; } cone_ln_w;
/* torch.nn.MultiheadAttention: packed in_proj [3d][d] rows Wq|Wk|Wv, in_proj_bias [3d] */
typedef struct { const float* in_proj_w; const float* in_proj_b; cone_linear_w out_proj; } cone_mha_w;
typedef struct { cone_mha_w self_attn; cone_linear_w linear1, linear2; cone_ln_w norm1, norm2; } cone_enc_layer_w;
typedef struct {
    cone_mha_w self_attn, cross_attn;
    cone_linear_w linear1, linear2;
    cone_ln_w norm1, norm2, norm3;
} cone_dec_layer_w;

/* The tensors of CONE.state_dict() (cone/model.py:19-80) that inference reads. */
typedef struct {
    int32_t hidden_dim, nheads, dim_ff, enc_layers, dec_layers, num_queries;
    int32_t n_input_proj, t_dim, v_dim, has_adapter;   /* v_dim: APPEARANCE clip features (pre-filter, proposal matching,
                                                        * adapter: cone/model.py:80, 186-208)                             */
    int32_t v_motion_dim;                              /* MOTION clip features = the window model's video input
                                                        * (input_vid_proj: cone/model.py:67); equal to v_dim in every
                                                        * shipped script (one LMDB serves both: cone/ego4d_mad_dataloader.py:77) */
    cone_ln_w vid_proj_ln[CONE_MAX_PROJ]; cone_linear_w vid_proj[CONE_MAX_PROJ]; /* input_vid_proj.{i} */
    cone_ln_w txt_proj_ln[CONE_MAX_PROJ]; cone_linear_w txt_proj[CONE_MAX_PROJ]; /* input_txt_proj.{i} */
    cone_enc_layer_w enc[CONE_MAX_LAYERS];   /* transformer.encoder.layers.{i} */
    cone_dec_layer_w dec[CONE_MAX_LAYERS];   /* transformer.decoder.layers.{i} */
    cone_ln_w dec_norm;                      /* transformer.decoder.norm        */
    const float* query_embed;                /* query_embed.weight [Nq][d]      */
    cone_linear_w class_embed;               /* [2][d]                          */
    cone_linear_w span_embed[3];             /* span_embed.layers.{0,1,2}       */
    cone_linear_w saliency_proj;             /* [1][d]                          */
    cone_linear_w adapter[2];                /* adapter_layer.layers.{0,1}      */
    const float* pos_dim_t;                  /* [d] temperature**(2*(i//2)/d), cone/position_encoding.py:66-67 */
    /* (ABI 5) --use_txt_pos (cone/config.py:115, cone/model.py:106): the position term of text token t of a query is
     * TrainablePositionalEncoding(src_txt) = LayerNorm(src_txt[t] + position_embeddings[t]) (cone/position_encoding.py:10-32).
     * txt_pos_embed = txt_position_embed.position_embeddings.weight [txt_pos_rows = max_q_l][d], txt_pos_ln its LayerNorm;
     * NULL = the option is off (every shipped configuration): text tokens carry a zero position term.  (ABI 7) With it set the
     * forward runs the table path when it gets the tokens' own position rows (cone_layer0.txt_pos / txt_pos_qk from
     * cone_layer0_text_positions; cone_forward_windows builds them itself), otherwise the general path (x + pos materialised
     * per token). */
    const float* txt_pos_embed; int32_t txt_pos_rows; cone_ln_w txt_pos_ln;
    /* (ABI 5) --pre_norm (cone/config.py:120 -> normalize_before, cone/transformer.py:19-36): pre_norm != 0 = every layer
     * normalises its input (forward_pre) and the encoder ends with enc_norm = transformer.encoder.norm, which exists only
     * then.  0 (every shipped configuration) = post-norm.  (ABI 6) such a model runs the table path as well: the fused layer
     * tail in its pre-norm form, first-layer row caches of in_proj(norm1(row)), the folded decoder cross-attention. */
    int32_t pre_norm; cone_ln_w enc_norm;
    /* (ABI 8) The longest window, in clips, this checkpoint is run on = max_v_l of build_model (cone/model.py:468-486,
     * WINDOW_LENGTH of the reference's scripts): cone_model_create builds the handle's position tables for windows of up to
     * this many clips (row lv (lv - 1) / 2 + p: a shorter bound is a prefix of a longer one; 4 096 rows = 21 MB for 90 clips
     * with two encoder layers, 32 641 rows = 167 MB for 255).  0 = CONE_TABLE_MAX_V_L.  Longer windows still run, on the
     * general path (x + pos materialised), or on tables the caller brings (cone_pos_tables, cone_layer0). */
    int32_t table_max_v_l;
} cone_weights;

const char* cone_last_error(void);
int cone_abi_version(void);

/* build_model + load_state_dict (cone/model.py:468-521, cone/inference.py:525-527). */
int cone_model_create(const cone_weights* w, cone_model** out);
void cone_model_destroy(cone_model* m);

/* ------------------------------------------------------------------ stage A: pre-filter */

/* A2, cone/inference.py:254-258: out = adapter(x)+x, then (renorm != 0) out /= ||out||_2 (no eps), row-wise;
 * renorm == 0 is the single-video localizer's form (run_on_video/cone_localizator.py:135-138).
 * x,out (n_rows, v_dim).  ws >= cone_adapter_norm_workspace(m, n_rows) bytes. */
size_t cone_adapter_norm_workspace(const cone_model* m, int64_t n_rows);
int cone_adapter_norm(const cone_model* m, const float* x, int64_t n_rows, float* out, int renorm,
                      void* ws, size_t ws_bytes, void* stream);

/* Row-wise L2 normalisation.  clamp == 0: x / (||x||_2 + eps) = l2_normalize_np_array
 * (utils/basic_utils.py:97-99); clamp != 0: x / max(||x||_2, eps) = torch.nn.functional.normalize
 * (run_on_video/cone_localizator.py:129-133). */
int cone_l2_normalize_rows(const float* x, int64_t n_rows, int dim, float eps, int clamp, float* out, void* stream);

/* A3+A4, cone/inference.py:284-296: frame_scores[q][f] = <vid[f], txt[q]>;
 * win_scores[q][i] = max(frame_scores[q][max((i-1)S,0) : min((i-1)S+W, ctx_l)]),
 * num_window = ceil(ctx_l/S)+1, S = W/2.  vid (ctx_l,dv), txt (nq,dv), win_scores (nq,num_window).
 * The window max is fused into the frame-score stream (a running max per half window of S frames; each frame belongs
 * to two windows), so the (nq,ctx_l) frame-score matrix -- which the reference computes only to take this max -- is
 * OPTIONAL: frame_scores may be NULL (nothing of that size is written), or receives the scores as before.
 * ws >= cone_prefilter_scores_workspace(ctx_l, nq, W) bytes (two floats per query and half window).
 * Forms (chosen by nq): 1 - 4 queries stream the clip rows once with non-temporal loads, the query vectors in registers (a
 * query's bits do not depend on the others of the launch); 5 or more run fp32-MFMA tiles of 16 / 32 / 64 queries per pass
 * (another summation order: ~1e-7 relative).
 * NaN: a NaN frame score is skipped by the window max, and a window with no number scores -inf -- nanmax, or -inf where there
 * is no number.  This is the documented deviation from torch.max, which would return NaN; the frame-score matrix itself keeps
 * the NaN.  It holds for every form (this entry, cone_prefilter_scores_split, cone_prefilter_batched and the bf16 entries).
 * Every fp32 form stays within dv u / (1 - dv u) sum_c |a_c b_c| + u |score| of the float64 score, u = 2^-24
 * (tests/test_prefilter_kernels_gpu.py). */
int64_t cone_num_windows(int64_t ctx_l, int W);
size_t cone_prefilter_scores_workspace(int64_t ctx_l, int nq, int W);
int cone_prefilter_scores(const float* vid, int64_t ctx_l, int dv, const float* txt, int nq,
                          int W, int S, float* frame_scores, float* win_scores, void* ws, size_t ws_bytes,
                          void* stream);

/* OPT-IN form of cone_prefilter_scores without the frame-score matrix: 8 or more queries over one video run on the bf16
 * matrix cores, every fp32 product as six partial products of three-piece bf16 operands with fp32 accumulation -- the
 * accuracy of the exact-fp32 MFMA chain (tools/probe/split_bf16_probe.hip) at a rate that leaves the 64-query stream
 * HBM-bound instead of matrix-pipe-bound.  Fewer than 8 queries take cone_prefilter_scores' own kernels (1 - 4: the streaming
 * kernel; 5 - 7: one 16-query tile of the exact-fp32 matrix-core kernel).
 * ws >= cone_prefilter_scores_split_workspace(...) bytes (the score planes + the split query image).  The default path
 * (cone_prefilter_scores, cone/inference.py's drop-in) stays exact fp32. */
size_t cone_prefilter_scores_split_workspace(int64_t ctx_l, int nq, int W, int dv);
int cone_prefilter_scores_split(const float* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W, int S,
                                float* win_scores, void* ws, size_t ws_bytes, void* stream);

/* A4, cone/inference.py:297-299 (+ [:topk], cone/ego4d_mad_dataloader.py:146): the first k entries
 * of the descending sort of each row of win_scores (nq,num_window); ties -> lower window index
 * first (stable order; -0.0 and +0.0 tie).  idx (nq,k) int32, val (nq,k) fp32 (val may be NULL).
 * NaN scores: a NaN is NEVER selected, in either form below -- the list is the stable descending order of the row's
 * numbers (+-inf included); a row with fewer than k numbers ends in (idx -1, val -inf) padding.
 * (cone_prefilter_batched ranks its short rows -- at most 1 024 windows -- by counting instead, and that ranking orders a NaN
 * FIRST, ahead of every number, as torch.sort does, so that its ranks stay a permutation.  The two rules never meet: window
 * scores produced by this library are never NaN -- the window max skips NaN frame scores, a window of NaN frames scores
 * -inf.  tests/test_index_kernels_gpu.py pins both.) */
int cone_topk_windows(const float* win_scores, int nq, int64_t num_window, int k,
                      int32_t* idx, float* val, void* stream);
/* The same with caller-owned scratch: rows longer than 8 192 windows (MAD scale) run as a two-level selection -- a
 * stable top-k per 4 096-window chunk (per-wave selection out of registers, no barrier inside the passes), then a merge of the chunk lists (same order, bit for bit) -- instead
 * of k passes over the whole row.  ws >= cone_topk_windows_workspace(...) bytes (0 for short rows). */
size_t cone_topk_windows_workspace(int nq, int64_t num_window, int k);
int cone_topk_windows_ws(const float* win_scores, int nq, int64_t num_window, int k, int32_t* idx, float* val,
                         void* ws, size_t ws_bytes, void* stream);

/* A3+A4 for a whole split in three launches.  The clip features of all videos sit back to back in
 * `arena` (rows, dv).  A group g = one video (rows g_row0[g] .. +g_ctx_l[g]) and up to 4 of its
 * queries g_q[g][0..3] (indices into cls (nq,dv); -1 = unused slot), so a video's rows are read once
 * per group.  Query q writes its frame scores at frame_scores + q_fs_off[q] (q_ctx_l[q] values) and its
 * window scores at win_scores + q_win_off[q]; topk_idx (nq,k) receives the first k windows of the
 * stable descending order, padded with -1 when the video has fewer than k windows.
 * max_ctx_l bounds every ctx_l (host-known, sizes the grid). */
int cone_prefilter_batched(const float* arena, int dv, const float* cls, const int64_t* g_row0,
                           const int32_t* g_ctx_l, const int32_t* g_q, int ng, int max_ctx_l,
                           const int64_t* q_fs_off, const int64_t* q_win_off, const int32_t* q_ctx_l,
                           int nq, int W, int S, float* frame_scores, float* win_scores, int k,
                           int32_t* topk_idx, void* stream);

/* ---- OPT-IN bf16 pre-filter (additive in ABI 8): bf16 context rows, bf16 operands, fp32 accumulation.
 * ONE arithmetic contract for every entry and every kernel form below:
 *     score[q][f] = sum_c bf16(ctx[f][c]) * bf16(cls[q][c])
 * both operands rounded ONCE, round to nearest even (the context rows by the producers below, the query vectors by the
 * scoring kernels -- the few-query streaming form rounds them too, so a query's ranks do not depend on how many queries
 * share its launch beyond a summation order); every product is exact in fp32, the sum is fp32 in the form's own order.
 * Window scores are the max over the same frame ranges as cone_prefilter_scores: win[i] = max over frames
 * [max((i-1)S,0), min((i-1)S+W, ctx_l)) = max(hm[i-1], hm[i], W odd ? score of frame (i+1)S : -inf) with hm[h] the max over
 * half window h = frames [hS, (h+1)S) -- the half windows that exist, 0 <= h < ceil(ctx_l/S).  No frame-score matrix.
 * NOT fp32-accurate: each operand carries a relative error of up to 2^-9, a score of unit-norm rows an absolute error of up
 * to ~2^-8; a pre-filter only RANKS windows, which is why a caller may accept that for half the arena bytes (and twice the
 * video length per GB).  The defaults (cone_prefilter_scores, cone_prefilter_batched) stay exact fp32.
 * Named checks: dv a multiple of 32 and <= 1024 (the model's own rule); the bf16 arena 16-B aligned. */

/* out = bf16_rne(x), x (n_rows, dim) fp32, dim a multiple of 4: for callers that index a resident video once (what
 * cone/inference.py:254-258 recomputes per call) and query it many times. */
int cone_rows_to_bf16(const float* x, int64_t n_rows, int dim, uint16_t* out, void* stream);

/* cone_adapter_norm (A2, cone/inference.py:254-258; renorm == 0: run_on_video/cone_localizator.py:135-138) whose LAST stage
 * stores bf16: out = bf16_rne(the fp32 value cone_adapter_norm stores), bit for bit.  With renorm != 0 the L2 norm's own
 * store is the bf16 one: the normalised fp32 rows are never written.  ws >= cone_adapter_norm_workspace(m, n_rows). */
int cone_adapter_norm_bf16(const cone_model* m, const float* x, int64_t n_rows, uint16_t* out, int renorm,
                           void* ws, size_t ws_bytes, void* stream);

/* A3+A4, cone/inference.py:284-296, under the contract above, for all queries of one video: vid (ctx_l,dv) bf16,
 * txt (nq,dv) fp32 (rounded here), win_scores (nq,num_window) fp32.  Forms (chosen by nq): 1 - 4 queries stream the rows
 * once (16-B non-temporal lane loads of 8 bf16, widened by a shift; a query's bits do not depend on the others of the
 * launch); 5 or more run v_mfma_f32_16x16x32_bf16 tiles of 16 / 32 / 64 queries per pass (another summation order).
 * ws >= cone_prefilter_scores_bf16_workspace(ctx_l, nq, W) bytes. */
size_t cone_prefilter_scores_bf16_workspace(int64_t ctx_l, int nq, int W);
int cone_prefilter_scores_bf16(const uint16_t* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W, int S,
                               float* win_scores, void* ws, size_t ws_bytes, void* stream);

/* A3+A4 for a whole split (cone/inference.py:276-301) under the contract above: cone_prefilter_batched with a bf16 arena
 * and without the frame scores (no q_fs_off / frame_scores).  Every group runs the streaming form: a query's window scores
 * are those of cone_prefilter_scores_bf16 with 1 - 4 queries on the same rows, bit for bit.  win_scores and topk_idx as
 * in cone_prefilter_batched. */
int cone_prefilter_batched_bf16(const uint16_t* arena, int dv, const float* cls, const int64_t* g_row0,
                                const int32_t* g_ctx_l, const int32_t* g_q, int ng, int max_ctx_l,
                                const int64_t* q_win_off, const int32_t* q_ctx_l, int nq, int W, int S,
                                float* win_scores, int k, int32_t* topk_idx, void* stream);

/* ---- OPT-IN certified pre-filter (additive in ABI 8): the bf16 scan's bytes, the exact-fp32 path's top-k windows.
 * For callers that index a video once and query it many times.  The fp32 rows stay resident BESIDE their bf16 shadow (1.5 x
 * the fp32 bytes).  Per call: the coarse window scores off the shadow (cone_prefilter_scores_bf16's forms, unchanged), the
 * n_cand best of them, those candidates' window scores again in the fp32 streaming form's own arithmetic, and a proof
 * per query, on the device, that no window outside the candidates can enter the top-k; a query whose proof fails gets the
 * full fp32 scan, still on the device.  One stream, no host read-back: the call can be captured in a graph.
 * A note on the contract above: round-to-nearest-even into bf16 (8 significand bits) has a worst relative error of
 * 2^-8 / (1 + 2^-8) per operand -- fp32 1 + 2^-8 rounds to 1.0 --, not the 2^-9 stated there.  Nothing here relies on
 * either figure: the index measures the rounding residual of the rows it stores. */

/* cone_rows_to_bf16 (the same bits in `out`) that also measures the shadow: err[0] = R >= max over rows of |x_f - bf16(x_f)|,
 * err[1] = N >= max over rows of max(|x_f|, |bf16(x_f)|) (2-norms; device memory, 2 floats, initialised here).  fp32 sums,
 * inflated by (1 + 2^-10) + 2^-55 over their own rounding and underflow.  A non-finite row (or one that rounds to a
 * non-finite bf16 row) makes R or N non-finite: queries on that index are never certified (and still answered exactly).
 * dim a multiple of 4, <= 16384. */
int cone_prefilter_index_bf16(const float* x, int64_t n_rows, int dim, uint16_t* out, float* err, void* stream);

/* The certified top-k.  vid_f32 (ctx_l,dv) fp32 and vid_bf16 = its shadow with err = its measures (cone_prefilter_index_bf16),
 * txt (nq,dv) fp32; dv in {256,512,768,1024} (the fp32 streaming form's rule); k <= 256.  n_cand = candidates per query:
 * 0 = the default min(num_window, max(4 k, 128)); otherwise min(k, num_window) <= n_cand <= min(num_window, 4096) (named
 * check: what the top-k entries support for one selection; while n_cand * ceil(num_window / 4096) <= 4096 the candidates are
 * selected as an unordered set in microseconds, past that by cone_topk_windows_ws, whose one-level form costs n_cand passes
 * over the row).  Outputs: idx (nq,k) int32, val (nq,k) fp32 = the fp32 window
 * scores, laid out and padded like cone_topk_windows' ((-1, -inf) where the row has fewer than k numbers; k may exceed
 * num_window here), certified (nq) int32.
 * CONTRACT: idx / val are those of cone_topk_windows on cone_prefilter_scores called with that query ALONE (the streaming
 * form), bit for bit, whatever certified[q] says.  certified[q] = 1: the query was answered from the bf16 scan and n_cand
 * rescored windows (every window is a candidate, or t - c_last > E(q) strictly with all quantities finite: t = the k-th
 * exact score, c_last = the smallest coarse score among the candidates,
 *     E(q) = (R |qh| + N |qh - q| + 2 g N max(|q|, |qh|)) (1 + 2^-10) + 2^-114 (1 + |qh| + N),
 * qh = bf16(q), g = (dv+1) u / (1 - (dv+1) u), u = 2^-24: a bound on |coarse - exact| of every window in any summation order,
 * DESIGN.md 3d).  certified[q] = 0: near-ties, too few candidates or non-finite data; the query's group of up to 4 queries
 * ran the full fp32 scan (a group of certified queries returns after reading the flags).
 * TRUST: the entry cannot check that its three arenas belong together -- it trusts that vid_bf16 and err are what
 * cone_prefilter_index_bf16 produced from vid_f32; with any other shadow or measures the proof, and with it the contract, is void.
 * ws >= cone_prefilter_topk_certified_workspace(ctx_l, nq, W, k, n_cand) bytes. */
size_t cone_prefilter_topk_certified_workspace(int64_t ctx_l, int nq, int W, int k, int n_cand);
int cone_prefilter_topk_certified(const float* vid_f32, const uint16_t* vid_bf16, int64_t ctx_l, int dv, const float* txt,
                                  int nq, int W, int S, int k, int n_cand, const float* err, int32_t* idx, float* val,
                                  int32_t* certified, void* ws, size_t ws_bytes, void* stream);

/* A5, eval branch of StartEndDataset.__getitem__ + collate (cone/ego4d_mad_dataloader.py:144-159, 229-234, 305-344) as
 * index arithmetic: win_idx (nq, K) int32 holds the ranked window indices of every query, valid entries first (a video of
 * fewer than K windows: the tail is -1 and never read).  Row b of every output is (query row_q[b], rank slot row_slot[b])
 * -- n_rows rows in annotation order, then rank order: the shape of the list is host metadata, a query owns
 * min(K, ceil(ctx_l / S) + 1) windows (cone/inference.py:286-299, cone/ego4d_mad_dataloader.py:146) -- or, with
 * row_q == row_slot == NULL and n_rows == nq * K, the dense list (b / K, b % K).  Per-query metadata: q_ctx_l (clips of the
 * query's video), q_vid_off (first arena
 * row of that video), tok_off / tok_len (the query's text rows).  Outputs (n_rows) int32 each: vid_row0, vid_len,
 * video_start (window i covers clips [max(0, (i-1) S), min(ctx_l, (i-1) S + max_v_l)), S = max_v_l / 2), txt_row0,
 * txt_len, cls_row, and pad_len = the zero-padded clip length of the window's reference batch -- the longest window among
 * the eval_bsz consecutive queries of the SPLIT it belongs to (hazard H3: cone/model.py:186-199 divides by a length
 * clipped to it).  batch_pad (n_batches) int32 is that table, indexed by (q_base + query) / eval_bsz with q_base = the
 * first query's index in the split: derive_pad != 0 computes it from these windows (only the reference's when the
 * queries are whole reference batches -- the caller's responsibility), derive_pad == 0 reads the split's table. */
int cone_window_table(const int32_t* win_idx, int nq, int K, const int32_t* row_q, const int32_t* row_slot, int n_rows,
                      const int32_t* q_ctx_l, const int32_t* q_vid_off,
                      const int32_t* tok_off, const int32_t* tok_len, int q_base, int eval_bsz, int max_v_l,
                      int32_t* batch_pad, int derive_pad, int n_batches, int32_t* vid_row0, int32_t* vid_len,
                      int32_t* video_start, int32_t* pad_len, int32_t* txt_row0, int32_t* txt_len, int32_t* cls_row,
                      void* stream);

/* --------------------------------------------------------- stage B: intra-window model */

/* A6, cone/model.py:100-101 (input_vid_proj / input_txt_proj): row-wise LN->Linear->ReLU->LN->Linear.
 * which: 0 = video (v_motion_dim in), 1 = text (t_dim in).  x (n_rows,din), out (n_rows,d). */
size_t cone_project_workspace(const cone_model* m, int which, int64_t n_rows);
int cone_project_tokens(const cone_model* m, int which, const float* x, int64_t n_rows, float* out,
                        void* ws, size_t ws_bytes, void* stream);

/* Optional taps for parity bisecting; any pointer may be NULL. */
typedef struct {
    float* memory;     /* (B, Lv_pad+Lq_pad, d): encoder output, valid tokens only, rest 0 */
    float* hs;         /* (dec_layers, B, Nq, d): decoder outputs after decoder.norm         */
    float* aux_logits; /* (dec_layers-1, B, Nq, 2)                                          */
    float* aux_spans;  /* (dec_layers-1, B, Nq, 2)                                          */
} cone_taps;

/* A6-A11, CONE.forward (cone/model.py:82-128) on zero-padded tensors exactly as
 * prepare_batch_inputs delivers them: vid (B,Lv_pad,v_motion_dim), txt (B,Lq_pad,t_dim); masks are prefix
 * masks given as valid lengths vid_len[B], txt_len[B] (int32, device).
 * (ABI 6) The batch is compacted first -- the valid clip / token rows are gathered by the first LayerNorm of their input
 * projection, padding is never projected -- the projections and the first encoder layer's q | k | v rows run once per compact
 * row (device-side row counts), and the windows enter the packed forward below as (row0, len) pairs with those row caches:
 * the SAME launches as the eval driver's arena path (gathering first layer, the handle's position tables, fused layer tails,
 * folded decoder cross-attention), the same bits for the same windows.  Lv_pad + Lq_pad <= CONE_MAX_WINDOW_TOKENS, or the
 * handle's "max_window_tokens" option where that was raised (then both entries are the general path, still one path).
 * Outputs: logits (B,Nq,2), spans (B,Nq,2) = sigmoid(center,width), saliency (B,Lv_pad; may be NULL: the
 * saliency head is then skipped -- cone/inference.py computes and never reads it, :54-59; likewise the heads and
 * decoder.norm of the intermediate decoder layers run only when taps ask for hs / aux_logits / aux_spans)
 * (entries at padded clips are written as 0; the reference leaves them unspecified/unused).
 * CONTRACT (lengths): 0 <= vid_len[b] <= Lv_pad and 0 <= txt_len[b] <= Lq_pad are TRUSTED, not checked: the lengths live on
 * the device.  The compact row offsets are the prefix sums of the lengths as given, while the source-row lists are written
 * for min(len, pad) rows per window, so a longer length leaves rows of the compact lists unwritten (read as stale workspace)
 * and lets the packed forward read past the window's rows.  cone_mask_lengths of an (B, L_pad) mask cannot exceed L_pad; a
 * caller that builds the lengths itself checks them on the host, as cone_criterion_forward's caller checks tgt_off.
 * CONTRACT (batch): B is at most the device's maxGridSize[1] (the per-window kernels put the window index in gridDim.y); a
 * larger B is refused by name ("... exceed the device's grid limit ...") before anything is launched or written.  The same
 * holds for cone_forward_packed.  Split such a batch into several calls. */
size_t cone_forward_workspace(const cone_model* m, int B, int Lv_pad, int Lq_pad);
int cone_forward_windows(const cone_model* m, const float* vid, const int32_t* vid_len,
                         const float* txt, const int32_t* txt_len, int B, int Lv_pad, int Lq_pad,
                         float* logits, float* spans, float* saliency, const cone_taps* taps,
                         void* ws, size_t ws_bytes, void* stream);

/* Valid lengths of the reference's prefix masks (pad_sequences_1d, utils/tensor_utils.py:50-52: 1 = valid, (B, L) fp32):
 * len[b] = sum_j mask[b][j] as int32 -- the vid_len / txt_len arguments of the two entry points above. */
int cone_mask_lengths(const float* mask, int B, int L, int32_t* len, void* stream);

/* Same computation on already-projected token arenas (cone_project_tokens outputs), windows given
 * by index: window b = vproj rows [vid_row0[b], +vid_len[b]) followed by tproj rows
 * [txt_row0[b], +txt_len[b]).  This is how the eval driver avoids re-projecting the clips shared by
 * overlapping windows and the text replicated across a query's windows.
 * Lv_max/Lq_max bound the lengths (host-known); saliency is (B, Lv_max). */
/* Optional row caches (+ caller-owned position tables).  Everything ahead of the first attention is row-wise, and the
 * position term enters every attention through a LINEAR map, so it can be split off and tabulated:
 *   (x + pos) W^T + b = (x W^T + b) + pos W^T.
 * qkv_vid (n_clips, 3d) / qkv_txt (n_tokens, 3d) = cone_layer0_project of the projected arenas: the FIRST encoder
 *   layer's in_proj once per clip / per text token instead of once per window row (two M-row GEMMs, ~10 % of the
 *   FLOPs, become a gather inside the attention kernel);
 * pos_rows (R, d), R = cone_pos_table_rows(max_v_l): row Lv(Lv-1)/2 + p = PositionEmbeddingSine of clip p of a
 *   window with Lv valid clips (cone/position_encoding.py:51-72); the LAST row (R - 1) is all zeros: the position of a
 *   text token (cone/model.py:106), added like any other row;
 * pos_qk (enc_layers, R, 2d): pos_rows [W_q | W_k]^T of every encoder layer (no bias).
 * With the tables the later encoder layers run ONE N = 3d GEMM on x (the attention kernel adds the pos_qk row to
 * q | k in its staging loads) and the decoder's cross-attention forms its keys memory + pos from pos_rows: no
 * x + pos matrix is ever written.
 * (ABI 6) The model handle OWNS such tables (built at cone_model_create for windows of up to CONE_TABLE_MAX_V_L clips: row
 * lv (lv - 1) / 2 + p is the same row whatever the bound).  pos_rows / pos_qk == NULL -- or the whole cone_layer0 == NULL --
 * means "the handle's": every call runs the table path.  qkv_vid / qkv_txt == NULL (no row caches): the packed layer input is
 * written once and the first layer runs like the later ones (one N = 3d GEMM on x, position rows from the table) -- the same
 * bits as with the caches, ~10 % more FLOPs when windows share clips / text.  max_v_l describes caller-owned tables only. */
typedef struct {
    const float* qkv_vid; const float* qkv_txt;
    const float* pos_qk; const float* pos_rows;
    int32_t max_v_l;
    /* (ABI 7) --use_txt_pos checkpoints (cone/config.py:115) on the table path: the position term of a text token is a
     * per-TOKEN row (cone/model.py:106) -- txt_pos (n_txt, d) and its images under every encoder layer's [W_q | W_k],
     * txt_pos_qk (enc_layers, n_txt, 2d), both from cone_layer0_text_positions on the projected token arena (row i of
     * either belongs to token row i of txt_proj).  NULL for such a model: the general path (x + pos materialised).
     * Ignored by models without the option. */
    const float* txt_pos; const float* txt_pos_qk;
    int64_t n_txt;
} cone_layer0;
int64_t cone_pos_table_rows(int max_v_l);
int cone_pos_tables(const cone_model* m, int max_v_l, float* pos_rows, float* pos_qk, void* stream);
/* (ABI 6) ws >= cone_layer0_project_workspace(m, n_rows) bytes: 0 for a post-norm model; a --pre_norm model's first in_proj
 * reads norm1(row) (cone/transformer.py:250-252), normalised into the scratch first. */
size_t cone_layer0_project_workspace(const cone_model* m, int64_t n_rows);
int cone_layer0_project(const cone_model* m, const float* proj_rows, int64_t n_rows, float* qkv, void* ws, size_t ws_bytes,
                        void* stream);
/* (ABI 7) --use_txt_pos: the text-side position rows of the table path, once per token of the projected text arena (they
 * are shared by all windows of a query, like the row caches).  tok_index[i] = index of token row i inside its query (0-based);
 * txt_pos[i] = LayerNorm(txt_proj_rows[i] + position_embeddings[tok_index[i]]) (cone/position_encoding.py:21-31, eval: no
 * dropout), txt_pos_qk[l][i] = txt_pos[i] [W_q | W_k]_l^T (no bias) for every encoder layer l.  Error for a model without
 * txt_pos_embed. */
int cone_layer0_text_positions(const cone_model* m, const float* txt_proj_rows, const int32_t* tok_index, int64_t n_rows,
                               float* txt_pos, float* txt_pos_qk, void* stream);

/* Workspace: 6 KiB per token row (B * (Lv_max + Lq_max) rows); 13 KiB on the general path (--use_txt_pos without its position rows, A/B switches). */
size_t cone_forward_packed_workspace(const cone_model* m, int B, int Lv_max, int Lq_max,
                                     const cone_layer0* l0 /* as passed to cone_forward_packed */);
int cone_forward_packed(const cone_model* m, const float* vproj, const int32_t* vid_row0,
                        const int32_t* vid_len, const float* tproj, const int32_t* txt_row0,
                        const int32_t* txt_len, int B, int Lv_max, int Lq_max,
                        float* logits, float* spans, float* saliency, const cone_taps* taps,
                        const cone_layer0* l0 /* may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* A12, CONE.forward_clip_matching (cone/model.py:130-152,178-210).  Gathered form:
 * proposal n of window b averages rows [s,e) of the window's clips vid[vid_row0[b] + ...] where
 * rows >= vid_len[b] count as the zero padding of a (pad_len[b])-long tensor (hazard H3):
 * mean = sum(rows s..min(e,vid_len)-1) / (min(e,pad_len[b]) - s).
 * cls (n_cls,dv) rows selected by cls_row[b]; spans (B,Nq,2) (center,width); match (B,Nq). */
size_t cone_clip_matching_workspace(const cone_model* m, int B);
int cone_clip_matching_gathered(const cone_model* m, const float* cls, const int32_t* cls_row,
                                const float* vid, const int32_t* vid_row0, const int32_t* vid_len,
                                const int32_t* pad_len, const float* spans, int B, float* match,
                                void* ws, size_t ws_bytes, void* stream);
/* Padded form with the reference's signature: cls (B,dv), vid (B,Lv_pad,dv). */
int cone_clip_matching(const cone_model* m, const float* cls, const float* vid, const int32_t* vid_len,
                       int Lv_pad, const float* spans, int B, float* match,
                       void* ws, size_t ws_bytes, void* stream);

/* A13, cone/inference.py:47-82: rows[b][n] = [st, ed, softmax(logits)[0], match] with
 * (st,ed) = (cxw->xx(spans) * duration[b] + video_start[b]) * clip_length in fp32, each window's
 * Nq rows sorted by proposal score (stable, descending) when sort != 0.  rows (B,Nq,4) fp32. */
int cone_compose_rows(const float* logits, const float* spans, const float* match,
                      const int32_t* duration, const int32_t* video_start, float clip_length,
                      int sort, int B, int Nq, float* rows, void* stream);

/* ------------------------------------------------------------ stage C: fusion + NMS */

/* A13 rounding + A14 + A15 for nq queries at once (cone/inference.py:83,103-127,205-217;
 * utils/temporal_nms.py:25-74), all in fp64 like the reference's Python floats:
 *   cand (nq,n_max,4) fp32 rows [st,ed,prop,match], n_valid[q] rows used per query -- or, cand_off != NULL (nq int64):
 *   the candidate rows of query q are rows cand_off[q] .. + n_valid[q] of ONE (rows, 4) matrix (the per-window rows of
 *   cone_compose_rows ARE that matrix: a query's windows are adjacent, no scatter into a padded layout);
 *   every number -> float(f"{x:.4f}"); min-max fusion; dict collapse on (st,ed);
 *   for score_idx in (2 fused, 0 proposal, 1 matching): stable sort desc, [:max_before],
 *   greedy NMS (pseudo-IoU, strict >), stop at max_after; nms_thd == -1 -> top max_after.
 * out_rows (3,nq,max_after,5) fp64 rows [st,ed,prop,match,fused]; out_n (3,nq) int32;
 * out_idx (3,nq,max_after) int32 = index into the query's cand rows (first occurrence of the key).  Every element of the
 * three outputs is written (rows past out_n: zeros, index -1): the buffers need no initialisation. */
int cone_fuse_nms(const float* cand, const int64_t* cand_off, const int32_t* n_valid, int nq, int n_max,
                  double nms_thd, int max_before, int max_after, double* out_rows, int32_t* out_n, int32_t* out_idx,
                  void* stream);

/* Same on fp64 candidate rows (e.g. rows that went through Python and are already rounded; the
 * rounding is idempotent on them). */
int cone_fuse_nms_f64(const double* cand, const int64_t* cand_off, const int32_t* n_valid, int nq, int n_max,
                      double nms_thd, int max_before, int max_after, double* out_rows, int32_t* out_n, int32_t* out_idx,
                      void* stream);

/* temporal_nms (utils/temporal_nms.py:25-74) on one list: pred (n,3) fp64 [st,ed,score];
 * keep_idx (max_after) indices into pred in output order, keep_n (1). */
int cone_temporal_nms(const double* pred, int n, double nms_thd, int max_after,
                      int32_t* keep_idx, int32_t* keep_n, void* stream);

/* A17, HungarianMatcher cost matrix for one target per window (cone/matcher.py:61-95):
 * C[b][n] = cost_span*L1(span_n, tgt_b) - cost_giou*GIoU - cost_class*softmax(logits)[0].
 * logits (B,Nq,2), spans (B,Nq,2) cxw, tgt (B,2) cxw, cost (B,Nq), best (B) = argmin_n. */
int cone_matcher_cost(const float* logits, const float* spans, const float* tgt, int B, int Nq,
                      float cost_span, float cost_giou, float cost_class, float* cost, int32_t* best,
                      void* stream);

/* SetCriterion.forward (cone/model.py:213-425) with its HungarianMatcher (cone/matcher.py:37-106): forward values of
 * one decoder layer's losses -- the matcher's exact assignment (<= 8 slots and <= 8 target spans per window, the
 * reference calls scipy's linear_sum_assignment), then loss_span = mean L1 of the matched (center, width) pairs,
 * loss_giou = mean (1 - GIoU), loss_label = mean over all slots (the negative window's too when neg_logits != NULL) of
 * the class-weighted cross-entropy (foreground = class 0 for matched slots, weight 1; background weight eos_coef),
 * class_error = 100 - top-1 accuracy of the matched slots, loss_saliency = hinge over the (pos, neg) clip pairs
 * (+ the negative window's maximum when neg_saliency != NULL), 0 when saliency == NULL.
 * logits, spans, neg_logits (B, Nq, 2); tgt (sum T, 2) (center, width), tgt_off (B + 1); tgt == NULL: no targets --
 * every slot is background and only loss_label is meaningful (:385-388).  saliency (B, L), pos_idx / neg_idx (B, P).
 * Outputs: assign (B, Nq) int32 (target index inside the window, -1 = unmatched; may be NULL), part (B, 8) scratch,
 * losses (5) = loss_span, loss_giou, loss_label, class_error, loss_saliency.
 * CONTRACT: Nq is checked here (1 .. 8), the target counts are NOT: the kernel trusts tgt_off, which lives on the device,
 * and a window with tgt_off[b + 1] - tgt_off[b] > 8 (or < 0) overruns the kernel's 8 x 8 cost matrix and its 256 DP
 * states.  The caller checks 0 <= T_b <= 8 on the host before it builds tgt_off (cone_amd.criterion raises
 * NotImplementedError); pos_idx / neg_idx must already be wrapped into [0, L). */
int cone_criterion_forward(const float* logits, const float* spans, const float* tgt, const int32_t* tgt_off,
                           const float* neg_logits, const float* saliency, int L, const int32_t* pos_idx,
                           const int32_t* neg_idx, int P, const float* neg_saliency, int L2, int B, int Nq,
                           float cost_span, float cost_giou, float cost_class, float eos_coef, float saliency_margin,
                           int32_t* assign, float* part, float* losses, void* stream);
/* loss_adapter (cone/model.py:249-264): (CE(sim / T, diag) + CE(sim^T / T, diag)) / 2 for sim (n, n); loss (1). */
int cone_adapter_nce(const float* sim, int n, float temperature, float* loss, void* stream);

/* ------------------------------------------------------------ video sessions (additive in ABI 8)
 * One resident video, indexed once, answering batches of queries: run_on_video/cone_localizator.py:121-221
 * (CONELocalizator.predict_moment) split into its video half (:129, :135-138, and the per-clip rows of :150-190: input_vid_proj
 * and the first encoder layer's q | k | v) and its query half.  CONTRACT: nothing new is computed -- both entries only
 * sequence the launchers above, with the arguments cone_amd/localizator.py passes them, so the kept moments carry the bits
 * of predict_moment on the same video and query (tests/test_session_gpu.py compares them with ==).  All memory is the caller's:
 * the resident rows live in ONE arena, every call's scratch in ONE workspace; nothing is allocated here, one stream, no host
 * read-back (both entries can be captured in a graph). */

/* What a caller sizing buffers around the opaque handle needs to know of it.  long_windows follows the handle's
 * "max_window_tokens" option at the moment of the call. */
typedef struct {
    int32_t hidden_dim, num_queries, enc_layers, t_dim, v_dim, v_motion_dim;
    int32_t txt_pos;       /* a --use_txt_pos checkpoint */
    int32_t long_windows;  /* max_window_tokens above CONE_MAX_WINDOW_TOKENS: every forward on the general path */
} cone_model_dims;
int cone_model_get_dims(const cone_model* m, cone_model_dims* out);

#define CONE_SESSION_BF16 1       /* the adapted rows are kept in bf16 only: the opt-in bf16 pre-filter (NOT fp32-accurate) */
#define CONE_SESSION_CERTIFIED 2  /* fp32 adapted rows + their bf16 shadow + its measures: the certified pre-filter; excludes BF16 */
#define CONE_SESSION_MAX_QUERIES 64

/* The resident half of a video: a plain host struct of device pointers into the caller's arena, filled by cone_session_index.
 * The library keeps no reference to it; it is valid while the arena and the handle it was indexed with live. */
typedef struct {
    const cone_model* model;        /* the handle it was indexed with: cone_session_localize refuses any other */
    int64_t ctx_l;                  /* clips */
    int32_t flags;                  /* CONE_SESSION_* */
    int32_t v_dim, hidden_dim;      /* row widths of the arrays below */
    const float* vid_norm;          /* (ctx_l, v_dim) F.normalize of the clips (:129) */
    const float* adapted;           /* (ctx_l, v_dim) adapter(x) + x, NOT re-normalised (:135-138); NULL with CONE_SESSION_BF16 */
    const uint16_t* adapted_bf16;   /* CONE_SESSION_BF16: the adapted rows in bf16; CONE_SESSION_CERTIFIED: their shadow */
    const float* err;               /* CONE_SESSION_CERTIFIED: the shadow's two measures (cone_prefilter_index_bf16) */
    const float* vproj;             /* (ctx_l, hidden_dim) input_vid_proj of the clips */
    const float* qkv_vid;           /* (ctx_l, 3 hidden_dim) first encoder layer's q | k | v rows; NULL on a long-window handle */
} cone_session;

/* The video half of run_on_video/cone_localizator.py:121-221, once per video: cone_l2_normalize_rows (eps 1e-5, clamp),
 * cone_adapter_norm / cone_adapter_norm_bf16 with renorm == 0, with CONE_SESSION_CERTIFIED cone_prefilter_index_bf16 on the
 * fp32 adapted rows, cone_project_tokens of the video side, and (not on a long-window handle) cone_layer0_project.
 * raw_vid (ctx_l, v_dim) fp32 with v_dim == v_motion_dim (the localizer feeds one feature to both sides).
 * arena >= cone_session_arena_bytes, 256-B aligned; ws >= cone_session_workspace (free again when the call's work is done).
 * Resident bytes per clip at 256 / 256: 1 KiB normalised + 1 KiB adapted (0.5 KiB bf16; 1.5 KiB certified) + 1 KiB projected
 * + 3 KiB q | k | v.  Refused by name: null arguments, flags with both modes, v_dim != v_motion_dim, a short arena or workspace. */
size_t cone_session_arena_bytes(const cone_model* m, int64_t ctx_l, int flags);
size_t cone_session_workspace(const cone_model* m, int64_t ctx_l, int flags);
int cone_session_index(const cone_model* m, const float* raw_vid, int64_t ctx_l, int flags, void* arena, size_t arena_bytes,
                       void* ws, size_t ws_bytes, cone_session* session, void* stream);

/* The per-call index metadata of nq queries on one video -- the shapes run_on_video/cone_localizator.py:121-221 builds on the
 * host per call (:150-170 pads every window to max_v_l, :191 scales by it) --, written on the device by ONE small launch with
 * no upload (what cone_amd/localizator.py keeps per shape in _const): the token lengths travel as kernel arguments.  tok_len is a HOST array
 * of nq lengths.  Outputs (device, int32): tok_off (nq + 1) exclusive prefix sums; tok_len_dev (nq); tok_idx (sum of the
 * lengths) = index of every token row inside its query, restarting at 0 per query (cone_layer0_text_positions); q_ctx_l (nq)
 * = ctx_l; q_vid_off (nq) = 0; batch_pad (nq) = max_v_l and full_w (nq * K) = max_v_l: every window counts as padded to
 * max_v_l (:150-170, :191); n_valid (nq) = K * Nq candidate rows per query.  Nothing else is written.
 * Refused by name: nq outside [1, CONE_SESSION_MAX_QUERIES]; a length outside [1, max_q_l]; K < 1; ctx_l outside [1, 2^31). */
int cone_session_query_layout(const int32_t* tok_len, int nq, int max_q_l, int64_t ctx_l, int K, int Nq, int max_v_l,
                              int32_t* tok_off, int32_t* tok_len_dev, int32_t* tok_idx, int32_t* q_ctx_l, int32_t* q_vid_off,
                              int32_t* batch_pad, int32_t* full_w, int32_t* n_valid, void* stream);

/* What the localizer fixes besides the checkpoint (run_on_video/cone_localizator.py:12-37, :200-219). */
typedef struct {
    int32_t max_v_l, max_q_l;   /* window length in clips (slide = max_v_l / 2), longest query in tokens */
    float clip_length;          /* seconds per clip */
    double nms_thd;             /* 0.5 */
    int32_t max_before, max_after;  /* 100, 5 */
} cone_session_params;

/* The query half of run_on_video/cone_localizator.py:121-221 for nq <= CONE_SESSION_MAX_QUERIES queries in ONE call:
 * cone_session_query_layout; cone_l2_normalize_rows of the token rows (:133); stage A -- cone_prefilter_scores (resp.
 * cone_prefilter_scores_bf16) in launches of at most 4 queries, the streaming form whose bits do not depend on the launch, then
 * cone_topk_windows_ws; or, on a CONE_SESSION_CERTIFIED session, cone_prefilter_topk_certified with n_cand (0: its default) --;
 * cone_window_table (eval_bsz 1, one batch per query); cone_project_tokens of the text side; cone_layer0_project and, for a
 * --use_txt_pos checkpoint, cone_layer0_text_positions; ONE cone_forward_packed over all nq * K windows (no saliency);
 * cone_clip_matching_gathered; cone_compose_rows (sort 0); cone_fuse_nms with a row per query.
 * tok: the queries' token rows back to back (sum of tok_len, t_dim) fp32, NOT normalised; tok_len: HOST array; cls (nq, v_dim)
 * raw cls vectors; K = windows per query, 1 <= K <= min(num_window, 256) (the localizer: min(topk_window, num_window)).
 * kept (3, nq, max_after, 5) fp64 and n_kept (3, nq) int32 are laid out as cone_fuse_nms writes them (the localizer reads
 * plane 0, the fused ranking).  certified (nq) int32, may be NULL: the flags of cone_prefilter_topk_certified (written only on
 * a certified session).  ws >= cone_session_localize_workspace for the same arguments: ONE function lays out both, every
 * buffer and every launcher's scratch has a region of its own (no two alias).  A workspace one byte short is refused by name. */
size_t cone_session_localize_workspace(const cone_model* m, const cone_session* session, const int32_t* tok_len, int nq, int K,
                                       int n_cand, const cone_session_params* params);
int cone_session_localize(const cone_model* m, const cone_session* session, const float* tok, const int32_t* tok_len, int nq,
                          const float* cls, int K, int n_cand, const cone_session_params* params, double* kept,
                          int32_t* n_kept, int32_t* certified, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ video libraries (additive in ABI 8)
 * Many resident videos in the rows of ONE arena, added and removed while it lives, and one call for a list of
 * (video, query) pairs on any mix of them: run_on_video/cone_localizator.py:121-221 with its video half done once per video
 * (as in a session) and its query half done for up to CONE_SESSION_MAX_QUERIES pairs at once.  CONTRACT: nothing new is
 * computed -- the entries sequence the launchers a session sequences, with a session's arguments, so every pair's kept moments
 * carry the bits of predict_moment on that video and query (tests/test_library_gpu.py compares them with ==).  A video is a
 * range of arena rows [row0, row0 + ctx_l); WHO owns which rows is the caller's business (cone_amd/library.py keeps a
 * first-fit free list), the entries only check that a range lies inside the arena.  The rules are the sessions': all memory
 * is the caller's, arena and workspaces 256-B aligned, one stream, nothing allocated, no host read-back, refusals by name on
 * the host before any pointer is read.  Out of scope: CONE_SESSION_CERTIFIED libraries (refused by name), growing a video in
 * place, indexing several videos in one launch.  (Compaction and resizing: "library maintenance" below.) */

/* A plain host struct of device pointers into the caller's arena, like cone_session; filled by cone_library_open. */
typedef struct {
    const cone_model* model;        /* the handle it was opened with: the other entries refuse any other */
    int64_t capacity;               /* clip rows the arena holds */
    int32_t flags;                  /* 0 or CONE_SESSION_BF16 */
    int32_t v_dim, hidden_dim;      /* row widths of the arrays below */
    float* vid_norm;                /* (capacity, v_dim) F.normalize of the clips (:129) */
    float* adapted;                 /* (capacity, v_dim) adapter(x) + x (:135-138); NULL with CONE_SESSION_BF16 */
    uint16_t* adapted_bf16;         /* CONE_SESSION_BF16: the adapted rows in bf16; NULL otherwise */
    float* vproj;                   /* (capacity, hidden_dim) input_vid_proj of the clips */
    float* qkv_vid;                 /* (capacity, 3 hidden_dim) first encoder layer's q | k | v rows; NULL on a long-window handle */
} cone_library;

/* Lays the regions of an arena for `capacity` rows out (the layout function of cone_session_arena_bytes, with capacity for
 * ctx_l) and fills *out; launches nothing, writes nothing to the arena (run_on_video/cone_localizator.py:121-221 keeps no
 * state; this is where the video half's results of many calls live).  Refused by name: null arguments, CONE_SESSION_CERTIFIED,
 * other flags than 0 / CONE_SESSION_BF16, capacity outside [1, 2^31), a misaligned or short arena, v_dim != v_motion_dim. */
size_t cone_library_arena_bytes(const cone_model* m, int64_t capacity, int flags);
int cone_library_open(const cone_model* m, int64_t capacity, int flags, void* arena, size_t arena_bytes, cone_library* out);

/* The video half of run_on_video/cone_localizator.py:121-221 for ONE video, written to rows [row0, row0 + n_rows) of the
 * arena: the launcher chain of cone_session_index (one function runs both; cone_session_index is the chain at row0 = 0) on
 * n_rows rows -- cone_l2_normalize_rows, cone_adapter_norm / cone_adapter_norm_bf16 with renorm == 0, cone_project_tokens of
 * the video side, cone_layer0_project unless the handle is a long-window handle.  Nothing outside those rows is written.
 * raw_clips (n_rows, v_dim) fp32; ws >= cone_library_add_workspace, free again when the call's work is done.
 * A row's bits depend on its clip alone, not on n_rows or on the row's place in the call (tests/test_library_ingest_gpu.py), so
 * a caller may index the rows of several adjacent videos, or the new clips behind a resident video, in one call
 * (cone_amd/library.py: add_many, extend).
 * Refused by name: null arguments, another handle than the library's, row0 < 0, n_rows < 1, row0 + n_rows > capacity, a
 * misaligned or short workspace. */
size_t cone_library_add_workspace(const cone_model* m, int64_t n_rows);
int cone_library_add(const cone_model* m, const cone_library* lib, int64_t row0, const float* raw_clips, int64_t n_rows, void* ws,
                     size_t ws_bytes, void* stream);

/* cone_session_query_layout with a video per query (run_on_video/cone_localizator.py:121-221: the shapes :150-170 and :191
 * build on the host): tok_len, q_row0, q_ctx_l are HOST arrays of nq entries and travel as kernel arguments, nothing is
 * uploaded; ONE one-workgroup launch, one writer per element.  Outputs as there, except q_ctx_l_dev (nq) = q_ctx_l and
 * q_vid_off (nq) = q_row0; n_valid = K * Nq, batch_pad = full_w = max_v_l.  Nothing else is written.
 * Refused by name: nq outside [1, CONE_SESSION_MAX_QUERIES]; a length outside [1, max_q_l]; q_ctx_l[q] < 1; q_row0[q] < 0;
 * q_row0[q] + q_ctx_l[q] >= 2^31; K outside [1, min(num_window of query q, 256)] (the message names q). */
int cone_library_query_layout(const int32_t* tok_len, const int32_t* q_row0, const int32_t* q_ctx_l, int nq, int max_q_l, int K,
                              int Nq, int max_v_l, int32_t* tok_off, int32_t* tok_len_dev, int32_t* tok_idx, int32_t* q_ctx_l_dev,
                              int32_t* q_vid_off, int32_t* batch_pad, int32_t* full_w, int32_t* n_valid, void* stream);

/* The query half of run_on_video/cone_localizator.py:121-221 for nq <= CONE_SESSION_MAX_QUERIES (video, query) pairs in ONE
 * call: cone_session_localize, except that query q runs on the video at rows [q_row0[q], q_row0[q] + q_ctx_l[q]).
 * Stage A runs per RUN of consecutive queries with the same (q_row0, q_ctx_l) -- cone_prefilter_scores (resp.
 * cone_prefilter_scores_bf16) on that video's adapted rows in launches of at most 4 queries, then one cone_topk_windows_ws,
 * in the form and with the arguments of a session on that video: that is what makes the bits predict_moment's (callers sort
 * by video to keep the runs few).  Everything after stage A is one launch over all nq * K windows as in a session:
 * cone_window_table, the text projection and layer-0 text rows / positions, ONE cone_forward_packed with the arena's vproj /
 * qkv_vid as bases, cone_clip_matching_gathered on vid_norm, cone_compose_rows, cone_fuse_nms with a row per query.
 * ONE K per call, 1 <= K <= min(num_window of every query's video, 256); q_row0, q_ctx_l, tok_len: HOST arrays; tok, cls,
 * kept, n_kept as in cone_session_localize.  ws >= cone_library_localize_workspace for the same arguments (ONE function lays
 * out both; 0 and cone_last_error on a refusal).
 * Refused by name, on the host, the pairs first: null arguments; nq outside [1, 64]; a length outside [1, max_q_l];
 * q_ctx_l[q] < 1; q_row0[q] < 0; q_row0[q] + q_ctx_l[q] > capacity; K outside the range above (the message names the query);
 * another handle than the library's; a misaligned or short workspace. */
size_t cone_library_localize_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                       const int32_t* tok_len, int nq, int K, const cone_session_params* params);
int cone_library_localize(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                          const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                          const cone_session_params* params, double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ library search (additive in ABI 8)
 * "Which of my resident videos shows this, and where?"  The coarse stage of the method (cone/inference.py:276-299: a window's
 * score is the best cosine of its clips with the query in the adapter's space, comparable across videos) over MANY videos of a
 * library in ONE pass over their arena rows, then the query half on the windows the scan found.  CONTRACT: for every
 * (query, video) the window list carries the bits of cone_prefilter_scores (the streaming form: launches of at most 4 queries) +
 * cone_topk_windows_ws on that video's rows alone -- what cone_library_localize's stage A computes per run --, so a search's
 * moments carry the bits of predict_moment on the videos it chose.  Rows outside the listed videos are never read; a half-block
 * and a window never cross a video's end.  fp32 libraries only: CONE_SESSION_BF16 and CONE_SESSION_CERTIFIED libraries are
 * refused by name. */

/* Stage A of run_on_video/cone_localizator.py:121-221 (:83-100; cone/inference.py:276-299) for nq queries against n_videos
 * videos of the library.  The videos come as a DEVICE table: v_row0 (n_videos) int64 first arena row, v_ctx_l (n_videos) int32
 * clips, v_hb_off (n_videos + 1) int64 exclusive prefix sums of ceil(v_ctx_l / S), S = max_v_l / 2; total_hb = v_hb_off[n_videos]
 * (the host knows it: cone_amd/library.py scan_table).  The ranges must be disjoint and inside the arena; a video whose range
 * leaves [0, capacity) is not read and scores -inf.  cls (nq, v_dim) fp32 on the device.
 * Outputs (device): widx / wval (nq, n_videos, K): the first K entries of the stable descending order of video v's window
 * scores for query q (the order, ties and values of cone_topk_windows_ws on that video's score row), padded with -1 / -inf where
 * the video has fewer than K windows -- a prefix of a stable list is the stable list of a smaller K, so one scan at
 * K = topk_window serves every video's own K.  rank_slot / rank_val (nq, n_rank): cone_topk_windows_ws over best[q][v] =
 * wval[q][v][0]: the n_rank best videos as TABLE SLOTS (ties to the lower slot) and their scores.
 * ws >= cone_library_scan_workspace, 256-B aligned: two planes (nq, total_hb), best (nq, n_videos), the ranking's scratch; no
 * frame score and no window score is written anywhere.
 * Refused by name ("library_scan: "), from host values first, before any pointer or the handle is looked at: nq outside [1, 64];
 * n_videos < 1; total_hb < n_videos or > capacity; K outside [1, 256]; n_rank outside [1, n_videos]; max_v_l < 2; a
 * CONE_SESSION_CERTIFIED or CONE_SESSION_BF16 library; then null arguments, another handle, a v_dim outside {256, 512, 768, 1024},
 * a misaligned or short workspace. */
size_t cone_library_scan_workspace(const cone_library* lib, int64_t n_videos, int64_t total_hb, int nq, int K, int n_rank);
int cone_library_scan(const cone_model* m, const cone_library* lib, const int64_t* v_row0, const int32_t* v_ctx_l,
                      const int64_t* v_hb_off, int64_t n_videos, int64_t total_hb, const float* cls, int nq, int K, int n_rank,
                      const cone_session_params* params, int32_t* widx, float* wval, int32_t* rank_slot, float* rank_val, void* ws,
                      size_t ws_bytes, void* stream);

/* cone_library_localize (run_on_video/cone_localizator.py:121-221, the query half) with stage A replaced by a gather: pair p's
 * window list is the first K entries of the scan's list of (query pair_query[p], table slot pair_slot[p]), copied by ONE small
 * launch; everything from cone_window_table on is cone_library_localize, the same function (cone/inference.py:276-299 has run in
 * the scan).  pair_query, pair_slot: HOST arrays of nq entries; scan_widx / scan_wval: the DEVICE outputs of a cone_library_scan
 * with scan_nq queries, scan_n_videos videos and scan_K entries per list; q_row0 / q_ctx_l must name the rows of the video at
 * that slot (the caller's table: cone_amd/library.py).  cls (nq, v_dim): the PAIRS' cls vectors.  ws >=
 * cone_library_localize_ranked_workspace (no score rows, no stage-A scratch).
 * Refused by name ("library_localize_ranked: "): everything cone_library_localize refuses, on the host, the pairs first; then
 * K > scan_K, a pair_query[p] outside [0, scan_nq), a pair_slot[p] outside [0, scan_n_videos); a CONE_SESSION_BF16 library. */
size_t cone_library_localize_ranked_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                              const int32_t* q_ctx_l, const int32_t* tok_len, int nq, int K,
                                              const cone_session_params* params);
int cone_library_localize_ranked(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                 const float* tok, const int32_t* tok_len, int nq, const float* cls, int K,
                                 const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                 const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K,
                                 double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ library maintenance (additive in ABI 8)
 * Compacting a library in place and resizing it into another arena.  run_on_video/cone_localizator.py:121-221 keeps no state
 * between calls; a library keeps the video half's results, per clip one row in each of four planes (vid_norm, adapted or
 * adapted_bf16, vproj, and qkv_vid unless the handle is a long-window handle).  A row's bits do not depend on where it lives,
 * so moving a video is a pure copy.  CONTRACT: the moved rows carry the bits they had -- every (video, query) pair answers
 * with the bits of predict_moment before and after, once the caller names the video's new rows.  WHO owns which rows stays the
 * caller's business (cone_amd/library.py plans the moves: compaction_moves, plan_steps).  CONE_SESSION_BF16 libraries and
 * long-window handles are supported; CONE_SESSION_CERTIFIED libraries are refused by name. */

/* Moves rows of the resident video halves (run_on_video/cone_localizator.py:121-221: nothing of it runs again).  The moves come
 * as a DEVICE table: move i copies rows [mv_src[i], mv_src[i] + n_i) of every present plane of src to rows [mv_dst[i], ...) of
 * the same plane of dst, n_i = mv_off[i + 1] - mv_off[i]; mv_off (n_moves + 1) int64 = the exclusive prefix sums, total_rows =
 * mv_off[n_moves] (the host knows it).  The moves laid end to end are the flat row list; ONE call moves its rows
 * [row_begin, row_end) and may begin and end inside a move.
 *   stage == NULL: direct, ONE launch, src rows to dst rows.  The caller guarantees that the call's dst rows and src rows are
 *     disjoint (another arena, or disjoint sets in the same one).
 *   stage != NULL: staged, TWO launches of the same kernel body: the call's rows are gathered into stage, packed plane by
 *     plane, then scattered to dst; stream order is the only synchronisation, so ANY overlap between the call's src and dst
 *     rows is fine.  stage: 256-B aligned, >= cone_library_move_stage_bytes(lib, row_end - row_begin) = the sum over the present
 *     planes of row bytes * n_rows, each plane rounded up to 256 B.
 * Nothing but the listed dst rows (and stage) is written; vacated src rows keep their content.  A move whose src range leaves
 * [0, src->capacity) or whose dst range leaves [0, dst->capacity) is skipped whole on the device: not read, not written.
 * Nothing is allocated, nothing read back, no atomics: both forms can be captured in a graph.
 * Refused by name ("library_move: "), from host values first, before any pointer or the handle is looked at: n_moves < 1;
 * total_rows < n_moves; row_begin / row_end outside 0 <= begin < end <= total_rows; a CONE_SESSION_CERTIFIED library; then
 * null arguments, total_rows > src->capacity, src and dst that differ in model, flags, v_dim, hidden_dim or in which planes are
 * present, another handle than the libraries', a misaligned or short stage. */
size_t cone_library_move_stage_bytes(const cone_library* lib, int64_t n_rows);
int cone_library_move_rows(const cone_model* m, const cone_library* src, const cone_library* dst, const int64_t* mv_src,
                           const int64_t* mv_dst, const int64_t* mv_off, int64_t n_moves, int64_t total_rows, int64_t row_begin,
                           int64_t row_end, void* stage, size_t stage_bytes, void* stream);

/* ------------------------------------------------------------ library window budgets (additive in ABI 8)
 * A search that spends a fixed budget of W windows per query wherever in the library the evidence is, instead of K windows on
 * each of n videos: twelve windows may go to one video, five to another, one each to three more.  Two pieces.
 * cone_library_budget picks, per query, the W best windows over every list of a cone_library_scan and says how many fall to
 * which video; cone_library_localize_ragged is the query half with a window count PER PAIR.  CONTRACT: a scan's lists are stable
 * and descending per (query, video), so the chosen windows of a video are a prefix of its list, and a prefix of a stable list is
 * the stable list of a smaller K: a pair that receives k windows answers with the bits of predict_moment at topk_window = k
 * (run_on_video/cone_localizator.py:121-221 on the first k windows of cone/inference.py:276-299;
 * tests/test_library_budget_gpu.py compares with ==).  Planning the pairs stays on the host: one small read-back between the
 * two.  fp32 libraries for the budget and the lists' form; the ragged call's own stage A serves CONE_SESSION_BF16 libraries. */

/* The W best windows of every query over all the lists of a scan (cone/inference.py:276-299 ranks the windows of ONE video; this
 * ranks the lists of many against each other -- the scores are cosines in the adapter's space, comparable across videos -- and
 * run_on_video/cone_localizator.py:121-221 then runs on the chosen ones).  wval (nq, n_videos, scan_K) fp32 on the device: a
 * cone_library_scan's values (its widx plays no part: padding carries -inf).
 * Per query: of the n_videos * scan_K entries those > -inf, ordered by value descending, ties to the lower table slot, then to
 * the lower list position (= the lower flat index slot * scan_K + j; -0.0 ties with +0.0, as in cone_topk_windows_ws, which does
 * the selection); the first min(W, their count) are chosen.  An entry of -inf is NEVER chosen -- list padding and a window of NaN
 * frames alike --, so a query with fewer than W finite entries SPENDS ITS BUDGET SHORT.  The lists must be descending per
 * (query, slot) -- the scan's guarantee --: the chosen entries of a slot are then a prefix of its list.
 * Outputs (device), every element written: n_pairs (nq); pair_slot / pair_k / pair_best (nq, W): the slots that receive a window
 * in order of first appearance (best score descending, ties to the lower slot: cone_library_scan's ranking order), the number
 * chosen from each, the value of its first; rows past n_pairs[q] are -1 / 0 / -inf.  sum of pair_k[q] = min(W, finite entries).
 * ws >= cone_library_budget_workspace, 256-B aligned: the selected (index, value) lists and the selection's scratch.
 * Refused by name ("library_budget: "), from host values first, before any pointer is looked at: nq outside [1, 64]; n_videos < 1;
 * scan_K outside [1, 256]; W outside [1, 256]; n_videos * scan_K >= 2^31 - 1; then null arguments, a misaligned or short
 * workspace. */
size_t cone_library_budget_workspace(int nq, int64_t n_videos, int scan_K, int W);
int cone_library_budget(const float* wval, int nq, int64_t n_videos, int scan_K, int W, int32_t* n_pairs, int32_t* pair_slot,
                        int32_t* pair_k, float* pair_best, void* ws, size_t ws_bytes, void* stream);

/* cone_library_localize / cone_library_localize_ranked (run_on_video/cone_localizator.py:121-221, the query half) with a HOST
 * array pair_k (nq) in place of the one K: pair p runs on its first pair_k[p] windows (cone/inference.py:276-299's order), B =
 * sum of pair_k window rows in all.  ONE one-workgroup launch writes the call's metadata -- what cone_library_query_layout writes,
 * plus row_q / row_slot / full_w for the B rows, n_valid[p] = pair_k[p] Nq and cand_off[p] = (rows before p) Nq --, stage A leaves
 * an (nq, Kmax) window list, Kmax = max pair_k, whose row p holds pair p's prefix (the rest is -1 / -inf and never read), and
 * everything behind it is the uniform call's launch over B windows: cone_window_table in its row_q / row_slot form, the forward,
 * cone_clip_matching_gathered, cone_compose_rows, cone_fuse_nms with cand_off.
 * Stage A has two forms, chosen by the lists' block pair_query, pair_slot, scan_widx, scan_wval (all four, or all four NULL):
 *   lists: as in cone_library_localize_ranked, ONE small launch copies the first pair_k[p] entries of the scan's list of
 *     (pair_query[p], pair_slot[p]);
 *   none (scan_nq, scan_n_videos, scan_K are then ignored): cone_library_localize's own stage A per run of consecutive pairs on
 *     one video -- the pre-filter in launches of at most 4, ONE cone_topk_windows_ws at the largest pair_k of the run -- and the
 *     same small launch copies every pair's prefix.  CONE_SESSION_BF16 libraries are served in this form.
 * Pairs of one video with different pair_k may be adjacent: they are one run.  kept / n_kept as in cone_library_localize.
 * ws >= cone_library_localize_ragged_workspace for the same pairs, counts and form (ranked != 0: the lists' form).
 * Refused by name ("library_localize_ragged: "): everything cone_library_localize refuses, on the host, the pairs first; then a
 * pair_k[p] outside [1, min(num_window of pair p, 256)] (the message names p; with nq <= 64 that bounds B by 64 * 256); with
 * lists: a CONE_SESSION_BF16 library, Kmax > scan_K, a pair_query[p] outside [0, scan_nq), a pair_slot[p] outside
 * [0, scan_n_videos), a block that is only partly there. */
size_t cone_library_localize_ragged_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                              const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const int32_t* pair_k,
                                              const cone_session_params* params, int ranked);
int cone_library_localize_ragged(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                 const float* tok, const int32_t* tok_len, int nq, const float* cls, const int32_t* pair_k,
                                 const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                 const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K,
                                 double* kept, int32_t* n_kept, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ library moment search (additive in ABI 8)
 * "The n best moments for this query in everything the library holds."  Every per-(video, query) answer above is normalised over
 * the candidates of that one pair (run_on_video/cone_localizator.py:200-206: each pair's best proposal becomes 1.0, whatever its
 * logit), so the lists of different videos cannot be merged.  The reference's own rule answers it: everything that came out of the
 * chosen windows is ONE candidate pool -- in predict_moment the topk_window windows of one video, here the W windows a budget chose
 * library-wide.  Two pieces: cone_library_localize_candidates is cone_library_localize_ragged stopped before its per-pair stage C;
 * cone_corpus_fuse_nms is stage C over a pool per query, where a moment belongs to a video. */

/* Stage C (run_on_video/cone_localizator.py:187-221; utils/temporal_nms.py:25-74) over one pool per query, the fused ranking only;
 * one workgroup per query, fp64, cone_fuse_nms' arithmetic.  cand: fp32 rows [st, ed, prop, match], the flat candidate buffer of
 * a whole search (device).  The segment table (device): query q owns segments [seg_off[q], seg_off[q + 1]) (seg_off (nq + 1)
 * int32), segment s is the seg_n[s] (int32) rows from row seg_cand[s] (int64) on, of the video seg_tag[s] (int32; equal tags
 * inside a query are one video).  The pool of a query = its segments in table order, each one's rows in buffer order:
 *   1. all four columns rounded to 4 decimals;  2. normalize_score on the pool's proposal column and on its matching column, each
 *   over the WHOLE pool (mn == mx: the raw values);  3. fused = (0 + a) + b;  4. a dict keyed by (tag, st, ed): the first
 *   occurrence fixes the position, the last the values;  5. stable descending sort by fused;  6. the first max_before;
 *   7. greedy temporal NMS in which a kept moment suppresses a later one only where the TAGS ARE EQUAL and pseudo-IoU > nms_thd
 *   (a list of one is returned untouched; nms_thd == -1 skips the NMS);  8. the first max_after.
 * Outputs (device), every element written: out_rows (nq, max_after, 5) fp64 [st, ed, prop, match, fused], zeros past the kept
 * rows; out_seg (nq, max_after) int32 = the kept moment's segment ordinal within its query (of its key's first occurrence), -1
 * past them; out_n (nq).  A query without segments answers 0.
 * At most 1 024 candidates per query.  The table is device data: the kernel takes candidates until a query's pool holds 1 024
 * and truncates the segment that crosses the cap, so a query whose table holds more answers for ITS FIRST 1 024 CANDIDATES;
 * segment indices are clamped to [0, n_seg), a negative seg_n counts as 0.  No atomics, no allocation, no read-back.
 * Refused by name ("corpus_fuse_nms: "), from host values first, before any pointer is looked at: nq outside [1, 1024];
 * n_seg < 0; max_after outside [1, 1024]; max_before < 1; then null arguments (cand and the three per-segment arrays may be NULL
 * where n_seg == 0). */
int cone_corpus_fuse_nms(const float* cand, const int32_t* seg_off, const int64_t* seg_cand, const int32_t* seg_n,
                         const int32_t* seg_tag, int nq, int n_seg, double nms_thd, int max_before, int max_after,
                         double* out_rows, int32_t* out_seg, int32_t* out_n, void* stream);

/* cone_library_localize_ragged (run_on_video/cone_localizator.py:121-198) with `float* cand` in place of kept / n_kept: the same
 * launches up to cone_compose_rows, which writes the call's B * Nq rows (B = sum of pair_k, Nq = the decoder's slots) straight
 * into cand -- pair order, then window order, then decoder slot: pair p's rows start at (window rows before p) * Nq -- and NO
 * cone_fuse_nms.  Both stage-A forms.  ws >= cone_library_localize_candidates_workspace (same arguments as the ragged size entry).
 * Refused by name ("library_localize_candidates: "): what cone_library_localize_ragged refuses, in its order. */
size_t cone_library_localize_candidates_workspace(const cone_model* m, const cone_library* lib, const int32_t* q_row0,
                                                  const int32_t* q_ctx_l, const int32_t* tok_len, int nq, const int32_t* pair_k,
                                                  const cone_session_params* params, int ranked);
int cone_library_localize_candidates(const cone_model* m, const cone_library* lib, const int32_t* q_row0, const int32_t* q_ctx_l,
                                     const float* tok, const int32_t* tok_len, int nq, const float* cls, const int32_t* pair_k,
                                     const cone_session_params* params, const int32_t* pair_query, const int32_t* pair_slot,
                                     const int32_t* scan_widx, const float* scan_wval, int scan_nq, int64_t scan_n_videos, int scan_K,
                                     float* cand, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ standing queries (additive in ABI 8)
 * A fixed set of queries asked again whenever a live video has grown by a few clips.  A window's candidate rows depend on nothing
 * outside the window: cone_window_table gives window wi the clips [max((wi - 1) S, 0), min((wi - 1) S + W, ctx_l)), S = W / 2,
 * batch_pad is W for every pair, and a row [st, ed, prop, match] is made from video_start and the window's own outputs
 * (run_on_video/cone_localizator.py:150-198).  So a watcher (cone_amd/watch.py) keeps the rows of every (query, window) it has
 * computed and runs cone_library_localize_candidates only on the listed windows it has not seen, or saw while they were still
 * growing; cone_corpus_fuse_nms then runs on the cache.  The answer carries the bits of predict_moment.
 *   cache (nq, n_win, Nq, 4) fp32: the Nq candidate rows of window wi for query q at row (q n_win + wi) Nq.
 *   stamp (nq, n_win) int32: the video's ctx_l when the entry was computed; 0 = never.
 * VALIDITY at the current ctx_l: entry (q, wi) is valid iff stamp == ctx_l, or stamp > 0 and (wi - 1) S + W <= stamp (the window
 * was full when it was computed: its clip range then is its clip range now).  A trim moves the first clip: the caller zeroes the
 * stamps.  Both entries are one small launch, one workgroup per query, plain vector loads and stores: no atomics, no allocation,
 * no read-back. */

/* The plan of one poll for nq queries.  widx / wval (nq, K): the lists of a cone_library_scan over ONE video (device).  An entry
 * j is LISTED when 0 <= widx < n_win (a device-side clamp; the padding -1 is not listed) and MISSING when it is listed and not
 * valid by the rule above.  Outputs (device), every element written:
 *   miss_widx / miss_wval (nq, K): the missing entries of query q in list order (stable) in [0, n_miss[q]), then -1 / -inf: the
 *     lists' block of a cone_library_localize_candidates call with pair_query = q, pair_slot = 0, scan_n_videos = 1, scan_K = K,
 *     pair_k = n_miss[q] (a query with n_miss == 0 is left out of that call);
 *   n_miss (nq);
 *   the DENSE segment table of cone_corpus_fuse_nms over the cache: seg_off (nq + 1) = q K; segment q K + j has seg_cand (int64) =
 *     (q n_win + widx) Nq and seg_n = Nq when entry j is listed, else 0 and 0; seg_tag = 0.  The table does not depend on hit or
 *     miss: a missing window's rows are in place (cone_watch_store) before stage C runs.
 * Refused by name ("watch_plan: "), from host values first, in this order, before any pointer is looked at: nq outside [1, 64];
 * K outside [1, 256]; Nq outside [1, 16]; n_win < 1; ctx_l < 1; W < 2; then null arguments. */
int cone_watch_plan(const int32_t* widx, const float* wval, int nq, int K, const int32_t* stamp, int n_win, int ctx_l, int W, int Nq,
                    int32_t* miss_widx, float* miss_wval, int32_t* n_miss, int32_t* seg_off, int64_t* seg_cand,
                    int32_t* seg_n, int32_t* seg_tag, void* stream);

/* Scatters the rows a cone_library_localize_candidates call wrote for the plan's miss lists into the cache and stamps them.
 * cand: that call's buffer -- query q's first row is Nq * (sum over q' < q of min(max(n_miss[q'], 0), K)): queries without a miss
 * contribute nothing, so leaving them out of the call shifts nobody.  For m < min(max(n_miss[q], 0), K) with wi = miss_widx[q][m]
 * inside [0, n_win): the Nq rows of 16 B go to cache rows (q n_win + wi) Nq .., stamp[q][wi] = ctx_l; an index outside is skipped.
 * Nothing else is written.  PRECONDITION: the window indices of one query are distinct (a top-k list guarantees it) -- two equal
 * indices would be two writers of one row.  cand and cache must be 16-B aligned.
 * Refused by name ("watch_store: "), from host values first, in this order: nq outside [1, 64]; K outside [1, 256]; n_win < 1;
 * ctx_l < 1; Nq outside [1, 16]; then null arguments, then a misaligned cand or cache. */
int cone_watch_store(const float* cand, const int32_t* miss_widx, const int32_t* n_miss, int nq, int K, int n_win, int ctx_l, int Nq,
                     float* cache, int32_t* stamp, void* stream);

/* ------------------------------------------------------------ standing queries over a library (additive, ABI 8)
 * The standing queries above, asked of EVERY resident video at once: the library moment search's contract (the budget's windows
 * are one pool per query) at the watcher's price (the window model runs only on chosen windows the cache does not hold).  One
 * cache and one stamp plane serve all watched videos (cone_amd/watch.py, LibraryWatcher):
 *   cache (nq, n_win_total, Nq, 4) fp32, stamp (nq, n_win_total) int32; table slot s of the scan owns the SLAB
 *   [v_win0[s], v_win0[s] + v_cap[s]) of the window axis: window wi of its video is axis entry v_win0[s] + wi, and its stamps are
 *   clip counts of that video, judged against v_ctx_l[s] by the rule above.  v_ctx_l / v_win0 / v_cap (V) int32, device.
 * The caller keeps slabs disjoint and inside the axis and zeroes a slab's stamps when its video is trimmed or the slab changes
 * hands.  Both entries are one small launch, plain vector loads and stores, every output element with one writer: no atomics, no
 * allocation, no read-back. */

/* The plan of one poll for nq queries; one workgroup of 256 threads per query.  widx / wval (nq, V, K): a cone_library_scan's
 * lists; n_pairs (nq), pair_slot / pair_k (nq, Wb): a cone_library_budget's outputs at W = Wb (all device).  The CHOSEN windows of
 * query q, in POOL ORDER: the pairs in the budget's order, of pair i the list positions 0 .. pair_k - 1 of (q, pair_slot[i]) --
 * the order in which cone_library_localize_candidates lays a search's pool.  Chosen window t (its ordinal) with list entry wi in
 * slot s is LISTED when 0 <= wi < v_cap[s] (and v_win0[s] >= 0, v_win0[s] + wi < n_win_total: an entry outside the axis is never
 * read) and MISSING when it is listed and stamp[q][v_win0[s] + wi] is not valid at v_ctx_l[s].
 * Device data is clamped, never trusted: n_pairs into [0, Wb]; pair_k into [0, K]; a slot outside [0, V) is an empty pair; chosen
 * windows past the first Wb are neither planned nor listed (a pair that crosses the cap is cut there).
 * Outputs (device), every element named here written:
 *   miss_widx / miss_wval in the scan's (nq, V, K) layout: for every pair with a planned window, row (q, slot) holds the pair's
 *     missing windows first, in list order (stable), then -1 / -inf up to the pair's planned count: the lists' block of a
 *     cone_library_localize_candidates call with the pair's own pair_query / pair_slot and pair_k = pair_miss.  Rows of slots
 *     the budget did not choose, and a row's entries past the planned count, are NOT written;
 *   pair_miss (nq, Wb): the missing windows of pair i, 0 past n_pairs;
 *   the DENSE segment table of cone_corpus_fuse_nms over the cache, one segment per chosen window: seg_off (nq + 1) = q Wb;
 *     segment q Wb + t has seg_cand (int64) = (q n_win_total + v_win0[s] + wi) Nq and seg_n = Nq when listed, else 0 and 0;
 *     seg_tag = s; t at or past the chosen count: 0, 0, 0.  The table does not depend on hit or miss.
 * PRECONDITION: the slots of one query's pairs are distinct (the budget guarantees it) -- two pairs on one slot would be two
 * writers of one miss row.
 * Refused by name ("watch_pool_plan: "), from host values first, in this order, before any pointer is looked at: nq outside
 * [1, 64]; V < 1; K outside [1, 256]; Wb outside [1, 256]; Nq outside [1, 16]; n_win_total < 1; W < 2; then null arguments. */
int cone_watch_pool_plan(const int32_t* widx, const float* wval, const int32_t* n_pairs, const int32_t* pair_slot,
                         const int32_t* pair_k, const int32_t* v_ctx_l, const int32_t* v_win0, const int32_t* v_cap,
                         const int32_t* stamp, int nq, int V, int K, int Wb, int n_win_total, int W, int Nq, int32_t* miss_widx,
                         float* miss_wval, int32_t* pair_miss, int32_t* seg_off, int64_t* seg_cand, int32_t* seg_n,
                         int32_t* seg_tag, void* stream);

/* Scatters the rows the cone_library_localize_candidates calls wrote for the plan's miss lists into the cache and stamps them;
 * one workgroup per job.  jobs (n_jobs, 4) int32 on the device, one per pair that missed something, in the order of the host's
 * planned calls: query, slot, n_miss, the pair's first row in cand (in rows of 16 B).  For m < min(max(n_miss, 0), K) with
 * wi = miss_widx[(query V + slot) K + m] inside [0, v_cap[slot]) (and inside the axis, as above): the Nq rows of 16 B from
 * cand row first + m Nq go to cache row (query n_win_total + v_win0[slot] + wi) Nq, and that stamp = v_ctx_l[slot]; an index
 * outside is skipped, as is a job whose query lies outside [0, nq), whose slot lies outside [0, V) or whose first row is
 * negative.  Nothing else is written.  PRECONDITION: the (query, slot) of the jobs are distinct and so are the window indices of
 * one list (a top-k list guarantees it).  cand and cache must be 16-B aligned.
 * Refused by name ("watch_pool_store: "), from host values first, in this order: nq outside [1, 64]; V < 1; K outside [1, 256];
 * Nq outside [1, 16]; n_win_total < 1; n_jobs < 1; then null arguments, then a misaligned cand or cache. */
int cone_watch_pool_store(const float* cand, const int32_t* jobs, int n_jobs, const int32_t* miss_widx, const int32_t* v_ctx_l,
                          const int32_t* v_win0, const int32_t* v_cap, int nq, int V, int K, int n_win_total, int Nq, float* cache,
                          int32_t* stamp, void* stream);

/* ------------------------------------------------------------ certified library budgets (additive, ABI 8)
 * cone_library_scan reads every listed row in fp32: the one part of a search that grows with the library.  A budgeted search
 * (cone_library_budget) wants the W <= 256 best windows of the WHOLE table per query, so the certified pre-filter's three steps fit
 * it: scan a bf16 SHADOW of the adapted rows at half the bytes, rescore a small candidate set in fp32 with the scan's own bits,
 * prove on the device that the budget's choice is unchanged (cone/inference.py:276-299 is the score,
 * run_on_video/cone_localizator.py:83-100 the stage it serves).  The library stays a plain fp32 library (flags 0: a CONE_SESSION_CERTIFIED
 * library is still refused everywhere) and every other entry runs on it unchanged; the shadow lives BESIDE it in its own
 * caller-owned arena and is a pure function of the adapted rows, row by row -- whoever writes or moves adapted rows re-indexes
 * those rows (cone_library_shadow_index), nothing teaches cone_library_move_rows a new plane.
 * CONTRACT: for a query with certified[q] == 1, cone_library_budget on the emitted wval produces bit for bit the outputs it
 * produces on cone_library_scan's lists at the same K, and the prefixes widx / wval[q, slot, :pair_k] of the chosen slots are the
 * fp32 scan's, bit for bit.  For certified[q] == 0 row q is well-formed (descending, padded) and the caller must not use it.
 * The rules are the libraries': all memory is the caller's, 256-B aligned, one stream, nothing allocated, no host read-back,
 * refusals by name from host values first, before any pointer is read. */

/* A plain host struct of device pointers into the caller's shadow arena; filled by cone_library_shadow_open. */
typedef struct {
    const cone_model* model;        /* the library's handle */
    int64_t capacity;               /* the library's capacity: row r of the shadow belongs to row r of lib->adapted */
    int32_t v_dim;
    uint16_t* rows_bf16;            /* (capacity, v_dim) round-to-nearest-even bf16 of lib->adapted */
    float* err;                     /* (capacity, 2) per row (r, n): r >= |v - bf16(v)|_2, n >= max(|v|_2, |bf16(v)|_2) */
} cone_library_shadow;

/* Bytes of a shadow arena for `lib` (2 v_dim + 8 per row, each plane rounded up to 256 B; 0 and cone_last_error on a refusal)
 * and its layout: launches nothing, writes nothing (run_on_video/cone_localizator.py:121-221 keeps no state).
 * Refused by name ("library_shadow: "): null arguments, a library that is not fp32 (flags != 0), capacity outside [1, 2^31), a
 * v_dim outside {256, 512, 768, 1024}, a misaligned or short arena. */
size_t cone_library_shadow_bytes(const cone_library* lib);
int cone_library_shadow_open(const cone_library* lib, void* arena, size_t arena_bytes, cone_library_shadow* out);

/* For rows [row0, row0 + n_rows): rows_bf16 = the round-to-nearest-even bf16 of lib->adapted (cone_prefilter_index_bf16's
 * bits, which are cone_rows_to_bf16's) and err[row] = (r, n) by that entry's arithmetic for ONE row -- the same fma chains,
 * butterfly, inflation and absolute term --, stored per row where that entry takes a maximum over the grid; a row with a
 * non-finite sum stores a NaN.  One wave per row, 16-B loads; nothing outside those rows is written (cone/inference.py:276-299:
 * the rows the coarse scores are taken from).
 * Refused by name ("library_shadow: "): null arguments, row0 < 0, n_rows < 1, row0 + n_rows > capacity, a shadow of another
 * library (capacity / v_dim / handle), another handle than the library's. */
int cone_library_shadow_index(const cone_model* m, const cone_library* lib, const cone_library_shadow* shadow, int64_t row0,
                              int64_t n_rows, void* stream);

/* cone_library_scan's window lists for a budget of W windows, from the shadow (run_on_video/cone_localizator.py:83-100;
 * cone/inference.py:276-299).  The table is cone_library_scan's plus v_win_off (n_videos + 1) int64: the exclusive prefix sums
 * of cone_num_windows(v_ctx_l, max_v_l); total_win = its last entry = total_hb + n_videos (the host knows it).
 * Stages, one stream: (1) the library scan's skeleton over rows_bf16 (bf16 operands, fp32 sums: cone_prefilter_scores_bf16's
 * streaming form, passes of at most 4 queries) into two planes (nq, total_hb); a table entry leaving [0, capacity) scores -inf;
 * rows outside the table are never addressed; (2) R = max r, N = max n over exactly the table's rows, a NaN sticks; (3) the
 * coarse window row (nq, total_win), window j of slot v at v_win_off[v] + j, from that video's own half-blocks; (4) the n_cand
 * best coarse entries as an unordered set (score descending, ties to the lower flat index), merged level by level; (5) the
 * candidates' exact fp32 scores off lib->adapted with cone_library_scan's bits; (6) per query: the candidates ordered by (exact
 * score descending, flat index ascending) are walked, skipping a candidate whose slot has already given min(K, its windows),
 * until W are taken; t = the last taken score, c_last = the smallest coarse score of the set; certified[q] = 1 iff every window
 * of the table is a candidate, or W were taken and t - c_last > E(q) strictly with every quantity finite (E: the certified
 * pre-filter's bound with the R, N of stage 2, in fp64).
 * Outputs (device): widx / wval (nq, n_videos, K) in the scan's layout, EVERY element written: -1 / -inf, then per slot its
 * taken candidates at positions 0.. in walk order (window index within the video, exact score); certified (nq) int32.  There
 * is no ranking output.  n_cand = 0: min(total_win, max(4 W, 128)); ws >= cone_library_scan_certified_workspace, 256-B aligned.
 * Refused by name ("library_scan_certified: "), from host values first: cone_library_scan's own (nq, n_videos, total_hb, K,
 * max_v_l, a CONE_SESSION_CERTIFIED or CONE_SESSION_BF16 library); W outside [1, 256]; total_win != total_hb + n_videos or
 * >= 2^31; n_cand outside [min(W, total_win), min(total_win, 4096)]; then null arguments, another handle, a shadow of another
 * library, a v_dim outside {256, 512, 768, 1024}, a misaligned or short workspace. */
size_t cone_library_scan_certified_workspace(const cone_library* lib, int64_t n_videos, int64_t total_hb, int64_t total_win, int nq,
                                             int K, int W, int n_cand);
int cone_library_scan_certified(const cone_model* m, const cone_library* lib, const cone_library_shadow* shadow,
                                const int64_t* v_row0, const int32_t* v_ctx_l, const int64_t* v_hb_off, const int64_t* v_win_off,
                                int64_t n_videos, int64_t total_hb, int64_t total_win, const float* cls, int nq, int K, int W,
                                int n_cand, const cone_session_params* params, int32_t* widx, float* wval, int32_t* certified,
                                void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------- metrics on the device
 * Recall@K / IoU counts from the kept rows (layout of cone_fuse_nms: rows (nq, max_after, 5) fp64 [st, ed, ...],
 * n (nq) valid rows) and one target span per query gt (nq, 2) fp64 seconds -- device pointers.  thresholds /
 * topk are HOST arrays (<= 8 / <= 16 entries).  hits (n_thr, n_topk) int64 on the device: number of queries
 * with a prediction of IoU > threshold among their first K rows; top1_iou (nq) fp64: IoU of the first row.
 * mode 0 = standalone_eval/evaluate_ego4d_nlq.py:41-60,93-103 (float64, union clamped at 0);
 * mode 1 = standalone_eval/evaluate_mad.py:33-38,87-104 (float32 arithmetic, thresholds as fp32). */
int cone_eval_recall(const double* rows, const int32_t* n, const double* gt, int nq, int max_after,
                     const double* thresholds, int n_thr, const int32_t* topk, int n_topk, int mode,
                     int64_t* hits, double* top1_iou, void* stream);
/* Window pre-filter recall, standalone_eval/evaluate_pre_filtered_window.py:45-66: win_idx (nq, k) int32 ranked
 * windows (-1 padded), gt (nq, 2) fp64 seconds; hits (n_topk) int64 = queries whose first K windows contain
 * one of floor(start/S) .. ceil(end/S), start/end in clips (seconds / clip_length), S = slide. */
int cone_eval_window_recall(const int32_t* win_idx, int nq, int k, const double* gt, double clip_length,
                            int slide, const int32_t* topk, int n_topk, int64_t* hits, void* stream);

/* -------------------------------------------------------------------- measurement
 * Opt-in per-launch timing with hipEvents on the launch stream (used by bench.py for the roofline
 * line).  cone_prof_enable(1) clears and starts recording, (0) stops.  After synchronising the
 * stream, cone_prof_collect fills up to max_rec records of 5 doubles {kind, a, b, c, milliseconds}:
 * kind 0/1/2 = GEMM tiles 128x128 / 128x128 with fused addend / 64x256 with fused LayerNorm, (a,b,c) =
 * (M rows actually processed, N, K); kind 3 = encoder attention (B windows, Lmax, source mode); kind 4 = frame-score
 * stream (ctx_l, dv, queries in the launch); kind 5/6 = 128x256 row-owning GEMM tile with 4 / 8 waves (M, N, K); kind 7 =
 * fused decoder cross-attention (B windows, Lmax, nq); kind 8 = fused feed-forward block on the persistent 128-row grid
 * (M rows, ff, 256): 4*M*ff*256 FLOPs; kind 9 = the same with the output projection: + 2*M*256*256.  One kind per KERNEL:
 * kinds 10 / 11 = kinds 8 / 9 computed by the wide form (ffn_wide_kernel: launches of a few row groups and the rows past the
 * last full round of a big launch -- a record of its own, with the rows it covered); 12 / 13 = the 64-row / 4-wave form;
 * 14 = the row GEMM's small form (16-row tiles).  The row GEMM's tall form (gemm_tall.hip: K = 256, many rows) books its launches
 * under kind 6 too: it computes what the 8-wave row tile computes, bit for bit, and the FLOP accounting by shape (M, N, K) of
 * that kind stays complete.  Returns the record count.  Not thread-safe. */
int cone_prof_enable(int on);
int64_t cone_prof_collect(double* out, int64_t max_rec);

/* -------------------------------------------------------------------- test hooks
 * Thin entry points onto single kernels so that parity tests can bisect; not needed by a binding. */
/* A/B switches of ONE model handle for the parity tests (not thread-safe; set them before using the handle).
 * "dec_fold" (default 2): decoder cross-attention with the memory K/V projections folded into one kernel per layer, its
 *   two 256-channel contractions on the matrix cores (dec_cross_mfma.hip).  2 = the first layer (the same queries for
 *   every window, windows of at most 128 tokens, position tables) on the rows-once form -- every memory row is read from
 *   HBM once, kept in registers and handed to the second contraction through LDS a 64-channel quarter at a time, two
 *   workgroups per CU -- and every other launch on the two-read form; 3 = the two-read form everywhere; 5 = the rows-once
 *   form wherever it can run (per-window queries too: measured slower there, its query fold has no idle issue slots to
 *   hide in); 4 (opt-in) = windows of at most 110 tokens on the LDS-resident persistent form (one HBM read per row as
 *   well, but one workgroup per CU: measured 1.3 - 1.4 x slower); 1 = on the VALU (dec_cross.hip); 0 = two stacked K/V
 *   GEMMs + per-head attention.
 * "l0_gather" (default 1): with a cone_layer0 cache the first encoder layer's attention gathers q|k|v from the
 *   caches in its staging loads; 0 = a packing kernel writes them to the workspace first.  Bit-identical.
 * "pos_tables" (default 1): later encoder layers and the decoder keys take the position term from the static
 *   tables of cone_layer0; 0 = from an x + pos matrix written by the previous layer's GEMM epilogue.
 * "dec0_const" (default 1): the first decoder layer's self-attention block and cross-attention queries (tgt = 0:
 *   the same for every window) are computed for one window and replicated; 0 = for all windows.  Bit-identical.
 * "ffn_fused" (default 2): 1 = linear1 + ReLU + linear2 + residual + LayerNorm of every transformer layer as ONE kernel
 *   that keeps the (M, dim_feedforward) hidden rows on chip (ffn.hip); 2 = the attention output projection + residual +
 *   LayerNorm ahead of it in that kernel too (everything of a layer behind its attention: one launch, the layer's
 *   intermediate rows never leave the CU); 0 = GEMMs through (M, 256) / (M, ff) buffers.
 * "split_bf16" (default 0, OPT-IN): every transformer layer's tail (ffn_fused 2) on the bf16 matrix cores -- each fp32
 *   product as six partial products of three-piece bf16 operands (x = xh + xm + xl exactly), fp32 accumulation
 *   (ffn_split.hip).  Measured against float64: the same error as the exact-fp32 MFMA chain (1.5e-7 .. 2.4e-7 of
 *   sum |a b| vs 2.0e-7 .. 2.1e-7), at 1.65x its speed.  The default stays exact fp32.
 * "bf16" (default 0, OPT-IN; excludes split_bf16: setting either to 1 while the other is 1 is an error): the GEMMs that
 *   split_bf16 moves to the bf16 matrix cores -- attention output projection, linear1, linear2, the next layer's fused
 *   q | k | v projection, the K = 256 row GEMMs, and here the first layer's q | k | v rows too (cone_layer0_project and the
 *   uncached first layer alike) -- with every operand rounded ONCE to bf16 (round to nearest even) and ONE MFMA per operand
 *   pair, fp32 accumulation (ffn_bf16.hip; weight images of one third the bytes).  Everything else -- bias, ReLU, the
 *   residual (taken from the unrounded fp32 input), LayerNorm, attention, decoder cross-attention, input projections, heads,
 *   matching, and all of stage A -- stays fp32 and activations stay fp32 in memory.  NOT fp32-accurate: errors are those
 *   of bf16 operands (bounded by the reference model's own bf16-autocast error, tests/test_bf16_gpu.py).  Needs what
 *   split_bf16 needs (hidden_dim 256, 8 heads, dim_feedforward % 32 == 0); 0 is always accepted.  --pre_norm handles run
 *   the pre-norm form of the same kernels (fused table path).  Every tail takes the 128-row-tile kernel whatever the row
 *   count (no spread form): for a handful of windows the default path can be the faster one.  With the diagnostic
 *   switches ffn_fused < 2 or pos_tables 0 the tails run fp32 while the q | k | v row GEMMs stay bf16 (A/B use only).
 * "qkv_fused" (default 1): the next encoder layer's q | k | v projection is computed by the fused layer tail from the
 *   registers that hold its output rows: 1 = on the split_bf16 path (bit-identical to the separate launch), 2 = on the
 *   exact-fp32 path as well (measured neutral; another summation order than the GEMM launch), 0 = always its own launch.
 * "res_gather" (default 1, with ffn_fused 2 + l0_gather + pos_tables): the first encoder layer's residual rows are read
 *   by the fused layer tail straight from the projected clip / text rows through a row index; 0 = from a packed copy of
 *   the layer input written by a packing pass.  Bit-identical.
 * "rows_chain" (default 1): for few rows (the regime of the row GEMM's 16-row form) decoder.norm + class head + span MLP +
 *   span head of a decoder layer, and the adapter pair of the proposal matching (d = 256 features), run as ONE launch each
 *   with the rows on chip in between (rows_chain.h); 0 = the separate launches.  Bit-identical.
 * "ffn_spread" (default 1): a projecting layer tail of at most 1 024 rows (the decoder slot rows of a small batch, the token
 *   rows of a few windows) runs as four launches over single-wave workgroups (ffn_wide.hip, fs_*_kernel) instead of one CU
 *   per 16 rows walking the whole block, and a row GEMM of at most 1 024 rows without a LayerNorm epilogue as one wave per
 *   16 x 16 output tile; 0 = the wide form / the workgroup-per-16-rows form.  Bit-identical.
 * "max_window_tokens" (default 256 = CONE_MAX_WINDOW_TOKENS; 256 .. 1024 = CONE_MAX_LONG_WINDOW_TOKENS, anything else is an
 *   error): the longest window (clips + text tokens) the handle's forwards accept; one token more is rejected by name.  A
 *   handle left at 256 is unchanged in every respect.  Above 256 the handle is a general-path handle: EVERY forward, through
 *   either entry and whatever the call's own Lv_max + Lq_max, runs the general launch sequence (x + pos materialised; no
 *   position tables, layer-0 caches or fused-path forms are read, and the fused path's A/B options are ignored as on a handle
 *   of another shape than 256 / 8) with the streaming attention core (general.hip: gen_attn_stream_kernel) for the encoder
 *   self-attention and the decoder cross-attention, so that a window's bits depend neither on its batch nor on the entry.
 *   Exact fp32 unless "general_bf16" is set: "bf16" / "split_bf16" = 1 are refused on such a handle, and raising the option is
 *   refused while one is on.
 * "general_bf16" (default 0, OPT-IN; a switch of its own, independent of bf16 / split_bf16 / max_window_tokens in either set
 *   order): the general path's layer GEMMs -- encoder q | k (the x + pos form), v, attention output projection, linear1,
 *   linear2; the stacked decoder K (memory + pos) and V; the decoder's self-attention in-projection (slot table as row-periodic
 *   residual) and output projection, cross-attention query and output projections, linear1, linear2; post-norm and pre-norm
 *   alike -- with both operands rounded ONCE to bf16 (round to nearest even; x + pos is summed in fp32 first), one
 *   v_mfma_f32_16x16x32_bf16 per operand pair, fp32 accumulation (gemm_bf16.hip).  Bias, ReLU, the residual (never rounded),
 *   every LayerNorm, both attention cores, the heads and saliency, the per-checkpoint tables, the input projections and the
 *   adapter stay fp32, and activations stay fp32 in memory (rows are rounded in flight).  NOT fp32-accurate: errors are those
 *   of bf16 operands (bounded by the reference model's own bf16-autocast error, tests/test_general_bf16_gpu.py).  1 is
 *   accepted when the handle runs the general path at that moment (another shape than 256 / 8, max_window_tokens above 256,
 *   or general_shape = 1) and dim_feedforward % 32 == 0 and <= 2048; else it is refused by name (a fused-path handle is
 *   pointed at "bf16").  The first 1 builds the weights' bf16 images (a few MB, synchronously; kept until
 *   cone_model_destroy); a failed build returns the error and leaves the option at 0.  0 is always accepted.  A later
 *   general_shape = 0 leaves the option set and inert: the fused path never reads it.
 * "gemm" (default 0 = by shape): tile family of every dense layer: 1 = register-staged 128x128 / 64x256 tiles,
 *   2 / 3 = 128x256 row-owning LDS-DMA tile with 4 waves x 32 rows (32x32x2) / 8 waves x 16 rows (16x16x4) -- all
 *   exact-fp32 fma chains per output element that walk k in different orders; 4 = the tall form of the row GEMM
 *   (gemm_tall.hip: K = 256, N % 32 == 0, no addend / second output / LayerNorm epilogue / periodic residual; the bits of 3),
 *   a launch it cannot run is refused by name.
 * "gemm_tall_min_rows" (default -1 = the built-in threshold): automatic launches of at least this many rows (host bound) that
 *   the tall form can run take it; 0 = never.  The bits do not depend on it.
 * "tail_packed" (additive, ABI 8; switch, default 1): the weight stream of the persistent row kernel of the exact-fp32 layer
 *   tail: 1 = from the handle's packed slab images (built at cone_model_create from the weights, freed with the handle: the
 *   ring's chunks in walking order, gather and swizzle resolved once), 0 = gathered from the row-major matrices.
 * "gemm_tall_packed" (additive, ABI 8; switch, default 0): the same for the tall row GEMM; its images (the N = 768
 *   in-projections) are built at the first 1, synchronously, and kept until cone_model_destroy; a tall launch whose weight has
 *   no image streams row-major.  Measured inside the noise against the row-major stream, hence off.
 *   The LDS contents are the same bytes in either form, so the bits depend on neither option. */
int cone_model_set_option(cone_model* m, const char* name, int value);
/* C = epi((A [+ A2]) W^T + bias); flags: 1 relu, 2 add residual R, 4 LayerNorm(g,b) (N must be 256), 8 = keep a launch of a few
 * row groups on the workgroup-per-16-rows form (else: one wave per 16 x 16 output tile, same bits);
 * bits 8-9 force a tile family (1 = 128x128 / 64x256 register-staged tiles, 2 = 128x256 row-owning LDS-DMA tile
 * with 4 waves x 32 rows, 3 = the same tile with 8 waves x 16 rows, 0 = automatic = 3 where the shape allows).  Optional second output C2 = C + ADD (row tile only). */
int cone_test_gemm(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                   const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                   const float* ADD, int M, int N, int K, int flags, void* stream);
/* cone_test_gemm with row strides lda / ldc (0: K / N; R shares ldc), a device-side row count M_dev (may be null) and, in bits
 * 8-10 of flags, the tile family including 4 = the tall form (gemm_tall.hip); bit 11 keeps an automatic launch (family 0) off the
 * tall form whatever its row count (the shipped forms, for A/B timing).  n_cu > 0: the tall form itself on a persistent
 * grid sized for n_cu CUs, so that a few hundred rows make a workgroup walk several tiles; n_cu == 0: through the dispatcher. */
int cone_test_gemm_tall(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                        const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                        const float* ADD, int M, int N, int K, int flags, int lda, int ldc, const int32_t* M_dev,
                        int n_cu, void* stream);
/* ---- packed fp32 weight streams (additive, ABI 8; tests and benchmarks only).  An image is a sequence of 32-KiB chunks
 * [slab 0..31][lane 0..63][4 floats]; with row = lane / 4, ch = (lane % 4) ^ ((0x1230 >> (4 * ((row / 4) % 4))) & 3):
 *   projection format, chunk c of W (N, 256):  slab s = W[32 c + 16 (s / 16) + row][16 (s % 16) + 4 ch ..]
 *   feed-forward format, chunk c:              slab s < 16 = W1[16 c + row][16 s + 4 ch ..], slab 16 + t = W2[16 t + row][16 c + 4 ch ..]
 * cone_test_f32_pack_tail: [Wo != NULL: its 8 chunks | ff / 16 feed-forward chunks | Wq != NULL: n_qkv / 32 chunks of Wq];
 * cone_test_f32_pack_rows: the N / 32 chunks of W.  The *_bytes entries return the image size (0: unsupported). */
size_t cone_test_f32_pack_tail_bytes(int ff, int proj, int n_qkv);
int cone_test_f32_pack_tail(const float* Wo, const float* W1, const float* W2, int ff, const float* Wq, int n_qkv, void* img,
                            void* stream);
size_t cone_test_f32_pack_rows_bytes(int N);
/* launches that streamed a packed image since the library was loaded: which 0 = the layer tail's row kernel, 1 = the tall GEMM */
long cone_test_f32_packed_launches(int which);
int cone_test_f32_pack_rows(const float* W, int N, void* img, void* stream);
/* The tall form itself (K = 256, contiguous operands; flags 1 relu, 2 residual R) streaming W's packed image img (NULL: the
 * row-major matrix); n_cu > 0 sizes the persistent grid. */
int cone_test_gemm_tall_packed(const float* A, const float* W, const float* bias, const float* R, float* C, int M, int N,
                               int flags, const int32_t* M_dev, int n_cu, const void* img, void* stream);
/* The persistent row kernel of the exact-fp32 tail (cone_test_proj_ffn's operands) streaming the packed image img (NULL: the
 * row-major matrices).  A == NULL: the feed-forward block alone on R as its input (an image without Wo chunks); Wq != NULL: with
 * the q | k | v ride, QKV (M, n_qkv) = OUT Wq^T + qb (an image with the Wq chunks); pre: the pre-norm form (OUT2 may be NULL);
 * nw = 8 (128-row tiles) | 4 (64-row tiles; no ride, no pre-norm form); n_cu > 0 sizes the persistent grid. */
int cone_test_tail_packed(const float* A, const float* Wo, const float* bo, const float* R, const float* pg, const float* pb,
                          const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                          const float* ln_b, float* OUT, int M, int ff, int pre, float* OUT2, const float* Wq, const float* qb,
                          float* QKV, int n_qkv, int nw, int n_cu, const void* img, void* stream);
/* The row GEMM of option "general_bf16" (gemm_bf16.hip): cone_test_gemm's arguments and
 *   C[m][n] = sum_k bf16(A[m][k] (+ A2[a2_mod ? m % a2_mod : m][k], added in fp32 first)) * bf16(W[n][k])   (fp32 accumulation)
 *             + bias[n],  then ReLU (flag 1),  then + R[r_mod ? m % r_mod : m][n] (flag 2; the residual is never rounded)
 * N a multiple of 16, K a multiple of 32 up to 2048 (cone_test_gemm_bf16_image_bytes returns 0 otherwise).  ln_g / ln_b /
 * flag 4, C2 / ADD are refused by name.  img: cone_test_gemm_bf16_image_bytes(N, K) bytes, into which W's bf16 image is
 * packed first; ldc: row stride of C (0 = N); r_mod: > 0 = the residual is row-periodic; M_dev: optional device-side row
 * count (rows past min(M, *M_dev) are not stored).  One tile form: a row's bits do not depend on M. */
size_t cone_test_gemm_bf16_image_bytes(int N, int K);
int cone_test_gemm_bf16(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                        const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                        const float* ADD, int M, int N, int K, int flags, void* img, int ldc, int r_mod,
                        const int32_t* M_dev, void* stream);
/* OUT = LayerNorm(X + W2 relu(W1 X + b1) + b2), the fused feed-forward block: X, OUT (M, 256), W1 (ff, 256), W2 (256, ff). */
int cone_test_ffn(const float* X, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* stream);
/* The same with the block input computed in the kernel: X = LayerNorm_p(R + A Wo^T + bo) -- the attention output projection,
 * its residual and norm (A, R (M, 256); Wo (256, 256)).  OUT may be R (in place). */
int cone_test_proj_ffn(const float* A, const float* Wo, const float* bo, const float* R, const float* pg, const float* pb,
                       const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                       const float* ln_b, float* OUT, int M, int ff, void* stream);
/* pack, in the three entries below: CONE_TEST_PACK = build the weight image(s) first; | CONE_TEST_SINGLE_PIECE = the
 * single-piece form of option "bf16" (operands rounded once, one MFMA per pair, ffn_bf16.hip), whose images fit the same
 * scratch sizes. */
#define CONE_TEST_PACK 1
#define CONE_TEST_SINGLE_PIECE 2
/* cone_test_ffn on the bf16 matrix cores (ffn_split.hip): every fp32 product as six partial products of three-piece bf16
 * operands with fp32 accumulation.  img = scratch of cone_test_ffn_split_image_bytes(ff) bytes for the split weight image
 * (pack != 0: built from W1 / W2 first; 0: reused from an earlier call). */
size_t cone_test_ffn_split_image_bytes(int ff);
int cone_test_ffn_split(const float* X, const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* img, int pack, void* stream);
/* C (M, N) = X (M, 256) W^T + bias (W (N, 256), N % 32 == 0) on the same split operands; img = scratch of
 * cone_test_rows_split_image_bytes(N) bytes. */
size_t cone_test_rows_split_image_bytes(int N);
int cone_test_rows_split(const float* X, const float* W, const float* bias, float* C, int M, int N, void* img, int pack,
                         void* stream);
/* The same block in its SPREAD form (ffn_wide.hip: four launches over single-wave workgroups; a handful of row groups only:
 * M <= CONE_FFN_SPREAD_MAX_ROWS); scratch of cone_test_proj_ffn_spread_scratch_bytes(ff) bytes.  Bit-identical rows. */
#define CONE_FFN_SPREAD_MAX_ROWS 1024
size_t cone_test_proj_ffn_spread_scratch_bytes(int ff);
int cone_test_proj_ffn_spread(const float* A, const float* Wo, const float* bo, const float* R, const float* pg, const float* pb,
                              const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                              const float* ln_b, float* OUT, int M, int ff, void* scratch, void* stream);
/* cone_test_proj_ffn in ONE forced form of the exact-fp32 tail (tests only; no option or production path reads this):
 * 128-row / 64-row persistent kernel, wide, spread (scratch as above), or the row rules of the launcher's ladder for an
 * ASSUMED CU count n_cu (full rounds of n_cu 128-row tiles + the wide form on the rows past them; post-norm only).  Optional:
 * r_idx / R2 (residual row i = R[r_idx[i]] or R2[~r_idx[i]]), M_dev (device-side row count), pre (the pre-norm tail: OUT = the
 * stream, OUT2 (may be null) = its LayerNorm; no 64-row form). */
enum { CONE_TAIL_FORM_ROWS128 = 0, CONE_TAIL_FORM_ROWS64 = 1, CONE_TAIL_FORM_WIDE = 2, CONE_TAIL_FORM_LADDER = 3,
       CONE_TAIL_FORM_SPREAD = 4 };
int cone_test_tail_form(const float* A, const float* Wo, const float* bo, const float* R, const float* pg, const float* pb,
                        const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                        const float* ln_b, float* OUT, int M, int ff, const int32_t* r_idx, const float* R2,
                        const int32_t* M_dev, int pre, float* OUT2, int form, int n_cu, void* scratch, void* stream);
/* cone_test_proj_ffn on the bf16 matrix cores; wo_img = scratch of cone_test_proj_split_image_bytes() bytes. */
size_t cone_test_proj_split_image_bytes(void);
int cone_test_proj_ffn_split(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                             const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* img, void* wo_img,
                             int pack, void* stream);
/* ---- every form of the matrix-core layer tails and their row GEMM (additive, ABI 8; tests only: no option or production path
 * reads these).  pack selects the mode and whether the images are built first, as in the three entries above.
 * cone_test_tail_mc: cone_test_proj_ffn_split's operands, then
 *   A == NULL       the feed-forward block alone on R as its input (cone_test_ffn_split's computation; no r_idx, pre or Wq);
 *   r_idx / R2      the gathered residual: row i = R[r_idx[i]] where r_idx[i] >= 0, else R2[~r_idx[i]] (both with stride ldr);
 *                   r_idx without R2 is refused by name;
 *   M_dev           optional device-side row count: rows past min(M, *M_dev) are neither computed nor stored;
 *   pre, OUT2       the pre-norm form, single-piece mode only (the split mode refuses it by name): OUT = the un-normalised
 *                   stream, OUT2 (may be NULL: then nothing but OUT is written) = its LayerNorm;
 *   Wq, qb, QKV     Wq != NULL: the q | k | v ride, QKV (M, n_qkv) = OUT Wq^T + qb from the registers that hold OUT (post-norm
 *                   only; n_qkv % 32 == 0; a ride whose ring, parameter rows and bias exceed the 160 KiB of LDS is refused by name);
 *   lda, ldr, ldo, ldo2, ldq   row strides in floats of A, R / R2, OUT, OUT2, QKV: 0 = dense (256, n_qkv), else a multiple of 4;
 *   n_cu            > 0: the persistent grid is sized for that many CUs, so that a few hundred rows make a workgroup walk
 *                   several 128-row tiles; 0: the device's count (what every production launch uses); < 0 is refused by name;
 *   img, wo_img, q_img   scratch of cone_test_ffn_split_image_bytes(ff), cone_test_proj_split_image_bytes() (A != NULL) and
 *                   cone_test_rows_split_image_bytes(n_qkv) (Wq != NULL) bytes.
 * cone_test_rows_mc: cone_test_rows_split with row strides ldx / ldc (0 = 256 / N), M_dev and n_cu as above. */
int cone_test_tail_mc(const float* A, const float* Wo, const float* bo, const float* R, const float* pg, const float* pb,
                      const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                      const float* ln_b, float* OUT, int M, int ff, const int32_t* r_idx, const float* R2,
                      const int32_t* M_dev, int pre, float* OUT2, const float* Wq, const float* qb, float* QKV, int n_qkv,
                      int lda, int ldr, int ldo, int ldo2, int ldq, int n_cu, void* img, void* wo_img, void* q_img, int pack,
                      void* stream);
int cone_test_rows_mc(const float* X, const float* W, const float* bias, float* C, int M, int N, void* img, int pack, int ldx,
                      int ldc, const int32_t* M_dev, int n_cu, void* stream);
/* Encoder self-attention core (cone/transformer.py:239, 8 heads x 32) over windows of packed tokens off[b] .. off[b+1]:
 * mode 0: QKV (M, 768) = q | k | v rows that already carry the position term; mode 2: the same without it, the kernel adds
 * pos_qk[(vlen[b], p)] (R, 512) to q | k of clip token p; mode 1: q | k | v gathered from per-clip rows qkv_vid[vrow0[b] + p]
 * and per-text-token rows qkv_txt[trow0[b] + t] (+ the pos_qk row for clips).  OUT (M, 256) ahead of out_proj.
 * mode | 0x200 (windows of <= 144 tokens) runs the second formulation -- one wave per (window, head), K / V resident in
 * registers, no LDS: the same bits as the default workgroup-per-(window, head) kernel. */
int cone_test_enc_attn(int mode, const float* QKV, const float* qkv_vid, const float* qkv_txt, const float* pos_qk,
                       const int32_t* vrow0, const int32_t* vlen, const int32_t* trow0, const int32_t* off, float* OUT,
                       int B, int Lmax, int pos_zero_row /* index of an all-zero row of pos_qk (modes 1, 2) */, void* stream);
/* Fused decoder cross-attention of one layer (cone/transformer.py:308-311) with the memory K / V projections folded in:
 * DQ (B * nq, 256) projected queries (+ bias), X (M, 256) memory rows packed by off (B + 1), pos_rows / vlen = the sine
 * table and the clip count of each window (keys = memory + position row for clip tokens), Wk (256, 256) = rows
 * 256 .. 511 of in_proj_weight, WvT (256, 256) = W_v transposed, bv (256).  OUT (B * nq, 256) = attention output ahead
 * of out_proj.  variant = the "dec_fold" value (cone_model_set_option): 2 default policy, 3 two-read, 5 rows-once, 4 LDS-
 * resident, 1 VALU.  qk_slabs != NULL (matrix-core forms): every window has the SAME nq query rows, the folded operand is
 * built once into that scratch of cone_test_dec_cross_slab_floats() floats. */
int cone_test_dec_cross(const float* DQ, const float* X, const float* pos_rows, const int32_t* vlen, const int32_t* off,
                        const float* Wk, const float* WvT, const float* bv, float* OUT, int B, int nq, int Lmax,
                        int variant, float* qk_slabs, void* stream);
size_t cone_test_dec_cross_slab_floats(void);
/* cone_test_enc_attn plus the text position rows of --use_txt_pos: txt_pos_qk (n_txt, 512) != NULL makes a text token j of
 * window b add row txt_pos_qk[trow0[b] + j] to its q | k instead of the zero row (modes 1 and 2: the ATTN_GATHER | 4 and
 * ATTN_POSADD | 4 builds; mode 0 ignores it).  txt_pos_qk == NULL: cone_test_enc_attn. */
int cone_test_enc_attn_txt(int mode, const float* QKV, const float* qkv_vid, const float* qkv_txt, const float* pos_qk,
                           const float* txt_pos_qk, const int32_t* vrow0, const int32_t* vlen, const int32_t* trow0,
                           const int32_t* off, float* OUT, int B, int Lmax, int pos_zero_row, void* stream);
/* The decoder's small attentions (cone/transformer.py:296-311, 8 heads x 32): nq <= 16 query rows b * nq .. of Q per window.
 * off == NULL: self-attention over the window's own nq rows of K / V; otherwise cross-attention to rows off[b] .. off[b + 1]
 * of K / V (<= 192 keys).  ld* = floats per row; OUT row b * nq + i, 256 columns. */
int cone_test_small_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* OUT, int ldo,
                         const int32_t* off, int B, int nq, int Lmax, void* stream);
/* cone_test_dec_cross with the remaining operands of its launchers: XP (M, 256) != NULL = the precomputed memory + pos
 * rows the keys are projected from (the --use_txt_pos decoder; pos_rows / vlen may then be NULL, X still feeds the values);
 * sal != NULL (matrix-core table forms): the launch also writes sal[b * sal_ld + p] = <X row of clip p, sal_w> + sal_b[0]
 * for p < min(vlen[b], sal_ld) and leaves the other entries alone.  What a form does not support it refuses by name. */
int cone_test_dec_cross_ex(const float* DQ, const float* XP, const float* X, const float* pos_rows, const int32_t* vlen,
                           const int32_t* off, const float* Wk, const float* WvT, const float* bv, float* OUT, int B, int nq,
                           int Lmax, int variant, float* qk_slabs, const float* sal_w, const float* sal_b, float* sal,
                           int sal_ld, void* stream);
int cone_test_layernorm(const float* x, const float* g, const float* b, float* out, int64_t n_rows,
                        int dim, void* stream);
/* Attention core of the general-shape path (any hidden_dim / nheads with head_dim in {16, 32, 64}): one workgroup per
 * (window b, head).  Query rows qoff[b] .. qoff[b + 1] of Q (qoff == NULL: the nq rows b * nq ..), key / value rows koff[b] ..
 * koff[b + 1] of K / V (koff == NULL: b * nq ..); head h reads / writes columns h * head_dim ..  OUT = softmax(q k^T /
 * sqrt(head_dim)) v per query row, ahead of out_proj; a window without queries or keys writes nothing.  kcap >= the longest key
 * count, <= 1024 (CONE_MAX_LONG_WINDOW_TOKENS).  kcap <= 256 (CONE_MAX_WINDOW_TOKENS): the LDS-resident kernel (all keys and
 * values of the window staged once, lane-per-key fma chains); kcap > 256: the streaming kernel (64-key blocks through LDS,
 * online softmax, fp32 matrix cores), whose result for a window depends neither on kcap nor on the other windows of the call. */
int cone_test_gen_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* OUT, int ldo,
                       const int32_t* qoff, const int32_t* koff, int B, int nq, int heads, int head_dim, int kcap, void* stream);

/* The glue kernels of stage B (window_ops.hip, rowops.hip, general.hip), one entry per internal launcher: exactly the launch
 * the forward path issues, on raw operand pointers, with no arithmetic and no argument checks of its own -- every pointer
 * must cover what the kernel touches.  All int arrays are int32 on the device.  d-wide ("gen") forms: d % 4 == 0, d <= 512.
 * Window b holds vlen[b] clip rows then qlen[b] token rows; off (B + 1) is the exclusive prefix sum of vlen + qlen. */
/* the device's maxGridSize[1] as cone_forward_packed / cone_forward_windows read it (0: the query failed) */
int cone_test_grid_limit_y(void);
/* off[0 .. B] = exclusive prefix sum of vlen[b] + qlen[b]; qlen == NULL: of vlen alone (the padded entry's two scans).
 * Writes exactly B + 1 ints.  One 1024-thread workgroup, any B >= 0. */
int cone_test_scan_lengths(const int32_t* vlen, const int32_t* qlen, int B, int32_t* off, void* stream);
/* vidx[voff[b] + p] = b * Lv_pad + p for p < min(vlen[b], Lv_pad), tidx[toff[b] + p] = b * Lq_pad + p for p <
 * min(qlen[b], Lq_pad); nothing else is written.  B in gridDim.y. */
int cone_test_compact_index(const int32_t* vlen, const int32_t* voff, int Lv_pad, int32_t* vidx, const int32_t* qlen,
                            const int32_t* toff, int Lq_pad, int32_t* tidx, int B, void* stream);
/* d = 256.  Row off[b] + p of X = vproj row vrow0[b] + p (p < vlen[b]) or tproj row trow0[b] + p - vlen[b]; of POS = the
 * sine row (vlen[b], p) computed per token from dim_t (256 floats) -- any vlen, no table -- or, for a token, zeros (tpe ==
 * NULL) / LayerNorm(x + tpe[p - vlen[b]]; tpg, tpb); XP = X + POS.  Rows off[B] .. are not written.  Lmax >= the longest
 * window.  X, POS and XP must all be given. */
int cone_test_pack_pos(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj, const int32_t* trow0,
                       const int32_t* qlen, const int32_t* off, const float* dim_t, float* X, float* POS, float* XP, int B,
                       int Lmax, const float* tpe, const float* tpg, const float* tpb, void* stream);
/* the same d wide, X and POS only (dim_t: d floats) */
int cone_test_gen_pack_pos(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj,
                           const int32_t* trow0, const int32_t* qlen, const int32_t* off, const float* dim_t, float* X, float* POS,
                           int d, int B, int Lmax, const float* tpe, const float* tpg, const float* tpb, void* stream);
/* d = 256.  X as cone_test_pack_pos.  POS != NULL: the sine row / zeros.  QK != NULL (then V too): QK row (512 floats) =
 * q | k of qkv_vid[clip] (768 floats per row) + pos_qk row vlen (vlen - 1) / 2 + p (512 floats per row), V row = its v part;
 * a token takes qkv_txt[token] unchanged.  POS == NULL / QK == NULL: that output is not touched and its inputs are not read. */
int cone_test_pack_l0(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj, const int32_t* trow0,
                      const int32_t* qlen, const int32_t* off, const float* dim_t, const float* qkv_vid, const float* qkv_txt,
                      const float* pos_qk, float* X, float* POS, float* QK, float* V, int B, int Lmax, void* stream);
/* ridx[off[b] + p] = vrow0[b] + p for a clip, ~(trow0[b] + p - vlen[b]) for a token */
int cone_test_row_index(const int32_t* vrow0, const int32_t* vlen, const int32_t* trow0, const int32_t* qlen, const int32_t* off,
                        int32_t* ridx, int B, int Lmax, void* stream);
/* d = 256.  XP row off[b] + p = MEM row + pos_rows row vlen (vlen - 1) / 2 + p for a clip; for a token MEM row + txt_pos row
 * trow0[b] + p - vlen[b], or (txt_pos == NULL: trow0 is then not read) the MEM row unchanged. */
int cone_test_add_pos_rows(const float* MEM, const int32_t* off, const int32_t* vlen, const float* pos_rows, float* XP, int B,
                           int Lmax, const float* txt_pos, const int32_t* trow0, void* stream);
/* out row i = LayerNorm(tproj row i + tpe row j; tpg, tpb), eps 1e-5, for i < (n_dev ? min(*n_dev, n) : n); j = tok_index[i],
 * or (tok_index == NULL) src_row[i] % mod; j is clamped to [0, n_emb - 1].  Rows past the count are not written. */
int cone_test_txt_pos_rows(const float* tproj, const int32_t* tok_index, const int32_t* src_row, int mod, int n_emb,
                           const float* tpe, const float* tpg, const float* tpb, int n, const int32_t* n_dev, float* out,
                           void* stream);
int cone_test_gen_txt_pos_rows(const float* tproj, const int32_t* tok_index, const int32_t* src_row, int mod, int n_emb,
                               const float* tpe, const float* tpg, const float* tpb, int n, const int32_t* n_dev, int d,
                               float* out, void* stream);
/* sal (B, Lv_out), may be NULL: <MEM row off[b] + p, w> + bias[0] for p < vlen[b], +0.0 for vlen[b] <= p < Lv_out.  mem_tap
 * (B, Lv_out + Lq_out, d), may be NULL: rows [0, Lv_out) = the window's clip rows then zero rows, rows [Lv_out, +Lq_out) =
 * its token rows then zero rows.  Lv_out >= every vlen, Lq_out >= every qlen (TRUSTED). */
int cone_test_saliency(const float* MEM, const int32_t* off, const int32_t* vlen, const int32_t* qlen, const float* w,
                       const float* bias, float* sal, int Lv_out, float* mem_tap, int Lq_out, int B, void* stream);
int cone_test_gen_saliency(const float* MEM, const int32_t* off, const int32_t* vlen, const int32_t* qlen, const float* w,
                           const float* bias, float* sal, int Lv_out, float* mem_tap, int Lq_out, int B, int d, void* stream);
/* out[r * ldo + n] = act(<X row r (ldx floats apart, ldx % 4 == 0), W row n> + b[n]), n < nout <= 2; act 1: the sigmoid
 * 1 / (1 + exp(-s)).  Nothing else of out is written. */
int cone_test_rowdot(const float* X, int ldx, const float* W, const float* b, float* out, int ldo, int64_t n_rows, int nout,
                     int act, void* stream);
int cone_test_gen_rowdot(const float* X, int ldx, const float* W, const float* b, float* out, int ldo, int64_t n_rows, int nout,
                         int act, int d, void* stream);
/* 256-float rows.  tile_rows: rows [period, n_rows) of x = row r % period of x (n_rows <= period: nothing is launched).
 * tile_rows2: rows [0, n_rows) of d0 / d1 = row r % period of s0 / s1. */
int cone_test_tile_rows(float* x, int period, int64_t n_rows, void* stream);
int cone_test_tile_rows2(float* d0, const float* s0, float* d1, const float* s1, int period, int64_t n_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONE_HIP_H */
