// Model handle, workspace carving and the launch sequences behind the C ABI (include/cone_hip.h).
//
// The window model runs on PACKED tokens: window b owns rows off[b] .. off[b+1] of every (M,*)
// activation matrix (its valid video clips, then its valid text tokens).  Padded keys never exist,
// so no masks are needed, and every dense layer is one tall GEMM over all windows of the batch.
#include <stdarg.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "gemm_tall.h"
#include "rows_chain.h"

namespace cone {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Linear { const float* w = nullptr; const float* b = nullptr; };
struct LNorm { const float* g = nullptr; const float* b = nullptr; };
struct Mha { const float* in_w = nullptr; const float* in_b = nullptr; Linear out; };
struct EncLayer { Mha sa; Linear l1, l2; LNorm n1, n2; };
struct DecLayer { Mha sa, ca; Linear l1, l2; LNorm n1, n2, n3; };

}  // namespace cone

struct cone_model {
    int d, heads, ff, n_enc, n_dec, nq, n_proj, dt, dv, dvm, has_adapter;     // dv: appearance clips (pre-filter, matching), dvm: motion clips (window model)
    float* arena = nullptr;  // every weight, one allocation
    cone::LNorm vproj_ln[CONE_MAX_PROJ], tproj_ln[CONE_MAX_PROJ];
    cone::Linear vproj[CONE_MAX_PROJ], tproj[CONE_MAX_PROJ];
    cone::EncLayer enc[CONE_MAX_LAYERS];
    cone::DecLayer dec[CONE_MAX_LAYERS];
    cone::LNorm dec_norm;
    const float* query_embed = nullptr;
    cone::Linear class_embed, span[3], saliency, adapter[2];
    const float* dim_t = nullptr;
    const float* txt_pos_emb = nullptr; int txt_pos_rows = 0; cone::LNorm txt_pos_ln;     // --use_txt_pos (NULL: off)
    int pre_norm = 0; cone::LNorm enc_norm;   // --pre_norm: normalize_before + the encoder's final LayerNorm
    // derived: the cross-attention K / V projections of all decoder layers stacked along N
    cone::Linear dec_k, dec_v;
    // derived: W_v^T of each decoder layer's cross-attention (256x256, [c][o]) for the fused cross-attention
    const float* dec_vT[CONE_MAX_LAYERS] = {};
    // derived: the first decoder layer's window-independent rows (tgt = 0, cone/transformer.py:66: its self-attention block
    // and its cross-attention queries depend on the checkpoint only): norm1 output (nq, 256) and the cross-attention query
    // projection (nq, 256), computed once at creation by the same kernels a step would run on ONE window's rows
    float* dec0_tgt1 = nullptr; float* dec0_dq = nullptr; float* dec0_scratch = nullptr;
    // derived: the slot-position term of the decoder's projections.  q = k = (tgt + query_embed) W^T + b is linear, so
    // (tgt + qe) W^T + b = tgt W^T + (qe W^T + b): per layer a (nq, 768) table [qe W_q^T + b_q | qe W_k^T + b_k | b_v] for the
    // self-attention in_proj (ONE N = 768 GEMM on tgt, the table as a row-periodic residual) and a (nq, 256) table
    // qe W_q^T + b_q for the cross-attention query projection -- the same move as the encoder's position tables
    float* dec_sa_tab[CONE_MAX_LAYERS] = {}; float* dec_ca_tab[CONE_MAX_LAYERS] = {};
    // derived (ABI 6; sized by cone_weights.table_max_v_l since ABI 8): the static position tables of this checkpoint (row
    // lv (lv - 1) / 2 + p: the same rows whatever the bound) -- every entry point runs the table path without the caller
    // building anything (cone_forward_windows, cone_forward_packed without a cone_layer0 or with caches only)
    float* tab_arena = nullptr; const float* tab_pos_rows = nullptr; const float* tab_pos_qk = nullptr; int tab_max_v_l = 0;
    // A/B switches of THIS handle (cone_model_set_option; parity tests only).  Defaults = the fast paths.
    int opt_dec_fold = 2;     // decoder memory K/V projections folded into the cross-attention kernel: 2 .. 5 = on the matrix
                              // cores (dec_cross_mfma.hip; which form: see launch_dec_cross_mfma), 1 = on the VALU
                              // (dec_cross.hip), 0 = K/V GEMMs + small_attn
    int opt_dec0_const = 1;   // first decoder layer's window-independent rows computed once and replicated
    int opt_l0_gather = 1;    // first encoder layer's attention gathers q|k|v from the layer-0 caches itself
    int opt_pos_tables = 1;   // later layers / decoder keys take the position term from the static tables
    int opt_gemm = 0;         // GEMM tile family forced for every dense layer (GEMM_AUTO = by shape)
    int opt_gemm_tall_min = -1;   // row threshold of the row GEMM's tall form (gemm_tall.hip): -1 = the built-in value, 0 = off
    // derived: every layer tail's operands (launch_layer_tail) -- the fp32 pointers and (d = 256, ff % 32 == 0) the weight
    // images of the two bf16 modes, each mode's in one allocation [encoder q | k | v images | per layer: Wo image, FFN image]:
    // split_img the three-piece images of ffn_split.hip, bf16_img the single-piece ones of ffn_bf16.hip (one third of the bytes)
    cone::TailWeights enc_tail[CONE_MAX_LAYERS] = {}, dec_tail[CONE_MAX_LAYERS] = {};
    char* split_img = nullptr; char* bf16_img = nullptr;
    int opt_qkv_fused = 1;    // the next encoder layer's q | k | v projection inside the fused layer tail (same launch): 1 = on
                              // the split_bf16 path (-0.3 ms), 2 = on the exact-fp32 path too (neutral), 0 = own launch
    int opt_split_bf16 = 0;   // OPT-IN: layer tails on the bf16 matrix cores (six partial products of three-piece operands,
                              // fp32 accumulation: fp32-MFMA accuracy); 0 = exact-fp32 MFMA (default)
    int opt_bf16 = 0;         // OPT-IN: the same GEMMs with operands rounded ONCE to bf16, one MFMA per operand pair, fp32
                              // accumulation (plain bf16 matrix arithmetic: NOT fp32-accurate); excludes split_bf16
    int opt_res_gather = 1;   // first encoder layer's residual rows gathered by the fused layer tail (no packed input copy)
    int opt_spread = 1;       // <= 16 row groups in a decoder tail: the spread form (four launches over single-wave workgroups)
    int opt_chain = 1;        // few rows: decoder.norm + class head + span MLP + span head, and the adapter pair of the proposal
                              // matching, as ONE launch each (rows_chain.h: the same arithmetic, bit-identical); 0 = separate launches
    int opt_ffn_fused = 2;    // 1: linear1 + ReLU + linear2 + residual + LayerNorm as one kernel (ffn.hip); 2: the attention
                              // output projection + residual + LayerNorm ahead of it in the same kernel as well; 0: GEMMs
    // the general-shape path (general.hip: plain LayerNorm / GEMM / attention launches at any supported d / heads): every
    // handle whose shape is not 256 / 8 (gen_native), or a 256 / 8 handle with option general_shape = 1 (A/B parity only)
    int gen_native = 0;
    int opt_general = 0;
    // OPT-IN (option general_bf16; general path only): its layer GEMMs -- encoder q | k, v, out_proj, linear1 / 2, the stacked
    // decoder K / V, the decoder's in-projections, out-projections and linear1 / 2 -- with operands rounded ONCE to bf16 on the
    // bf16 matrix cores (gemm_bf16.hip: NOT fp32-accurate).  Their weight images: one allocation, built at the first
    // general_bf16 = 1 and kept until the handle is destroyed, found by the fp32 weight's address.
    int opt_general_bf16 = 0;
    char* gen_bf16_img = nullptr;
    struct GenImage { const float* W; const void* img; };
    std::vector<GenImage> gen_bf16_images;
    // option max_window_tokens (default CONE_MAX_WINDOW_TOKENS; up to CONE_MAX_LONG_WINDOW_TOKENS): the longest window this
    // handle takes.  Above 256 EVERY forward of the handle runs the general path, whatever the call's own lengths, and its
    // attention launches carry this value as their key capacity (the streaming core of general.hip) -- a window's bits
    // depend neither on the batch it rides in nor on the entry it came through
    int opt_max_tokens = CONE_MAX_WINDOW_TOKENS;
    // derived (256 / 8 handles with an ff the fused tail takes): the packed fp32 weight streams of the two weight-ring kernels
    // (tail_pack.hip), freed with the handle: f32_img, built with the weights, per layer tail [Wo | W1 W2 | the riding layer's
    // q | k | v] (TailWeights::pk); f32_tall_img, built at the first gemm_tall_packed = 1 (the tall GEMM's default stream is
    // the row-major one), the N = 768 in-projections the tall row GEMM runs (encoder layers, decoder self-attention), found by
    // the weight's address (tall_image).  The options pick the stream form per kernel; the bits do not depend on them.
    char* f32_img = nullptr; char* f32_tall_img = nullptr;
    struct TallImage { const float* W; int N; const char* img; };
    std::vector<TallImage> tall_images;
    int opt_tail_packed = CONE_TAIL_PACKED_DEFAULT;         // the layer tail's row kernel streams its packed image
    int opt_gemm_tall_packed = CONE_GEMM_TALL_PACKED_DEFAULT;   // the tall row GEMM streams W's packed image where W has one
    // the image of the N rows at W: W may start at any multiple of 32 rows inside a packed matrix
    const void* tall_image(const float* W, int N) const {
        for (const TallImage& t : tall_images) {
            const uintptr_t w = (uintptr_t)W, base = (uintptr_t)t.W;        // (W may lie in another allocation: no pointer difference)
            if (w < base || (w - base) % (32 * 256 * sizeof(float)) != 0) continue;
            const size_t off = (w - base) / sizeof(float);
            if (off / 256 + (size_t)N <= (size_t)t.N) return t.img + (size_t)(off / (32 * 256)) * cone::F32_PACK_CHUNK_BYTES;
        }
        return nullptr;
    }
    bool long_windows() const { return opt_max_tokens > CONE_MAX_WINDOW_TOKENS; }
    bool general() const { return gen_native || opt_general || long_windows(); }
};

namespace cone {

// ------------------------------------------------------------------------------ weights
struct ArenaBuilder {
    struct Item { const float* src; size_t n; const float** dst; };
    std::vector<Item> items;
    size_t total = 0;
    void add(const float* src, size_t n, const float** dst) {
        items.push_back({src, n, dst});
        total += align_up(n, 64);
    }
};

static int dec0_constants(cone_model* m, hipStream_t s);
static int build_pos_tables(const cone_model* m, int max_v_l, float* pos_rows, float* pos_qk, hipStream_t s);
static int64_t pos_table_rows(int max_v_l) { return (int64_t)max_v_l * (max_v_l + 1) / 2 + 1; }

static void free_model(cone_model* m) {
    if (m->arena) (void)hipFree(m->arena);
    if (m->split_img) (void)hipFree(m->split_img);
    if (m->bf16_img) (void)hipFree(m->bf16_img);
    if (m->gen_bf16_img) (void)hipFree(m->gen_bf16_img);
    if (m->f32_img) (void)hipFree(m->f32_img);
    if (m->f32_tall_img) (void)hipFree(m->f32_tall_img);
    if (m->tab_arena) (void)hipFree(m->tab_arena);
    delete m;
}

// One numeric mode's weight images of every layer tail (13 MB split_bf16 / 4.4 MB bf16 at ff = 1024; opt-in paths), one
// allocation: the encoder layers' q | k | v projections (768 x 256), then per layer (encoder, decoder) [Wo image | FFN image].
static const TailMode* const TAIL_MODES[TAIL_IMG_MODES] = {&TAIL_MODE_SPLIT, &TAIL_MODE_BF16};
static int build_tail_images(cone_model* m, int mode, char** img) {
    const TailMode& k = *TAIL_MODES[mode];
    const size_t per = k.proj_image_bytes() + k.ffn_image_bytes(m->ff), qkv = k.rows_image_bytes(768);
    if (hipMalloc((void**)img, per * (size_t)(m->n_enc + m->n_dec) + qkv * (size_t)m->n_enc) != hipSuccess) {
        set_error("model_create: building the split-bf16 / bf16 weight images failed");
        return CONE_E_HIP;
    }
    char* ip = *img;
    for (int l = 0; l < m->n_enc; ++l, ip += qkv) {
        if (int rc = k.pack(m->enc_tail[l].Wq, nullptr, 768, ip, nullptr)) return rc;
        m->enc_tail[l].img[mode].qkv = ip;
    }
    for (int i = 0; i < m->n_enc + m->n_dec; ++i, ip += per) {
        TailWeights& t = i < m->n_enc ? m->enc_tail[i] : m->dec_tail[i - m->n_enc];
        if (int rc = k.pack(t.Wo, nullptr, 256, ip, nullptr)) return rc;
        if (int rc = k.pack(t.W1, t.W2, m->ff, ip + k.proj_image_bytes(), nullptr)) return rc;
        t.img[mode].wo = ip; t.img[mode].ffn = ip + k.proj_image_bytes();
    }
    return 0;
}

// The packed fp32 streams of the layer tails (cone_model::f32_img): 2.25 MB per tail at ff = 1024 (+ 0.75 MB where the next
// encoder layer's q | k | v projection can ride) -- 9.75 MB for the shipped two-plus-two layers.
static int build_f32_images(cone_model* m) {
    const int ff = m->ff, nl = m->n_enc + m->n_dec;
    size_t total = 0;
    for (int i = 0; i < nl; ++i) total += f32_pack_tail_bytes(ff, true, i + 1 < m->n_enc ? 768 : 0);
    if (hipMalloc((void**)&m->f32_img, total) != hipSuccess) {
        set_error("model_create: hipMalloc of %zu bytes of packed fp32 weight streams failed", total);
        return CONE_E_HIP;
    }
    char* ip = m->f32_img;
    for (int i = 0; i < nl; ++i) {
        TailWeights& t = i < m->n_enc ? m->enc_tail[i] : m->dec_tail[i - m->n_enc];
        const float* Wq = i + 1 < m->n_enc ? m->enc_tail[i + 1].Wq : nullptr;
        if (int rc = launch_f32_pack_tail(t.Wo, t.W1, t.W2, ff, Wq, 768, ip, nullptr)) return rc;
        t.pk = ip; t.pk_nq = Wq ? 768 : 0;
        ip += f32_pack_tail_bytes(ff, true, t.pk_nq);
    }
    return 0;
}
// The tall row GEMM's images (cone_model::f32_tall_img; 0.75 MB per N = 768 in-projection: encoder layers, decoder
// self-attention).  The tall GEMM's default stream is the row-major one (profiles/tail_packed_measured.txt), so these are
// built only where the packed one is asked for: at the first gemm_tall_packed = 1 (synchronously), kept until the handle goes.
static int build_tall_images(cone_model* m) {
    if (m->f32_tall_img) return 0;
    const int nl = m->n_enc + m->n_dec;
    if (hipMalloc((void**)&m->f32_tall_img, (size_t)nl * f32_pack_rows_bytes(768)) != hipSuccess) {
        set_error("gemm_tall_packed: hipMalloc of %zu bytes of packed fp32 weight streams failed", (size_t)nl * f32_pack_rows_bytes(768));
        return CONE_E_HIP;
    }
    char* ip = m->f32_tall_img;
    std::vector<cone_model::TallImage> images;
    int rc = 0;
    for (int i = 0; i < nl && rc == 0; ++i, ip += f32_pack_rows_bytes(768)) {
        const float* W = i < m->n_enc ? m->enc[i].sa.in_w : m->dec[i - m->n_enc].sa.in_w;
        rc = launch_f32_pack_rows(W, 768, ip, nullptr);
        images.push_back({W, 768, ip});
    }
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) {
        set_error("gemm_tall_packed: building the weight images failed");
        rc = CONE_E_HIP;
    }
    if (rc) { (void)hipFree(m->f32_tall_img); m->f32_tall_img = nullptr; return rc; }
    m->tall_images.swap(images);
    return 0;
}

static int build_model(const cone_weights* w, cone_model** out) {
    CONE_REQUIRE(w && out, "model_create: null argument");
    const bool shipped = w->hidden_dim == 256 && w->nheads == 8;
    CONE_REQUIRE(shipped || gen_shape_supported(w->hidden_dim, w->nheads),
                 "model_create: unsupported model shape hidden_dim=%d nheads=%d -- supported: hidden_dim a multiple of 64 in "
                 "[64, 512] with head_dim = hidden_dim / nheads in {16, 32, 64} (256 / 8, every shipped CONE configuration, runs "
                 "the fused kernels; other shapes the general path); also required: dim_feedforward a multiple of 128, "
                 "num_queries <= 16, feature dims multiples of 32 up to 1024, at most 256 tokens (clips + words) per window (up to 1024 with "
                 "option max_window_tokens)",
                 w->hidden_dim, w->nheads);
    CONE_REQUIRE(w->dim_ff % 128 == 0 && w->dim_ff >= 128, "model_create: dim_feedforward=%d must be a multiple of 128", w->dim_ff);
    CONE_REQUIRE(w->enc_layers >= 1 && w->enc_layers <= CONE_MAX_LAYERS && w->dec_layers >= 1 &&
                     w->dec_layers <= CONE_MAX_LAYERS, "model_create: layer counts out of range");
    CONE_REQUIRE(w->num_queries >= 1 && w->num_queries <= 16, "model_create: num_queries=%d not in [1,16]", w->num_queries);
    CONE_REQUIRE(w->n_input_proj >= 1 && w->n_input_proj <= CONE_MAX_PROJ, "model_create: n_input_proj out of range");
    CONE_REQUIRE(w->t_dim % 32 == 0 && w->v_dim % 32 == 0 && w->v_motion_dim % 32 == 0 && w->t_dim <= 1024 && w->v_dim <= 1024 &&
                     w->v_motion_dim <= 1024 && w->t_dim > 0 && w->v_dim > 0 && w->v_motion_dim > 0,
                 "model_create: feature dims must be multiples of 32 and <= 1024 (t=%d v_appear=%d v_motion=%d)", w->t_dim,
                 w->v_dim, w->v_motion_dim);
    cone_model* m = new cone_model();
    m->d = w->hidden_dim; m->heads = w->nheads; m->gen_native = !shipped; m->ff = w->dim_ff; m->n_enc = w->enc_layers; m->n_dec = w->dec_layers;
    m->nq = w->num_queries; m->n_proj = w->n_input_proj; m->dt = w->t_dim; m->dv = w->v_dim; m->dvm = w->v_motion_dim;
    m->has_adapter = w->has_adapter;
    const size_t d = m->d, ff = m->ff;
    ArenaBuilder ab;
    auto lin = [&](const cone_linear_w& s, size_t nout, size_t nin, Linear& dst) {
        ab.add(s.w, nout * nin, &dst.w);
        ab.add(s.b, nout, &dst.b);
    };
    auto ln = [&](const cone_ln_w& s, size_t n, LNorm& dst) { ab.add(s.g, n, &dst.g); ab.add(s.b, n, &dst.b); };
    auto mha = [&](const cone_mha_w& s, Mha& dst) {
        ab.add(s.in_proj_w, 3 * d * d, &dst.in_w);
        ab.add(s.in_proj_b, 3 * d, &dst.in_b);
        lin(s.out_proj, d, d, dst.out);
    };
    for (int i = 0; i < m->n_proj; ++i) {
        ln(w->vid_proj_ln[i], i == 0 ? m->dvm : d, m->vproj_ln[i]);
        lin(w->vid_proj[i], d, i == 0 ? m->dvm : d, m->vproj[i]);
        ln(w->txt_proj_ln[i], i == 0 ? m->dt : d, m->tproj_ln[i]);
        lin(w->txt_proj[i], d, i == 0 ? m->dt : d, m->tproj[i]);
    }
    for (int i = 0; i < m->n_enc; ++i) {
        mha(w->enc[i].self_attn, m->enc[i].sa);
        lin(w->enc[i].linear1, ff, d, m->enc[i].l1);
        lin(w->enc[i].linear2, d, ff, m->enc[i].l2);
        ln(w->enc[i].norm1, d, m->enc[i].n1);
        ln(w->enc[i].norm2, d, m->enc[i].n2);
    }
    for (int i = 0; i < m->n_dec; ++i) {
        mha(w->dec[i].self_attn, m->dec[i].sa);
        mha(w->dec[i].cross_attn, m->dec[i].ca);
        lin(w->dec[i].linear1, ff, d, m->dec[i].l1);
        lin(w->dec[i].linear2, d, ff, m->dec[i].l2);
        ln(w->dec[i].norm1, d, m->dec[i].n1);
        ln(w->dec[i].norm2, d, m->dec[i].n2);
        ln(w->dec[i].norm3, d, m->dec[i].n3);
    }
    ln(w->dec_norm, d, m->dec_norm);
    ab.add(w->query_embed, (size_t)m->nq * d, &m->query_embed);
    lin(w->class_embed, 2, d, m->class_embed);
    lin(w->span_embed[0], d, d, m->span[0]);
    lin(w->span_embed[1], d, d, m->span[1]);
    lin(w->span_embed[2], 2, d, m->span[2]);
    lin(w->saliency_proj, 1, d, m->saliency);
    if (m->has_adapter) {
        lin(w->adapter[0], d, m->dv, m->adapter[0]);
        lin(w->adapter[1], m->dv, d, m->adapter[1]);
    }
    ab.add(w->pos_dim_t, d, &m->dim_t);
    if (w->txt_pos_embed) {     // --use_txt_pos
        if (w->txt_pos_rows < 1 || w->txt_pos_rows > 4096 || !w->txt_pos_ln.g || !w->txt_pos_ln.b) {
            free_model(m);
            set_error("model_create: txt_pos_embed needs txt_pos_rows in [1, 4096] (got %d) and its LayerNorm", w->txt_pos_rows);
            return CONE_E_INVALID;
        }
        m->txt_pos_rows = w->txt_pos_rows;
        ab.add(w->txt_pos_embed, (size_t)w->txt_pos_rows * d, &m->txt_pos_emb);
        ln(w->txt_pos_ln, d, m->txt_pos_ln);
    }
    if (w->pre_norm) {          // --pre_norm
        m->pre_norm = 1;
        ln(w->enc_norm, d, m->enc_norm);
    }
    for (auto& it : ab.items)
        if (!it.src) {
            free_model(m);
            set_error("model_create: a required weight pointer is null");
            return CONE_E_INVALID;
        }
    const size_t dec0_floats = (size_t)m->nq * (d * 2 + d + 3 * d + d) + 6 * 64 +
                               (size_t)m->n_dec * (align_up((size_t)m->nq * 3 * d, 64) + align_up((size_t)m->nq * d, 64));
    const size_t stacked = (size_t)m->n_dec * (d * d + d) * 2 + 4 * 64 + (size_t)m->n_dec * d * d + dec0_floats;
    hipError_t e = hipMalloc((void**)&m->arena, (ab.total + stacked) * sizeof(float));
    if (e != hipSuccess) {
        free_model(m);
        set_error("model_create: hipMalloc of %zu bytes failed: %s", (ab.total + stacked) * sizeof(float),
                  hipGetErrorString(e));
        return CONE_E_HIP;
    }
    size_t cur = 0;
    for (auto& it : ab.items) {
        e = hipMemcpy(m->arena + cur, it.src, it.n * sizeof(float), hipMemcpyDefault);
        if (e != hipSuccess) {
            free_model(m);
            set_error("model_create: weight copy failed: %s", hipGetErrorString(e));
            return CONE_E_HIP;
        }
        *it.dst = m->arena + cur;
        cur += align_up(it.n, 64);
    }
    // stack W_k / W_v (rows [d:2d] / [2d:3d] of each layer's multihead_attn.in_proj) along N
    float* kw = m->arena + cur; cur += align_up((size_t)m->n_dec * d * d, 64);
    float* kb = m->arena + cur; cur += align_up((size_t)m->n_dec * d, 64);
    float* vw = m->arena + cur; cur += align_up((size_t)m->n_dec * d * d, 64);
    float* vb = m->arena + cur; cur += align_up((size_t)m->n_dec * d, 64);
    for (int i = 0; i < m->n_dec; ++i) {
        const float* iw = m->dec[i].ca.in_w;
        const float* ib = m->dec[i].ca.in_b;
        (void)hipMemcpy(kw + (size_t)i * d * d, iw + d * d, d * d * sizeof(float), hipMemcpyDeviceToDevice);
        (void)hipMemcpy(kb + (size_t)i * d, ib + d, d * sizeof(float), hipMemcpyDeviceToDevice);
        (void)hipMemcpy(vw + (size_t)i * d * d, iw + 2 * d * d, d * d * sizeof(float), hipMemcpyDeviceToDevice);
        e = hipMemcpy(vb + (size_t)i * d, ib + 2 * d, d * sizeof(float), hipMemcpyDeviceToDevice);
    }
    if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        free_model(m);
        set_error("model_create: stacking decoder K/V weights failed");
        return CONE_E_HIP;
    }
    m->dec_k = {kw, kb};
    m->dec_v = {vw, vb};
    {   // W_v^T per decoder layer (host transpose; 256 KiB each, once per model)
        std::vector<float> h(d * d), ht(d * d);
        for (int i = 0; i < m->n_dec; ++i) {
            float* dst = m->arena + cur; cur += d * d;
            e = hipMemcpy(h.data(), m->dec[i].ca.in_w + 2 * d * d, d * d * sizeof(float), hipMemcpyDeviceToHost);
            for (size_t o = 0; o < d; ++o)
                for (size_t c = 0; c < d; ++c) ht[c * d + o] = h[o * d + c];
            if (e == hipSuccess) e = hipMemcpy(dst, ht.data(), d * d * sizeof(float), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                free_model(m);
                set_error("model_create: transposing decoder V weights failed: %s", hipGetErrorString(e));
                return CONE_E_HIP;
            }
            m->dec_vT[i] = dst;
        }
    }
    m->dec0_tgt1 = m->arena + cur; cur += align_up((size_t)m->nq * d, 64);
    m->dec0_dq = m->arena + cur; cur += align_up((size_t)m->nq * d, 64);
    m->dec0_scratch = m->arena + cur; cur += align_up((size_t)m->nq * (d + 3 * d + d), 64);
    for (int i = 0; i < m->n_dec; ++i) {
        m->dec_sa_tab[i] = m->arena + cur; cur += align_up((size_t)m->nq * 3 * d, 64);
        m->dec_ca_tab[i] = m->arena + cur; cur += align_up((size_t)m->nq * d, 64);
    }
    auto tail = [](const Linear& o, const Linear& l1, const Linear& l2, const LNorm& in, const LNorm& outn) {
        TailWeights t{};
        t.Wo = o.w; t.bo = o.b; t.W1 = l1.w; t.b1 = l1.b; t.W2 = l2.w; t.b2 = l2.b;
        t.in_g = in.g; t.in_b = in.b; t.out_g = outn.g; t.out_b = outn.b;
        return t;
    };
    for (int l = 0; l < m->n_enc; ++l) {    // pre-norm: norm2 sits ahead of the block, the second output carries the next consumer's norm
        const EncLayer& el = m->enc[l];
        const LNorm& nxt = l + 1 < m->n_enc ? m->enc[l + 1].n1 : m->enc_norm;
        m->enc_tail[l] = m->pre_norm ? tail(el.sa.out, el.l1, el.l2, el.n2, nxt) : tail(el.sa.out, el.l1, el.l2, el.n1, el.n2);
        m->enc_tail[l].Wq = el.sa.in_w; m->enc_tail[l].qb = el.sa.in_b;
    }
    for (int l = 0; l < m->n_dec; ++l) {
        const DecLayer& dl = m->dec[l];
        m->dec_tail[l] = m->pre_norm ? tail(dl.ca.out, dl.l1, dl.l2, dl.n3, m->dec_norm) : tail(dl.ca.out, dl.l1, dl.l2, dl.n2, dl.n3);
    }
    if (!m->gen_native && TAIL_MODES[TAIL_IMG_SPLIT]->ffn_supported(m->ff)) {
        int rc = build_tail_images(m, TAIL_IMG_SPLIT, &m->split_img);
        if (rc == 0) rc = build_tail_images(m, TAIL_IMG_BF16, &m->bf16_img);
        if (rc == 0 && hipDeviceSynchronize() != hipSuccess) {
            set_error("model_create: building the split-bf16 / bf16 weight images failed");
            rc = CONE_E_HIP;
        }
        if (rc != 0) {
            free_model(m);
            return CONE_E_HIP;
        }
    }
    if (!m->gen_native && ffn_fused_supported(m->ff)) {
        if (build_f32_images(m) != 0 || hipDeviceSynchronize() != hipSuccess || (m->opt_gemm_tall_packed && build_tall_images(m) != 0)) {
            free_model(m);
            return CONE_E_HIP;
        }
    }
    if (dec0_constants(m, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) {
        free_model(m);
        return CONE_E_HIP;
    }
    if (!m->gen_native) {   // the handle's own position tables, for the window lengths this checkpoint is built for (ABI 8: cone_weights.
        // table_max_v_l; rows (256 + 512 per encoder layer) floats each: 21 MB at 90 clips, 167 MB at 255 with two layers; the
        // general path, which every other shape runs, reads no tables)
        const int tab_l = (w->table_max_v_l >= 1 && w->table_max_v_l <= CONE_TABLE_MAX_V_L) ? w->table_max_v_l : CONE_TABLE_MAX_V_L;
        const size_t rows = (size_t)pos_table_rows(tab_l);
        e = hipMalloc((void**)&m->tab_arena, rows * (256 + 512 * (size_t)m->n_enc) * sizeof(float));
        int rc = e == hipSuccess ? 0 : CONE_E_HIP;
        if (rc == 0) rc = build_pos_tables(m, tab_l, m->tab_arena, m->tab_arena + rows * 256, nullptr);
        if (rc != 0 || hipDeviceSynchronize() != hipSuccess) {
            if (e != hipSuccess) set_error("model_create: hipMalloc of the position tables failed: %s", hipGetErrorString(e));
            free_model(m);
            return CONE_E_HIP;
        }
        m->tab_pos_rows = m->tab_arena; m->tab_pos_qk = m->tab_arena + rows * 256; m->tab_max_v_l = tab_l;
    }
    *out = m;
    return 0;
}

// ------------------------------------------------------------------------------ workspace
struct Carver {
    char* base; size_t cap, cur = 0; bool ok = true;
    Carver(void* p, size_t n) : base((char*)p), cap(n) {}
    template <typename T> T* take(size_t n) {
        const size_t bytes = align_up(n * sizeof(T), 256);
        T* r = (T*)(base + cur);
        cur += bytes;
        if (cur > cap) ok = false;
        return r;
    }
};

static GemmArgs G(const cone_model* m, const float* A, int lda, const float* W, int ldw, const float* bias, float* C,
                  int ldc, int M, const int* M_dev, int N, int K, int flags = 0) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc;
    g.M = M; g.M_dev = M_dev; g.N = N; g.K = K; g.flags = flags;
    g.variant = m ? m->opt_gemm | ((m->opt_gemm_tall_min + 1) << GEMM_TALL_MIN_SHIFT) : GEMM_AUTO;
    if (m && !m->opt_spread) g.flags |= GEMM_NO_SPREAD;        // option ffn_spread = 0: no spread forms anywhere
    if (m && m->opt_gemm_tall_packed && K == 256 && ldw == 256) g.Wimg = m->tall_image(W, N);   // (only the tall form reads it)
    return g;
}

#define RUN(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// Per-checkpoint constants of the decoder (cone/transformer.py:296-311).  (1) The slot-position tables of every layer (see
// cone_model).  (2) The first layer on tgt = 0 (:66): its self-attention over the nq slots (q | k | v = the table rows), out_proj
// + norm1, and its cross-attention queries -- no window enters, so the nq rows are constants too.  Computed with the kernels
// and the row count (nq) a step uses for one window, hence the same bits as the per-window path (dec0_const = 0).
// (A handle of another shape than 256 / 8 has the tables only: the general path runs its first decoder layer per window.)
static int dec0_constants(cone_model* m, hipStream_t s) {
    const int nq = m->nq, d = m->d;
    float* TGT = m->dec0_scratch;                       // (nq, d) zeros
    float* QKV = TGT + (size_t)nq * 256;                // (nq, 768)
    float* DATT = QKV + (size_t)nq * 768;               // (nq, 256)
    CONE_CHECK_HIP(hipMemsetAsync(TGT, 0, (size_t)nq * d * sizeof(float), s));
    for (int l = 0; l < m->n_dec; ++l) {
        const DecLayer& dl = m->dec[l];
        // [qe W_q^T + b_q | qe W_k^T + b_k]  and  b_v rows (0 W_v^T + b_v)
        RUN(launch_gemm(G(m, m->query_embed, d, dl.sa.in_w, d, dl.sa.in_b, m->dec_sa_tab[l], 3 * d, nq, nullptr, 2 * d, d), s));
        RUN(launch_gemm(G(m, TGT, d, dl.sa.in_w + 2 * d * d, d, dl.sa.in_b + 2 * d, m->dec_sa_tab[l] + 2 * d, 3 * d, nq, nullptr, d, d), s));
        RUN(launch_gemm(G(m, m->query_embed, d, dl.ca.in_w, d, dl.ca.in_b, m->dec_ca_tab[l], d, nq, nullptr, d, d), s));
    }
    if (m->gen_native) return 0;
    const DecLayer& d0 = m->dec[0];
    GemmArgs g = G(m, TGT, 256, d0.sa.in_w, 256, nullptr, QKV, 768, nq, nullptr, 768, 256, EPI_RESIDUAL);
    g.R = m->dec_sa_tab[0]; g.ldr = 768; g.r_mod = nq;
    RUN(launch_gemm(g, s));
    RUN(launch_small_attn(QKV, 768, QKV + 256, 768, QKV + 512, 768, DATT, 256, nullptr, 1, nq, nq, s));
    g = G(m, DATT, 256, d0.sa.out.w, 256, d0.sa.out.b, m->dec0_tgt1, 256, nq, nullptr, 256, 256, EPI_RESIDUAL | EPI_LN);
    g.R = TGT; g.ldr = 256; g.ln_g = d0.n1.g; g.ln_b = d0.n1.b;
    RUN(launch_gemm(g, s));
    g = G(m, m->dec0_tgt1, 256, d0.ca.in_w, 256, nullptr, m->dec0_dq, 256, nq, nullptr, 256, 256, EPI_RESIDUAL);
    g.R = m->dec_ca_tab[0]; g.ldr = 256; g.r_mod = nq;
    RUN(launch_gemm(g, s));
    return 0;
}

// rows (lv, p), p < lv <= max_v_l, then ONE all-zero row: the position term of a text token (cone/model.py:106), which the
// encoder attention adds unconditionally instead of branching on the token kind
static int build_pos_tables(const cone_model* m, int max_v_l, float* pos_rows, float* pos_qk, hipStream_t s) {
    const int64_t rows = pos_table_rows(max_v_l);
    if (m->d != 256) {      // (the same rows d wide: sine rows, zero row, pos [W_q | W_k]^T per encoder layer)
        const int d = m->d;
        RUN(launch_gen_pos_rows(m->dim_t, max_v_l, d, pos_rows, s));
        CONE_CHECK_HIP(hipMemsetAsync(pos_rows + (size_t)(rows - 1) * d, 0, d * sizeof(float), s));
        for (int l = 0; l < m->n_enc; ++l)
            RUN(launch_gemm(G(m, pos_rows, d, m->enc[l].sa.in_w, d, nullptr, pos_qk + (size_t)l * rows * 2 * d, 2 * d, (int)rows,
                              nullptr, 2 * d, d), s));
        return 0;
    }
    RUN(launch_pos_rows(m->dim_t, max_v_l, pos_rows, s));
    CONE_CHECK_HIP(hipMemsetAsync(pos_rows + (size_t)(rows - 1) * 256, 0, 256 * sizeof(float), s));    // the zero row
    // pos W_q^T | pos W_k^T of every encoder layer, no bias (the bias travels with the clip / token rows): zero row -> zeros
    for (int l = 0; l < m->n_enc; ++l)
        RUN(launch_gemm(G(m, pos_rows, 256, m->enc[l].sa.in_w, 256, nullptr, pos_qk + (size_t)l * rows * 512, 512,
                          (int)rows, nullptr, 512, 256), s));
    return 0;
}

// Encoder layer l's q | k | v = X in_proj^T + b (N = 768) in the handle's numeric mode -- the one place that picks its kernel:
//   bf16       : the mode's row GEMM for every layer, the first included, and for the layer-0 row caches;
//   split_bf16 : the mode's row GEMM only where split_ok (the post-norm layer loop) and only for l > 0: layer 0 keeps the
//                kernel of cone_layer0_project, so that a window's bits do not depend on who projected it; never for the
//                caches and never on the pre-norm path;
//   otherwise  : the exact-fp32 GEMM (any hidden_dim: the general path's caches come through here too).
static int encoder_qkv(const cone_model* m, int l, const float* X, float* QKV, int M, const int* M_dev, hipStream_t s,
                       bool split_ok) {
    const TailWeights& t = m->enc_tail[l];
    const int d = m->d;
    const int mode = m->opt_bf16 && m->bf16_img && !m->general()               ? TAIL_IMG_BF16
                     : split_ok && l > 0 && m->opt_split_bf16 && m->split_img ? TAIL_IMG_SPLIT
                                                                               : -1;
    if (mode >= 0) return TAIL_MODES[mode]->rows256(X, 256, t.img[mode].qkv, t.qb, QKV, 768, M, M_dev, 768, s, 0);
    return launch_gemm(G(m, X, d, t.Wq, d, t.qb, QKV, 3 * d, M, M_dev, 3 * d, d), s);
}

// First encoder layer's in_proj hoisted out of the window loop: q | k | v = in_proj(x) once per projected clip / text token
// (post-norm, cone/transformer.py:237-239), resp. in_proj(norm1(x)) (--pre_norm, :250-252; tmp = n rows of scratch).
static int layer0_rows(const cone_model* m, const float* rows, int n, const int* n_dev, float* qkv, float* tmp, hipStream_t s) {
    const float* a = rows;
    const int d = m->d;
    if (m->pre_norm) {
        RUN(launch_layernorm(rows, d, m->enc[0].n1.g, m->enc[0].n1.b, tmp, d, n, n_dev, d, s));
        a = tmp;
    }
    return encoder_qkv(m, 0, a, qkv, n, n_dev, s, false);
}

// input_{vid,txt}_proj: LN -> Linear -> ReLU (all but last) with the next LN fused into the GEMM epilogue.
// (d != 256: the GEMM's LayerNorm epilogue is instantiated for N == 256 only -- a LayerNorm launch behind the GEMM instead,
// through a third d-wide buffer)
static size_t project_ws_bytes(const cone_model* m, int which, int64_t n) {
    const size_t din = which == 0 ? m->dvm : m->dt;
    return align_up(n * din * 4, 256) + (m->d == 256 ? 2 : 3) * align_up(n * m->d * 4, 256);
}
// src_row != null: row i of the projection reads row src_row[i] of x (the valid rows of a zero-padded batch, compacted by the
// first LayerNorm's loads); n_dev != null: only the first *n_dev rows exist (device-side count, n bounds it)
static int project_tokens(const cone_model* m, int which, const float* x, int64_t n, float* out, void* ws,
                          size_t ws_bytes, hipStream_t s, const int* src_row = nullptr, const int* n_dev = nullptr) {
    CONE_REQUIRE(n < (1ll << 31), "project: too many rows");
    const int din = which == 0 ? m->dvm : m->dt;
    const LNorm* lns = which == 0 ? m->vproj_ln : m->tproj_ln;
    const Linear* lin = which == 0 ? m->vproj : m->tproj;
    const int d = m->d;
    Carver c(ws, ws_bytes);
    float* t0 = c.take<float>((size_t)n * din);
    float* ta = c.take<float>((size_t)n * d);
    float* tb = c.take<float>((size_t)n * d);
    float* tc = d == 256 ? nullptr : c.take<float>((size_t)n * d);
    if (!c.ok) { set_error("project: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    RUN(launch_layernorm(x, din, lns[0].g, lns[0].b, t0, din, n, n_dev, din, s, src_row));
    const float* cur = t0;
    int K = din;
    for (int i = 0; i < m->n_proj; ++i) {
        const bool last = i == m->n_proj - 1;
        float* dst = last ? out : (cur == ta ? tb : ta);
        GemmArgs g = G(m, cur, K, lin[i].w, K, lin[i].b, last || tc == nullptr ? dst : tc, d, (int)n, n_dev, d, K,
                       last ? 0 : EPI_RELU);
        if (!last && !tc) { g.flags |= EPI_LN; g.ln_g = lns[i + 1].g; g.ln_b = lns[i + 1].b; }
        RUN(launch_gemm(g, s));
        if (!last && tc) RUN(launch_layernorm(tc, d, lns[i + 1].g, lns[i + 1].b, dst, d, n, n_dev, d, s));
        cur = dst;
        K = d;
    }
    return 0;
}

// ------------------------------------------------------------------------------ packed forward
// Workspace of one batch of B windows (M = B * Lmax token rows at most).  Two layouts:
//   table path (layer-0 cache + position tables; the eval driver): X, X1 and ONE (M, ff) region that holds, in
//     turn, the layer's q|k|v (M, 768) + attention output (M, 256) and then the FFN hidden rows -- q|k|v are dead
//     once the attention has run, its output once out_proj has, and FFN1 writes only after that: 4 * (2 * 256 +
//     max(ff, 1024)) = 6 KiB per token row at ff = 1024;
//   general path (--use_txt_pos, and the A/B switches of the parity tests): additionally POS and XP = X + POS, and the
//     stacked decoder K / V rows when the cross-attention fold is off.
struct FwdBuffers {
    int* off; int* RIDX;
    float *X, *POS, *XP, *QKV, *ATT, *X1, *H, *KD, *VD;
    float *TGT, *TGT1, *TGT2, *DQK, *DV, *DATT, *DQ, *DH, *HS, *S1, *S2, *LG, *SP, *QKS, *SPR;
};
// One call of the window model, as every internal forward function takes it (the extern "C" entries fill it after their
// null checks): window b = rows vrow0[b] .. + vlen[b] of the projected clip rows, then rows trow0[b] .. + qlen[b] of the
// projected token rows.
struct FwdCall {
    const float* vproj; const int* vrow0; const int* vlen;
    const float* tproj; const int* trow0; const int* qlen;
    int B, Lv_max, Lq_max;                      // windows; host bounds of the lengths
    float *logits, *spans, *saliency;           // saliency == null: not wanted
    const cone_taps* taps;                      // may be null
};
// Every path decision of a forward, made once (plan_forward) and read by the workspace carve, the workspace-size entries and
// the forward bodies alike.
enum { BODY_GENERAL, BODY_PRENORM_PLAIN, BODY_PACKED };     // forward_general / forward_packed_prenorm / forward_packed's own body
enum { CROSS_SMALL = 0, CROSS_VALU = 1 };                   // a layer's cross-attention form; 2 .. 5: launch_dec_cross_mfma's form
struct FwdPlan {
    int body = BODY_GENERAL;
    bool pre = false;           // --pre_norm on BODY_PACKED: the fused pre-norm tails, LayerNorms ahead of the decoder fronts
    bool long_ok = false;       // windows beyond 192 tokens run (the default table path with 3 / 5 / 8 slots only)
    bool tables = false;        // encoder position term from the static tables (one N = 768 GEMM per layer, no x + pos matrix)
    bool fold = false;          // decoder memory K / V projections inside the cross-attention kernel
    bool dec_xp = false;        // --use_txt_pos on the table path: the keys memory + pos written once behind the encoder
    bool dec_tab = false;       // the cross-attention kernels add the position rows from the table themselves
    bool have_l0 = false; cone_layer0 l0{};     // what the call runs on (effective_l0); the padded entry fills in what it builds:
    bool mk_caches = false, mk_txt_pos = false; //   the first layer's row caches / the text position rows (own_rows)
    bool caches = false;        // the first layer reads the row caches
    bool gather0 = false;       // ... its attention gathers q | k | v from them itself (else a packing pass writes them out)
    bool gather_res = false;    // ... and its tail gathers the residual rows through a row index: no packed copy of the input
    bool own_ridx = false;      // the row index has its own buffer (pre-norm); else it lives in the X1 region, unused by then
    int cross[CONE_MAX_LAYERS] = {};
    bool sal_ride = false;      // the saliency head rides in the first cross-attention launch
    bool dec0 = false;          // first decoder layer's front replicated from the per-checkpoint constants
    bool slabs = false;         // ... and its cross-attention builds the folded-key operand once for all windows
    bool want_aux = false; int h0 = 0;  // intermediate layers' heads asked for; first decoder layer whose heads are computed
    bool heads_chain = false;   // decoder.norm + heads of a layer's rows as one launch (rows_chain.h)
};
// The caller's cone_layer0 with the handle's position tables filled in where it brings none (ABI 6: a NULL cone_layer0, or
// one with the row caches only, still takes the table path), or nothing for --use_txt_pos without the tokens' own position
// rows (cone_layer0_text_positions: handed over in l0, or -- own_rows, the padded entry -- built by the caller itself) and for
// windows longer than the handle's tables cover.
static const cone_layer0* effective_l0(const cone_model* m, const cone_layer0* l0, int Lv_max, cone_layer0* eff, bool own_rows) {
    if (m->txt_pos_emb && !(own_rows || (l0 && l0->txt_pos && l0->txt_pos_qk))) return nullptr;
    *eff = l0 ? *l0 : cone_layer0{};
    if (!m->txt_pos_emb) eff->txt_pos = eff->txt_pos_qk = nullptr;
    if (!eff->qkv_vid || !eff->qkv_txt) eff->qkv_vid = eff->qkv_txt = nullptr;
    if (!eff->pos_rows || !eff->pos_qk) {                   // no (complete) tables of the caller's: the handle's
        if (Lv_max > m->tab_max_v_l) return nullptr;
        eff->pos_rows = m->tab_pos_rows; eff->pos_qk = m->tab_pos_qk; eff->max_v_l = m->tab_max_v_l;
    }
    return eff;
}
// The one place that reads the forward-level inputs: the options dec_fold, pos_tables, l0_gather, res_gather, dec0_const,
// rows_chain (and ffn_fused / ffn_spread / gemm where they gate a path), pre_norm, txt_pos_emb, general(), the *_supported
// predicates, and what the caller handed over (cone_layer0, taps, saliency wanted).  own_rows: the padded entry, which
// builds the row caches and the text position rows the plan asks for (mk_caches, mk_txt_pos) itself.  The workspace-size
// entries call it with the sizes only.  In order:
//
//   body     general()                                            BODY_GENERAL: nothing below is read
//            pre_norm without all of {tables, matrix-core fold,   BODY_PRENORM_PLAIN: plain LayerNorm / GEMM / attention launches,
//              ffn_fused = 2, an ff the fused tails take}           no tables, no fold, no caches
//            otherwise                                            BODY_PACKED (pre: with the fused pre-norm tails)
//   l0       effective_l0; caches GIVEN = its row caches, resp. (own_rows) pos_tables and l0_gather both on
//   tables   l0 there, pos_tables, and (no caches given or l0_gather); off again when the decoder is unfolded and the fold
//            is switched off by option or nq = 5 (the fold off BY OPTION keeps meaning the whole general launch sequence)
//   dec_xp   tables and --use_txt_pos; dec_tab = tables and not dec_xp
//   fold     dec_fold >= 2: dec_cross_mfma_supported (its table form only with dec_tab); dec_fold = 1: dec_cross_supported
//   --use_txt_pos with l0 there but tables off: the WHOLE general launch sequence -- l0 dropped (its row caches do not
//            carry the text position term), everything above derived again without it
//   gather_res  caches given, l0_gather, tables, ffn_fused = 2 with an ff it takes, res_gather
//   gather0     post-norm: caches given and l0_gather; pre-norm: gather_res (its in_proj reads norm1(x): all or nothing)
//   caches      post-norm: given; pre-norm: gather_res
//   cross[l]    no fold: CROSS_SMALL; dec_fold = 1: CROSS_VALU; pre-norm: form 3; dec_fold = 2: form 5 for the first layer,
//               3 behind it (by LAYER, never by the batch: a window's bits must not depend on the batch it rides in); else dec_fold
//   sal_ride    post-norm, saliency wanted, dec_tab, fold, dec_fold in {2, 3, 5} (table form of the two-read kernel)
//   dec0        post-norm and dec0_const; slabs: dec0 and more than one window
//   want_aux    a tap asks for hs / aux_logits / aux_spans; h0 = 0 then, else the last layer (pre-norm: heads_and_taps
//               computes every layer's whatever the taps)
//   heads_chain post-norm, rows_chain, the automatic GEMM family, rows_chain_supported(B nq) and not the spread GEMM's rows
static FwdPlan plan_forward(const cone_model* m, const FwdCall& c, const cone_layer0* l0, bool own_rows) {
    FwdPlan p;
    if (m->general()) return p;
    const int Lmax = c.Lv_max + c.Lq_max, T = c.B * m->nq, fo = m->opt_dec_fold;
    const bool pre = m->pre_norm != 0, txt = m->txt_pos_emb != nullptr;
    const bool tail2 = m->opt_ffn_fused >= 2 && ffn_fused_supported(m->ff);
    p.long_ok = fo >= 2 && dec_cross_mfma_supported(m->nq, Lmax, true) && !txt && m->opt_pos_tables;
    const cone_layer0* e = effective_l0(m, l0, c.Lv_max, &p.l0, own_rows);
    bool given = e && (own_rows ? m->opt_pos_tables && m->opt_l0_gather : e->qkv_vid != nullptr);
    auto paths = [&](bool have_tables, bool caches) {
        p.tables = have_tables && m->opt_pos_tables && (!caches || m->opt_l0_gather);
        p.dec_xp = p.tables && txt;
        p.fold = fo >= 2 ? dec_cross_mfma_supported(m->nq, Lmax, p.tables && !p.dec_xp) : (fo == 1 && dec_cross_supported(m->nq, Lmax));
        if (pre) p.tables = p.fold = p.tables && p.fold && fo >= 2 && tail2;
        // the unfolded decoder projects its keys from memory + pos rows: on the table path that matrix is written once behind
        // the encoder (launch_add_pos_rows) -- slot counts other than 5 keep the encoder's fast path
        else if (!p.fold && !(fo && m->nq != 5)) p.tables = false;
        if (!p.tables) p.dec_xp = false;
    };
    paths(e != nullptr, given);
    if (txt && e && !p.tables) { e = nullptr; given = false; paths(false, false); }
    p.have_l0 = e != nullptr;
    if (!e) p.l0 = cone_layer0{};
    p.body = pre && !p.tables ? BODY_PRENORM_PLAIN : BODY_PACKED;
    p.pre = pre; p.own_ridx = pre;
    p.dec_tab = p.tables && !p.dec_xp;
    p.mk_caches = own_rows && given; p.mk_txt_pos = own_rows && txt && p.tables;
    p.gather_res = given && m->opt_l0_gather && p.tables && tail2 && m->opt_res_gather;
    p.gather0 = pre ? p.gather_res : given && m->opt_l0_gather;
    p.caches = pre ? p.gather_res : given;
    for (int l = 0; l < m->n_dec; ++l)
        p.cross[l] = !p.fold ? CROSS_SMALL : fo < 2 ? CROSS_VALU : pre ? 3 : fo == 2 ? (l == 0 ? 5 : 3) : fo;
    p.sal_ride = !pre && c.saliency && p.dec_tab && p.fold && (fo == 2 || fo == 3 || fo == 5);
    p.dec0 = !pre && m->opt_dec0_const;
    p.slabs = p.dec0 && c.B != 1;
    p.want_aux = c.taps && (c.taps->hs || c.taps->aux_logits || c.taps->aux_spans);
    p.h0 = p.want_aux ? 0 : m->n_dec - 1;
    p.heads_chain = !pre && m->opt_chain && m->opt_gemm == GEMM_AUTO && rows_chain_supported(T) &&
                    !(m->opt_spread && gemm_rows_spread_rows(T));     // (few rows: the spread GEMM launches are faster)
    return p;
}
static void carve_fwd(const cone_model* m, Carver& c, int B, int Lmax, const FwdPlan& p, FwdBuffers& f) {
    const size_t M = (size_t)B * Lmax, T = (size_t)B * m->nq, nd = m->n_dec;
    const size_t wide = m->ff > 1024 ? m->ff : 1024;
    f.off = c.take<int>(B + 1);
    f.RIDX = p.own_ridx ? c.take<int>(M) : nullptr;
    f.X = c.take<float>(M * 256); f.X1 = c.take<float>(M * 256);
    if (!f.RIDX) f.RIDX = reinterpret_cast<int*>(f.X1);     // (post-norm: the X1 region is unused while the row index lives)
    f.H = c.take<float>(M * wide);
    f.QKV = f.H; f.ATT = f.H + M * 768;            // aliases of the FFN hidden region (see above)
    f.POS = f.XP = f.KD = f.VD = nullptr;
    if (!p.tables) {
        f.POS = c.take<float>(M * 256); f.XP = c.take<float>(M * 256);
        f.QKV = c.take<float>(M * 768); f.ATT = c.take<float>(M * 256);
    }
    if (!p.fold) { f.KD = c.take<float>(M * 256 * nd); f.VD = c.take<float>(M * 256 * nd); }
    if ((!p.fold || p.dec_xp) && p.tables) f.XP = c.take<float>(M * 256);   // memory + pos for the unfolded decoder / the
                                                                            // x + pos form of the fold (launch_add_pos_rows)
    f.TGT = c.take<float>(T * 256); f.TGT1 = c.take<float>(T * 256); f.TGT2 = c.take<float>(T * 256);
    f.DQK = c.take<float>(T * 768); f.DV = nullptr; f.DATT = c.take<float>(T * 256);      // DQK: the slots' q | k | v
    f.DQ = c.take<float>(T * 256); f.DH = c.take<float>(T * m->ff);
    f.HS = c.take<float>(nd * T * 256); f.S1 = c.take<float>(nd * T * 256); f.S2 = c.take<float>(nd * T * 256);
    f.LG = c.take<float>(nd * T * 2); f.SP = c.take<float>(nd * T * 2);
    f.QKS = c.take<float>(dec_cross_mfma_slab_floats());
    f.SPR = ffn_spread_supported((int)T, m->ff) || ffn_spread_supported((int)M, m->ff)                       // the spread tail's rows
                ? c.take<float>(ffn_spread_scratch_floats(m->ff)) : nullptr;
}

// The hs / aux_* taps: all layers' normalised slot rows and the intermediate layers' head outputs, from the workspace.
static int copy_taps(const cone_taps* taps, const float* HS, const float* LG, const float* SP, int nd, int T, int d, hipStream_t s) {
    if (!taps) return 0;
    const size_t last = (size_t)(nd - 1) * T * 2;
    if (taps->hs)
        CONE_CHECK_HIP(hipMemcpyAsync(taps->hs, HS, (size_t)nd * T * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (taps->aux_logits && nd > 1)
        CONE_CHECK_HIP(hipMemcpyAsync(taps->aux_logits, LG, last * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (taps->aux_spans && nd > 1)
        CONE_CHECK_HIP(hipMemcpyAsync(taps->aux_spans, SP, last * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
// The plain epilogue of a forward (cone/model.py:112-117): class head, span MLP and span head of every layer's rows HS (nd * T, d)
// into the workspace, the last layer's rows out, the taps, the saliency head of the memory rows.  gen: the d-wide row-dot /
// saliency kernels of general.hip (the general path, also when it is forced at d = 256), else the 256-channel ones.
struct HeadBufs { float *HS, *S1, *S2, *LG, *SP; const int* off; };
static int heads_and_taps(const cone_model* m, const FwdCall& c, const HeadBufs& f, const float* MEM, bool gen, hipStream_t s) {
    const int d = m->d, B = c.B, T = B * m->nq, nd = m->n_dec, HT = nd * T;
    const cone_taps* taps = c.taps;
    auto rowdot = [&](const float* X, const Linear& h, float* out, int act) {
        return gen ? launch_gen_rowdot(X, d, h.w, h.b, out, 2, HT, 2, act, d, s) : launch_rowdot(X, d, h.w, h.b, out, 2, HT, 2, act, s);
    };
    RUN(rowdot(f.HS, m->class_embed, f.LG, 0));
    RUN(launch_gemm(G(m, f.HS, d, m->span[0].w, d, m->span[0].b, f.S1, d, HT, nullptr, d, d, EPI_RELU), s));
    RUN(launch_gemm(G(m, f.S1, d, m->span[1].w, d, m->span[1].b, f.S2, d, HT, nullptr, d, d, EPI_RELU), s));
    RUN(rowdot(f.S2, m->span[2], f.SP, 1));
    const size_t last = (size_t)(nd - 1) * T * 2;
    CONE_CHECK_HIP(hipMemcpyAsync(c.logits, f.LG + last, (size_t)T * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    CONE_CHECK_HIP(hipMemcpyAsync(c.spans, f.SP + last, (size_t)T * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    RUN(copy_taps(taps, f.HS, f.LG, f.SP, nd, T, d, s));
    float* mem_tap = taps ? taps->memory : nullptr;
    if (!c.saliency && !mem_tap) return 0;
    return gen ? launch_gen_saliency(MEM, f.off, c.vlen, c.qlen, m->saliency.w, m->saliency.b, c.saliency, c.Lv_max, mem_tap, c.Lq_max, B, d, s)
               : launch_saliency(MEM, f.off, c.vlen, c.qlen, m->saliency.w, m->saliency.b, c.saliency, c.Lv_max, mem_tap, c.Lq_max, B, s);
}

// ---- stages the 256-wide bodies share (each issues exactly the launches written here, in this order)
// A decoder layer ahead of its cross-attention (cone/transformer.py:296-311, pre: :319-331): the slots' q | k | v in ONE
// N = 768 GEMM, the slot-position term from the layer's table as a row-periodic residual; their self-attention; out_proj +
// residual (post-norm: + norm1 in the epilogue, into TGT1); the cross-attention queries, slot term from the table, into DQ.
// pre: norm1 / norm2 as LayerNorm launches ahead of the two projections, the residual stream stays in TGT.
static int dec_layer_front(const cone_model* m, const FwdBuffers& f, int l, int B, bool pre, hipStream_t s) {
    const DecLayer& dl = m->dec[l];
    const int T = B * m->nq;
    if (pre) RUN(launch_layernorm(f.TGT, 256, dl.n1.g, dl.n1.b, f.TGT1, 256, T, nullptr, 256, s));          // tgt2 = norm1(tgt)
    GemmArgs g = G(m, pre ? f.TGT1 : f.TGT, 256, dl.sa.in_w, 256, nullptr, f.DQK, 768, T, nullptr, 768, 256, EPI_RESIDUAL);
    g.R = m->dec_sa_tab[l]; g.ldr = 768; g.r_mod = m->nq;
    RUN(launch_gemm(g, s));
    RUN(launch_small_attn(f.DQK, 768, f.DQK + 256, 768, f.DQK + 512, 768, f.DATT, 256, nullptr, B, m->nq, m->nq, s));
    g = G(m, f.DATT, 256, dl.sa.out.w, 256, dl.sa.out.b, pre ? f.TGT : f.TGT1, 256, T, nullptr, 256, 256,
          pre ? EPI_RESIDUAL : EPI_RESIDUAL | EPI_LN);
    g.R = f.TGT; g.ldr = 256;
    if (!pre) { g.ln_g = dl.n1.g; g.ln_b = dl.n1.b; }
    RUN(launch_gemm(g, s));
    if (pre) RUN(launch_layernorm(f.TGT, 256, dl.n2.g, dl.n2.b, f.TGT1, 256, T, nullptr, 256, s));          // tgt2 = norm2(tgt)
    g = G(m, f.TGT1, 256, dl.ca.in_w, 256, nullptr, f.DQ, 256, T, nullptr, 256, 256, EPI_RESIDUAL);
    g.R = m->dec_ca_tab[l]; g.ldr = 256; g.r_mod = m->nq;
    return launch_gemm(g, s);
}
// Decoder layer l's cross-attention in the form the plan picked, queries DQ -> DATT.  The folded forms take their keys
// memory + pos either from the table inside the kernel (dec_tab) or as the matrix XP; the unfolded one reads the layer's
// columns of the stacked K / V rows.  In the first layer's matrix-core launch the saliency head may ride (every memory row
// of the batch is in registers anyway), and the folded-key operand is built once when its queries are the replicated ones.
static int dec_cross_attn(const cone_model* m, const FwdCall& c, const FwdPlan& p, const FwdBuffers& f, int l, const float* MEM,
                          hipStream_t s) {
    const DecLayer& dl = m->dec[l];
    const int nd = m->n_dec, Lmax = c.Lv_max + c.Lq_max;
    const float* XP = p.dec_tab ? nullptr : f.XP;
    const float* pos = p.dec_tab ? p.l0.pos_rows : nullptr;
    if (p.cross[l] == CROSS_SMALL)
        return launch_small_attn(f.DQ, 256, f.KD + l * 256, 256 * nd, f.VD + l * 256, 256 * nd, f.DATT, 256, f.off, c.B, m->nq, Lmax, s);
    if (p.cross[l] == CROSS_VALU)
        return launch_dec_cross(f.DQ, XP, MEM, pos, c.vlen, f.off, dl.ca.in_w + 256 * 256, m->dec_vT[l], dl.ca.in_b + 512, f.DATT, c.B,
                                m->nq, Lmax, s);
    const bool ride = l == 0 && p.sal_ride;
    if (ride) CONE_CHECK_HIP(hipMemsetAsync(c.saliency, 0, (size_t)c.B * c.Lv_max * sizeof(float), s));     // padded clips: 0
    return launch_dec_cross_mfma(f.DQ, XP, MEM, pos, c.vlen, f.off, dl.ca.in_w + 256 * 256, m->dec_vT[l], dl.ca.in_b + 512, f.DATT,
                                 c.B, m->nq, Lmax, l == 0 && p.slabs ? f.QKS : nullptr, s, p.cross[l], ride ? m->saliency.w : nullptr,
                                 ride ? m->saliency.b : nullptr, ride ? c.saliency : nullptr, ride ? c.Lv_max : 0);
}
// Encoder layer l's attention source on the table path, less where q | k | v come from: the layer's pos W_qk^T rows (and,
// --use_txt_pos, the tokens' own), which the kernel adds to q | k in its staging loads ((x + pos) W^T = x W^T + pos W^T)
static AttnSrc table_attn_src(const FwdCall& c, const cone_layer0& l0, int l) {
    const size_t rows = (size_t)pos_table_rows(l0.max_v_l);
    AttnSrc src{};
    src.vlen = c.vlen; src.pos_zero_row = (int)rows - 1;
    src.pos_qk = l0.pos_qk + (size_t)l * rows * 512;
    if (l0.txt_pos_qk) { src.txt_pos_qk = l0.txt_pos_qk + (size_t)l * l0.n_txt * 512; src.trow0 = c.trow0; }
    return src;
}

// --pre_norm (cone/config.py:120 -> normalize_before, cone/transformer.py:19-36): every layer normalises its INPUT
// (forward_pre, :248-260 / :319-342), the residual stream stays un-normalised, and the encoder ends with its own LayerNorm.
// Off in every shipped configuration: built from the plain blocks (LayerNorm kernel, row GEMMs with residual epilogue, the
// packed encoder attention, the small decoder attentions) -- no fused tails, no caches.
static int forward_packed_prenorm(const cone_model* m, const FwdCall& c, const FwdPlan& p, FwdBuffers& f, hipStream_t s) {
    const int B = c.B, Lmax = c.Lv_max + c.Lq_max, Mmax = B * Lmax, T = B * m->nq, nd = m->n_dec, ff = m->ff;
    const int* Mdev = f.off + B;
    RUN(launch_scan_lengths(c.vlen, c.qlen, B, f.off, s));
    RUN(launch_pack_pos(c.vproj, c.vrow0, c.vlen, c.tproj, c.trow0, c.qlen, f.off, m->dim_t, f.X, f.POS, f.XP, B, Lmax, s,
                        m->txt_pos_emb, m->txt_pos_ln.g, m->txt_pos_ln.b));
    GemmArgs g;
    for (int l = 0; l < m->n_enc; ++l) {
        const EncLayer& e = m->enc[l];
        RUN(launch_layernorm(f.X, 256, e.n1.g, e.n1.b, f.X1, 256, Mmax, Mdev, 256, s));                 // src2 = norm1(src)
        float* QK = f.QKV; float* V = f.QKV + (size_t)Mmax * 512;
        g = G(m, f.X1, 256, e.sa.in_w, 256, e.sa.in_b, QK, 512, Mmax, Mdev, 512, 256);                  // q | k = (src2 + pos) W^T
        g.A2 = f.POS; g.lda2 = 256;
        RUN(launch_gemm(g, s));
        RUN(launch_gemm(G(m, f.X1, 256, e.sa.in_w + 512 * 256, 256, e.sa.in_b + 512, V, 256, Mmax, Mdev, 256, 256), s));
        AttnSrc src{};
        src.Q = QK; src.K = QK + 256; src.V = V; src.ldq = src.ldk = 512; src.ldv = 256;
        RUN(launch_enc_attn(ATTN_PACKED, src, f.ATT, f.off, B, Lmax, s));
        g = G(m, f.ATT, 256, e.sa.out.w, 256, e.sa.out.b, f.X, 256, Mmax, Mdev, 256, 256, EPI_RESIDUAL);
        g.R = f.X; g.ldr = 256;                                                                        // src += attn Wo^T + bo
        RUN(launch_gemm(g, s));
        RUN(launch_layernorm(f.X, 256, e.n2.g, e.n2.b, f.X1, 256, Mmax, Mdev, 256, s));                 // src2 = norm2(src)
        RUN(launch_gemm(G(m, f.X1, 256, e.l1.w, 256, e.l1.b, f.H, ff, Mmax, Mdev, ff, 256, EPI_RELU), s));
        g = G(m, f.H, ff, e.l2.w, ff, e.l2.b, f.X, 256, Mmax, Mdev, 256, ff, EPI_RESIDUAL);
        g.R = f.X; g.ldr = 256;                                                                        // src += ffn(src2)
        RUN(launch_gemm(g, s));
    }
    RUN(launch_layernorm(f.X, 256, m->enc_norm.g, m->enc_norm.b, f.X1, 256, Mmax, Mdev, 256, s));       // memory = encoder.norm(src)
    const float* MEM = f.X1;
    // decoder keys / values of all layers: k = (memory + pos) W_k^T, v = memory W_v^T (cone/transformer.py:333-336)
    g = G(m, MEM, 256, m->dec_k.w, 256, m->dec_k.b, f.KD, 256 * nd, Mmax, Mdev, 256 * nd, 256);
    g.A2 = f.POS; g.lda2 = 256;
    RUN(launch_gemm(g, s));
    RUN(launch_gemm(G(m, MEM, 256, m->dec_v.w, 256, m->dec_v.b, f.VD, 256 * nd, Mmax, Mdev, 256 * nd, 256), s));
    CONE_CHECK_HIP(hipMemsetAsync(f.TGT, 0, (size_t)T * 256 * sizeof(float), s));                       // tgt = 0 (:66)
    for (int l = 0; l < nd; ++l) {
        const DecLayer& dl = m->dec[l];
        RUN(dec_layer_front(m, f, l, B, true, s));
        RUN(dec_cross_attn(m, c, p, f, l, MEM, s));                                                     // (CROSS_SMALL: no fold here)
        g = G(m, f.DATT, 256, dl.ca.out.w, 256, dl.ca.out.b, f.TGT, 256, T, nullptr, 256, 256, EPI_RESIDUAL);
        g.R = f.TGT; g.ldr = 256;
        RUN(launch_gemm(g, s));
        RUN(launch_layernorm(f.TGT, 256, dl.n3.g, dl.n3.b, f.TGT1, 256, T, nullptr, 256, s));           // tgt2 = norm3(tgt)
        RUN(launch_gemm(G(m, f.TGT1, 256, dl.l1.w, 256, dl.l1.b, f.DH, ff, T, nullptr, ff, 256, EPI_RELU), s));
        g = G(m, f.DH, ff, dl.l2.w, ff, dl.l2.b, f.TGT, 256, T, nullptr, 256, ff, EPI_RESIDUAL);
        g.R = f.TGT; g.ldr = 256;
        RUN(launch_gemm(g, s));
        RUN(launch_layernorm(f.TGT, 256, m->dec_norm.g, m->dec_norm.b, f.HS + (size_t)l * T * 256, 256, T, nullptr, 256, s));
    }
    return heads_and_taps(m, c, HeadBufs{f.HS, f.S1, f.S2, f.LG, f.SP, f.off}, MEM, false, s);
}

// ------------------------------------------------------------------------------ the layer tail
// Everything of a transformer layer behind its attention, for encoder and decoder layers, post-norm and pre-norm: the one
// place that reads the options (bf16, split_bf16, ffn_fused, ffn_spread, qkv_fused), the spread scratch f.SPR and the
// *_supported / *_qkv_fits predicates, and picks a launcher.  The caller fills a TailArgs from enc_tail[l] / dec_tail[l] and
// its buffers; t.next != null OFFERS the ride of the next encoder layer's q | k | v projection (QKV, n_qkv set), *rode says
// whether it was taken (rode may be null where none is offered).  Every choice is by the host-known row bound t.M, never by *t.M_dev.  First matching row wins:
//
//   t.pre (the fused pre-norm path; plan_forward admits it only with ffn_fused = 2 and an ff the fused kernels take;
//   split_bf16 is not consulted; no ride)
//     1  bf16                                                     TAIL_MODES[TAIL_IMG_BF16]->proj_ffn_prenorm
//     2  ffn_spread, scratch, <= 64 row groups, ff % 256 == 0     launch_proj_ffn_spread (pre)
//     3  ffn_spread, <= FFN_WIDE_GROUPS row groups, a wide ff     launch_proj_ffn_prenorm_wide (ffn_spread = 0 switches it off too)
//     4  otherwise                                                launch_proj_ffn_prenorm (persistent 128-row kernel)
//   post-norm with ffn_fused = 2, an ff the fused kernels take and no x + pos second output wanted (t.C2 == null)
//     5  bf16                                                     TAIL_MODES[TAIL_IMG_BF16]->proj_ffn; rides if qkv_fused >= 1 and it fits the LDS
//     6  split_bf16                                               TAIL_MODES[TAIL_IMG_SPLIT]->proj_ffn; rides likewise
//     7  exact fp32, ride offered, qkv_fused = 2, fits the LDS    launch_proj_ffn_fused with the ride (persistent 128-row kernel)
//     8  exact fp32, ffn_spread, scratch, <= 64 row groups, ...   launch_proj_ffn_spread
//     9  exact fp32 otherwise                                     launch_proj_ffn_fused: wide form (<= FFN_WIDE_GROUPS), 64-row
//                                                                 form, 128-row form + wide remainder -- chosen INSIDE it (ffn.hip)
//   post-norm otherwise (ffn_fused = 1 / 0, an ff the fused kernels do not take, or t.C2: the encoder off the table path,
//   whose next layer reads x + pos -- only the GEMM epilogue writes that)
//    10  out-proj GEMM with residual + LayerNorm epilogue into t.X1, then
//          ffn_fused >= 1, ff taken, no t.C2                      launch_ffn_fused (the block as one kernel)
//          else                                                   GEMM + ReLU into t.H, GEMM + residual + LayerNorm (+ C2 = OUT + ADD)
//   (The bf16 modes exist only with their images, and images only for an ff the fused kernels take: rows 5 / 6 need no
//   check of their own.  A decoder layer offers no ride and has no M_dev; otherwise its ladder is the encoder's.)
static int launch_layer_tail(const cone_model* m, const FwdBuffers& f, TailArgs t, hipStream_t s, bool* rode = nullptr) {
    bool no_ride;
    if (!rode) rode = &no_ride;
    const TailWeights* next = t.next;
    const int ff = t.ff;
    const bool bf16 = m->opt_bf16 && m->bf16_img, split = m->opt_split_bf16 && m->split_img;
    const bool spread = m->opt_spread && f.SPR && ffn_spread_supported(t.M, ff);
    t.next = nullptr;
    t.scratch = f.SPR;
    t.packed = m->opt_tail_packed != 0;
    *rode = false;
    if (t.pre) {
        if (bf16) return TAIL_MODES[TAIL_IMG_BF16]->proj_ffn_prenorm(t, s);
        if (spread) return launch_proj_ffn_spread(t, s);
        if (m->opt_spread && (t.M + 15) / 16 <= FFN_WIDE_GROUPS && ffn_wide_supported(ff)) return launch_proj_ffn_prenorm_wide(t, s);
        return launch_proj_ffn_prenorm(t, s);
    }
    const bool block_fused = !t.C2 && m->opt_ffn_fused && ffn_fused_supported(ff);
    if (block_fused && m->opt_ffn_fused >= 2) {
        if (bf16 || split) {
            const TailMode& k = *TAIL_MODES[bf16 ? TAIL_IMG_BF16 : TAIL_IMG_SPLIT];
            *rode = next && m->opt_qkv_fused && k.qkv_fits(ff, t.n_qkv);
            if (*rode) t.next = next;
            return k.proj_ffn(t, s);
        }
        // (the ride on the exact-fp32 kernel: measured neutral against the separate GEMM launch -- 44.3 vs 44.1 ms of kernel
        // time per step -- so only on request: qkv_fused = 2)
        *rode = next && m->opt_qkv_fused >= 2 && ffn_fused_qkv_fits(ff, t.n_qkv);
        if (*rode) t.next = next;
        else if (spread) return launch_proj_ffn_spread(t, s);
        return launch_proj_ffn_fused(t, s);
    }
    const TailWeights& w = *t.w;
    GemmArgs g = G(m, t.A, t.lda, w.Wo, 256, w.bo, t.X1, 256, t.M, t.M_dev, 256, 256, EPI_RESIDUAL | EPI_LN);
    g.R = t.R; g.ldr = t.ldr; g.ln_g = w.in_g; g.ln_b = w.in_b;
    RUN(launch_gemm(g, s));                                                             // LN_in(R + A Wo^T + bo)
    if (block_fused)
        return launch_ffn_fused(t.X1, 256, w.W1, w.b1, w.W2, w.b2, w.out_g, w.out_b, t.OUT, t.ldo, t.M, t.M_dev, ff, s);
    RUN(launch_gemm(G(m, t.X1, 256, w.W1, 256, w.b1, t.H, ff, t.M, t.M_dev, ff, 256, EPI_RELU), s));
    g = G(m, t.H, ff, w.W2, ff, w.b2, t.OUT, t.ldo, t.M, t.M_dev, 256, ff, EPI_RESIDUAL | EPI_LN);
    g.R = t.X1; g.ldr = 256; g.ln_g = w.out_g; g.ln_b = w.out_b;
    g.C2 = t.C2; g.ADD = t.ADD;
    return launch_gemm(g, s);                                                           // LN_out(x1 + ffn(x1))
}
// a tail on 256-float rows: attention rows A, residual R, output OUT (may be R)
static TailArgs tail_args(const TailWeights* w, const float* A, const float* R, float* OUT, int M, const int* M_dev, int ff) {
    TailArgs t{};
    t.A = A; t.lda = 256; t.R = R; t.ldr = 256; t.w = w; t.OUT = OUT; t.ldo = 256; t.M = M; t.M_dev = M_dev; t.ff = ff;
    return t;
}

// ------------------------------------------------------------------------------ general-shape forward
// Any supported (d, heads), post-norm and pre-norm (cone/transformer.py:233-260, 296-342), built from plain launches:
// LayerNorm, row GEMMs with residual / ReLU epilogues, the attention core of general.hip (encoder self-attention over the
// packed tokens, decoder self-attention over the slots, cross-attention to the window's memory: up to 256 keys resident in LDS, up to 1024 streamed), and the
// d-wide pack / head / saliency kernels.  What it does not fuse: the LayerNorms (own launches, no GEMM epilogue), the layer
// tails, the decoder's memory K / V projections (two GEMMs over all layers), the first decoder layer (run per window, from
// tgt = 0, only the slot-position tables are per-checkpoint constants) -- and it reads no layer-0 caches or position tables:
// q | k take x + pos as the GEMM's second A operand.
struct GenBuffers {
    int* off;
    float *X, *X1, *T1, *POS, *QKV, *ATT, *H, *KD, *VD;
    float *TGT, *TGT1, *TGT2, *DQK, *DATT, *DQ, *DH, *HS, *S1, *S2, *LG, *SP;
};
static void carve_gen(const cone_model* m, Carver& c, int B, int Lmax, GenBuffers& f) {
    const size_t M = (size_t)B * Lmax, T = (size_t)B * m->nq, nd = m->n_dec, d = m->d;
    f.off = c.take<int>(B + 1);
    f.X = c.take<float>(M * d); f.X1 = c.take<float>(M * d); f.T1 = c.take<float>(M * d); f.POS = c.take<float>(M * d);
    f.QKV = c.take<float>(M * 3 * d); f.ATT = c.take<float>(M * d); f.H = c.take<float>(M * m->ff);
    f.KD = c.take<float>(M * d * nd); f.VD = c.take<float>(M * d * nd);
    f.TGT = c.take<float>(T * d); f.TGT1 = c.take<float>(T * d); f.TGT2 = c.take<float>(T * d);
    f.DQK = c.take<float>(T * 3 * d); f.DATT = c.take<float>(T * d); f.DQ = c.take<float>(T * d); f.DH = c.take<float>(T * m->ff);
    f.HS = c.take<float>(nd * T * d); f.S1 = c.take<float>(nd * T * d); f.S2 = c.take<float>(nd * T * d);
    f.LG = c.take<float>(nd * T * 2); f.SP = c.take<float>(nd * T * 2);
}
// workspace of the body the plan picked
static size_t fwd_ws_bytes(const cone_model* m, int B, int Lmax, const FwdPlan& p) {
    Carver c(nullptr, ~(size_t)0);
    FwdBuffers f;
    GenBuffers g;
    if (p.body == BODY_GENERAL) carve_gen(m, c, B, Lmax, g);
    else carve_fwd(m, c, B, Lmax, p, f);
    return c.cur;
}

static int forward_general(const cone_model* m, const FwdCall& call, void* ws, size_t ws_bytes, hipStream_t s) {
    const int d = m->d, hd = m->d / m->heads, nh = m->heads, B = call.B;
    const int Lmax = call.Lv_max + call.Lq_max, Mmax = B * Lmax, T = B * m->nq, nd = m->n_dec, ff = m->ff, nq = m->nq;
    const bool pre = m->pre_norm != 0;
    // key capacity of the attention over the window's tokens: the call's bound, or (a long-window handle) the handle's, so
    // that the kernel form does not depend on the call
    const int kcap = m->long_windows() ? m->opt_max_tokens : Lmax;
    Carver c(ws, ws_bytes);
    GenBuffers f;
    carve_gen(m, c, B, Lmax, f);
    if (!c.ok) { set_error("forward: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    const int* Mdev = f.off + B;
    RUN(launch_scan_lengths(call.vlen, call.qlen, B, f.off, s));
    RUN(launch_gen_pack_pos(call.vproj, call.vrow0, call.vlen, call.tproj, call.trow0, call.qlen, f.off, m->dim_t, f.X, f.POS, d, B,
                            Lmax, s, m->txt_pos_emb, m->txt_pos_ln.g, m->txt_pos_ln.b));
    GemmArgs g;
    // a layer GEMM in the handle's numeric mode: exact fp32, or (general_bf16) the bf16 row GEMM on the weight's image
    auto gemm = [&](const GemmArgs& a) {
        if (!m->opt_general_bf16) return launch_gemm(a, s);
        const void* img = nullptr;
        for (const cone_model::GenImage& gi : m->gen_bf16_images)
            if (gi.W == a.W) { img = gi.img; break; }
        CONE_REQUIRE(img, "forward: general_bf16 is set but a weight has no bf16 image");
        return launch_gemm_bf16(a, img, s);
    };
    auto residual = [&](const float* A, int K, const Linear& lin, const float* R, float* C, int M, const int* M_dev) {
        GemmArgs r = G(m, A, K, lin.w, K, lin.b, C, d, M, M_dev, d, K, EPI_RESIDUAL);   // C = A W^T + b + R
        r.R = R; r.ldr = d;
        return gemm(r);
    };
    for (int l = 0; l < m->n_enc; ++l) {
        const EncLayer& e = m->enc[l];
        const float* A = f.X;
        if (pre) {                                                                                       // src2 = norm1(src)
            RUN(launch_layernorm(f.X, d, e.n1.g, e.n1.b, f.X1, d, Mmax, Mdev, d, s));
            A = f.X1;
        }
        g = G(m, A, d, e.sa.in_w, d, e.sa.in_b, f.QKV, 3 * d, Mmax, Mdev, 2 * d, d);                    // q | k = (a + pos) W^T
        g.A2 = f.POS; g.lda2 = d;
        RUN(gemm(g));
        RUN(gemm(G(m, A, d, e.sa.in_w + 2 * d * d, d, e.sa.in_b + 2 * d, f.QKV + 2 * d, 3 * d, Mmax, Mdev, d, d)));
        RUN(launch_gen_attn(f.QKV, 3 * d, f.QKV + d, 3 * d, f.QKV + 2 * d, 3 * d, f.ATT, d, f.off, f.off, B, 0, nh, hd, kcap, s));
        if (pre) {
            RUN(residual(f.ATT, d, e.sa.out, f.X, f.X, Mmax, Mdev));                                      // src += attn
            RUN(launch_layernorm(f.X, d, e.n2.g, e.n2.b, f.X1, d, Mmax, Mdev, d, s));                     // src2 = norm2(src)
            RUN(gemm(G(m, f.X1, d, e.l1.w, d, e.l1.b, f.H, ff, Mmax, Mdev, ff, d, EPI_RELU)));
            RUN(residual(f.H, ff, e.l2, f.X, f.X, Mmax, Mdev));                                           // src += ffn(src2)
        } else {
            RUN(residual(f.ATT, d, e.sa.out, f.X, f.T1, Mmax, Mdev));
            RUN(launch_layernorm(f.T1, d, e.n1.g, e.n1.b, f.X1, d, Mmax, Mdev, d, s));                    // norm1(src + attn)
            RUN(gemm(G(m, f.X1, d, e.l1.w, d, e.l1.b, f.H, ff, Mmax, Mdev, ff, d, EPI_RELU)));
            RUN(residual(f.H, ff, e.l2, f.X1, f.T1, Mmax, Mdev));
            RUN(launch_layernorm(f.T1, d, e.n2.g, e.n2.b, f.X, d, Mmax, Mdev, d, s));                     // norm2(src + ffn)
        }
    }
    const float* MEM = f.X;
    if (pre) {                                                                                           // memory = encoder.norm(src)
        RUN(launch_layernorm(f.X, d, m->enc_norm.g, m->enc_norm.b, f.X1, d, Mmax, Mdev, d, s));
        MEM = f.X1;
    }
    // decoder keys / values of all layers: k = (memory + pos) W_k^T + b_k, v = memory W_v^T + b_v (cone/transformer.py:308-311)
    g = G(m, MEM, d, m->dec_k.w, d, m->dec_k.b, f.KD, d * nd, Mmax, Mdev, d * nd, d);
    g.A2 = f.POS; g.lda2 = d;
    RUN(gemm(g));
    RUN(gemm(G(m, MEM, d, m->dec_v.w, d, m->dec_v.b, f.VD, d * nd, Mmax, Mdev, d * nd, d)));
    CONE_CHECK_HIP(hipMemsetAsync(f.TGT, 0, (size_t)T * d * sizeof(float), s));                          // tgt = 0 (:66)
    auto ln = [&](const float* x, const LNorm& n, float* out) { return launch_layernorm(x, d, n.g, n.b, out, d, T, nullptr, d, s); };
    for (int l = 0; l < nd; ++l) {
        const DecLayer& dl = m->dec[l];
        // self-attention: q | k | v = a W^T + the slot-position table (q, k: (a + query_pos) W^T + b; v: a W_v^T + b_v)
        const float* A = f.TGT;
        if (pre) { RUN(ln(f.TGT, dl.n1, f.TGT1)); A = f.TGT1; }
        g = G(m, A, d, dl.sa.in_w, d, nullptr, f.DQK, 3 * d, T, nullptr, 3 * d, d, EPI_RESIDUAL);
        g.R = m->dec_sa_tab[l]; g.ldr = 3 * d; g.r_mod = nq;
        RUN(gemm(g));
        RUN(launch_gen_attn(f.DQK, 3 * d, f.DQK + d, 3 * d, f.DQK + 2 * d, 3 * d, f.DATT, d, nullptr, nullptr, B, nq, nh, hd, nq, s));
        if (pre) {
            RUN(residual(f.DATT, d, dl.sa.out, f.TGT, f.TGT, T, nullptr));                                // tgt += sa
            RUN(ln(f.TGT, dl.n2, f.TGT1)); A = f.TGT1;                                                    // tgt2 = norm2(tgt)
        } else {
            RUN(residual(f.DATT, d, dl.sa.out, f.TGT, f.TGT2, T, nullptr));
            RUN(ln(f.TGT2, dl.n1, f.TGT)); A = f.TGT;                                                     // tgt = norm1(tgt + sa)
        }
        // cross-attention: query (a + query_pos) W_q^T + b_q = a W_q^T + the table; keys / values of this layer from KD / VD
        g = G(m, A, d, dl.ca.in_w, d, nullptr, f.DQ, d, T, nullptr, d, d, EPI_RESIDUAL);
        g.R = m->dec_ca_tab[l]; g.ldr = d; g.r_mod = nq;
        RUN(gemm(g));
        RUN(launch_gen_attn(f.DQ, d, f.KD + (size_t)l * d, d * nd, f.VD + (size_t)l * d, d * nd, f.DATT, d, nullptr, f.off, B, nq, nh,
                            hd, kcap, s));
        if (pre) {
            RUN(residual(f.DATT, d, dl.ca.out, f.TGT, f.TGT, T, nullptr));                                // tgt += ca
            RUN(ln(f.TGT, dl.n3, f.TGT1));                                                                // tgt2 = norm3(tgt)
            RUN(gemm(G(m, f.TGT1, d, dl.l1.w, d, dl.l1.b, f.DH, ff, T, nullptr, ff, d, EPI_RELU)));
            RUN(residual(f.DH, ff, dl.l2, f.TGT, f.TGT, T, nullptr));                                     // tgt += ffn(tgt2)
        } else {
            RUN(residual(f.DATT, d, dl.ca.out, f.TGT, f.TGT2, T, nullptr));
            RUN(ln(f.TGT2, dl.n2, f.TGT1));                                                               // tgt = norm2(tgt + ca)
            RUN(gemm(G(m, f.TGT1, d, dl.l1.w, d, dl.l1.b, f.DH, ff, T, nullptr, ff, d, EPI_RELU)));
            RUN(residual(f.DH, ff, dl.l2, f.TGT1, f.TGT2, T, nullptr));
            RUN(ln(f.TGT2, dl.n3, f.TGT));                                                                // tgt = norm3(tgt + ffn)
        }
        RUN(ln(f.TGT, m->dec_norm, f.HS + (size_t)l * T * d));                                            // decoder.norm (intermediate)
    }
    return heads_and_taps(m, call, HeadBufs{f.HS, f.S1, f.S2, f.LG, f.SP, f.off}, MEM, true, s);
}

// Most windows one call may hold: launch_pack_pos, launch_pack_l0, launch_row_index, launch_add_pos_rows, launch_saliency,
// launch_compact_index and their d-wide forms put the window index in gridDim.y, so B is bounded by the device's
// maxGridSize[1] -- read from the device properties once per device (0: the query failed).
static int grid_limit_y() {
    static std::mutex mu;
    static int limit[CONE_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= CONE_MAX_DEVICES) return 0;
    std::lock_guard<std::mutex> lk(mu);
    if (limit[dev] <= 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxGridDimY, dev) == hipSuccess) limit[dev] = v;
    }
    return limit[dev];
}
#define CONE_REQUIRE_GRID_Y(what, B)                                                                                          \
    do {                                                                                                                       \
        const int lim_ = grid_limit_y();                                                                                       \
        CONE_REQUIRE(lim_ > 0, what ": the device's grid limit could not be read");                                            \
        CONE_REQUIRE((B) <= lim_, what ": %d windows in one call exceed the device's grid limit of %d (gridDim.y)", (B), lim_); \
    } while (0)

// The forward behind every entry, on the plan its caller made (plan_forward).  Its own body is the 256-wide packed path,
// post-norm and (p.pre, table path only) pre-norm with the fused tails: the same launches either way -- position tables, ONE
// N = 768 GEMM per encoder layer, the fused layer tail, the folded decoder cross-attention.  Pre-norm differs in where the
// LayerNorms sit (Z = the normalised rows the next consumer reads, the tail's second output), in that its first layer reads
// the row caches all or nothing, and in that it has no first-decoder-layer constants and computes every layer's heads.
static int forward_packed(const cone_model* m, const FwdCall& c, const FwdPlan& p, void* ws, size_t ws_bytes, hipStream_t s) {
    const int B = c.B, Lv_max = c.Lv_max, Lq_max = c.Lq_max;
    CONE_REQUIRE(B > 0 && Lv_max > 0 && Lq_max >= 0, "forward: bad sizes B=%d Lv=%d Lq=%d", B, Lv_max, Lq_max);
    CONE_REQUIRE_GRID_Y("forward", B);
    const int Lmax = Lv_max + Lq_max;
    if (m->long_windows())
        CONE_REQUIRE(Lmax <= m->opt_max_tokens, "forward: window length %d + %d exceeds the handle's max_window_tokens = %d",
                     Lv_max, Lq_max, m->opt_max_tokens);
    else
        CONE_REQUIRE(Lmax <= CONE_MAX_WINDOW_TOKENS, "forward: window length %d + %d exceeds %d tokens", Lv_max, Lq_max,
                     CONE_MAX_WINDOW_TOKENS);
    // beyond 192 tokens only the default path exists (the 256-key forms of the encoder attention and of the folded cross-
    // attention): the A/B forms and the unfolded decoder stop at 192 keys (the general path: any length up to the limit)
    if (p.body != BODY_GENERAL)
        CONE_REQUIRE(Lmax <= 192 || p.long_ok,
                     "forward: windows of %d tokens (> 192) run only on the default table path with 3 / 5 / 8 decoder slots", Lmax);
    CONE_REQUIRE((int64_t)B * Lmax < (1ll << 24), "forward: batch too large (B * L >= 2^24 tokens)");
    if (m->txt_pos_emb)
        CONE_REQUIRE(Lq_max <= m->txt_pos_rows, "forward: %d text tokens but txt_position_embed has %d rows (max_q_l)", Lq_max,
                     m->txt_pos_rows);
    if (p.body == BODY_GENERAL) return forward_general(m, c, ws, ws_bytes, s);      // (no layer-0 caches or tables read)
    const cone_layer0& l0 = p.l0;
    if (p.have_l0)  // (the handle's own tables or the caller's: either must cover the longest window of the call)
        CONE_REQUIRE(l0.pos_qk && l0.max_v_l >= Lv_max,
                     "forward: position tables / layer-0 cache built for a shorter window (%d < %d clips)", l0.max_v_l, Lv_max);
    Carver cv(ws, ws_bytes);
    FwdBuffers f;
    carve_fwd(m, cv, B, Lmax, p, f);
    if (!cv.ok) { set_error("forward: workspace too small (%zu < %zu)", ws_bytes, cv.cur); return CONE_E_WORKSPACE; }
    if (p.body == BODY_PRENORM_PLAIN) return forward_packed_prenorm(m, c, p, f, s);
    const int Mmax = B * Lmax, T = B * m->nq, nd = m->n_dec, ff = m->ff;
    const int* Mdev = f.off + B;
    float* Z = f.X1;                                    // pre: the normalised rows

    RUN(launch_scan_lengths(c.vlen, c.qlen, B, f.off, s));
    if (p.gather_res) {
        // first layer entirely from the per-clip / per-token rows: attention gathers q|k|v, the fused layer tail gathers its
        // residual rows through a row index -- no packed copy of the input
        RUN(launch_row_index(c.vrow0, c.vlen, c.trow0, c.qlen, f.off, f.RIDX, B, Lmax, s));
    } else if (p.caches) {
        // X (and, off the table path, POS): the first layer's attention gathers q|k|v from the caches itself; with
        // the gather switched off a packing pass writes them out first
        RUN(launch_pack_l0(c.vproj, c.vrow0, c.vlen, c.tproj, c.trow0, c.qlen, f.off, m->dim_t, l0.qkv_vid, l0.qkv_txt,
                           l0.pos_qk, f.X, f.POS, p.gather0 ? nullptr : f.QKV, p.gather0 ? nullptr : f.QKV + (size_t)Mmax * 512,
                           B, Lmax, s));
    } else if (p.tables) {
        // no row caches (a caller that hands over projected rows only): the packed layer input, nothing else -- the first
        // layer then runs like the later ones (one N = 768 GEMM on x, position rows from the table)
        RUN(launch_pack_l0(c.vproj, c.vrow0, c.vlen, c.tproj, c.trow0, c.qlen, f.off, m->dim_t, nullptr, nullptr, nullptr, f.X,
                           nullptr, nullptr, nullptr, B, Lmax, s));
    } else {
        RUN(launch_pack_pos(c.vproj, c.vrow0, c.vlen, c.tproj, c.trow0, c.qlen, f.off, m->dim_t, f.X, f.POS, f.XP, B, Lmax, s,
                            m->txt_pos_emb, m->txt_pos_ln.g, m->txt_pos_ln.b));
    }
    if (p.pre && !p.gather_res)
        RUN(launch_layernorm(f.X, 256, m->enc[0].n1.g, m->enc[0].n1.b, Z, 256, Mmax, Mdev, 256, s));    // norm1 of layer 0

    bool qkv_fused = false;               // this layer's q | k | v rows were written by the previous layer's tail
    for (int l = 0; l < m->n_enc; ++l) {  // cone/transformer.py:233-246, pre: :248-260
        const EncLayer& e = m->enc[l];
        AttnSrc src{};
        int mode = ATTN_PACKED;
        if (l == 0 && p.gather0) {
            mode = ATTN_GATHER;
            src = table_attn_src(c, l0, 0);
            src.qkv_vid = l0.qkv_vid; src.qkv_txt = l0.qkv_txt; src.vrow0 = c.vrow0; src.trow0 = c.trow0;
        } else if (l == 0 && p.caches) {                    // packed by pack_l0: (M, 512) q|k then (M, 256) v
            src.Q = f.QKV; src.K = f.QKV + 256; src.V = f.QKV + (size_t)Mmax * 512;
            src.ldq = src.ldk = 512; src.ldv = 256;
        } else if (p.tables) {
            // q | k | v = x W^T + b in ONE N = 768 GEMM on x (pre: on norm1(x)); the attention adds pos W_qk^T of this layer
            // from the static table: no x + pos matrix, no second A operand
            if (!qkv_fused)     // (else: written by the previous layer's tail from the registers that held its output rows)
                RUN(encoder_qkv(m, l, p.pre ? Z : f.X, f.QKV, Mmax, Mdev, s, !p.pre));
            mode = ATTN_POSADD;
            src = table_attn_src(c, l0, l);
            src.Q = f.QKV; src.K = f.QKV + 256; src.V = f.QKV + 512; src.ldq = src.ldk = src.ldv = 768;
        } else {
            float* QK = f.QKV; float* V = f.QKV + (size_t)Mmax * 512;
            RUN(launch_gemm(G(m, f.XP, 256, e.sa.in_w, 256, e.sa.in_b, QK, 512, Mmax, Mdev, 512, 256), s));  // q | k = (x+pos) W^T
            RUN(launch_gemm(G(m, f.X, 256, e.sa.in_w + 512 * 256, 256, e.sa.in_b + 512, V, 256, Mmax, Mdev, 256, 256), s));
            src.Q = QK; src.K = QK + 256; src.V = V; src.ldq = src.ldk = 512; src.ldv = 256;
        }
        RUN(launch_enc_attn(mode, src, f.ATT, f.off, B, Lmax, s));
        // everything behind the attention: norm2(x1 + ffn(x1)), x1 = norm1(x + attn Wo^T + bo) -- by default ONE launch, in place
        // (a workgroup reads its 128 rows of x before it writes them, and nobody else touches them), in which the next layer's
        // q | k | v projection may ride (its input rows are that kernel's output; ATT and QKV are disjoint parts of the H region)
        const bool g0 = l == 0 && p.gather_res;
        TailArgs t = tail_args(&m->enc_tail[l], f.ATT, g0 ? c.vproj : f.X, f.X, Mmax, Mdev, ff);
        if (g0) { t.r_idx = f.RIDX; t.R2 = c.tproj; }
        if (p.pre) {
            t.pre = true; t.OUT2 = Z; t.ldo2 = 256;         // Z = the next consumer's norm of the stream
        } else {
            if (l + 1 < m->n_enc) t.next = &m->enc_tail[l + 1];
            t.QKV = f.QKV; t.ldq = 768; t.n_qkv = 768;
            t.X1 = f.X1; t.H = f.H;
            if (!p.tables) { t.C2 = f.XP; t.ADD = f.POS; }  // x + pos for the next layer's q/k / the decoder's keys
        }
        RUN(launch_layer_tail(m, f, t, s, &qkv_fused));
    }
    const float* MEM = p.pre ? Z : f.X;                     // (pre: encoder.norm(src))

    // decoder (cone/transformer.py:296-317, 117-146, pre: :319-342).  Default: the memory K / V projections are folded into
    // the cross-attention kernel (dec_cross.hip); otherwise memory K/V for all layers in two GEMMs.
    const int h0 = p.h0, HT = (nd - h0) * T;
    const size_t hoff = (size_t)h0 * T;
    // only the last layer's heads wanted (the eval pipeline): they write straight into the caller's logits / spans; with the
    // intermediate layers' too, all layers go to the workspace and the last layer's rows are copied out
    float* LGo = p.want_aux ? f.LG + hoff * 2 : c.logits;
    float* SPo = p.want_aux ? f.SP + hoff * 2 : c.spans;
    // the position rows come from the tables inside the cross-attention kernels -- unless text tokens carry their own
    // (--use_txt_pos): then memory + pos is written once (dec_xp) and the kernels run their x + pos form
    if (p.dec_xp) RUN(launch_add_pos_rows(MEM, f.off, c.vlen, l0.pos_rows, f.XP, B, Lmax, s, l0.txt_pos, c.trow0));
    if (!p.fold) {
        if (p.dec_tab) RUN(launch_add_pos_rows(MEM, f.off, c.vlen, l0.pos_rows, f.XP, B, Lmax, s));
        GemmArgs g = G(m, f.XP, 256, m->dec_k.w, 256, m->dec_k.b, f.KD, 256 * nd, Mmax, Mdev, 256 * nd, 256);
        RUN(launch_gemm(g, s));                                                             // k = (memory+pos) W_k^T
        RUN(launch_gemm(G(m, MEM, 256, m->dec_v.w, 256, m->dec_v.b, f.VD, 256 * nd, Mmax, Mdev, 256 * nd, 256), s));
    }
    if (!p.dec0)                     // tgt = 0 is only read by the first layer's own projections (constants otherwise)
        CONE_CHECK_HIP(hipMemsetAsync(f.TGT, 0, (size_t)T * 256 * sizeof(float), s));
    for (int l = 0; l < nd; ++l) {
        // Layer 0 starts from tgt = 0 (cone/transformer.py:66): its self-attention block and its cross-attention queries do
        // not depend on the window: per-checkpoint constants (dec0_constants, at cone_model_create, by the same kernels on
        // ONE window's nq rows: identical bits), replicated to the T rows of the batch in one launch
        if (l == 0 && p.dec0) RUN(launch_tile_rows2(f.TGT1, m->dec0_tgt1, f.DQ, m->dec0_dq, m->nq, T, s));
        else RUN(dec_layer_front(m, f, l, B, p.pre, s));
        RUN(dec_cross_attn(m, c, p, f, l, MEM, s));
        if (p.pre) {
            TailArgs t = tail_args(&m->dec_tail[l], f.DATT, f.TGT, f.TGT, T, nullptr, ff);
            t.pre = true; t.OUT2 = f.HS + (size_t)l * T * 256; t.ldo2 = 256;                // decoder.norm of this layer's rows
            RUN(launch_layer_tail(m, f, t, s));
            continue;
        }
        TailArgs t = tail_args(&m->dec_tail[l], f.DATT, f.TGT1, f.TGT, T, nullptr, ff);    // tgt = norm3(x1 + ffn(x1)), x1 = norm2(tgt1 + ca)
        t.X1 = f.TGT2; t.H = f.DH;
        RUN(launch_layer_tail(m, f, t, s));
        // decoder.norm + heads on an intermediate layer only feed aux_outputs / the hs tap (unused by inference,
        // cone/inference.py:54-59): computed on request only
        if (l == nd - 1 || p.want_aux) {
            if (p.heads_chain) {
                // few rows: decoder.norm -> class head, span MLP -> span head of THIS layer's rows in one launch (rows_chain.h);
                // the normalised rows are written only when the hs tap asks for them
                ChainArgs ca{};
                ca.A = f.TGT; ca.lda = 256; ca.M = T; ca.n_stages = 3;
                const size_t ro = (size_t)(l - h0) * T * 2;
                ChainStage& c0 = ca.st[0];
                c0.kind = 1; c0.ln_g = m->dec_norm.g; c0.ln_b = m->dec_norm.b;
                c0.C = c.taps && c.taps->hs ? f.HS + (size_t)l * T * 256 : nullptr; c0.ldc = 256;
                c0.hw = m->class_embed.w; c0.hb = m->class_embed.b; c0.hout = LGo + ro; c0.hld = 2; c0.hnout = 2; c0.hact = 0;
                ChainStage& c1 = ca.st[1];
                c1.kind = 0; c1.K = 256; c1.W = m->span[0].w; c1.bias = m->span[0].b; c1.flags = EPI_RELU;
                ChainStage& c2 = ca.st[2];
                c2.kind = 0; c2.K = 256; c2.W = m->span[1].w; c2.bias = m->span[1].b; c2.flags = EPI_RELU;
                c2.hw = m->span[2].w; c2.hb = m->span[2].b; c2.hout = SPo + ro; c2.hld = 2; c2.hnout = 2; c2.hact = 1;
                RUN(launch_rows_chain(ca, s));
            } else {
                RUN(launch_layernorm(f.TGT, 256, m->dec_norm.g, m->dec_norm.b, f.HS + (size_t)l * T * 256, 256, T, nullptr,
                                     256, s));
            }
        }
    }
    if (p.pre) return heads_and_taps(m, c, HeadBufs{f.HS, f.S1, f.S2, f.LG, f.SP, f.off}, MEM, false, s);
    // heads (cone/model.py:112-117); the last layer is the prediction
    if (!p.heads_chain) {
        RUN(launch_rowdot(f.HS + hoff * 256, 256, m->class_embed.w, m->class_embed.b, LGo, 2, HT, 2, 0, s));
        RUN(launch_gemm(G(m, f.HS + hoff * 256, 256, m->span[0].w, 256, m->span[0].b, f.S1, 256, HT, nullptr, 256, 256, EPI_RELU), s));
        RUN(launch_gemm(G(m, f.S1, 256, m->span[1].w, 256, m->span[1].b, f.S2, 256, HT, nullptr, 256, 256, EPI_RELU), s));
        RUN(launch_rowdot(f.S2, 256, m->span[2].w, m->span[2].b, SPo, 2, HT, 2, 1, s));
    }
    const size_t last = (size_t)(nd - 1) * T * 2;
    if (p.want_aux) {
        CONE_CHECK_HIP(hipMemcpyAsync(c.logits, f.LG + last, (size_t)T * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
        CONE_CHECK_HIP(hipMemcpyAsync(c.spans, f.SP + last, (size_t)T * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    RUN(copy_taps(c.taps, f.HS, f.LG, f.SP, nd, T, 256, s));
    if ((c.saliency && !p.sal_ride) || (c.taps && c.taps->memory))  // saliency == NULL: not wanted (cone/inference.py never reads it)
        RUN(launch_saliency(MEM, f.off, c.vlen, c.qlen, m->saliency.w, m->saliency.b, p.sal_ride ? nullptr : c.saliency, Lv_max,
                            c.taps ? c.taps->memory : nullptr, Lq_max, B, s));
    return 0;
}

__global__ void iota_fill_kernel(int* a, int* b, int n, int stride, int v) {    // a[i] = i * stride, b[i] = v
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = i * stride; b[i] = v; }
}

}  // namespace cone

using namespace cone;

extern "C" const char* cone_last_error(void) { return g_err; }
extern "C" int cone_abi_version(void) { return CONE_HIP_ABI_VERSION; }

extern "C" int cone_model_create(const cone_weights* w, cone_model** out) { return build_model(w, out); }
extern "C" void cone_model_destroy(cone_model* m) {
    if (m) free_model(m);
}

extern "C" size_t cone_adapter_norm_workspace(const cone_model* m, int64_t n_rows) {
    return align_up((size_t)n_rows * m->d * 4, 256) + align_up((size_t)n_rows * m->dv * 4, 256);
}
extern "C" int cone_adapter_norm(const cone_model* m, const float* x, int64_t n_rows, float* out, int renorm,
                                 void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && x && out, "adapter_norm: null argument");
    CONE_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "adapter_norm: bad row count");
    hipStream_t s = (hipStream_t)stream;
    if (!m->has_adapter) {  // adapter_module == "none": features pass through (cone/inference.py:259-260)
        if (out != x)
            CONE_CHECK_HIP(hipMemcpyAsync(out, x, (size_t)n_rows * m->dv * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    Carver c(ws, ws_bytes);
    const int d = m->d;       // the adapter's hidden width is hidden_dim (cone/model.py:80)
    float* h = c.take<float>((size_t)n_rows * d);
    float* y = c.take<float>((size_t)n_rows * m->dv);
    if (!c.ok) { set_error("adapter_norm: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    RUN(launch_gemm(G(m, x, m->dv, m->adapter[0].w, m->dv, m->adapter[0].b, h, d, (int)n_rows, nullptr, d, m->dv, EPI_RELU), s));
    GemmArgs g = G(m, h, d, m->adapter[1].w, d, m->adapter[1].b, renorm ? y : out, m->dv, (int)n_rows, nullptr, m->dv,
                   d, EPI_RESIDUAL);
    g.R = x; g.ldr = m->dv;
    RUN(launch_gemm(g, s));
    if (!renorm) return 0;                       // run_on_video/cone_localizator.py:135-138 keeps the raw sum
    return launch_l2norm(y, n_rows, m->dv, 0.f, out, s);
}

extern "C" int cone_l2_normalize_rows(const float* x, int64_t n_rows, int dim, float eps, int clamp, float* out,
                                      void* stream) {
    return launch_l2norm(x, n_rows, dim, eps, out, (hipStream_t)stream, clamp);
}

extern "C" int cone_rows_to_bf16(const float* x, int64_t n_rows, int dim, uint16_t* out, void* stream) {
    CONE_REQUIRE(x && out, "rows_to_bf16: null argument");
    CONE_REQUIRE(n_rows > 0, "rows_to_bf16: bad row count");
    CONE_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0, "rows_to_bf16: x must be 16-B aligned, out 8-B aligned");
    return launch_rows_to_bf16(x, n_rows, dim, out, (hipStream_t)stream);
}

// cone_adapter_norm whose LAST stage stores bf16 (the same launches up to it, so the same fp32 values go into the rounding)
extern "C" int cone_adapter_norm_bf16(const cone_model* m, const float* x, int64_t n_rows, uint16_t* out, int renorm,
                                      void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && x && out, "adapter_norm_bf16: null argument");
    CONE_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "adapter_norm_bf16: bad row count");
    CONE_REQUIRE(((uintptr_t)out & 15) == 0, "adapter_norm_bf16: out must be 16-B aligned (the bf16 pre-filter's arena)");
    hipStream_t s = (hipStream_t)stream;
    if (!m->has_adapter)    // adapter_module == "none": the features pass through, rounded
        return launch_rows_to_bf16(x, n_rows, m->dv, out, s);
    Carver c(ws, ws_bytes);
    const int d = m->d;
    float* h = c.take<float>((size_t)n_rows * d);
    float* y = c.take<float>((size_t)n_rows * m->dv);
    if (!c.ok) { set_error("adapter_norm_bf16: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    RUN(launch_gemm(G(m, x, m->dv, m->adapter[0].w, m->dv, m->adapter[0].b, h, d, (int)n_rows, nullptr, d, m->dv, EPI_RELU), s));
    GemmArgs g = G(m, h, d, m->adapter[1].w, d, m->adapter[1].b, y, m->dv, (int)n_rows, nullptr, m->dv, d, EPI_RESIDUAL);
    g.R = x; g.ldr = m->dv;
    RUN(launch_gemm(g, s));
    // renorm: the L2 norm's own store is the bf16 one (the normalised fp32 rows never reach memory); the localizer's raw sum
    // (renorm == 0) is converted from the GEMM's fp32 output
    return renorm ? launch_l2norm_bf16(y, n_rows, m->dv, 0.f, out, s) : launch_rows_to_bf16(y, n_rows, m->dv, out, s);
}

extern "C" size_t cone_project_workspace(const cone_model* m, int which, int64_t n_rows) {
    return project_ws_bytes(m, which, n_rows);
}
extern "C" int cone_project_tokens(const cone_model* m, int which, const float* x, int64_t n_rows, float* out,
                                   void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && x && out && (which == 0 || which == 1), "project_tokens: bad argument");
    if (n_rows <= 0) return 0;
    return project_tokens(m, which, x, n_rows, out, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" size_t cone_forward_packed_workspace(const cone_model* m, int B, int Lv_max, int Lq_max,
                                                const cone_layer0* l0) {
    FwdCall c{};
    c.B = B; c.Lv_max = Lv_max; c.Lq_max = Lq_max;
    return fwd_ws_bytes(m, B, Lv_max + Lq_max, plan_forward(m, c, l0, false));
}
extern "C" int cone_forward_packed(const cone_model* m, const float* vproj, const int32_t* vid_row0,
                                   const int32_t* vid_len, const float* tproj, const int32_t* txt_row0,
                                   const int32_t* txt_len, int B, int Lv_max, int Lq_max, float* logits,
                                   float* spans, float* saliency, const cone_taps* taps, const cone_layer0* l0,
                                   void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && vproj && tproj && vid_row0 && vid_len && txt_row0 && txt_len && logits && spans,
                 "forward_packed: null argument");
    const FwdCall c{vproj, vid_row0, vid_len, tproj, txt_row0, txt_len, B, Lv_max, Lq_max, logits, spans, saliency, taps};
    return forward_packed(m, c, plan_forward(m, c, l0, false), ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int64_t cone_pos_table_rows(int max_v_l) { return pos_table_rows(max_v_l); }

extern "C" int cone_pos_tables(const cone_model* m, int max_v_l, float* pos_rows, float* pos_qk, void* stream) {
    CONE_REQUIRE(m && pos_rows && pos_qk && max_v_l >= 1 && max_v_l <= CONE_TABLE_MAX_V_L, "pos_tables: bad argument");
    return build_pos_tables(m, max_v_l, pos_rows, pos_qk, (hipStream_t)stream);
}

// --use_txt_pos on the table path: the tokens' own position rows and their images under every encoder layer's [W_q | W_k]
// (rows of a GEMM are independent: an arena row and the same token as a compact row of the padded entry get the same bits)
static int text_positions(const cone_model* m, const float* tproj, const int* tok_index, const int* src_row, int mod, int n,
                          const int* n_dev, float* txt_pos, float* txt_pos_qk, hipStream_t s) {
    const int d = m->d;
    if (d == 256)
        RUN(launch_txt_pos_rows(tproj, tok_index, src_row, mod, m->txt_pos_rows, m->txt_pos_emb, m->txt_pos_ln.g, m->txt_pos_ln.b, n,
                                n_dev, txt_pos, s));
    else
        RUN(launch_gen_txt_pos_rows(tproj, tok_index, src_row, mod, m->txt_pos_rows, m->txt_pos_emb, m->txt_pos_ln.g, m->txt_pos_ln.b,
                                    n, n_dev, d, txt_pos, s));
    for (int l = 0; l < m->n_enc; ++l)
        RUN(launch_gemm(G(m, txt_pos, d, m->enc[l].sa.in_w, d, nullptr, txt_pos_qk + (size_t)l * n * 2 * d, 2 * d, n, n_dev, 2 * d,
                          d), s));
    return 0;
}
extern "C" int cone_layer0_text_positions(const cone_model* m, const float* txt_proj_rows, const int32_t* tok_index,
                                          int64_t n_rows, float* txt_pos, float* txt_pos_qk, void* stream) {
    CONE_REQUIRE(m && txt_proj_rows && tok_index && txt_pos && txt_pos_qk && n_rows < (1ll << 31), "layer0_text_positions: bad argument");
    CONE_REQUIRE(m->txt_pos_emb, "layer0_text_positions: the model has no txt_position_embed (--use_txt_pos)");
    if (n_rows <= 0) return 0;
    return text_positions(m, txt_proj_rows, tok_index, nullptr, 1, (int)n_rows, nullptr, txt_pos, txt_pos_qk, (hipStream_t)stream);
}

extern "C" size_t cone_layer0_project_workspace(const cone_model* m, int64_t n_rows) {
    return m && m->pre_norm ? align_up((size_t)n_rows * m->d * 4, 256) : 0;
}
extern "C" int cone_layer0_project(const cone_model* m, const float* proj_rows, int64_t n_rows, float* qkv, void* ws,
                                   size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && proj_rows && qkv && n_rows < (1ll << 31), "layer0_project: bad argument");
    if (n_rows <= 0) return 0;
    CONE_REQUIRE(ws_bytes >= cone_layer0_project_workspace(m, n_rows) && (ws || !m->pre_norm), "layer0_project: workspace too small");
    return layer0_rows(m, proj_rows, (int)n_rows, nullptr, qkv, (float*)ws, (hipStream_t)stream);
}

// The padded entry.  A zero-padded batch is first COMPACTED: the valid clip rows and the valid token rows are gathered by the
// first LayerNorm of their input projection (padding is never projected), every later row-wise step -- the projections, the
// first encoder layer's q | k | v rows -- runs on the compact rows with a device-side row count, and the windows enter
// forward_packed as (row0, len) pairs into them: from there on this IS the arena path of the eval driver (gathering first
// layer, position tables, fused layer tails, folded decoder), bit for bit.
struct PaddedCarve {
    int *voff, *toff, *vidx, *tidx;
    float *vp, *tp, *qv, *qt, *pt, *ptqk;
    char* pws; size_t pw;
};
static void carve_padded(const cone_model* m, Carver& c, int B, int Lv_pad, int Lq_pad, const FwdPlan& plan, PaddedCarve& p) {
    const size_t nv = (size_t)B * Lv_pad, nt = (size_t)B * Lq_pad;
    p.voff = c.take<int>(B + 1); p.toff = c.take<int>(B + 1);
    p.vidx = c.take<int>(nv); p.tidx = c.take<int>(nt);
    p.vp = c.take<float>(nv * m->d); p.tp = c.take<float>(nt * m->d);
    p.qv = p.qt = p.pt = p.ptqk = nullptr;
    if (plan.mk_caches) { p.qv = c.take<float>(nv * 768); p.qt = c.take<float>(nt * 768); }
    if (plan.mk_txt_pos) { p.pt = c.take<float>(nt * 256); p.ptqk = c.take<float>((size_t)m->n_enc * nt * 512); }   // --use_txt_pos
    p.pw = project_ws_bytes(m, 0, nv);
    const size_t pt = project_ws_bytes(m, 1, nt);
    if (pt > p.pw) p.pw = pt;
    p.pws = c.take<char>(p.pw);
}
extern "C" size_t cone_forward_workspace(const cone_model* m, int B, int Lv_pad, int Lq_pad) {
    FwdCall call{};
    call.B = B; call.Lv_max = Lv_pad; call.Lq_max = Lq_pad;
    const FwdPlan plan = plan_forward(m, call, nullptr, true);
    Carver c(nullptr, ~(size_t)0);
    PaddedCarve p;
    carve_padded(m, c, B, Lv_pad, Lq_pad, plan, p);
    return c.cur + fwd_ws_bytes(m, B, Lv_pad + Lq_pad, plan);
}
extern "C" int cone_forward_windows(const cone_model* m, const float* vid, const int32_t* vid_len, const float* txt,
                                    const int32_t* txt_len, int B, int Lv_pad, int Lq_pad, float* logits,
                                    float* spans, float* saliency, const cone_taps* taps, void* ws,
                                    size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && vid && txt && vid_len && txt_len && logits && spans, "forward_windows: null argument");
    CONE_REQUIRE(B > 0 && Lv_pad > 0 && Lq_pad > 0, "forward_windows: bad sizes");
    CONE_REQUIRE_GRID_Y("forward_windows", B);
    CONE_REQUIRE((int64_t)B * Lv_pad < (1ll << 31) && (int64_t)B * Lq_pad < (1ll << 31), "forward_windows: batch too large");
    hipStream_t s = (hipStream_t)stream;
    const size_t nv = (size_t)B * Lv_pad, nt = (size_t)B * Lq_pad;
    // what the packed forward will run on: the handle's tables, and the first-layer row caches / (--use_txt_pos) the text
    // position rows this entry builds itself where the plan asks for them
    FwdCall call{nullptr, nullptr, vid_len, nullptr, nullptr, txt_len, B, Lv_pad, Lq_pad, logits, spans, saliency, taps};
    FwdPlan plan = plan_forward(m, call, nullptr, true);
    Carver c(ws, ws_bytes);
    PaddedCarve p;
    carve_padded(m, c, B, Lv_pad, Lq_pad, plan, p);
    if (!c.ok) { set_error("forward_windows: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    // compact row lists of the valid clips / tokens: offsets (= the windows' first rows), source-row indices, device counts
    RUN(launch_scan_lengths(vid_len, nullptr, B, p.voff, s));
    RUN(launch_scan_lengths(txt_len, nullptr, B, p.toff, s));
    RUN(launch_compact_index(vid_len, p.voff, Lv_pad, p.vidx, txt_len, p.toff, Lq_pad, p.tidx, B, s));
    RUN(project_tokens(m, 0, vid, nv, p.vp, p.pws, p.pw, s, p.vidx, p.voff + B));
    RUN(project_tokens(m, 1, txt, nt, p.tp, p.pws, p.pw, s, p.tidx, p.toff + B));
    cone_layer0& l0 = plan.l0;
    if (plan.mk_caches) {   // the first encoder layer's in_proj once per compact row (cone_layer0_project's kernel)
        RUN(layer0_rows(m, p.vp, (int)nv, p.voff + B, p.qv, (float*)p.pws, s));     // (scratch: the projections are done with it)
        RUN(layer0_rows(m, p.tp, (int)nt, p.toff + B, p.qt, (float*)p.pws, s));
        l0.qkv_vid = p.qv; l0.qkv_txt = p.qt;
    }
    if (plan.mk_txt_pos) {   // a compact token row's index in its query = its column in the padded batch (masks are prefixes)
        RUN(text_positions(m, p.tp, nullptr, p.tidx, Lq_pad, (int)nt, p.toff + B, p.pt, p.ptqk, s));
        l0.txt_pos = p.pt; l0.txt_pos_qk = p.ptqk; l0.n_txt = (int64_t)nt;
    }
    call.vproj = p.vp; call.vrow0 = p.voff; call.tproj = p.tp; call.trow0 = p.toff;
    return forward_packed(m, call, plan, (char*)ws + c.cur, ws_bytes - c.cur, s);
}

extern "C" size_t cone_clip_matching_workspace(const cone_model* m, int B) {
    const size_t T = (size_t)B * m->nq;
    return 2 * align_up(T * m->dv * 4, 256) + align_up(T * m->d * 4, 256) + 3 * align_up((size_t)B * 4, 256);
}
extern "C" int cone_clip_matching_gathered(const cone_model* m, const float* cls, const int32_t* cls_row,
                                           const float* vid, const int32_t* vid_row0, const int32_t* vid_len,
                                           const int32_t* pad_len, const float* spans, int B, float* match,
                                           void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(m && cls && vid && vid_row0 && vid_len && pad_len && spans && match, "clip_matching: null argument");
    if (B <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int T = B * m->nq, dv = m->dv, d = m->d;
    Carver c(ws, ws_bytes);
    float* pf = c.take<float>((size_t)T * dv);
    float* pa = c.take<float>((size_t)T * dv);
    float* h = c.take<float>((size_t)T * d);
    if (!c.ok) { set_error("clip_matching: workspace too small (%zu < %zu)", ws_bytes, c.cur); return CONE_E_WORKSPACE; }
    RUN(launch_proposal_mean(vid, vid_row0, vid_len, pad_len, spans, B, m->nq, dv, pf, s));
    const float* feat = pf;
    if (m->has_adapter && dv == 256 && d == 256 && m->opt_chain && m->opt_gemm == GEMM_AUTO && rows_chain_supported(T) &&
        !(m->opt_spread && gemm_rows_spread_rows(T))) {
        ChainArgs ca{};     // few proposals: both adapter layers in one launch (rows_chain.h; the same arithmetic)
        ca.A = pf; ca.lda = dv; ca.M = T; ca.n_stages = 2;
        ca.st[0].kind = 0; ca.st[0].K = dv; ca.st[0].W = m->adapter[0].w; ca.st[0].bias = m->adapter[0].b; ca.st[0].flags = EPI_RELU;
        ca.st[1].kind = 0; ca.st[1].K = 256; ca.st[1].W = m->adapter[1].w; ca.st[1].bias = m->adapter[1].b;
        ca.st[1].flags = EPI_RESIDUAL; ca.st[1].R = pf; ca.st[1].ldr = dv; ca.st[1].C = pa; ca.st[1].ldc = dv;
        RUN(launch_rows_chain(ca, s));
        feat = pa;
    } else if (m->has_adapter) {
        RUN(launch_gemm(G(m, pf, dv, m->adapter[0].w, dv, m->adapter[0].b, h, d, T, nullptr, d, dv, EPI_RELU), s));
        GemmArgs g = G(m, h, d, m->adapter[1].w, d, m->adapter[1].b, pa, dv, T, nullptr, dv, d, EPI_RESIDUAL);
        g.R = pf; g.ldr = dv;
        RUN(launch_gemm(g, s));
        feat = pa;
    }
    return launch_cosine_match(feat, cls, cls_row, B, m->nq, dv, match, s);
}
extern "C" int cone_clip_matching(const cone_model* m, const float* cls, const float* vid, const int32_t* vid_len,
                                  int Lv_pad, const float* spans, int B, float* match, void* ws, size_t ws_bytes,
                                  void* stream) {
    CONE_REQUIRE(m && ws, "clip_matching: null argument");
    if (B <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    Carver c(ws, ws_bytes);
    int* vrow0 = c.take<int>(B);
    int* padl = c.take<int>(B);
    if (!c.ok) { set_error("clip_matching: workspace too small"); return CONE_E_WORKSPACE; }
    hipLaunchKernelGGL(iota_fill_kernel, dim3((B + 255) / 256), dim3(256), 0, s, vrow0, padl, B, Lv_pad, Lv_pad);
    CONE_LAUNCH_CHECK();
    return cone_clip_matching_gathered(m, cls, nullptr, vid, vrow0, vid_len, padl, spans, B, match,
                                       (char*)ws + c.cur, ws_bytes - c.cur, stream);
}

// The weight images of option general_bf16: every matrix forward_general's layer GEMMs read, each rounded to nearest even once
// into the slab layout of gemm_bf16.hip (a few MB; one allocation).  Synchronous, like the constants the gemm option rebuilds.
static int build_general_bf16_images(cone_model* m) {
    struct Item { const float* W; int N, K; };
    std::vector<Item> items;
    const int d = m->d, ff = m->ff, nd = m->n_dec;
    for (int l = 0; l < m->n_enc; ++l) {
        const EncLayer& e = m->enc[l];
        items.push_back({e.sa.in_w, 2 * d, d});                         // q | k
        items.push_back({e.sa.in_w + (size_t)2 * d * d, d, d});         // v
        items.push_back({e.sa.out.w, d, d});
        items.push_back({e.l1.w, ff, d});
        items.push_back({e.l2.w, d, ff});
    }
    items.push_back({m->dec_k.w, d * nd, d});
    items.push_back({m->dec_v.w, d * nd, d});
    for (int l = 0; l < nd; ++l) {
        const DecLayer& dl = m->dec[l];
        items.push_back({dl.sa.in_w, 3 * d, d});
        items.push_back({dl.sa.out.w, d, d});
        items.push_back({dl.ca.in_w, d, d});                            // the cross-attention query projection
        items.push_back({dl.ca.out.w, d, d});
        items.push_back({dl.l1.w, ff, d});
        items.push_back({dl.l2.w, d, ff});
    }
    size_t total = 0;
    for (const Item& it : items) {
        CONE_REQUIRE(gemm_bf16_image_bytes(it.N, it.K), "set_option: general_bf16: a %d x %d weight has no bf16 image form", it.N, it.K);
        total += gemm_bf16_image_bytes(it.N, it.K);
    }
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, total);
    if (e != hipSuccess) {
        set_error("set_option: general_bf16: hipMalloc of %zu bytes of weight images failed: %s", total, hipGetErrorString(e));
        return CONE_E_HIP;
    }
    std::vector<cone_model::GenImage> images;
    char* ip = base;
    int rc = 0;
    for (const Item& it : items) {
        rc = launch_gemm_bf16_pack(it.W, it.K, it.N, it.K, ip, nullptr);
        if (rc) break;
        images.push_back({it.W, ip});
        ip += gemm_bf16_image_bytes(it.N, it.K);
    }
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) {
        set_error("set_option: general_bf16: building the weight images failed");
        rc = CONE_E_HIP;
    }
    if (rc) { (void)hipFree(base); return rc; }
    m->gen_bf16_img = base;
    m->gen_bf16_images.swap(images);
    return 0;
}

// The options that are a field and a range: value != 0 for a switch, else inclusive bounds.
struct OptionRow { const char* name; int cone_model::*field; int lo, hi; bool is_switch; };
static const OptionRow OPTION_ROWS[] = {
    {"dec_fold", &cone_model::opt_dec_fold, 0, 5, false},
    {"l0_gather", &cone_model::opt_l0_gather, 0, 1, true},
    {"dec0_const", &cone_model::opt_dec0_const, 0, 1, true},
    {"pos_tables", &cone_model::opt_pos_tables, 0, 1, true},
    {"ffn_fused", &cone_model::opt_ffn_fused, 0, 2, false},
    {"qkv_fused", &cone_model::opt_qkv_fused, 0, 2, false},
    // general_shape 1: a 256 / 8 handle runs the general-shape path (A/B parity only); 0: the shipped path (a handle of any
    // other shape has only the general path, whatever the value)
    {"general_shape", &cone_model::opt_general, 0, 1, true},
    {"res_gather", &cone_model::opt_res_gather, 0, 1, true},
    {"rows_chain", &cone_model::opt_chain, 0, 1, true},
    {"ffn_spread", &cone_model::opt_spread, 0, 1, true},
    {"gemm_tall_min_rows", &cone_model::opt_gemm_tall_min, -1, GEMM_TALL_MIN_MAX, false},
    // the weight stream of the two ring kernels: 1 = from the handle's packed images, 0 = gathered from the row-major matrices
    {"tail_packed", &cone_model::opt_tail_packed, 0, 1, true},
};
extern "C" int cone_model_set_option(cone_model* m, const char* name, int value) {
    CONE_REQUIRE(m && name, "set_option: null argument");
    for (const OptionRow& o : OPTION_ROWS) {
        if (strcmp(name, o.name)) continue;
        CONE_REQUIRE(o.is_switch || (value >= o.lo && value <= o.hi), "set_option: %s %d not in [%d, %d]", name, value, o.lo, o.hi);
        m->*o.field = o.is_switch ? value != 0 : value;
        return 0;
    }
    // the longest window of this handle; above CONE_MAX_WINDOW_TOKENS the handle is a general-path handle (exact fp32 only)
    if (!strcmp(name, "max_window_tokens")) {
        CONE_REQUIRE(value >= CONE_MAX_WINDOW_TOKENS && value <= CONE_MAX_LONG_WINDOW_TOKENS,
                     "set_option: max_window_tokens %d not in [%d, %d]", value, CONE_MAX_WINDOW_TOKENS, CONE_MAX_LONG_WINDOW_TOKENS);
        CONE_REQUIRE(value == CONE_MAX_WINDOW_TOKENS || !(m->opt_bf16 || m->opt_split_bf16),
                     "set_option: max_window_tokens %d while bf16 / split_bf16 = 1: windows beyond %d tokens run in exact fp32 "
                     "only (set the mode to 0 first)", value, CONE_MAX_WINDOW_TOKENS);
        m->opt_max_tokens = value;
        return 0;
    }
    // the two bf16 modes need their weight images and exclude each other
    const bool split = !strcmp(name, "split_bf16");
    if (split || !strcmp(name, "bf16")) {
        const char* other = split ? "bf16" : "split_bf16";
        CONE_REQUIRE(value == 0 || !m->long_windows(),
                     "set_option: %s on a handle with max_window_tokens = %d: windows beyond %d tokens run the general path, "
                     "exact fp32 only", name, m->opt_max_tokens, CONE_MAX_WINDOW_TOKENS);
        CONE_REQUIRE(value == 0 || (split ? m->split_img : m->bf16_img),
                     "set_option: %s needs hidden_dim 256 with 8 heads and dim_feedforward %% 32 == 0 "
                     "(<= 2048); this handle is hidden_dim %d with %d heads, dim_feedforward %d", name, m->d, m->heads, m->ff);
        CONE_REQUIRE(value == 0 || !(split ? m->opt_bf16 : m->opt_split_bf16),
                     "set_option: %s = 1 while %s = 1: the two modes exclude each other (set %s = 0 first)", name, other, other);
        (split ? m->opt_split_bf16 : m->opt_bf16) = value != 0;
        return 0;
    }
    // the general path's bf16 GEMMs: a switch of its own (bf16 keeps its meaning and its refusals); needs a handle that runs
    // the general path at this moment; the weight images are built at the first 1
    if (!strcmp(name, "general_bf16")) {
        if (value == 0) { m->opt_general_bf16 = 0; return 0; }
        CONE_REQUIRE(m->general(),
                     "set_option: general_bf16 applies to the general path only; this handle runs the fused path: use bf16 "
                     "(or general_shape = 1 / max_window_tokens first)");
        CONE_REQUIRE(m->ff % 32 == 0 && m->ff <= 2048,
                     "set_option: general_bf16 needs dim_feedforward %% 32 == 0 and <= 2048; this handle has dim_feedforward %d", m->ff);
        if (!m->gen_bf16_img)
            if (int rc = build_general_bf16_images(m)) return rc;
        m->opt_general_bf16 = 1;
        return 0;
    }
    // the tall GEMM's packed stream: its images are built at the first 1 (a handle of another shape than 256 / 8 has none: inert)
    if (!strcmp(name, "gemm_tall_packed")) {
        if (value != 0 && !m->gen_native)
            if (int rc = build_tall_images(m)) return rc;
        m->opt_gemm_tall_packed = value != 0;
        return 0;
    }
    if (!strcmp(name, "gemm")) {
        CONE_REQUIRE(value >= GEMM_AUTO && value <= GEMM_TALL, "set_option: gemm tile family %d not in [0, 4]", value);
        m->opt_gemm = value;
        // the first decoder layer's constants come from these GEMMs: keep them what a step would compute
        if (dec0_constants(m, nullptr) != 0 || hipDeviceSynchronize() != hipSuccess) return CONE_E_HIP;
        return 0;
    }
    cone::set_error("set_option: unknown option '%s'", name);
    return CONE_E_INVALID;
}

// what a sequencing entry outside this file (session.hip) has to know of the opaque handle to size its buffers
extern "C" int cone_model_get_dims(const cone_model* m, cone_model_dims* out) {
    CONE_REQUIRE(m && out, "model_get_dims: null argument");
    out->hidden_dim = m->d; out->num_queries = m->nq; out->enc_layers = m->n_enc;
    out->t_dim = m->dt; out->v_dim = m->dv; out->v_motion_dim = m->dvm;
    out->txt_pos = m->txt_pos_emb != nullptr;
    out->long_windows = m->long_windows();
    return 0;
}

extern "C" int cone_test_gemm(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                              const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                              const float* ADD, int M, int N, int K, int flags, void* stream) {
    GemmArgs g = G(nullptr, A, K, W, K, bias, C, N, M, nullptr, N, K, flags & 0xff);
    g.variant = (flags >> 8) & 3;          // test hook: bits 8-9 pick the tile family (0 automatic)
    g.A2 = A2; g.lda2 = K; g.a2_mod = a2_mod; g.R = R; g.ldr = N; g.ln_g = ln_g; g.ln_b = ln_b;
    g.C2 = C2; g.ADD = ADD;
    return launch_gemm(g, (hipStream_t)stream);
}
// cone_test_gemm's arguments (bits 8-10 of flags: the tile family, 4 = the tall form; bit 11: an automatic launch never takes the
// tall form), then lda / ldc (0: K / N), M_dev and n_cu: n_cu > 0 runs the tall form itself on a persistent grid sized for that
// many CUs, n_cu == 0 goes through the dispatcher
extern "C" int cone_test_gemm_tall(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                                   const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                                   const float* ADD, int M, int N, int K, int flags, int lda, int ldc, const int32_t* M_dev,
                                   int n_cu, void* stream) {
    GemmArgs g = G(nullptr, A, lda ? lda : K, W, K, bias, C, ldc ? ldc : N, M, M_dev, N, K, flags & 0xff);
    g.variant = ((flags >> 8) & 7) | (((flags >> 11) & 1) << GEMM_TALL_MIN_SHIFT);
    g.A2 = A2; g.lda2 = K; g.a2_mod = a2_mod; g.R = R; g.ldr = ldc ? ldc : N; g.ln_g = ln_g; g.ln_b = ln_b;
    g.C2 = C2; g.ADD = ADD;
    CONE_REQUIRE(n_cu >= 0, "gemm tall hook: negative CU count");
    return n_cu > 0 ? launch_gemm_tall(g, n_cu, (hipStream_t)stream) : launch_gemm(g, (hipStream_t)stream);
}
// The packed fp32 weight streams (tail_pack.hip) and the two ring kernels on them.
extern "C" size_t cone_test_f32_pack_tail_bytes(int ff, int proj, int n_qkv) { return f32_pack_tail_bytes(ff, proj != 0, n_qkv); }
extern "C" int cone_test_f32_pack_tail(const float* Wo, const float* W1, const float* W2, int ff, const float* Wq, int n_qkv,
                                       void* img, void* stream) {
    return launch_f32_pack_tail(Wo, W1, W2, ff, Wq, n_qkv, img, (hipStream_t)stream);
}
extern "C" long cone_test_f32_packed_launches(int which) { return f32_packed_launches(which); }
extern "C" size_t cone_test_f32_pack_rows_bytes(int N) { return f32_pack_rows_bytes(N); }
extern "C" int cone_test_f32_pack_rows(const float* W, int N, void* img, void* stream) {
    return launch_f32_pack_rows(W, N, img, (hipStream_t)stream);
}
// cone_test_gemm_tall on contiguous operands with W's packed image (null: the row-major stream): always the tall form itself
extern "C" int cone_test_gemm_tall_packed(const float* A, const float* W, const float* bias, const float* R, float* C, int M,
                                          int N, int flags, const int32_t* M_dev, int n_cu, const void* img, void* stream) {
    GemmArgs g = G(nullptr, A, 256, W, 256, bias, C, N, M, M_dev, N, 256, flags & (EPI_RELU | EPI_RESIDUAL));
    g.variant = GEMM_TALL; g.R = R; g.ldr = N; g.Wimg = img;
    CONE_REQUIRE(n_cu >= 0, "gemm tall hook: negative CU count");
    return launch_gemm_tall(g, n_cu, (hipStream_t)stream);
}
extern "C" size_t cone_test_gemm_bf16_image_bytes(int N, int K) { return gemm_bf16_image_bytes(N, K); }
// cone_test_gemm's arguments, then: img (cone_test_gemm_bf16_image_bytes(N, K) bytes: W is packed into it first), ldc (0: N),
// r_mod, M_dev
extern "C" int cone_test_gemm_bf16(const float* A, const float* A2, int a2_mod, const float* W, const float* bias,
                                   const float* R, const float* ln_g, const float* ln_b, float* C, float* C2,
                                   const float* ADD, int M, int N, int K, int flags, void* img, int ldc, int r_mod,
                                   const int32_t* M_dev, void* stream) {
    GemmArgs g = G(nullptr, A, K, W, K, bias, C, ldc ? ldc : N, M, M_dev, N, K, flags & 0xff);
    g.A2 = A2; g.lda2 = K; g.a2_mod = a2_mod; g.R = R; g.ldr = N; g.r_mod = r_mod; g.ln_g = ln_g; g.ln_b = ln_b;
    g.C2 = C2; g.ADD = ADD;
    if (int rc = launch_gemm_bf16_pack(W, K, N, K, img, (hipStream_t)stream)) return rc;
    return launch_gemm_bf16(g, img, (hipStream_t)stream);
}
extern "C" int cone_test_ffn(const float* X, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* stream) {
    return launch_ffn_fused(X, 256, W1, b1, W2, b2, ln_g, ln_b, OUT, 256, M, nullptr, ff, (hipStream_t)stream);
}
// the tail of the cone_test_* entries: raw operand pointers, 256-float rows, no device-side count
static TailArgs test_tail(TailWeights* w, const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                          const float* pb, const float* W1, const float* b1, const float* W2, const float* b2, const float* ln_g,
                          const float* ln_b, float* OUT, int M, int ff) {
    *w = TailWeights{};
    w->Wo = Wo; w->bo = bo; w->W1 = W1; w->b1 = b1; w->W2 = W2; w->b2 = b2; w->in_g = pg; w->in_b = pb; w->out_g = ln_g; w->out_b = ln_b;
    return tail_args(w, A, R, OUT, M, nullptr, ff);
}
extern "C" int cone_test_proj_ffn(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                  const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                                  const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* stream) {
    TailWeights w;
    return launch_proj_ffn_fused(test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff), (hipStream_t)stream);
}
extern "C" size_t cone_test_proj_ffn_spread_scratch_bytes(int ff) { return ffn_spread_scratch_floats(ff) * sizeof(float); }
extern "C" int cone_test_proj_ffn_spread(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                         const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                                         const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* scratch,
                                         void* stream) {
    TailWeights w;
    TailArgs t = test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff);
    t.scratch = (float*)scratch;
    return launch_proj_ffn_spread(t, (hipStream_t)stream);
}
extern "C" int cone_test_tail_form(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                   const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                                   const float* ln_g, const float* ln_b, float* OUT, int M, int ff, const int32_t* r_idx,
                                   const float* R2, const int32_t* M_dev, int pre, float* OUT2, int form, int n_cu, void* scratch,
                                   void* stream) {
    TailWeights w;
    TailArgs t = test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff);
    t.r_idx = r_idx; t.R2 = R2; t.M_dev = M_dev; t.pre = pre != 0; t.OUT2 = OUT2; t.ldo2 = 256; t.scratch = (float*)scratch;
    return launch_tail_f32_form(t, form, n_cu, (hipStream_t)stream);
}
// The row kernel of the exact-fp32 tail on the packed stream img (null: the row-major one); A == null: the block alone on R;
// Wq != null: with the q | k | v ride (qb, QKV (M, n_qkv)); pre: the pre-norm form (OUT2 may be null); nw: 8 | 4 waves; n_cu > 0:
// a persistent grid sized for that many CUs
extern "C" int cone_test_tail_packed(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                     const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                                     const float* ln_g, const float* ln_b, float* OUT, int M, int ff, int pre, float* OUT2,
                                     const float* Wq, const float* qb, float* QKV, int n_qkv, int nw, int n_cu, const void* img,
                                     void* stream) {
    TailWeights w, nx{};
    TailArgs t = test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff);
    t.pre = pre != 0; t.OUT2 = OUT2; t.ldo2 = 256;
    if (Wq) { nx.Wq = Wq; nx.qb = qb; t.next = &nx; t.QKV = QKV; t.ldq = n_qkv; t.n_qkv = n_qkv; }
    return launch_tail_f32_rows_hook(t, img, nw, n_cu, (hipStream_t)stream);
}
// pack: CONE_TEST_SINGLE_PIECE selects the single-piece form (ffn_bf16.hip), which packs only with CONE_TEST_PACK; the split
// form packs with any non-zero value
static int test_tail_mode(int pack, bool* do_pack) {
    const bool single = pack & CONE_TEST_SINGLE_PIECE;
    *do_pack = single ? pack & CONE_TEST_PACK : pack;
    return single ? TAIL_IMG_BF16 : TAIL_IMG_SPLIT;
}
extern "C" size_t cone_test_ffn_split_image_bytes(int ff) {
    const TailMode& k = *TAIL_MODES[TAIL_IMG_SPLIT];
    return k.ffn_supported(ff) ? k.ffn_image_bytes(ff) : 0;
}
extern "C" int cone_test_ffn_split(const float* X, const float* W1, const float* b1, const float* W2, const float* b2,
                                   const float* ln_g, const float* ln_b, float* OUT, int M, int ff, void* img, int pack,
                                   void* stream) {
    bool do_pack;
    const TailMode& k = *TAIL_MODES[test_tail_mode(pack, &do_pack)];
    if (do_pack) {
        const int rc = k.pack(W1, W2, ff, img, (hipStream_t)stream);
        if (rc) return rc;
    }
    return k.ffn(X, 256, img, b1, b2, ln_g, ln_b, OUT, 256, M, nullptr, ff, (hipStream_t)stream, 0);
}
extern "C" size_t cone_test_rows_split_image_bytes(int N) {
    const TailMode& k = *TAIL_MODES[TAIL_IMG_SPLIT];
    return k.rows_supported(N) ? k.rows_image_bytes(N) : 0;
}
extern "C" int cone_test_rows_split(const float* X, const float* W, const float* bias, float* C, int M, int N, void* img,
                                    int pack, void* stream) {
    bool do_pack;
    const TailMode& k = *TAIL_MODES[test_tail_mode(pack, &do_pack)];
    if (do_pack) {
        const int rc = k.pack(W, nullptr, N, img, (hipStream_t)stream);
        if (rc) return rc;
    }
    return k.rows256(X, 256, img, bias, C, N, M, nullptr, N, (hipStream_t)stream, 0);
}
extern "C" size_t cone_test_proj_split_image_bytes(void) { return TAIL_MODES[TAIL_IMG_SPLIT]->proj_image_bytes(); }
extern "C" int cone_test_proj_ffn_split(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                        const float* pb, const float* W1, const float* b1, const float* W2,
                                        const float* b2, const float* ln_g, const float* ln_b, float* OUT, int M, int ff,
                                        void* img, void* wo_img, int pack, void* stream) {
    bool do_pack;
    const int mode = test_tail_mode(pack, &do_pack);
    const TailMode& k = *TAIL_MODES[mode];
    if (do_pack) {
        int rc = k.pack(W1, W2, ff, img, (hipStream_t)stream);
        if (rc) return rc;
        rc = k.pack(Wo, nullptr, 256, wo_img, (hipStream_t)stream);
        if (rc) return rc;
    }
    TailWeights w;
    const TailArgs t = test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff);
    w.img[mode] = TailImages{wo_img, img, nullptr};
    return k.proj_ffn(t, (hipStream_t)stream);
}
// The matrix-core tails in every form their launchers have, as cone_test_tail_packed is for the exact-fp32 one: A == null: the
// block alone on R as its input (no gather, ride or pre-norm form); Wq != null: the q | k | v ride; pre: the pre-norm form (the
// single-piece mode only; OUT2 may be null); r_idx / R2: the gathered residual; M_dev; row strides (0 = dense); n_cu > 0: a
// persistent grid sized for that many CUs.  The images are packed first where `pack` says so (test_tail_mode).
extern "C" int cone_test_tail_mc(const float* A, const float* Wo, const float* bo, const float* R, const float* pg,
                                 const float* pb, const float* W1, const float* b1, const float* W2, const float* b2,
                                 const float* ln_g, const float* ln_b, float* OUT, int M, int ff, const int32_t* r_idx,
                                 const float* R2, const int32_t* M_dev, int pre, float* OUT2, const float* Wq, const float* qb,
                                 float* QKV, int n_qkv, int lda, int ldr, int ldo, int ldo2, int ldq, int n_cu, void* img,
                                 void* wo_img, void* q_img, int pack, void* stream) {
    bool do_pack;
    const int mode = test_tail_mode(pack, &do_pack);
    const TailMode& k = *TAIL_MODES[mode];
    hipStream_t s = (hipStream_t)stream;
    CONE_REQUIRE(!pre || k.proj_ffn_prenorm, "tail hook: the three-piece split tail has no pre-norm form");
    CONE_REQUIRE(!pre || !Wq, "tail hook: the pre-norm form has no q|k|v ride");
    CONE_REQUIRE(A || (!pre && !Wq && !r_idx), "tail hook: the block alone has no pre-norm, ride or gather form");
    CONE_REQUIRE(!Wq || q_img, "tail hook: the ride needs its image buffer");
    if (do_pack) {
        if (int rc = k.pack(W1, W2, ff, img, s)) return rc;
        if (A)
            if (int rc = k.pack(Wo, nullptr, 256, wo_img, s)) return rc;
        if (Wq)
            if (int rc = k.pack(Wq, nullptr, n_qkv, q_img, s)) return rc;
    }
    if (!A) return k.ffn(R, ldr ? ldr : 256, img, b1, b2, ln_g, ln_b, OUT, ldo ? ldo : 256, M, M_dev, ff, s, n_cu);
    TailWeights w, nx{};
    TailArgs t = test_tail(&w, A, Wo, bo, R, pg, pb, W1, b1, W2, b2, ln_g, ln_b, OUT, M, ff);
    w.img[mode] = TailImages{wo_img, img, nullptr};
    if (lda) t.lda = lda;
    if (ldr) t.ldr = ldr;
    if (ldo) t.ldo = ldo;
    t.r_idx = r_idx; t.R2 = R2; t.M_dev = M_dev; t.pre = pre != 0; t.OUT2 = OUT2; t.ldo2 = ldo2 ? ldo2 : 256; t.n_cu = n_cu;
    if (Wq) {
        nx.Wq = Wq; nx.qb = qb; nx.img[mode] = TailImages{nullptr, nullptr, q_img};
        t.next = &nx; t.QKV = QKV; t.n_qkv = n_qkv; t.ldq = ldq ? ldq : n_qkv;
    }
    return pre ? k.proj_ffn_prenorm(t, s) : k.proj_ffn(t, s);
}
// cone_test_rows_split with row strides (0 = dense), a device-side row count and a CU count for the persistent grid
extern "C" int cone_test_rows_mc(const float* X, const float* W, const float* bias, float* C, int M, int N, void* img, int pack,
                                 int ldx, int ldc, const int32_t* M_dev, int n_cu, void* stream) {
    bool do_pack;
    const TailMode& k = *TAIL_MODES[test_tail_mode(pack, &do_pack)];
    if (do_pack) {
        const int rc = k.pack(W, nullptr, N, img, (hipStream_t)stream);
        if (rc) return rc;
    }
    return k.rows256(X, ldx ? ldx : 256, img, bias, C, ldc ? ldc : N, M, M_dev, N, (hipStream_t)stream, n_cu);
}
extern "C" int cone_test_enc_attn(int mode, const float* QKV, const float* qkv_vid, const float* qkv_txt,
                                  const float* pos_qk, const int32_t* vrow0, const int32_t* vlen, const int32_t* trow0,
                                  const int32_t* off, float* OUT, int B, int Lmax, int pos_zero_row, void* stream) {
    AttnSrc a{};
    a.pos_zero_row = pos_zero_row;
    a.Q = QKV; a.K = QKV ? QKV + 256 : nullptr; a.V = QKV ? QKV + 512 : nullptr; a.ldq = a.ldk = a.ldv = 768;
    a.qkv_vid = qkv_vid; a.qkv_txt = qkv_txt; a.pos_qk = pos_qk; a.vrow0 = vrow0; a.vlen = vlen; a.trow0 = trow0;
    a.form = (mode >> 8) & 3;                     // mode | 0x200: the wave-per-(window, head) form (enc_attn_wave_kernel)
    return launch_enc_attn(mode & 0xff, a, OUT, off, B, Lmax, (hipStream_t)stream);
}
extern "C" int cone_test_dec_cross(const float* DQ, const float* X, const float* pos_rows, const int32_t* vlen,
                                   const int32_t* off, const float* Wk, const float* WvT, const float* bv, float* OUT,
                                   int B, int nq, int Lmax, int variant, float* qk_slabs, void* stream) {
    if (variant == 1)
        return launch_dec_cross(DQ, nullptr, X, pos_rows, vlen, off, Wk, WvT, bv, OUT, B, nq, Lmax, (hipStream_t)stream);
    return launch_dec_cross_mfma(DQ, nullptr, X, pos_rows, vlen, off, Wk, WvT, bv, OUT, B, nq, Lmax, qk_slabs,
                                 (hipStream_t)stream, variant);
}
extern "C" size_t cone_test_dec_cross_slab_floats(void) { return dec_cross_mfma_slab_floats(); }
extern "C" int cone_test_enc_attn_txt(int mode, const float* QKV, const float* qkv_vid, const float* qkv_txt,
                                      const float* pos_qk, const float* txt_pos_qk, const int32_t* vrow0,
                                      const int32_t* vlen, const int32_t* trow0, const int32_t* off, float* OUT, int B,
                                      int Lmax, int pos_zero_row, void* stream) {
    AttnSrc a{};
    a.pos_zero_row = pos_zero_row;
    a.Q = QKV; a.K = QKV ? QKV + 256 : nullptr; a.V = QKV ? QKV + 512 : nullptr; a.ldq = a.ldk = a.ldv = 768;
    a.qkv_vid = qkv_vid; a.qkv_txt = qkv_txt; a.pos_qk = pos_qk; a.vrow0 = vrow0; a.vlen = vlen; a.trow0 = trow0;
    a.txt_pos_qk = txt_pos_qk;                    // non-NULL: the ATTN_GATHER | 4 / ATTN_POSADD | 4 builds
    a.form = (mode >> 8) & 3;
    return launch_enc_attn(mode & 0xff, a, OUT, off, B, Lmax, (hipStream_t)stream);
}
extern "C" int cone_test_small_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* OUT,
                                    int ldo, const int32_t* off, int B, int nq, int Lmax, void* stream) {
    return launch_small_attn(Q, ldq, K, ldk, V, ldv, OUT, ldo, off, B, nq, Lmax, (hipStream_t)stream);
}
extern "C" int cone_test_dec_cross_ex(const float* DQ, const float* XP, const float* X, const float* pos_rows,
                                      const int32_t* vlen, const int32_t* off, const float* Wk, const float* WvT,
                                      const float* bv, float* OUT, int B, int nq, int Lmax, int variant, float* qk_slabs,
                                      const float* sal_w, const float* sal_b, float* sal, int sal_ld, void* stream) {
    if (variant == 1) {
        CONE_REQUIRE(!sal, "fused decoder cross-attention: the VALU kernel has no saliency ride");
        return launch_dec_cross(DQ, XP, X, pos_rows, vlen, off, Wk, WvT, bv, OUT, B, nq, Lmax, (hipStream_t)stream);
    }
    return launch_dec_cross_mfma(DQ, XP, X, pos_rows, vlen, off, Wk, WvT, bv, OUT, B, nq, Lmax, qk_slabs, (hipStream_t)stream,
                                 variant, sal_w, sal_b, sal, sal_ld);
}
extern "C" int cone_test_layernorm(const float* x, const float* g, const float* b, float* out, int64_t n_rows,
                                   int dim, void* stream) {
    return launch_layernorm(x, dim, g, b, out, dim, n_rows, nullptr, dim, (hipStream_t)stream);
}
extern "C" int cone_test_gen_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* OUT, int ldo,
                                  const int32_t* qoff, const int32_t* koff, int B, int nq, int heads, int head_dim, int kcap,
                                  void* stream) {
    return launch_gen_attn(Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, B, nq, heads, head_dim, kcap, (hipStream_t)stream);
}

// The glue kernels of stage B, one entry per launcher, raw operand pointers (tests/test_glue_kernels_gpu.py).  Each entry is
// the launcher the forward path calls and nothing else: no arithmetic, no checks of its own.
extern "C" int cone_test_grid_limit_y(void) { return grid_limit_y(); }
extern "C" int cone_test_scan_lengths(const int32_t* vlen, const int32_t* qlen, int B, int32_t* off, void* stream) {
    return launch_scan_lengths(vlen, qlen, B, off, (hipStream_t)stream);
}
extern "C" int cone_test_compact_index(const int32_t* vlen, const int32_t* voff, int Lv_pad, int32_t* vidx, const int32_t* qlen,
                                       const int32_t* toff, int Lq_pad, int32_t* tidx, int B, void* stream) {
    return launch_compact_index(vlen, voff, Lv_pad, vidx, qlen, toff, Lq_pad, tidx, B, (hipStream_t)stream);
}
extern "C" int cone_test_pack_pos(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj,
                                  const int32_t* trow0, const int32_t* qlen, const int32_t* off, const float* dim_t, float* X,
                                  float* POS, float* XP, int B, int Lmax, const float* tpe, const float* tpg, const float* tpb,
                                  void* stream) {
    return launch_pack_pos(vproj, vrow0, vlen, tproj, trow0, qlen, off, dim_t, X, POS, XP, B, Lmax, (hipStream_t)stream, tpe, tpg,
                           tpb);
}
extern "C" int cone_test_gen_pack_pos(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj,
                                      const int32_t* trow0, const int32_t* qlen, const int32_t* off, const float* dim_t, float* X,
                                      float* POS, int d, int B, int Lmax, const float* tpe, const float* tpg, const float* tpb,
                                      void* stream) {
    return launch_gen_pack_pos(vproj, vrow0, vlen, tproj, trow0, qlen, off, dim_t, X, POS, d, B, Lmax, (hipStream_t)stream, tpe,
                               tpg, tpb);
}
extern "C" int cone_test_pack_l0(const float* vproj, const int32_t* vrow0, const int32_t* vlen, const float* tproj,
                                 const int32_t* trow0, const int32_t* qlen, const int32_t* off, const float* dim_t,
                                 const float* qkv_vid, const float* qkv_txt, const float* pos_qk, float* X, float* POS, float* QK,
                                 float* V, int B, int Lmax, void* stream) {
    return launch_pack_l0(vproj, vrow0, vlen, tproj, trow0, qlen, off, dim_t, qkv_vid, qkv_txt, pos_qk, X, POS, QK, V, B, Lmax,
                          (hipStream_t)stream);
}
extern "C" int cone_test_row_index(const int32_t* vrow0, const int32_t* vlen, const int32_t* trow0, const int32_t* qlen,
                                   const int32_t* off, int32_t* ridx, int B, int Lmax, void* stream) {
    return launch_row_index(vrow0, vlen, trow0, qlen, off, ridx, B, Lmax, (hipStream_t)stream);
}
extern "C" int cone_test_add_pos_rows(const float* MEM, const int32_t* off, const int32_t* vlen, const float* pos_rows, float* XP,
                                      int B, int Lmax, const float* txt_pos, const int32_t* trow0, void* stream) {
    return launch_add_pos_rows(MEM, off, vlen, pos_rows, XP, B, Lmax, (hipStream_t)stream, txt_pos, trow0);
}
extern "C" int cone_test_txt_pos_rows(const float* tproj, const int32_t* tok_index, const int32_t* src_row, int mod, int n_emb,
                                      const float* tpe, const float* tpg, const float* tpb, int n, const int32_t* n_dev,
                                      float* out, void* stream) {
    return launch_txt_pos_rows(tproj, tok_index, src_row, mod, n_emb, tpe, tpg, tpb, n, n_dev, out, (hipStream_t)stream);
}
extern "C" int cone_test_gen_txt_pos_rows(const float* tproj, const int32_t* tok_index, const int32_t* src_row, int mod, int n_emb,
                                          const float* tpe, const float* tpg, const float* tpb, int n, const int32_t* n_dev, int d,
                                          float* out, void* stream) {
    return launch_gen_txt_pos_rows(tproj, tok_index, src_row, mod, n_emb, tpe, tpg, tpb, n, n_dev, d, out, (hipStream_t)stream);
}
extern "C" int cone_test_saliency(const float* MEM, const int32_t* off, const int32_t* vlen, const int32_t* qlen, const float* w,
                                  const float* bias, float* sal, int Lv_out, float* mem_tap, int Lq_out, int B, void* stream) {
    return launch_saliency(MEM, off, vlen, qlen, w, bias, sal, Lv_out, mem_tap, Lq_out, B, (hipStream_t)stream);
}
extern "C" int cone_test_gen_saliency(const float* MEM, const int32_t* off, const int32_t* vlen, const int32_t* qlen,
                                      const float* w, const float* bias, float* sal, int Lv_out, float* mem_tap, int Lq_out, int B,
                                      int d, void* stream) {
    return launch_gen_saliency(MEM, off, vlen, qlen, w, bias, sal, Lv_out, mem_tap, Lq_out, B, d, (hipStream_t)stream);
}
extern "C" int cone_test_rowdot(const float* X, int ldx, const float* W, const float* b, float* out, int ldo, int64_t n_rows,
                                int nout, int act, void* stream) {
    return launch_rowdot(X, ldx, W, b, out, ldo, n_rows, nout, act, (hipStream_t)stream);
}
extern "C" int cone_test_gen_rowdot(const float* X, int ldx, const float* W, const float* b, float* out, int ldo, int64_t n_rows,
                                    int nout, int act, int d, void* stream) {
    return launch_gen_rowdot(X, ldx, W, b, out, ldo, n_rows, nout, act, d, (hipStream_t)stream);
}
extern "C" int cone_test_tile_rows(float* x, int period, int64_t n_rows, void* stream) {
    return launch_tile_rows(x, period, n_rows, (hipStream_t)stream);
}
extern "C" int cone_test_tile_rows2(float* d0, const float* s0, float* d1, const float* s1, int period, int64_t n_rows,
                                    void* stream) {
    return launch_tile_rows2(d0, s0, d1, s1, period, n_rows, (hipStream_t)stream);
}
