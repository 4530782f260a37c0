// What the exact-fp32 layer-tail files share: ffn.hip (the persistent 128-row / 64-row kernel) and ffn_wide.hip (the wide
// kernel and the four spread kernels).  Every form must produce the same bits for a row, so everything outside the MFMA
// schedules is the same text, and it is here, once: the operand-slab primitives (LDS-DMA, chunk swizzle), the register
// LayerNorm and its apply, the residual row with its gather, the clamped load row, the launch's row count, ONE
// kernel-argument layout with the host function that fills it from a TailArgs, the argument checks, and what ffn.hip calls in
// ffn_wide.hip.  Each .hip keeps its ring, its MFMA schedule and its launchers (see their headers, and DESIGN.md 3).
//
// The steps inside a kernel body are macros over the names every kernel declares (lg; t is the macro's own tile index):
// tail_bf16_common.h records why -- as __forceinline__ functions such steps moved hipcc's scheduling -- and the device code
// is meant to stay what it was.  tf_swz16 / tf_layernorm_regs were functions before and still are.
#pragma once

#include "common.h"

namespace cone {

// ---- operand slabs: [16 rows][16 floats], unpadded 64-B rows, fetched by LDS-DMA (16 B per lane), the 16-B chunk
// XOR-swizzled on the source address and on the ds_read_b128 address (conflict-free for lane = (row, chunk))
#define TF_GLDS16(src, dst) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

__device__ __forceinline__ int tf_swz16(int row) { return (0x1230 >> (((row >> 2) & 3) * 4)) & 3; }

// ---- LayerNorm over a token's 256 channels held as v[16] (channel 16 t + 4 lg + r in v[t][r]): 4 lanes x 64 registers.
// Leaves v centred (v - mean) and returns rstd: the forms' bit-identity rests on every one of them taking these moments.
__device__ __forceinline__ void tf_layernorm_regs(f32x4 (&v)[16], float& rstd) {
    float s1 = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) s1 += (v[t][0] + v[t][1]) + (v[t][2] + v[t][3]);
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    const float mean = s1 * (1.0f / 256.0f);
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[t][r] -= mean; s2 = fmaf(v[t][r], v[t][r], s2); }
    }
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    rstd = 1.0f / sqrtf(s2 * (1.0f / 256.0f) + 1e-5f);
}
// The apply: o = v[t] * rstd * gamma + beta for the lane's four channels of tile t.  gp / bp = the per-channel vectors (256
// floats each) wherever the kernel keeps them: LDS in ffn.hip, global memory in the wide and spread kernels.
#define TF_LN_TILE(o, v, rstd, gp, bp, t)                                                       \
    {                                                                                           \
        const f32x4 g_ = *reinterpret_cast<const f32x4*>((gp) + 16 * (t) + 4 * lg);             \
        const f32x4 b_ = *reinterpret_cast<const f32x4*>((bp) + 16 * (t) + 4 * lg);             \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) o[r] = v[t][r] * rstd * g_[r] + b_[r];    \
    }
// ... in registers
#define TF_LN_APPLY(v, rstd, gp, bp) \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) TF_LN_TILE(v[t], v, rstd, gp, bp, t)
// ... stored to the row op (= the row + 4 lg), the tiles t for which WHEN holds (an expression in t); KEEP: the result also
// replaces v[t] (the q | k | v ride goes on with it)
#define TF_LN_STORE(op, v, rstd, gp, bp, WHEN, KEEP)             \
    _Pragma("unroll") for (int t = 0; t < 16; ++t) {             \
        if (WHEN) {                                              \
            f32x4 o_;                                            \
            TF_LN_TILE(o_, v, rstd, gp, bp, t)                   \
            *reinterpret_cast<f32x4*>((op) + 16 * t) = o_;       \
            if (KEEP) v[t] = o_;                                 \
        }                                                        \
    }

// ---- rows.  The launch's row count: the host bound, cut to the device-side count of the whole job where there is one (m_off
// = the job's row that is this launch's row 0); the row a lane loads for `row` (rows past M re-read row M - 1: they feed
// unstored outputs); the lane's residual row + off (r_idx != null: gathered, row i = R[r_idx[i]] or R2[~r_idx[i]]).
#define TF_LAUNCH_ROWS(M, p, m_off) \
    int M = (p).M;                  \
    if ((p).M_dev) { const int md_ = *(p).M_dev - (m_off); M = md_ < M ? md_ : M; }
#define TF_LD_ROW(row, M) ((size_t)((row) < (M) ? (row) : (M) - 1))
#define TF_RES_ROW(rp, p, ld_row, off)                                                                               \
    const float* rp = (p).R + (ld_row) * (p).ldr + (off);                                                            \
    if ((p).r_idx) {                                                                                                 \
        const int ix_ = (p).r_idx[ld_row];                                                                           \
        rp = (ix_ >= 0 ? (p).R + (size_t)ix_ * (p).ldr : (p).R2 + (size_t)(~ix_) * (p).ldr) + (off);                 \
    }

// ---- kernel arguments.  One layout; the two type names only keep the kernels' symbols (ffn_fused_kernel<...>(FfnArgs),
// ffn_wide_kernel<...>(FfnWideArgs), fs_*_kernel(FfnWideArgs, ...)).
struct TailF32Args {
    const float* X; int ldx;                      // (M, 256) block input = residual of the feed-forward block
    const float* W1; const float* b1;             // (ff, 256), (ff)
    const float* W2; const float* b2;             // (256, ff), (256)
    const float* ln_g; const float* ln_b;         // (256)
    float* OUT; int ldo;                          // (M, 256)
    int M; const int* M_dev;                      // rows; *M_dev wins when non-null (grid sized by M)
    int ff;
    // PROJ: the block input is itself  LayerNorm(R + A Wo^T + bo)  (attention output projection + residual + norm,
    // cone/transformer.py:239-241, 308-312), computed here instead of being read: A (M, 256) attention output,
    // R (M, 256) residual; X is unused.
    const float* A; int lda; const float* R; int ldr;
    const float* Wo; const float* bo; const float* pg; const float* pb;
    // r_idx != null: the residual rows are gathered: row i = R[r_idx[i]] (r_idx[i] >= 0) or R2[~r_idx[i]]
    const int* r_idx; const float* R2;
    // QKV (ffn.hip only): the NEXT layer's q | k | v projection of the rows this kernel produces (Wq (n_qkv, 256), qb), computed
    // from the registers that hold them and written to QKV (M, n_qkv): no second pass over the rows, no extra launch
    const float* Wq; const float* qb; float* QKV; int ldq; int n_qkv;
    // PRE (pre-norm layers, cone/transformer.py:248-260 / 319-342; PROJ only): OUT = x1 + W2 relu(W1 LN_p(x1) + b1) + b2 with
    // x1 = R + A Wo^T + bo -- the residual stream stays un-normalised, (pg, pb) is the norm AHEAD of the feed-forward block --
    // and OUT2 (may be null) = LayerNorm(OUT; ln_g, ln_b): what the next consumer reads (the next layer's norm1, the
    // encoder's / decoder's final norm)
    float* OUT2; int ldo2;
    // wide and spread forms: the rows are rows m_off .. m_off + M of a larger job whose device-side count is *M_dev
    int m_off;
    // row kernels of ffn.hip: the packed weight stream (tail_pack.hip), starting at the first chunk the kernel walks; null:
    // the pieces are gathered from the row-major matrices
    const void* Wimg;
};
struct FfnArgs : TailF32Args {};
struct FfnWideArgs : TailF32Args {};

// ---- host side
enum { TF_FORM_ROWS = 0, TF_FORM_WIDE = 1, TF_FORM_SPREAD = 2 };     // which kernels a launch is checked for

bool ffn_fused_supported(int ff);
bool ffn_wide_supported(int ff);
bool ffn_spread_supported(int M, int ff);

// the q | k | v ride: post-norm only, and only the row kernels of ffn.hip run it (a launch with a ride takes no other form)
static inline bool tail_f32_rides(const TailArgs& t) { return !t.pre && t.next && t.next->Wq; }

// The kernel arguments of the projecting tail t: pre-norm (t.pre) without an outer LayerNorm of its own normalises OUT2 with
// the inner one's vectors (never read when OUT2 is null).
static inline TailF32Args tail_f32_args(const TailArgs& t) {
    const TailWeights& w = *t.w;
    TailF32Args a{};
    a.A = t.A; a.lda = t.lda; a.Wo = w.Wo; a.bo = w.bo; a.R = t.R; a.ldr = t.ldr; a.pg = w.in_g; a.pb = w.in_b;
    a.r_idx = t.r_idx; a.R2 = t.R2;
    a.W1 = w.W1; a.b1 = w.b1; a.W2 = w.W2; a.b2 = w.b2;
    a.ln_g = t.pre && !w.out_g ? w.in_g : w.out_g; a.ln_b = t.pre && !w.out_b ? w.in_b : w.out_b;
    a.OUT = t.OUT; a.ldo = t.ldo; a.M = t.M; a.M_dev = t.M_dev; a.ff = t.ff; a.m_off = t.m_off;
    if (t.pre) { a.OUT2 = t.OUT2; a.ldo2 = t.ldo2; }
    if (tail_f32_rides(t)) { a.Wq = t.next->Wq; a.qb = t.next->qb; a.QKV = t.QKV; a.ldq = t.ldq; a.n_qkv = t.n_qkv; }
    // an image with ride chunks serves a launch without a ride (they are never reached); a ride needs its own chunks
    if (t.packed && w.pk && (!a.Wq || w.pk_nq == a.n_qkv)) a.Wimg = w.pk;
    return a;
}

// What every launcher of a projecting tail checks before it fills the kernel's arguments; `what` names the entry in the text.
static inline int tail_f32_check(const TailArgs& t, int form, const char* what) {
    const TailWeights& w = *t.w;
    CONE_REQUIRE(form != TF_FORM_SPREAD || (ffn_spread_supported(t.M, t.ff) && t.scratch), "%s: unsupported size M=%d ff=%d", what,
                 t.M, t.ff);
    CONE_REQUIRE(!t.r_idx || t.R2, "%s: a gathered residual needs both source matrices", what);
    CONE_REQUIRE(form == TF_FORM_SPREAD || (form == TF_FORM_WIDE ? ffn_wide_supported(t.ff) : ffn_fused_supported(t.ff)),
                 "%s: dim_feedforward=%d unsupported", what, t.ff);
    CONE_REQUIRE(t.A && w.Wo && w.bo && t.R && w.in_g && w.in_b && w.W1 && w.b1 && w.W2 && w.b2 && t.OUT &&
                     (t.pre ? !t.OUT2 || (w.out_g && w.out_b) : w.out_g && w.out_b), "%s: null argument", what);
    CONE_REQUIRE(t.lda % 4 == 0 && t.ldr % 4 == 0 && t.ldo % 4 == 0 && (!t.pre || !t.OUT2 || t.ldo2 % 4 == 0),
                 "%s: row strides must be multiples of 4", what);
    CONE_REQUIRE(form != TF_FORM_ROWS || !tail_f32_rides(t) ||
                     (t.next->qb && t.QKV && t.n_qkv >= 32 && t.n_qkv % 32 == 0 && t.ldq % 4 == 0), "%s: bad q|k|v arguments", what);
    return 0;
}

// ---- what ffn.hip calls in ffn_wide.hip: the wide kernel on filled arguments (proj: the projecting tail, else the block on
// a.X; pre: the pre-norm tail), and the spread form's four launches
int launch_tail_f32_wide(const TailF32Args& a, bool proj, bool pre, hipStream_t s);
int launch_tail_f32_spread(const TailF32Args& a, bool pre, float* scratch, hipStream_t s);

}  // namespace cone
