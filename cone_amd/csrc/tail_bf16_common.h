// What the two bf16-matrix-core layer-tail files share: ffn_split.hip (three-piece operands, six products: fp32-accurate)
// and ffn_bf16.hip (single-piece operands, one product).  Both run the same fused tail and the same K = 256 row GEMM in the
// same orientation (a wave owns 16 token rows; lane (li = l % 16, lg = l / 16) holds channels 16 t + 4 lg + r of row li as
// float4 number t), read 1-KiB weight slabs laid out by the same pack kernel, and are launched by the same host code.
// Here, once: the vector types and instruction wrappers, the kernel-argument layout, the named steps of the kernels
// (prologue, parameter staging, row loads, residual gather, register LayerNorm, weight-image address, slot store), the
// pack kernel and every host launcher, written over a per-mode trait.  Each .hip keeps its ring, its operand preparation
// and its product unit (see their headers, and DESIGN.md 3a / 3b).
//
// The kernels' steps are macros over the names every kernel declares (tid, lane, wave, li, lg, M; PROJ, QKV, NP, nc in
// the fused tail): written as __forceinline__ functions they moved hipcc's scheduling and register allocation in every
// one of these kernels (a few instructions each), and the device code is meant to stay what it was.
#pragma once

#include "common.h"

namespace cone {

typedef float tb_f4 __attribute__((ext_vector_type(4)));
typedef float tb_f2 __attribute__((ext_vector_type(2)));
typedef short tb_s8 __attribute__((ext_vector_type(8)));
typedef unsigned tb_u4 __attribute__((ext_vector_type(4)));
typedef __bf16 tb_b2 __attribute__((ext_vector_type(2)));

constexpr int TB_ROWS = 128;                       // token rows per workgroup (8 waves x 16)
constexpr int TB_SLAB = 1024;                      // one operand slab = one wave's ds_read_b128 = one LDS-DMA piece
constexpr int TB_LDS_MAX = 160 * 1024;             // the CU's LDS

#define TB_GLDS16(src, dst) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)
#define TB_SB() __builtin_amdgcn_sched_barrier(0)
#define TB_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0)

// two floats -> packed bf16 pair (round to nearest even: v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned tb_pk(float a, float b) {
    const tb_b2 v = __builtin_convertvector(tb_f2{a, b}, tb_b2);
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float tb_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float tb_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// (a, b) -> the three packed piece pairs: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
__device__ __forceinline__ void tb_split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = tb_pk(a, b);
    const float ra = a - tb_lo(h), rb = b - tb_hi(h);
    m = tb_pk(ra, rb);
    l = tb_pk(ra - tb_lo(m), rb - tb_hi(m));
}

// ---- kernel arguments.  One layout; the two type names per kernel only keep the modes' kernel symbols apart.
struct TailKernArgs {
    const float* X; int ldx;                      // (M, 256) block input = residual
    const void* Wimg;                             // packed weight image: 2 * (ff / 32) slots
    const float* b1; const float* b2;             // (ff), (256)
    const float* ln_g; const float* ln_b;         // (256)
    float* OUT; int ldo;
    int M; const int* M_dev;
    int ff;
    // PROJ: the block input is LayerNorm(R + A Wo^T + bo), computed here (ffn.hip's PROJ form): A (M, 256) attention rows,
    // R residual rows (r_idx != null: gathered, row i = R[r_idx[i]] or R2[~r_idx[i]]), Woimg = Wo's image (8 slots)
    const float* A; int lda; const float* R; int ldr; const int* r_idx; const float* R2;
    const void* Woimg; const float* bo; const float* pg; const float* pb;
    // QKV: the NEXT layer's q | k | v projection of the rows this kernel produces, computed from the registers that hold
    // them: Qimg = its weight image (n_qkv / 32 slots), qb its bias, QKV (M, n_qkv) its output
    const void* Qimg; const float* qb; float* QKV; int ldq; int n_qkv;
};
struct FfnSplitArgs : TailKernArgs {};
struct FfnBf16Args : TailKernArgs {
    // PRE (--pre_norm, with PROJ): x1 = R + A Wo^T + bo stays UNNORMALISED as the residual, the block reads LayerNorm(x1; pg,
    // pb), OUT = x1 + ffn(...) is stored as it is, and OUT2 (if not null) = LayerNorm(OUT; ln_g, ln_b): the next consumer's norm
    float* OUT2; int ldo2;
};
struct RowsKernArgs {
    const float* X; int ldx; const void* Wimg; const float* bias; float* C; int ldc; int M; const int* M_dev; int N;
};
struct RowsSplitArgs : RowsKernArgs {};
struct RowsBf16Args : RowsKernArgs {};

// ---- the parameter rows in LDS, behind the ring and b1 (ff floats): 256 floats each, then the q | k | v bias
enum { PRM_B2 = 0, PRM_LN_G = 256, PRM_LN_B = 512, PRM_BO = 768, PRM_PG = 1024, PRM_PB = 1280, PRM_QB = 1536 };

// the row bound (M, clamped by *M_dev), the workgroup's exit when it has no tile, and the lane decomposition
#define TB_PROLOGUE(p)                                                     \
    int M = (p).M;                                                         \
    if ((p).M_dev) { const int md = *(p).M_dev; M = md < M ? md : M; }     \
    const int n_tiles = (M + TB_ROWS - 1) / TB_ROWS;                       \
    if ((int)blockIdx.x >= n_tiles) return;                                \
    const int tid = threadIdx.x, lane = tid & 63;                          \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);             \
    const int li = lane & 15, lg = lane >> 4

// the tile's row of this lane, and the row it reads for it (rows past M re-read row M - 1)
#define TB_ROW_OF(tile) ((tile) * TB_ROWS + wave * 16 + li)
#define TB_LD_ROW(row) ((size_t)((row) < M ? (row) : M - 1))

// b1 to b1s, the parameter rows to prm and the q | k | v bias behind them (512 threads).  OUT_LN: the output LayerNorm is applied
#define TB_STAGE_ROW(dst, src) reinterpret_cast<tb_f4*>(dst)[tid] = reinterpret_cast<const tb_f4*>(src)[tid]
#define TB_STAGE_PARAMS(p, b1s, prm, ff, OUT_LN)                                                    \
    for (int i = tid; i < ((ff) >> 2); i += 512)                                                    \
        reinterpret_cast<tb_f4*>(b1s)[i] = reinterpret_cast<const tb_f4*>((p).b1)[i];               \
    if (tid < 64) {                                                                                 \
        TB_STAGE_ROW(prm + PRM_B2, (p).b2);                                                         \
        if (OUT_LN) { TB_STAGE_ROW(prm + PRM_LN_G, (p).ln_g); TB_STAGE_ROW(prm + PRM_LN_B, (p).ln_b); } \
        if (PROJ) { TB_STAGE_ROW(prm + PRM_BO, (p).bo); TB_STAGE_ROW(prm + PRM_PG, (p).pg); TB_STAGE_ROW(prm + PRM_PB, (p).pb); } \
    }                                                                                               \
    if (QKV)                                                                                        \
        for (int i = tid; i < ((p).n_qkv >> 2); i += 512)                                           \
            reinterpret_cast<tb_f4*>(prm + PRM_QB)[i] = reinterpret_cast<const tb_f4*>((p).qb)[i]
// the row GEMM's bias (zeros without one)
#define TB_STAGE_BIAS(bs, bias, N)                 \
    for (int i = tid; i < ((N) >> 2); i += 512)    \
        reinterpret_cast<tb_f4*>(bs)[i] = (bias) ? reinterpret_cast<const tb_f4*>(bias)[i] : tb_f4{0.f, 0.f, 0.f, 0.f}

// the lane's 64 values of a row: xp = the row + 4 lg
#define TB_LOAD_ROW(xr, xp)                                                                                        \
    {                                                                                                              \
        const float* xp_ = (xp);                                                                                   \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const tb_f4*>(xp_ + 16 * q);      \
    }
// v += the row's residual (gathered through r_idx where there is one: row r_idx[row] of R, or row ~r_idx[row] of R2) + bo
#define TB_ADD_RESIDUAL(v, p, row, prm)                                                                            \
    {                                                                                                              \
        const float* rp = (p).R + (row) * (p).ldr + 4 * lg;                                                        \
        if ((p).r_idx) {                                                                                           \
            const int ix = (p).r_idx[row];                                                                         \
            rp = (ix >= 0 ? (p).R + (size_t)ix * (p).ldr : (p).R2 + (size_t)(~ix) * (p).ldr) + 4 * lg;             \
        }                                                                                                          \
        _Pragma("unroll") for (int q = 0; q < 16; ++q)                                                             \
            v[q] += *reinterpret_cast<const tb_f4*>(rp + 16 * q) + *reinterpret_cast<const tb_f4*>(prm + PRM_BO + 16 * q + 4 * lg); \
    }

// Register LayerNorm over the 256 channels of a row = v[16] in four lanes (l, l ^ 16, l ^ 32, l ^ 48).  Declares mu and
// rstd; CENTRE: v is left centred (v - mu).  The association order is part of the result's bits.
#define TB_LN_MOMENTS(v, CENTRE, mu, rstd)                                                   \
    float mu, rstd;                                                                          \
    {                                                                                        \
        float s1 = 0.f;                                                                      \
        _Pragma("unroll") for (int t = 0; t < 16; ++t) s1 += (v[t][0] + v[t][1]) + (v[t][2] + v[t][3]); \
        s1 += __shfl_xor(s1, 16, 64);                                                        \
        s1 += __shfl_xor(s1, 32, 64);                                                        \
        mu = s1 * (1.0f / 256.0f);                                                           \
        float s2 = 0.f;                                                                      \
        _Pragma("unroll") for (int t = 0; t < 16; ++t) {                                     \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                  \
                const float cv = v[t][r] - mu;                                               \
                if (CENTRE) v[t][r] = cv;                                                    \
                s2 = fmaf(cv, cv, s2);                                                       \
            }                                                                                \
        }                                                                                    \
        s2 += __shfl_xor(s2, 16, 64);                                                        \
        s2 += __shfl_xor(s2, 32, 64);                                                        \
        rstd = 1.0f / sqrtf(s2 * (1.0f / 256.0f) + 1e-5f);                                   \
    }
// dst = float4 number t of the row, normalised: CV = its centred element r, gamma / beta = the rows at prm + G / prm + B
#define TB_LN_APPLY(dst, CV, rstd, prm, G, B, t)                                                       \
    {                                                                                                  \
        const tb_f4 g4 = *reinterpret_cast<const tb_f4*>(prm + G + 16 * (t) + 4 * lg);                 \
        const tb_f4 b4 = *reinterpret_cast<const tb_f4*>(prm + B + 16 * (t) + 4 * lg);                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) dst[r] = (CV) * rstd * g4[r] + b4[r];            \
    }

// image of slot g of a tile's G = NP + 2 nc + NQ slots: Wo's image, then the W1 | W2 image, then the q | k | v image
#define TB_SLOT_IMAGE(woimg, wimg, qimg, g, SLOT)                                                      \
    (PROJ && (g) < NP ? woimg + (size_t)(g) * SLOT                                                     \
                      : (QKV && (g) >= NP + 2 * nc ? qimg + (size_t)((g) - NP - 2 * nc) * SLOT         \
                                                    : wimg + (size_t)((g) - NP) * SLOT))
// a W1-form slot's 32 output channels of the lane's row, from the accumulators, + bias
#define TB_STORE_SLOT(row, bias, g, a0, a1)                                                                                \
    {                                                                                                                      \
        *reinterpret_cast<tb_f4*>(row + 32 * (g)) = a0 + *reinterpret_cast<const tb_f4*>(bias + 32 * (g) + 4 * lg);        \
        *reinterpret_cast<tb_f4*>(row + 32 * (g) + 16) = a1 + *reinterpret_cast<const tb_f4*>(bias + 32 * (g) + 16 + 4 * lg); \
    }

// ---- weight images (once per model).  One thread per 16-B fragment (8 bf16 of one piece): slot g, slab sl, lane l.
// W2 != null: W1 (ff, 256) and W2 (256, ff) -> 2 * (ff / 32) slots of 16 PIECES slabs (slot 2 c: W1 rows of hidden chunk c,
// slab = (tile * 8 + step) * PIECES + piece; slot 2 c + 1: W2 columns, slab = channel tile * PIECES + piece).  W2 == null:
// W1 is any (N = ff, 256) weight of a 256-channel product: N / 32 slots in the W1 slab order.  PIECES = 3: h, m, l of the
// three-piece split; 1: h alone.
template <int PIECES>
__global__ __launch_bounds__(256) void tail_pack_kernel(const float* __restrict__ W1, const float* __restrict__ W2, int ff,
                                                        unsigned* __restrict__ img) {
    constexpr int SLABS = 16 * PIECES;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)(W2 ? 2 : 1) * (ff / 32) * SLABS * 64;
    if (idx >= total) return;
    const int l = (int)(idx & 63);
    const int sl = (int)((idx >> 6) % SLABS);
    const int g = (int)(idx / (SLABS * 64));
    const int unit = sl / PIECES, piece = sl % PIECES;
    const int c = W2 ? g >> 1 : g, li = l & 15, lg = l >> 4;
    float v[8];
    if (!W2 || (g & 1) == 0) {      // W1 image
        const int t = unit >> 3, s = unit & 7;
        const float* row = W1 + (size_t)(32 * c + 16 * t + li) * 256;
        for (int j = 0; j < 8; ++j) v[j] = row[32 * s + 16 * (j >> 2) + 4 * lg + (j & 3)];
    } else {                        // W2 image
        const float* row = W2 + (size_t)(16 * unit + li) * ff + 32 * c;
        for (int j = 0; j < 8; ++j) v[j] = row[16 * (j >> 2) + 4 * lg + (j & 3)];
    }
    unsigned* dst = img + idx * 4;
    for (int e = 0; e < 4; ++e) {
        unsigned h, m, lo;
        tb_split2(v[2 * e], v[2 * e + 1], h, m, lo);
        dst[e] = piece == 0 ? h : (piece == 1 ? m : lo);
    }
}

// ---- the host side, over a mode trait:
//   FfnArgs, RowsArgs      the kernels' argument types
//   ffn_kernel<PROJ, QKV, PRE>(), rows_kernel()    the kernels
//   IMG                    TAIL_IMG_*;  NAME  the mode's name in error texts;  HAS_PRE  whether the pre-norm form exists
//   SLOT, NSLOT            bytes per ring slot and ring depth;  PIECES  bf16 pieces per weight
// the kernels' LDS: the ring, b1, the six parameter rows and the q | k | v bias
template <class Mode> static size_t tail_lds(int ff, int n_qkv) {
    return (size_t)Mode::NSLOT * Mode::SLOT + (size_t)(ff + PRM_QB + n_qkv) * sizeof(float);
}
static bool tail_ffn_supported(int ff) { return ff >= 64 && ff % 32 == 0 && ff <= 2048; }
template <class Mode> static size_t tail_ffn_image_bytes(int ff) { return (size_t)2 * (ff / 32) * Mode::SLOT; }
template <class Mode> static size_t tail_proj_image_bytes() { return (size_t)8 * Mode::SLOT; }
// does the fused tail + a q | k | v projection of n_qkv outputs fit the CU's LDS (ring + b1 + parameter rows + its bias)?
template <class Mode> static bool tail_qkv_fits(int ff, int n_qkv) {
    return tail_ffn_supported(ff) && n_qkv >= 32 && n_qkv % 32 == 0 && tail_lds<Mode>(ff, n_qkv) <= (size_t)TB_LDS_MAX;
}
static bool tail_rows_supported(int N) { return N >= 32 && N % 32 == 0 && N <= 3072; }
template <class Mode> static size_t tail_rows_image_bytes(int N) { return (size_t)(N / 32) * Mode::SLOT; }

// n_cu, in every launcher below: the CU count that sizes the persistent grid; 0 = the device's, which is what every production
// caller passes; > 0 (the test hooks) makes a workgroup walk several tiles at a few hundred rows
template <class Mode, bool PROJ, bool QKV, bool PRE = false>
static int tail_launch_kernel(const typename Mode::FfnArgs& a, int n_cu, hipStream_t s) {
    CONE_REQUIRE(n_cu >= 0, "%s fused layer tail: negative CU count", Mode::NAME);
    const size_t lds = tail_lds<Mode>(a.ff, QKV ? a.n_qkv : 0);
    CONE_REQUIRE(lds <= (size_t)TB_LDS_MAX, "%s fused layer tail: %zu bytes of LDS (ff %d, q|k|v %d) exceed 160 KiB", Mode::NAME, lds,
                 a.ff, a.n_qkv);
    constexpr auto kernel = Mode::template ffn_kernel<PROJ, QKV, PRE>();
    static DeviceOnce once;
    int dev_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TB_LDS_MAX);
    }, &dev_cu));
    if (!n_cu) n_cu = dev_cu;
    const int tiles = (a.M + TB_ROWS - 1) / TB_ROWS;
    const int grid = tiles < n_cu ? tiles : n_cu;
    // FLOPs of a record = 4 M ff 256 (+ 2 M 256 256 with the projection); the fused q | k | v projection adds
    // 2 M n_qkv 256 = 4 M (n_qkv / 2) 256: it is booked as n_qkv / 2 extra hidden units
    ProfScope ps(PROJ ? PK_FFN_PROJ : PK_FFN_FUSED, a.M, a.ff + (QKV ? a.n_qkv / 2 : 0), 256, a.M_dev, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), lds, s, a);
    CONE_LAUNCH_CHECK();
    return 0;
}

template <class Mode>
static int tail_launch_ffn(const float* X, int ldx, const void* Wimg, const float* b1, const float* b2, const float* ln_g,
                           const float* ln_b, float* OUT, int ldo, int M, const int* M_dev, int ff, hipStream_t s, int n_cu) {
    CONE_REQUIRE(tail_ffn_supported(ff), "%s fused FFN: dim_feedforward=%d unsupported", Mode::NAME, ff);
    CONE_REQUIRE(X && Wimg && b1 && b2 && ln_g && ln_b && OUT, "%s fused FFN: null argument", Mode::NAME);
    CONE_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0, "%s fused FFN: row strides must be multiples of 4", Mode::NAME);
    if (M <= 0) return 0;
    typename Mode::FfnArgs a{};
    a.X = X; a.ldx = ldx; a.Wimg = Wimg; a.b1 = b1; a.b2 = b2; a.ln_g = ln_g; a.ln_b = ln_b;
    a.OUT = OUT; a.ldo = ldo; a.M = M; a.M_dev = M_dev; a.ff = ff;
    return tail_launch_kernel<Mode, false, false>(a, n_cu, s);
}

// the projecting tail: post-norm (with the ride where t.next is set), and PRE = the --pre_norm form where the mode has one
template <class Mode, bool PRE>
static int tail_launch_proj_ffn(const TailArgs& t, hipStream_t s) {
    static_assert(!PRE || Mode::HAS_PRE, "this mode has no pre-norm kernel");
    const char* const form = PRE ? "pre-norm" : "fused";
    const TailWeights& w = *t.w;
    const void* Woimg = w.img[Mode::IMG].wo;
    const void* Wimg = w.img[Mode::IMG].ffn;
    const void* Qimg = !PRE && t.next ? t.next->img[Mode::IMG].qkv : nullptr;
    CONE_REQUIRE(tail_ffn_supported(t.ff), "%s %s layer tail: dim_feedforward=%d unsupported", Mode::NAME, form, t.ff);
    CONE_REQUIRE(t.A && Woimg && w.bo && t.R && w.in_g && w.in_b && Wimg && w.b1 && w.b2 && (PRE || (w.out_g && w.out_b)) && t.OUT,
                 "%s %s layer tail: null argument", Mode::NAME, form);
    CONE_REQUIRE(!PRE || !t.OUT2 || (w.out_g && w.out_b), "%s %s layer tail: a normalised second output needs its LayerNorm",
                 Mode::NAME, form);
    CONE_REQUIRE(!t.r_idx || t.R2, "%s %s layer tail: a gathered residual needs both source matrices", Mode::NAME, form);
    CONE_REQUIRE(t.lda % 4 == 0 && t.ldr % 4 == 0 && t.ldo % 4 == 0 && (!PRE || t.ldo2 % 4 == 0),
                 "%s %s layer tail: row strides must be multiples of 4", Mode::NAME, form);
    if (t.M <= 0) return 0;
    typename Mode::FfnArgs a{};
    a.A = t.A; a.lda = t.lda; a.Woimg = Woimg; a.bo = w.bo; a.R = t.R; a.ldr = t.ldr; a.pg = w.in_g; a.pb = w.in_b;
    a.r_idx = t.r_idx; a.R2 = t.R2;
    a.Wimg = Wimg; a.b1 = w.b1; a.b2 = w.b2; a.ln_g = w.out_g; a.ln_b = w.out_b;
    a.OUT = t.OUT; a.ldo = t.ldo; a.M = t.M; a.M_dev = t.M_dev; a.ff = t.ff;
    if constexpr (PRE) {
        a.OUT2 = t.OUT2; a.ldo2 = t.ldo2;
        return tail_launch_kernel<Mode, true, false, true>(a, t.n_cu, s);
    } else {
        if (Qimg) {
            CONE_REQUIRE(t.next->qb && t.QKV && t.n_qkv >= 32 && t.n_qkv % 32 == 0 && t.ldq % 4 == 0,
                         "%s fused layer tail: bad q|k|v arguments", Mode::NAME);
            a.Qimg = Qimg; a.qb = t.next->qb; a.QKV = t.QKV; a.ldq = t.ldq; a.n_qkv = t.n_qkv;
            return tail_launch_kernel<Mode, true, true>(a, t.n_cu, s);
        }
        return tail_launch_kernel<Mode, true, false>(a, t.n_cu, s);
    }
}

template <class Mode>
static int tail_launch_rows256(const float* X, int ldx, const void* Wimg, const float* bias, float* C, int ldc, int M,
                               const int* M_dev, int N, hipStream_t s, int n_cu) {
    CONE_REQUIRE(tail_rows_supported(N), "%s row GEMM: N=%d unsupported", Mode::NAME, N);
    CONE_REQUIRE(n_cu >= 0, "%s row GEMM: negative CU count", Mode::NAME);
    CONE_REQUIRE(X && Wimg && C && ldx % 4 == 0 && ldc % 4 == 0, "%s row GEMM: bad argument", Mode::NAME);
    if (M <= 0) return 0;
    static DeviceOnce once;
    int dev_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        return hipFuncSetAttribute((const void*)Mode::rows_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   Mode::NSLOT * Mode::SLOT + 3072 * (int)sizeof(float));
    }, &dev_cu));
    if (!n_cu) n_cu = dev_cu;
    typename Mode::RowsArgs a{{X, ldx, Wimg, bias, C, ldc, M, M_dev, N}};
    const int tiles = (M + TB_ROWS - 1) / TB_ROWS;
    const int grid = tiles < n_cu ? tiles : n_cu;
    ProfScope ps(PK_GEMM_ROWS16, M, N, 256, M_dev, s);
    hipLaunchKernelGGL(Mode::rows_kernel(), dim3((unsigned)grid), dim3(512),
                       (size_t)Mode::NSLOT * Mode::SLOT + (size_t)N * sizeof(float), s, a);
    CONE_LAUNCH_CHECK();
    return 0;
}

template <class Mode>
static int tail_launch_pack(const float* W1, const float* W2, int ff, void* img, hipStream_t s) {
    CONE_REQUIRE(W2 ? tail_ffn_supported(ff) : (ff >= 32 && ff % 32 == 0), "%s weight image: %d rows unsupported", Mode::NAME, ff);
    CONE_REQUIRE(W1 && img, "%s weight image: null argument", Mode::NAME);
    const size_t total = (size_t)(W2 ? 2 : 1) * (ff / 32) * (16 * Mode::PIECES) * 64;
    hipLaunchKernelGGL(tail_pack_kernel<Mode::PIECES>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, W1, W2, ff,
                       reinterpret_cast<unsigned*>(img));
    CONE_LAUNCH_CHECK();
    return 0;
}

// (not constexpr: a constant-initialised const object would be emitted for the device too, with host functions in it)
template <class Mode>
static TailMode tail_mode() {
    TailMode k{};
    k.ffn_supported = tail_ffn_supported; k.ffn_image_bytes = tail_ffn_image_bytes<Mode>; k.proj_image_bytes = tail_proj_image_bytes<Mode>;
    k.qkv_fits = tail_qkv_fits<Mode>; k.rows_supported = tail_rows_supported; k.rows_image_bytes = tail_rows_image_bytes<Mode>;
    k.pack = tail_launch_pack<Mode>; k.ffn = tail_launch_ffn<Mode>; k.rows256 = tail_launch_rows256<Mode>;
    k.proj_ffn = tail_launch_proj_ffn<Mode, false>;
    if constexpr (Mode::HAS_PRE) k.proj_ffn_prenorm = tail_launch_proj_ffn<Mode, true>;
    return k;
}

}  // namespace cone
