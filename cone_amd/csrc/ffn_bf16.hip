// The single-piece form of ffn_split.hip: the same fused layer tail (attention output projection + residual + LayerNorm,
// linear1 + ReLU + linear2 + residual + LayerNorm, the next layer's q | k | v projection) and the same K = 256 row GEMM,
// with every GEMM operand rounded ONCE to bf16 (round to nearest even, v_cvt_pk_bf16_f32) and ONE
// v_mfma_f32_16x16x32_bf16 per operand pair, accumulated in fp32.  Bias, ReLU, residual and LayerNorm stay fp32, and the
// residual is the UNROUNDED fp32 block input (kept in registers beside its bf16 image).  OPT-IN (cone_model_set_option
// "bf16"): this is plain bf16 matrix arithmetic with a bounded, stated loss of accuracy -- not the fp32-accurate split.
//
// Orientation, operand maps and k permutations are those of ffn_split.hip (a wave owns 16 token rows = the MFMA column
// index; accumulators feed the next product without lane movement; 1-KiB weight slabs [lg][li][8 bf16] read with
// lane-linear ds_read_b128).  The weight image holds the high piece only: 16 slabs = 16 KiB per slot (one third of the
// three-piece image): W1-form slot = [tile 2][step 8] slabs of 32 output units over 256 channels, W2-form slot =
// [channel tile 16] slabs over a chunk's 32 hidden units.
//
// LDS ring (DESIGN.md "bf16 layer tails"): BF_NSLOT = 8 slots of 16 KiB = 128 KiB, one workgroup of 8 waves per CU (the
// register tile -- 64 accumulators, 64 fp32 residual values, 32 operand registers, two fragment sets -- needs the 256
// registers of two waves per SIMD, so a second workgroup would not fit whatever the LDS).  A slot is consumed in 16 MFMAs
// per wave (~0.2 us at two waves per SIMD), far less than an L2 round trip, so the LDS-DMA stream runs BF_AHEAD = 7 slots
// (112 KiB, ~1.5 us) ahead of the slot being read: the pieces of slot g + 7 are issued while slot g is read, into the ring
// slot that slot g - 1 left free at the last barrier.  Every wave issues BF_NPIECE = 2 pieces per slot, in slot order, so at
// the end of slot g "at most (BF_AHEAD - 1) * BF_NPIECE VMEM operations outstanding" means everything issued before slot
// g's own pieces -- slot g + 1 among it -- has landed (VMEM operations of a wave retire in order; a tile's row loads and
// stores that fall in between only make the count more conservative).
#include <mutex>

#include "common.h"

namespace cone {

typedef float bf_f4 __attribute__((ext_vector_type(4)));
typedef float bf_f2 __attribute__((ext_vector_type(2)));
typedef short bf_s8 __attribute__((ext_vector_type(8)));
typedef unsigned bf_u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf_b2 __attribute__((ext_vector_type(2)));

constexpr int BF_ROWS = 128;                       // token rows per workgroup (8 waves x 16)
constexpr int BF_WAVES = 8;
constexpr int BF_SLAB = 1024;                      // one operand slab = one wave's ds_read_b128 = one LDS-DMA piece
constexpr int BF_SLOT = 16 * BF_SLAB;              // bytes per ring slot: 16 slabs
constexpr int BF_NSLOT = 8;                        // ring depth
constexpr int BF_AHEAD = BF_NSLOT - 1;             // slots the LDS-DMA stream runs ahead of the slot being read
constexpr int BF_NPIECE = BF_SLOT / BF_SLAB / BF_WAVES;   // LDS-DMA pieces per wave per slot
constexpr int BF_WAIT = (BF_AHEAD - 1) * BF_NPIECE;       // VMEM operations that may stay outstanding at the end of a slot
constexpr int BF_LDS_MAX = 160 * 1024;
static_assert(BF_NPIECE * BF_SLAB * BF_WAVES == BF_SLOT, "the waves' pieces must tile a slot exactly");
static_assert(BF_NPIECE == 2, "the unit loops issue exactly two pieces per slot (units 3 and 11)");
static_assert(BF_AHEAD + 1 == BF_NSLOT, "the piece issued during slot g + 1 lands in the ring slot of slot g, freed at the last barrier");
static_assert(BF_WAIT == 12, "the s_waitcnt immediates below are written as BF_WAIT; 12 is what DESIGN.md derives");
static_assert((BF_NSLOT & (BF_NSLOT - 1)) == 0, "ring indices wrap with a mask");
static_assert(BF_WAIT >= 0 && BF_WAIT <= 63, "vmcnt is a 6-bit counter");

#define BF_GLDS16(src, dst) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

// two floats -> packed bf16 pair (round to nearest even: v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned bf_pk(float a, float b) {
    const bf_b2 v = __builtin_convertvector(bf_f2{a, b}, bf_b2);
    return __builtin_bit_cast(unsigned, v);
}
// eight fp32 values (two float4) -> one 8-element bf16 operand: one conversion per element pair
__device__ __forceinline__ bf_s8 bf_cvt8(const bf_f4& v0, const bf_f4& v1) {
    const bf_u4 u = {bf_pk(v0[0], v0[1]), bf_pk(v0[2], v0[3]), bf_pk(v1[0], v1[1]), bf_pk(v1[2], v1[3])};
    return __builtin_bit_cast(bf_s8, u);
}

struct FfnBf16Args {
    const float* X; int ldx;                      // (M, 256) block input = residual
    const void* Wimg;                             // packed weight image: 2 * (ff / 32) slots of 16 KiB
    const float* b1; const float* b2;             // (ff), (256)
    const float* ln_g; const float* ln_b;         // (256)
    float* OUT; int ldo;
    int M; const int* M_dev;
    int ff;
    // PROJ: the block input is LayerNorm(R + A Wo^T + bo), computed here; Woimg = Wo's image (8 slots)
    const float* A; int lda; const float* R; int ldr; const int* r_idx; const float* R2;
    const void* Woimg; const float* bo; const float* pg; const float* pb;
    // QKV: the next layer's q | k | v projection of the rows this kernel produces; Qimg = its image (n_qkv / 32 slots)
    const void* Qimg; const float* qb; float* QKV; int ldq; int n_qkv;
    // PRE (--pre_norm, with PROJ): x1 = R + A Wo^T + bo stays UNNORMALISED as the residual, the block reads LayerNorm(x1; pg,
    // pb), OUT = x1 + ffn(...) is stored as it is, and OUT2 (if not null) = LayerNorm(OUT; ln_g, ln_b): the next consumer's norm
    float* OUT2; int ldo2;
};

#define BF_SB() __builtin_amdgcn_sched_barrier(0)
#define BF_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0)
#define BF_CUR_SLOT() (bf_smem + rs * BF_SLOT)      /* the ring slot being read */
#define BF_RD(slot, slab) (*reinterpret_cast<const bf_s8*>((slot) + (slab) * BF_SLAB + lane * 16))
// end of a slot: this wave's reads of it have returned, the next slot has landed (all but the BF_WAIT operations issued
// last, which belong to the slots after it), and every wave is done with the slot the next pieces will overwrite
#define BF_END_SLOT()                                                                      \
    {                                                                                      \
        BF_SB();                                                                           \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");          \
        __builtin_amdgcn_s_barrier();                                                      \
        BF_SB();                                                                           \
        rs = (rs + 1) & (BF_NSLOT - 1);                                                    \
    }
// 16 slabs of a W1-form slot against the rows' 8 k steps: a0 = output units 0 .. 15, a1 = 16 .. 31 of the slot; the
// fragments travel four at a time, one set ahead of the MFMAs that use them; the slot's two LDS-DMA pieces go out at units
// 3 and 11
#define BF_W1_SLOT(sa, a0, a1, xh)                                                                      \
    {                                                                                                   \
        bf_s8 f[2][4];                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) f[0][j] = BF_RD(sa, j);                           \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                 \
            if (q < 3) { _Pragma("unroll") for (int j = 0; j < 4; ++j) f[(q + 1) & 1][j] = BF_RD(sa, 4 * (q + 1) + j); } \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                             \
                const int u = 4 * q + j;                                                                \
                if (u < 8) BF_MFMA(a0, f[q & 1][j], xh[u & 7]); else BF_MFMA(a1, f[q & 1][j], xh[u & 7]); \
            }                                                                                           \
            if (q == 0) stream_piece(0);                                                                \
            if (q == 2) { stream_piece(1); stream_advance(); }                                          \
        }                                                                                               \
    }

template <bool PROJ, bool QKV, bool PRE>
__global__ __launch_bounds__(512, 2) void ffn_bf16_kernel(FfnBf16Args p) {
    extern __shared__ __attribute__((aligned(16))) char bf_smem[];
    float* b1s = reinterpret_cast<float*>(bf_smem + BF_NSLOT * BF_SLOT);
    int M = p.M;
    if (p.M_dev) { const int md = *p.M_dev; M = md < M ? md : M; }
    const int n_tiles = (M + BF_ROWS - 1) / BF_ROWS;
    if ((int)blockIdx.x >= n_tiles) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int ff = p.ff, nc = ff >> 5;            // 32-unit hidden chunks
    constexpr int NP = PROJ ? 8 : 0;              // leading slots of the output projection (32 channels each)
    const int NQ = QKV ? p.n_qkv >> 5 : 0;        // trailing slots of the next layer's q | k | v projection
    const int G = NP + 2 * nc + NQ;               // ring slots per tile

    float* prm = b1s + ff;                        // b2, ln_g, ln_b (+ bo, pg, pb)
    for (int i = tid; i < (ff >> 2); i += 512)
        reinterpret_cast<bf_f4*>(b1s)[i] = reinterpret_cast<const bf_f4*>(p.b1)[i];
    if (tid < 64) {
        reinterpret_cast<bf_f4*>(prm)[tid] = reinterpret_cast<const bf_f4*>(p.b2)[tid];
        if (!PRE || p.OUT2) {
            reinterpret_cast<bf_f4*>(prm + 256)[tid] = reinterpret_cast<const bf_f4*>(p.ln_g)[tid];
            reinterpret_cast<bf_f4*>(prm + 512)[tid] = reinterpret_cast<const bf_f4*>(p.ln_b)[tid];
        }
        if (PROJ) {
            reinterpret_cast<bf_f4*>(prm + 768)[tid] = reinterpret_cast<const bf_f4*>(p.bo)[tid];
            reinterpret_cast<bf_f4*>(prm + 1024)[tid] = reinterpret_cast<const bf_f4*>(p.pg)[tid];
            reinterpret_cast<bf_f4*>(prm + 1280)[tid] = reinterpret_cast<const bf_f4*>(p.pb)[tid];
        }
    }
    float* qbs = prm + 1536;                      // q | k | v bias
    if (QKV)
        for (int i = tid; i < (p.n_qkv >> 2); i += 512)
            reinterpret_cast<bf_f4*>(qbs)[i] = reinterpret_cast<const bf_f4*>(p.qb)[i];

    // LDS-DMA.  The weight stream is one endless sequence of slots (a tile's G slots, then the next tile's: the same
    // weights), issued strictly in order: wg = image slot of the slot being issued, ws = its ring slot, rs = the ring slot
    // being read.  Piece i = 1 KiB at image offset wg * 16 KiB + (2 wave + i) KiB, lane * 16 B inside it; destination = the
    // same offset in ring slot ws.
    int rs = 0, ws = 0, wg = 0;
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    const char* woimg = reinterpret_cast<const char*>(p.Woimg);
    const char* qimg = reinterpret_cast<const char*>(p.Qimg);
    auto stream_piece = [&](int i) {
        char* dstp = bf_smem + ws * BF_SLOT + (wave * BF_NPIECE + i) * BF_SLAB;
        const char* ub = (PROJ && wg < NP ? woimg + (size_t)wg * BF_SLOT
                          : (QKV && wg >= NP + 2 * nc ? qimg + (size_t)(wg - NP - 2 * nc) * BF_SLOT
                                                       : wimg + (size_t)(wg - NP) * BF_SLOT)) +
                         (size_t)(wave * BF_NPIECE + i) * BF_SLAB;
        asm volatile("" : "+s"(ub));
        BF_GLDS16(ub + (unsigned)(lane * 16), dstp);
    };
    auto stream_advance = [&]() {
        ws = (ws + 1) & (BF_NSLOT - 1);
        wg = wg + 1 == G ? 0 : wg + 1;
    };
    for (int g = 0; g < BF_AHEAD; ++g) {
#pragma unroll
        for (int i = 0; i < BF_NPIECE; ++i) stream_piece(i);
        stream_advance();
    }

    // a tile's rows (PROJ: the attention rows = B operand of the projection, else the block input) are requested from
    // the previous tile's epilogue, ahead of its LayerNorm and stores
    bf_f4 xr[16];
    auto load_rows = [&](int tile) {
        const int row = tile * BF_ROWS + wave * 16 + li;
        const size_t lr = (size_t)(row < M ? row : M - 1);
        const float* xp = (PROJ ? p.A + lr * p.lda : p.X + lr * p.ldx) + 4 * lg;
#pragma unroll
        for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const bf_f4*>(xp + 16 * q);
    };
    load_rows(blockIdx.x);
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int my_row = tile * BF_ROWS + wave * 16 + li;
    const size_t ld_row = (size_t)(my_row < M ? my_row : M - 1);
    // rounded once: xh[s] = B operand of GEMM1's step s (channels 32 s + 16 (j / 4) + 4 lg + j % 4)
    bf_s8 xh[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
    if (first) {        // slot 0 has landed everywhere and the parameter rows are written
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");
        __builtin_amdgcn_s_barrier();
        BF_SB();
        first = false;
    }
    if (PROJ) {
        // ---- attention output projection: slot g = channels [32 g, 32 g + 32) of A Wo^T
#pragma unroll
        for (int g = 0; g < NP; ++g) {
            const char* sa = BF_CUR_SLOT();
            bf_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            BF_END_SLOT()
            xr[2 * g] = a0; xr[2 * g + 1] = a1;       // (the attention rows are dead: xh holds their image)
        }
        // + bo + residual rows, LayerNorm: the block input (fp32: the residual of the FFN), rounded once for GEMM1
        {
            const float* rp = p.R + ld_row * p.ldr + 4 * lg;
            if (p.r_idx) {
                const int ix = p.r_idx[ld_row];
                rp = (ix >= 0 ? p.R + (size_t)ix * p.ldr : p.R2 + (size_t)(~ix) * p.ldr) + 4 * lg;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                xr[q] += *reinterpret_cast<const bf_f4*>(rp + 16 * q) + *reinterpret_cast<const bf_f4*>(prm + 768 + 16 * q + 4 * lg);
        }
        float t1 = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) t1 += (xr[t][0] + xr[t][1]) + (xr[t][2] + xr[t][3]);
        t1 += __shfl_xor(t1, 16, 64);
        t1 += __shfl_xor(t1, 32, 64);
        const float mu = t1 * (1.0f / 256.0f);
        float t2 = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float cv = xr[t][r] - mu;
                if (!PRE) xr[t][r] = cv;
                t2 = fmaf(cv, cv, t2);
            }
        }
        t2 += __shfl_xor(t2, 16, 64);
        t2 += __shfl_xor(t2, 32, 64);
        const float prstd = 1.0f / sqrtf(t2 * (1.0f / 256.0f) + 1e-5f);
        if (!PRE) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const bf_f4 g4 = *reinterpret_cast<const bf_f4*>(prm + 1024 + 16 * t + 4 * lg);
                const bf_f4 b4 = *reinterpret_cast<const bf_f4*>(prm + 1280 + 16 * t + 4 * lg);
#pragma unroll
                for (int r = 0; r < 4; ++r) xr[t][r] = xr[t][r] * prstd * g4[r] + b4[r];
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
        } else {        // the residual xr stays as it is; only the block's bf16 operand is normalised
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                bf_f4 n[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf_f4 g4 = *reinterpret_cast<const bf_f4*>(prm + 1024 + 16 * (2 * s + h) + 4 * lg);
                    const bf_f4 b4 = *reinterpret_cast<const bf_f4*>(prm + 1280 + 16 * (2 * s + h) + 4 * lg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) n[h][r] = (xr[2 * s + h][r] - mu) * prstd * g4[r] + b4[r];
                }
                xh[s] = bf_cvt8(n[0], n[1]);
            }
        }
    }
    bf_f4 y[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] = bf_f4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nc; ++c) {
        // ---- GEMM1: the chunk's two 16-unit tiles over the 256 channels (slot 2 c)
        const char* sa = BF_CUR_SLOT();
        bf_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        BF_W1_SLOT(sa, a0, a1, xh)
        // bias + ReLU + the one rounding: the B operand of GEMM2 (k slot (lg, j) <-> unit 16 (j / 4) + 4 lg + j % 4)
        a0 += *reinterpret_cast<const bf_f4*>(b1s + 32 * c + 4 * lg);
        a1 += *reinterpret_cast<const bf_f4*>(b1s + 32 * c + 16 + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) { a0[r] = fmaxf(a0[r], 0.f); a1[r] = fmaxf(a1[r], 0.f); }
        const bf_s8 hh = bf_cvt8(a0, a1);
        BF_END_SLOT()
        // ---- GEMM2: all 256 output channels over the chunk's 32 hidden units (slot 2 c + 1: [channel tile] slabs)
        const char* sw = BF_CUR_SLOT();
        {
            bf_s8 f[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) f[0][j] = BF_RD(sw, j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < 3) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[(q + 1) & 1][j] = BF_RD(sw, 4 * (q + 1) + j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) BF_MFMA(y[4 * q + j], f[q & 1][j], hh);
                if (q == 0) stream_piece(0);
                if (q == 2) { stream_piece(1); stream_advance(); }
            }
        }
        BF_END_SLOT()
    }
    // ---- epilogue: + b2 + the fp32 residual (xr is in the accumulator layout: channel 16 t + 4 lg + r), LayerNorm, store
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] += xr[t] + *reinterpret_cast<const bf_f4*>(prm + 16 * t + 4 * lg);
    BF_SB();
    // the residual is consumed: the next tile's rows travel under the LayerNorm and the stores (after the last tile a
    // valid tile is simply re-read, so that the register tile has one definition per iteration)
    load_rows(tile + (int)gridDim.x < n_tiles ? tile + (int)gridDim.x : tile);
    BF_SB();
    if (PRE && my_row < M) {        // the unnormalised residual stream
        float* op = p.OUT + (size_t)my_row * p.ldo + 4 * lg;
#pragma unroll
        for (int t = 0; t < 16; ++t) *reinterpret_cast<bf_f4*>(op + 16 * t) = y[t];
    }
    if (!PRE || p.OUT2) {
    float s1 = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) s1 += (y[t][0] + y[t][1]) + (y[t][2] + y[t][3]);
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    const float mean = s1 * (1.0f / 256.0f);
    float s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { y[t][r] -= mean; s2 = fmaf(y[t][r], y[t][r], s2); }
    }
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    const float rstd = 1.0f / sqrtf(s2 * (1.0f / 256.0f) + 1e-5f);
    if (my_row < M) {
        float* op = (PRE ? p.OUT2 + (size_t)my_row * p.ldo2 : p.OUT + (size_t)my_row * p.ldo) + 4 * lg;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const bf_f4 g = *reinterpret_cast<const bf_f4*>(prm + 256 + 16 * t + 4 * lg);
            const bf_f4 be = *reinterpret_cast<const bf_f4*>(prm + 512 + 16 * t + 4 * lg);
            bf_f4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = y[t][r] * rstd * g[r] + be[r];
            *reinterpret_cast<bf_f4*>(op + 16 * t) = o;
            if (QKV) y[t] = o;
        }
    } else if (QKV) {       // rows past M feed unstored outputs: any finite values
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = bf_f4{0.f, 0.f, 0.f, 0.f};
    }
    }   // LayerNorm of the output
    if (QKV) {
        // ---- the next layer's q | k | v projection of these rows, straight from the registers: rounded once, then NQ
        // slots of 32 output channels each, stored from the accumulators
#pragma unroll
        for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(y[2 * s], y[2 * s + 1]);
        float* qrow = p.QKV + (size_t)my_row * p.ldq + 4 * lg;
        for (int g = 0; g < NQ; ++g) {
            const char* sa = BF_CUR_SLOT();
            bf_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            if (my_row < M) {
                *reinterpret_cast<bf_f4*>(qrow + 32 * g) = a0 + *reinterpret_cast<const bf_f4*>(qbs + 32 * g + 4 * lg);
                *reinterpret_cast<bf_f4*>(qrow + 32 * g + 16) = a1 + *reinterpret_cast<const bf_f4*>(qbs + 32 * g + 16 + 4 * lg);
            }
            BF_END_SLOT()
        }
    }
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------------------------
// C = X W^T + bias for K = 256 and any N % 32 == 0 with the same single-piece operands: the projection phase of the kernel
// above on its own (W streams as N / 32 W1-form slots; every slot's 32 output channels are stored from the accumulators).
struct RowsBf16Args {
    const float* X; int ldx; const void* Wimg; const float* bias; float* C; int ldc; int M; const int* M_dev; int N;
};

__global__ __launch_bounds__(512, 2) void rows256_bf16_kernel(RowsBf16Args p) {
    extern __shared__ __attribute__((aligned(16))) char bf_smem[];
    float* bs = reinterpret_cast<float*>(bf_smem + BF_NSLOT * BF_SLOT);
    int M = p.M;
    if (p.M_dev) { const int md = *p.M_dev; M = md < M ? md : M; }
    const int n_tiles = (M + BF_ROWS - 1) / BF_ROWS;
    if ((int)blockIdx.x >= n_tiles) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int G = p.N >> 5;                         // ring slots per tile
    for (int i = tid; i < (p.N >> 2); i += 512)
        reinterpret_cast<bf_f4*>(bs)[i] = p.bias ? reinterpret_cast<const bf_f4*>(p.bias)[i] : bf_f4{0.f, 0.f, 0.f, 0.f};
    int rs = 0, ws = 0, wg = 0;                     // as in ffn_bf16_kernel
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    auto stream_piece = [&](int i) {
        char* dstp = bf_smem + ws * BF_SLOT + (wave * BF_NPIECE + i) * BF_SLAB;
        const char* ub = wimg + (size_t)wg * BF_SLOT + (size_t)(wave * BF_NPIECE + i) * BF_SLAB;
        asm volatile("" : "+s"(ub));
        BF_GLDS16(ub + (unsigned)(lane * 16), dstp);
    };
    auto stream_advance = [&]() {
        ws = (ws + 1) & (BF_NSLOT - 1);
        wg = wg + 1 == G ? 0 : wg + 1;
    };
    for (int g = 0; g < BF_AHEAD; ++g) {
#pragma unroll
        for (int i = 0; i < BF_NPIECE; ++i) stream_piece(i);
        stream_advance();
    }
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int my_row = tile * BF_ROWS + wave * 16 + li;
        const size_t ld_row = (size_t)(my_row < M ? my_row : M - 1);
        bf_s8 xh[8];
        {
            const float* xp = p.X + ld_row * p.ldx + 4 * lg;
            bf_f4 xr[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const bf_f4*>(xp + 16 * q);
#pragma unroll
            for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
        }
        if (first) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");
            __builtin_amdgcn_s_barrier();
            BF_SB();
            first = false;
        }
        float* crow = p.C + (size_t)my_row * p.ldc + 4 * lg;
        for (int g = 0; g < G; ++g) {
            const char* sa = BF_CUR_SLOT();
            bf_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            if (my_row < M) {
                *reinterpret_cast<bf_f4*>(crow + 32 * g) = a0 + *reinterpret_cast<const bf_f4*>(bs + 32 * g + 4 * lg);
                *reinterpret_cast<bf_f4*>(crow + 32 * g + 16) = a1 + *reinterpret_cast<const bf_f4*>(bs + 32 * g + 16 + 4 * lg);
            }
            BF_END_SLOT()
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#undef BF_SB
#undef BF_MFMA
#undef BF_W1_SLOT
#undef BF_END_SLOT
#undef BF_RD
#undef BF_CUR_SLOT

// the ring + b1 + six parameter rows (+ the q | k | v bias) within the CU's 160 KiB of LDS
static size_t ffn_bf16_lds(int ff, int n_qkv) { return (size_t)BF_NSLOT * BF_SLOT + (size_t)(ff + 6 * 256 + n_qkv) * sizeof(float); }
bool ffn_bf16_supported(int ff) { return ff >= 64 && ff % 32 == 0 && ff <= 2048; }
size_t ffn_bf16_image_bytes(int ff) { return (size_t)2 * (ff / 32) * BF_SLOT; }
size_t ffn_bf16_proj_image_bytes() { return (size_t)8 * BF_SLOT; }
bool ffn_bf16_qkv_fits(int ff, int n_qkv) {
    return ffn_bf16_supported(ff) && n_qkv >= 32 && n_qkv % 32 == 0 && ffn_bf16_lds(ff, n_qkv) <= (size_t)BF_LDS_MAX;
}

template <bool PROJ, bool QKV, bool PRE = false>
static int launch_ffn_bf16_t(const FfnBf16Args& a, hipStream_t s) {
    const size_t lds = ffn_bf16_lds(a.ff, QKV ? a.n_qkv : 0);
    CONE_REQUIRE(lds <= (size_t)BF_LDS_MAX, "bf16 fused layer tail: %zu bytes of LDS (ff %d, q|k|v %d) exceed 160 KiB", lds, a.ff, a.n_qkv);
    static DeviceOnce once;
    int n_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        return hipFuncSetAttribute((const void*)ffn_bf16_kernel<PROJ, QKV, PRE>, hipFuncAttributeMaxDynamicSharedMemorySize, BF_LDS_MAX);
    }, &n_cu));
    const int tiles = (a.M + BF_ROWS - 1) / BF_ROWS;
    const int grid = tiles < n_cu ? tiles : n_cu;
    ProfScope ps(PROJ ? PK_FFN_PROJ : PK_FFN_FUSED, a.M, a.ff + (QKV ? a.n_qkv / 2 : 0), 256, a.M_dev, s);
    hipLaunchKernelGGL((ffn_bf16_kernel<PROJ, QKV, PRE>), dim3((unsigned)grid), dim3(512), lds, s, a);
    CONE_LAUNCH_CHECK();
    return 0;
}

int launch_ffn_bf16(const float* X, int ldx, const void* Wimg, const float* b1, const float* b2, const float* ln_g,
                    const float* ln_b, float* OUT, int ldo, int M, const int* M_dev, int ff, hipStream_t s) {
    CONE_REQUIRE(ffn_bf16_supported(ff), "bf16 fused FFN: dim_feedforward=%d unsupported", ff);
    CONE_REQUIRE(X && Wimg && b1 && b2 && ln_g && ln_b && OUT, "bf16 fused FFN: null argument");
    CONE_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0, "bf16 fused FFN: row strides must be multiples of 4");
    if (M <= 0) return 0;
    FfnBf16Args a{};
    a.X = X; a.ldx = ldx; a.Wimg = Wimg; a.b1 = b1; a.b2 = b2; a.ln_g = ln_g; a.ln_b = ln_b;
    a.OUT = OUT; a.ldo = ldo; a.M = M; a.M_dev = M_dev; a.ff = ff;
    return launch_ffn_bf16_t<false, false>(a, s);
}

int launch_proj_ffn_bf16(const TailArgs& t, hipStream_t s) {
    const TailWeights& w = *t.w;
    const void* Woimg = w.img[TAIL_IMG_BF16].wo;
    const void* Wimg = w.img[TAIL_IMG_BF16].ffn;
    const void* Qimg = t.next ? t.next->img[TAIL_IMG_BF16].qkv : nullptr;
    CONE_REQUIRE(ffn_bf16_supported(t.ff), "bf16 fused layer tail: dim_feedforward=%d unsupported", t.ff);
    CONE_REQUIRE(t.A && Woimg && w.bo && t.R && w.in_g && w.in_b && Wimg && w.b1 && w.b2 && w.out_g && w.out_b && t.OUT,
                 "bf16 fused layer tail: null argument");
    CONE_REQUIRE(!t.r_idx || t.R2, "bf16 fused layer tail: a gathered residual needs both source matrices");
    CONE_REQUIRE(t.lda % 4 == 0 && t.ldr % 4 == 0 && t.ldo % 4 == 0, "bf16 fused layer tail: row strides must be multiples of 4");
    if (t.M <= 0) return 0;
    FfnBf16Args a{};
    a.A = t.A; a.lda = t.lda; a.Woimg = Woimg; a.bo = w.bo; a.R = t.R; a.ldr = t.ldr; a.pg = w.in_g; a.pb = w.in_b;
    a.r_idx = t.r_idx; a.R2 = t.R2;
    a.Wimg = Wimg; a.b1 = w.b1; a.b2 = w.b2; a.ln_g = w.out_g; a.ln_b = w.out_b;
    a.OUT = t.OUT; a.ldo = t.ldo; a.M = t.M; a.M_dev = t.M_dev; a.ff = t.ff;
    if (Qimg) {
        CONE_REQUIRE(t.next->qb && t.QKV && t.n_qkv >= 32 && t.n_qkv % 32 == 0 && t.ldq % 4 == 0,
                     "bf16 fused layer tail: bad q|k|v arguments");
        a.Qimg = Qimg; a.qb = t.next->qb; a.QKV = t.QKV; a.ldq = t.ldq; a.n_qkv = t.n_qkv;
        return launch_ffn_bf16_t<true, true>(a, s);
    }
    return launch_ffn_bf16_t<true, false>(a, s);
}

int launch_proj_ffn_bf16_prenorm(const TailArgs& t, hipStream_t s) {
    const TailWeights& w = *t.w;
    const void* Woimg = w.img[TAIL_IMG_BF16].wo;
    const void* Wimg = w.img[TAIL_IMG_BF16].ffn;
    CONE_REQUIRE(ffn_bf16_supported(t.ff), "bf16 pre-norm layer tail: dim_feedforward=%d unsupported", t.ff);
    CONE_REQUIRE(t.A && Woimg && w.bo && t.R && w.in_g && w.in_b && Wimg && w.b1 && w.b2 && t.OUT, "bf16 pre-norm layer tail: null argument");
    CONE_REQUIRE(!t.OUT2 || (w.out_g && w.out_b), "bf16 pre-norm layer tail: a normalised second output needs its LayerNorm");
    CONE_REQUIRE(!t.r_idx || t.R2, "bf16 pre-norm layer tail: a gathered residual needs both source matrices");
    CONE_REQUIRE(t.lda % 4 == 0 && t.ldr % 4 == 0 && t.ldo % 4 == 0 && t.ldo2 % 4 == 0,
                 "bf16 pre-norm layer tail: row strides must be multiples of 4");
    if (t.M <= 0) return 0;
    FfnBf16Args a{};
    a.A = t.A; a.lda = t.lda; a.Woimg = Woimg; a.bo = w.bo; a.R = t.R; a.ldr = t.ldr; a.pg = w.in_g; a.pb = w.in_b;
    a.r_idx = t.r_idx; a.R2 = t.R2;
    a.Wimg = Wimg; a.b1 = w.b1; a.b2 = w.b2; a.ln_g = w.out_g; a.ln_b = w.out_b;
    a.OUT = t.OUT; a.ldo = t.ldo; a.OUT2 = t.OUT2; a.ldo2 = t.ldo2; a.M = t.M; a.M_dev = t.M_dev; a.ff = t.ff;
    return launch_ffn_bf16_t<true, false, true>(a, s);
}

bool rows256_bf16_supported(int N) { return N >= 32 && N % 32 == 0 && N <= 3072; }
size_t rows256_bf16_image_bytes(int N) { return (size_t)(N / 32) * BF_SLOT; }

int launch_rows256_bf16(const float* X, int ldx, const void* Wimg, const float* bias, float* C, int ldc, int M,
                        const int* M_dev, int N, hipStream_t s) {
    CONE_REQUIRE(rows256_bf16_supported(N), "bf16 row GEMM: N=%d unsupported", N);
    CONE_REQUIRE(X && Wimg && C && ldx % 4 == 0 && ldc % 4 == 0, "bf16 row GEMM: bad argument");
    if (M <= 0) return 0;
    static DeviceOnce once;
    int n_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        return hipFuncSetAttribute((const void*)rows256_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   BF_NSLOT * BF_SLOT + 3072 * (int)sizeof(float));
    }, &n_cu));
    RowsBf16Args a{X, ldx, Wimg, bias, C, ldc, M, M_dev, N};
    const int tiles = (M + BF_ROWS - 1) / BF_ROWS;
    const int grid = tiles < n_cu ? tiles : n_cu;
    ProfScope ps(PK_GEMM_ROWS16, M, N, 256, M_dev, s);
    hipLaunchKernelGGL(rows256_bf16_kernel, dim3((unsigned)grid), dim3(512),
                       (size_t)BF_NSLOT * BF_SLOT + (size_t)N * sizeof(float), s, a);
    CONE_LAUNCH_CHECK();
    return 0;
}

// ---- weight images (once per model): the single-piece form of ffn_split_pack_kernel.  One thread per 16-B fragment:
// slot g, slab sl, lane l.  W2 != null: W1 (ff, 256) and W2 (256, ff) -> 2 * (ff / 32) slots (slot 2 c: W1 rows of hidden
// chunk c as [tile 2][step 8] slabs, slot 2 c + 1: W2 columns as [channel tile 16] slabs).  W2 == null: W1 is any
// (N = ff, 256) weight of a 256-channel product: N / 32 slots in the W1 slab order.
__global__ __launch_bounds__(256) void ffn_bf16_pack_kernel(const float* __restrict__ W1, const float* __restrict__ W2,
                                                            int ff, unsigned* __restrict__ img) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)(W2 ? 2 : 1) * (ff / 32) * 16 * 64;
    if (idx >= total) return;
    const int l = (int)(idx & 63);
    const int sl = (int)((idx >> 6) & 15);
    const int g = (int)(idx >> 10);
    const int c = W2 ? g >> 1 : g, li = l & 15, lg = l >> 4;
    float v[8];
    if (!W2 || (g & 1) == 0) {      // W1 image: slab = tile * 8 + step
        const int t = sl >> 3, s = sl & 7;
        const float* row = W1 + (size_t)(32 * c + 16 * t + li) * 256;
        for (int j = 0; j < 8; ++j) v[j] = row[32 * s + 16 * (j >> 2) + 4 * lg + (j & 3)];
    } else {                        // W2 image: slab = channel tile
        const float* row = W2 + (size_t)(16 * sl + li) * ff + 32 * c;
        for (int j = 0; j < 8; ++j) v[j] = row[16 * (j >> 2) + 4 * lg + (j & 3)];
    }
    unsigned* dst = img + idx * 4;
    for (int e = 0; e < 4; ++e) dst[e] = bf_pk(v[2 * e], v[2 * e + 1]);
}

int launch_ffn_bf16_pack(const float* W1, const float* W2, int ff, void* img, hipStream_t s) {
    CONE_REQUIRE(W2 ? ffn_bf16_supported(ff) : (ff >= 32 && ff % 32 == 0), "bf16 weight image: %d rows unsupported", ff);
    CONE_REQUIRE(W1 && img, "bf16 weight image: null argument");
    const size_t total = (size_t)(W2 ? 2 : 1) * (ff / 32) * 16 * 64;
    hipLaunchKernelGGL(ffn_bf16_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, W1, W2, ff,
                       reinterpret_cast<unsigned*>(img));
    CONE_LAUNCH_CHECK();
    return 0;
}

}  // namespace cone
