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
//
// This file keeps what is the single-piece form's own: the ring (8 slots of 16 KiB with running rs / ws / wg, 7 slots ahead,
// vmcnt(BF_WAIT) and the static_asserts that tie them), the operand preparation (bf_cvt8), the one-product unit, the
// residual kept as fp32 registers, and the PRE form.  The steps it shares with ffn_split.hip, the pack kernel and the host
// side are in tail_bf16_common.h.
#include <mutex>

#include "tail_bf16_common.h"

namespace cone {

constexpr int BF_WAVES = 8;
constexpr int BF_SLOT = 16 * TB_SLAB;              // bytes per ring slot: 16 slabs
constexpr int BF_NSLOT = 8;                        // ring depth
constexpr int BF_AHEAD = BF_NSLOT - 1;             // slots the LDS-DMA stream runs ahead of the slot being read
constexpr int BF_NPIECE = BF_SLOT / TB_SLAB / BF_WAVES;   // LDS-DMA pieces per wave per slot
constexpr int BF_WAIT = (BF_AHEAD - 1) * BF_NPIECE;       // VMEM operations that may stay outstanding at the end of a slot
static_assert(BF_NPIECE * TB_SLAB * BF_WAVES == BF_SLOT, "the waves' pieces must tile a slot exactly");
static_assert(BF_NPIECE == 2, "the unit loops issue exactly two pieces per slot (units 3 and 11)");
static_assert(BF_AHEAD + 1 == BF_NSLOT, "the piece issued during slot g + 1 lands in the ring slot of slot g, freed at the last barrier");
static_assert(BF_WAIT == 12, "the s_waitcnt immediates below are written as BF_WAIT; 12 is what DESIGN.md derives");
static_assert((BF_NSLOT & (BF_NSLOT - 1)) == 0, "ring indices wrap with a mask");
static_assert(BF_WAIT >= 0 && BF_WAIT <= 63, "vmcnt is a 6-bit counter");

// eight fp32 values (two float4) -> one 8-element bf16 operand: one conversion per element pair
__device__ __forceinline__ tb_s8 bf_cvt8(const tb_f4& v0, const tb_f4& v1) {
    const tb_u4 u = {tb_pk(v0[0], v0[1]), tb_pk(v0[2], v0[3]), tb_pk(v1[0], v1[1]), tb_pk(v1[2], v1[3])};
    return __builtin_bit_cast(tb_s8, u);
}

#define BF_CUR_SLOT() (bf_smem + rs * BF_SLOT)      /* the ring slot being read */
#define BF_RD(slot, slab) (*reinterpret_cast<const tb_s8*>((slot) + (slab) * TB_SLAB + lane * 16))
// end of a slot: this wave's reads of it have returned, the next slot has landed (all but the BF_WAIT operations issued
// last, which belong to the slots after it), and every wave is done with the slot the next pieces will overwrite
#define BF_END_SLOT()                                                                      \
    {                                                                                      \
        TB_SB();                                                                           \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");          \
        __builtin_amdgcn_s_barrier();                                                      \
        TB_SB();                                                                           \
        rs = (rs + 1) & (BF_NSLOT - 1);                                                    \
    }
// 16 slabs of a W1-form slot against the rows' 8 k steps: a0 = output units 0 .. 15, a1 = 16 .. 31 of the slot; the
// fragments travel four at a time, one set ahead of the MFMAs that use them; the slot's two LDS-DMA pieces go out at units
// 3 and 11
#define BF_W1_SLOT(sa, a0, a1, xh)                                                                      \
    {                                                                                                   \
        tb_s8 f[2][4];                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) f[0][j] = BF_RD(sa, j);                           \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                 \
            if (q < 3) { _Pragma("unroll") for (int j = 0; j < 4; ++j) f[(q + 1) & 1][j] = BF_RD(sa, 4 * (q + 1) + j); } \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                             \
                const int u = 4 * q + j;                                                                \
                if (u < 8) TB_MFMA(a0, f[q & 1][j], xh[u & 7]); else TB_MFMA(a1, f[q & 1][j], xh[u & 7]); \
            }                                                                                           \
            if (q == 0) stream_piece(0);                                                                \
            if (q == 2) { stream_piece(1); stream_advance(); }                                          \
        }                                                                                               \
    }

template <bool PROJ, bool QKV, bool PRE>
__global__ __launch_bounds__(512, 2) void ffn_bf16_kernel(FfnBf16Args p) {
    extern __shared__ __attribute__((aligned(16))) char bf_smem[];
    float* b1s = reinterpret_cast<float*>(bf_smem + BF_NSLOT * BF_SLOT);
    TB_PROLOGUE(p);
    const int ff = p.ff, nc = ff >> 5;            // 32-unit hidden chunks
    constexpr int NP = PROJ ? 8 : 0;              // leading slots of the output projection (32 channels each)
    const int NQ = QKV ? p.n_qkv >> 5 : 0;        // trailing slots of the next layer's q | k | v projection
    const int G = NP + 2 * nc + NQ;               // ring slots per tile

    float* prm = b1s + ff;                        // the parameter rows (PRM_*)
    float* qbs = prm + PRM_QB;                    // q | k | v bias
    TB_STAGE_PARAMS(p, b1s, prm, ff, !PRE || p.OUT2);

    // LDS-DMA.  The weight stream is one endless sequence of slots (a tile's G slots, then the next tile's: the same
    // weights), issued strictly in order: wg = image slot of the slot being issued, ws = its ring slot, rs = the ring slot
    // being read.  Piece i = 1 KiB at image offset wg * 16 KiB + (2 wave + i) KiB, lane * 16 B inside it; destination = the
    // same offset in ring slot ws.
    int rs = 0, ws = 0, wg = 0;
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    const char* woimg = reinterpret_cast<const char*>(p.Woimg);
    const char* qimg = reinterpret_cast<const char*>(p.Qimg);
    auto stream_piece = [&](int i) {
        char* dstp = bf_smem + ws * BF_SLOT + (wave * BF_NPIECE + i) * TB_SLAB;
        const char* ub = TB_SLOT_IMAGE(woimg, wimg, qimg, wg, BF_SLOT) + (size_t)(wave * BF_NPIECE + i) * TB_SLAB;
        asm volatile("" : "+s"(ub));
        TB_GLDS16(ub + (unsigned)(lane * 16), dstp);
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
    tb_f4 xr[16];
    auto load_rows = [&](int tile) {
        const int row = TB_ROW_OF(tile);
        const size_t lr = TB_LD_ROW(row);
        TB_LOAD_ROW(xr, (PROJ ? p.A + lr * p.lda : p.X + lr * p.ldx) + 4 * lg)
    };
    load_rows(blockIdx.x);
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int my_row = TB_ROW_OF(tile);
    const size_t ld_row = TB_LD_ROW(my_row);
    // rounded once: xh[s] = B operand of GEMM1's step s (channels 32 s + 16 (j / 4) + 4 lg + j % 4)
    tb_s8 xh[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
    if (first) {        // slot 0 has landed everywhere and the parameter rows are written
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");
        __builtin_amdgcn_s_barrier();
        TB_SB();
        first = false;
    }
    if (PROJ) {
        // ---- attention output projection: slot g = channels [32 g, 32 g + 32) of A Wo^T
#pragma unroll
        for (int g = 0; g < NP; ++g) {
            const char* sa = BF_CUR_SLOT();
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            BF_END_SLOT()
            xr[2 * g] = a0; xr[2 * g + 1] = a1;       // (the attention rows are dead: xh holds their image)
        }
        // + bo + residual rows, LayerNorm: the block input (fp32: the residual of the FFN), rounded once for GEMM1
        TB_ADD_RESIDUAL(xr, p, ld_row, prm)
        TB_LN_MOMENTS(xr, !PRE, mu, prstd)
        if (!PRE) {
#pragma unroll
            for (int t = 0; t < 16; ++t) TB_LN_APPLY(xr[t], xr[t][r], prstd, prm, PRM_PG, PRM_PB, t)
#pragma unroll
            for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
        } else {        // the residual xr stays as it is; only the block's bf16 operand is normalised
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                tb_f4 n[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) TB_LN_APPLY(n[h], xr[2 * s + h][r] - mu, prstd, prm, PRM_PG, PRM_PB, 2 * s + h)
                xh[s] = bf_cvt8(n[0], n[1]);
            }
        }
    }
    tb_f4 y[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] = tb_f4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nc; ++c) {
        // ---- GEMM1: the chunk's two 16-unit tiles over the 256 channels (slot 2 c)
        const char* sa = BF_CUR_SLOT();
        tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        BF_W1_SLOT(sa, a0, a1, xh)
        // bias + ReLU + the one rounding: the B operand of GEMM2 (k slot (lg, j) <-> unit 16 (j / 4) + 4 lg + j % 4)
        a0 += *reinterpret_cast<const tb_f4*>(b1s + 32 * c + 4 * lg);
        a1 += *reinterpret_cast<const tb_f4*>(b1s + 32 * c + 16 + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) { a0[r] = fmaxf(a0[r], 0.f); a1[r] = fmaxf(a1[r], 0.f); }
        const tb_s8 hh = bf_cvt8(a0, a1);
        BF_END_SLOT()
        // ---- GEMM2: all 256 output channels over the chunk's 32 hidden units (slot 2 c + 1: [channel tile] slabs)
        const char* sw = BF_CUR_SLOT();
        {
            tb_s8 f[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) f[0][j] = BF_RD(sw, j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < 3) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[(q + 1) & 1][j] = BF_RD(sw, 4 * (q + 1) + j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) TB_MFMA(y[4 * q + j], f[q & 1][j], hh);
                if (q == 0) stream_piece(0);
                if (q == 2) { stream_piece(1); stream_advance(); }
            }
        }
        BF_END_SLOT()
    }
    // ---- epilogue: + b2 + the fp32 residual (xr is in the accumulator layout: channel 16 t + 4 lg + r), LayerNorm, store
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] += xr[t] + *reinterpret_cast<const tb_f4*>(prm + PRM_B2 + 16 * t + 4 * lg);
    TB_SB();
    // the residual is consumed: the next tile's rows travel under the LayerNorm and the stores (after the last tile a
    // valid tile is simply re-read, so that the register tile has one definition per iteration)
    load_rows(tile + (int)gridDim.x < n_tiles ? tile + (int)gridDim.x : tile);
    TB_SB();
    if (PRE && my_row < M) {        // the unnormalised residual stream
        float* op = p.OUT + (size_t)my_row * p.ldo + 4 * lg;
#pragma unroll
        for (int t = 0; t < 16; ++t) *reinterpret_cast<tb_f4*>(op + 16 * t) = y[t];
    }
    if (!PRE || p.OUT2) {
    TB_LN_MOMENTS(y, true, mean, rstd)
    if (my_row < M) {
        float* op = (PRE ? p.OUT2 + (size_t)my_row * p.ldo2 : p.OUT + (size_t)my_row * p.ldo) + 4 * lg;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            tb_f4 o;
            TB_LN_APPLY(o, y[t][r], rstd, prm, PRM_LN_G, PRM_LN_B, t)
            *reinterpret_cast<tb_f4*>(op + 16 * t) = o;
            if (QKV) y[t] = o;
        }
    } else if (QKV) {       // rows past M feed unstored outputs: any finite values
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = tb_f4{0.f, 0.f, 0.f, 0.f};
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
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            if (my_row < M) TB_STORE_SLOT(qrow, qbs, g, a0, a1)
            BF_END_SLOT()
        }
    }
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------------------------
// C = X W^T + bias for K = 256 and any N % 32 == 0 with the same single-piece operands: the projection phase of the kernel
// above on its own (W streams as N / 32 W1-form slots; every slot's 32 output channels are stored from the accumulators).
__global__ __launch_bounds__(512, 2) void rows256_bf16_kernel(RowsBf16Args p) {
    extern __shared__ __attribute__((aligned(16))) char bf_smem[];
    float* bs = reinterpret_cast<float*>(bf_smem + BF_NSLOT * BF_SLOT);
    TB_PROLOGUE(p);
    const int G = p.N >> 5;                         // ring slots per tile
    TB_STAGE_BIAS(bs, p.bias, p.N);
    int rs = 0, ws = 0, wg = 0;                     // as in ffn_bf16_kernel
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    auto stream_piece = [&](int i) {
        char* dstp = bf_smem + ws * BF_SLOT + (wave * BF_NPIECE + i) * TB_SLAB;
        const char* ub = wimg + (size_t)wg * BF_SLOT + (size_t)(wave * BF_NPIECE + i) * TB_SLAB;
        asm volatile("" : "+s"(ub));
        TB_GLDS16(ub + (unsigned)(lane * 16), dstp);
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
        const int my_row = TB_ROW_OF(tile);
        tb_s8 xh[8];
        {
            tb_f4 xr[16];
            TB_LOAD_ROW(xr, p.X + TB_LD_ROW(my_row) * p.ldx + 4 * lg)
#pragma unroll
            for (int s = 0; s < 8; ++s) xh[s] = bf_cvt8(xr[2 * s], xr[2 * s + 1]);
        }
        if (first) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BF_WAIT) : "memory");
            __builtin_amdgcn_s_barrier();
            TB_SB();
            first = false;
        }
        float* crow = p.C + (size_t)my_row * p.ldc + 4 * lg;
        for (int g = 0; g < G; ++g) {
            const char* sa = BF_CUR_SLOT();
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            BF_W1_SLOT(sa, a0, a1, xh)
            if (my_row < M) TB_STORE_SLOT(crow, bs, g, a0, a1)
            BF_END_SLOT()
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#undef BF_W1_SLOT
#undef BF_END_SLOT
#undef BF_RD
#undef BF_CUR_SLOT

struct Bf16Mode {
    using FfnArgs = FfnBf16Args;
    using RowsArgs = RowsBf16Args;
    static constexpr int IMG = TAIL_IMG_BF16, SLOT = BF_SLOT, NSLOT = BF_NSLOT, PIECES = 1;
    static constexpr const char* NAME = "bf16";
    static constexpr bool HAS_PRE = true;
    template <bool PROJ, bool QKV, bool PRE> static constexpr auto ffn_kernel() { return &ffn_bf16_kernel<PROJ, QKV, PRE>; }
    static constexpr auto rows_kernel() { return &rows256_bf16_kernel; }
};
extern const TailMode TAIL_MODE_BF16 = tail_mode<Bf16Mode>();

}  // namespace cone
