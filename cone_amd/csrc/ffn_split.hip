// Fused feed-forward block (ffn.hip's computation: out = LayerNorm(x + W2 relu(W1 x + b1) + b2)) with every fp32
// product carried by the bf16 matrix cores as SIX partial products of three-piece operands:
//     x = xh + xm + xl,  w = wh + wm + wl   (bf16 pieces: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): exact, 24 bits)
//     x w ~= xl wh + xh wl + xm wm + xh wm + xm wh + xh wh        (the three dropped products are <= 2^-24 |x w|)
// accumulated in fp32 by v_mfma_f32_16x16x32_bf16.  Measured on this part (tools/probe/split_bf16_probe.hip, K = 256 and
// 1024, against float64): max |error| / sum |a b| = 1.5e-7 .. 2.4e-7, the exact-fp32 v_mfma_f32_16x16x4_f32 chain of
// ffn.hip: 2.0e-7 .. 2.1e-7 -- the same accuracy, at 16 / 6 = 2.7x the matrix-core rate.  OPT-IN (cone_model_set_option
// "split_bf16"): the default path stays on the fp32 MFMA.
//
// Orientation and operand maps are those of ffn.hip (a wave owns 16 token rows = the MFMA column index; accumulators feed
// the next product without lane movement), on v_mfma_f32_16x16x32_bf16: lane (li = l % 16, lg = l / 16) holds
// A[row li][k = 8 lg + j], B[k = 8 lg + j][col li], j = 0 .. 7, and D[row 4 lg + r][col li], r = 0 .. 3.  The k index is
// permuted identically on both operands so that operands come out of the registers they already live in:
//   GEMM1 (K = 256 channels, step s = 32 channels): k slot (lg, j) <-> channel 32 s + 16 (j / 4) + 4 lg + j % 4, i.e. the
//          two float4 x[token][32 s + 4 lg ..] and x[token][32 s + 16 + 4 lg ..] -- which are also the accumulator
//          layout of the output (channel 16 t + 4 lg + r), so the residual is rebuilt from the very same registers;
//   GEMM2 (K = 32 hidden units of a chunk): k slot (lg, j) <-> unit 16 (j / 4) + 4 lg + j % 4 = accumulator register
//          j % 4 of the chunk's GEMM1 tile j / 4.
// Weights are static: they are split and laid out ONCE (cone_ffn_split_pack) in exactly the order the kernel reads them,
// as 1-KiB operand slabs [lg][li][8 bf16] (a wave's ds_read_b128 of a slab is linear in the lane index: conflict-free),
// 48 slabs = 48 KiB per ring slot: slot 2 c = W1 image of hidden chunk c ([tile 2][step 8][piece 3] slabs), slot
// 2 c + 1 = W2 image ([channel tile 16][piece 3]).  The stream is linear, so a piece's LDS-DMA source is base + lane * 16.
//
// This file keeps what is the split form's own: the ring (3 slots of 48 KiB indexed by sb + g, 6 pieces per wave and slot,
// vmcnt(SP_NPIECE)), the operand preparation (sp_split8), the six-product unit (SP_MM6) and the residual rebuilt from the
// pieces.  The steps it shares with ffn_bf16.hip, the pack kernel and the host side are in tail_bf16_common.h.
#include <mutex>

#include "tail_bf16_common.h"

namespace cone {

constexpr int SP_SLOT = 48 * 1024;                 // bytes per ring slot
constexpr int SP_NSLOT = 3;
constexpr int SP_NPIECE = 6;                       // 1-KiB LDS-DMA pieces per wave per slot (48 / 8)

// eight fp32 values (two float4) -> three 8-element bf16 operands
__device__ __forceinline__ void sp_split8(const tb_f4& v0, const tb_f4& v1, tb_s8& h, tb_s8& m, tb_s8& l) {
    unsigned a[4], b[4], c[4];
    tb_split2(v0[0], v0[1], a[0], b[0], c[0]);
    tb_split2(v0[2], v0[3], a[1], b[1], c[1]);
    tb_split2(v1[0], v1[1], a[2], b[2], c[2]);
    tb_split2(v1[2], v1[3], a[3], b[3], c[3]);
    const tb_u4 uh = {a[0], a[1], a[2], a[3]}, um = {b[0], b[1], b[2], b[3]}, ul = {c[0], c[1], c[2], c[3]};
    h = __builtin_bit_cast(tb_s8, uh); m = __builtin_bit_cast(tb_s8, um); l = __builtin_bit_cast(tb_s8, ul);
}

// the six partial products of one (weight fragment triple, activation triple), small terms first
#define SP_MM6(acc, wh, wm, wl, xh, xm, xl) \
    {                                        \
        TB_MFMA(acc, wl, xh);                \
        TB_MFMA(acc, wh, xl);                \
        TB_MFMA(acc, wm, xm);                \
        TB_MFMA(acc, wm, xh);                \
        TB_MFMA(acc, wh, xm);                \
        TB_MFMA(acc, wh, xh);                \
    }

// a finished GEMM1 tile: + b1, ReLU, and the three piece pairs of its two element pairs
#define SP_BIAS_RELU_SPLIT(a, b1p, h, m, l)                                \
    {                                                                      \
        a += *reinterpret_cast<const tb_f4*>(b1p);                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) a[r] = fmaxf(a[r], 0.f); \
        tb_split2(a[0], a[1], h[0], m[0], l[0]);                           \
        tb_split2(a[2], a[3], h[1], m[1], l[1]);                           \
    }

template <bool PROJ, bool QKV>
__global__ __launch_bounds__(512, 2) void ffn_split_kernel(FfnSplitArgs p) {
    extern __shared__ __attribute__((aligned(16))) char sp_smem[];
    float* b1s = reinterpret_cast<float*>(sp_smem + SP_NSLOT * SP_SLOT);
    TB_PROLOGUE(p);
    const int ff = p.ff, nc = ff >> 5;            // 32-unit hidden chunks
    constexpr int NP = PROJ ? 8 : 0;              // leading slots of the output projection (32 channels each)
    const int NQ = QKV ? p.n_qkv >> 5 : 0;        // trailing slots of the next layer's q | k | v projection
    const int G = NP + 2 * nc + NQ;               // ring slots per tile

    float* prm = b1s + ff;                        // the parameter rows (PRM_*)
    float* qbs = prm + PRM_QB;                    // q | k | v bias
    TB_STAGE_PARAMS(p, b1s, prm, ff, true);

    // LDS-DMA: piece i of slot g (of the current tile; g >= G: the next tile's first slots, the same weights) = 1 KiB
    // at image offset g * 48 KiB + (6 wave + i) KiB, lane * 16 B inside it; destination = the same offset in ring slot
    // (sb + g) % 3.
    int sb = 0;
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    const char* woimg = reinterpret_cast<const char*>(p.Woimg);
    const char* qimg = reinterpret_cast<const char*>(p.Qimg);
    auto stream_piece = [&](int g, int i) {
        const int gg = g < G ? g : g - G;
        char* dstp = sp_smem + ((sb + g) % SP_NSLOT) * SP_SLOT + (wave * SP_NPIECE + i) * 1024;
        const char* ub = TB_SLOT_IMAGE(woimg, wimg, qimg, gg, SP_SLOT) + (size_t)(wave * SP_NPIECE + i) * 1024;
        asm volatile("" : "+s"(ub));
        TB_GLDS16(ub + (unsigned)(lane * 16), dstp);
    };
#define SP_SLOT_OF(g) (sp_smem + ((sb + (g)) % SP_NSLOT) * SP_SLOT)
#define SP_RD(slot, slab) (*reinterpret_cast<const tb_s8*>((slot) + (slab) * 1024 + lane * 16))
    // end of a slot: the next slot has landed (all but the pieces issued last, which belong to the slot after it), and
    // every wave is done with the slot that the next pieces will overwrite
#define SP_END_SLOT()                                                             \
    {                                                                             \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SP_NPIECE) : "memory");          \
        __builtin_amdgcn_s_barrier();                                             \
    }
    // A W1-form slot (ring slot g; [tile 2][step 8][piece 3] slabs) against the rows' pieces xh / xm / xl: 16 units of
    // (3 fragments, 6 MFMAs), a0 = output units 0 .. 15, a1 = 16 .. 31 of the slot.  The fragments of unit u + 1 are
    // requested ahead of the MFMAs of unit u (the empty asm is where the wait for them lands: after those MFMAs, before
    // the next request); the odd units issue the six LDS-DMA pieces of slot g + 2; AT_UNIT_9 runs once tile 0 is complete.
#define SP_W1_SLOT(g, a0, a1, AT_UNIT_9)                                                                              \
    {                                                                                                                 \
        const char* sa = SP_SLOT_OF(g);                                                                               \
        f[0][0] = SP_RD(sa, 0); f[0][1] = SP_RD(sa, 1); f[0][2] = SP_RD(sa, 2);                                       \
        _Pragma("unroll") for (int u = 0; u < 16; ++u) {                                                              \
            TB_SB();                                                                                                  \
            asm volatile("" : "+v"(f[u & 1][0]), "+v"(f[u & 1][1]), "+v"(f[u & 1][2]));                               \
            TB_SB();                                                                                                  \
            if (u < 15) {                                                                                             \
                f[(u + 1) & 1][0] = SP_RD(sa, (u + 1) * 3 + 0); f[(u + 1) & 1][1] = SP_RD(sa, (u + 1) * 3 + 1);       \
                f[(u + 1) & 1][2] = SP_RD(sa, (u + 1) * 3 + 2);                                                       \
            }                                                                                                         \
            TB_SB();                                                                                                  \
            if (u < 8) { SP_MM6(a0, f[u & 1][0], f[u & 1][1], f[u & 1][2], xh[u & 7], xm[u & 7], xl[u & 7]) }         \
            else { SP_MM6(a1, f[u & 1][0], f[u & 1][1], f[u & 1][2], xh[u & 7], xm[u & 7], xl[u & 7]) }               \
            if ((u & 1) && (u >> 1) < SP_NPIECE) stream_piece((g) + 2, u >> 1);                                       \
            if (u == 9) { AT_UNIT_9; }                                                                                \
        }                                                                                                             \
        TB_SB();                                                                                                      \
    }

#pragma unroll
    for (int i = 0; i < SP_NPIECE; ++i) stream_piece(0, i);
#pragma unroll
    for (int i = 0; i < SP_NPIECE; ++i) stream_piece(1, i);

    // a tile's rows (PROJ: the attention rows = B operand of the projection, else the block input) are requested from
    // the previous tile's epilogue -- once its operand pieces are dead, ahead of its stores -- and split at the tile's top
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
    // split once: xh / xm / xl [s] = B operand of GEMM1's step s (channels 32 s + 16 (j / 4) + 4 lg + j % 4)
    tb_s8 xh[8], xm[8], xl[8];
    const size_t ld_row = TB_LD_ROW(my_row);
#pragma unroll
    for (int s = 0; s < 8; ++s) sp_split8(xr[2 * s], xr[2 * s + 1], xh[s], xm[s], xl[s]);
    if (first) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SP_NPIECE) : "memory");
        __syncthreads();
        first = false;
    }
    tb_s8 f[2][3];                                  // ping-pong fragment sets (statically indexed: loops are unrolled)
    if (PROJ) {
        // ---- attention output projection: slot g = channels [32 g, 32 g + 32) of A Wo^T
        tb_f4 x1[16];
#pragma unroll
        for (int g = 0; g < NP; ++g) {
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            SP_W1_SLOT(g, a0, a1, )
            x1[2 * g] = a0; x1[2 * g + 1] = a1;
            SP_END_SLOT()
        }
        // + bo + residual rows, LayerNorm: the block input, split for GEMM1 (the attention pieces are dead)
        TB_ADD_RESIDUAL(x1, p, ld_row, prm)
        TB_LN_MOMENTS(x1, true, mu, rs)
#pragma unroll
        for (int t = 0; t < 16; ++t) TB_LN_APPLY(x1[t], x1[t][r], rs, prm, PRM_PG, PRM_PB, t)
#pragma unroll
        for (int s = 0; s < 8; ++s) sp_split8(x1[2 * s], x1[2 * s + 1], xh[s], xm[s], xl[s]);
    }
    tb_f4 y[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] = tb_f4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < nc; ++c) {
        // ---- GEMM1: the chunk's two 16-unit tiles over the 256 channels (slot 2 c), tile by tile: bias + ReLU + split of
        // tile 0 run under tile 1's MFMAs
        tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        unsigned p0h[2], p0m[2], p0l[2];
        SP_W1_SLOT(NP + 2 * c, a0, a1, SP_BIAS_RELU_SPLIT(a0, b1s + 32 * c + 4 * lg, p0h, p0m, p0l))
        SP_END_SLOT()
        // ---- GEMM2: all 256 output channels over the chunk's 32 hidden units (slot 2 c + 1: [channel tile][piece]); its
        // first fragments are requested ahead of tile 1's bias + ReLU + split
        const char* sw = SP_SLOT_OF(NP + 2 * c + 1);
        f[0][0] = SP_RD(sw, 0); f[0][1] = SP_RD(sw, 1); f[0][2] = SP_RD(sw, 2);
        TB_SB();
        // the B operand of GEMM2 (k slot (lg, j) <-> unit 16 (j / 4) + 4 lg + j % 4): tile 0's pieces, then tile 1's
        tb_s8 hh, hm, hl;
        {
            unsigned p1h[2], p1m[2], p1l[2];
            SP_BIAS_RELU_SPLIT(a1, b1s + 32 * c + 16 + 4 * lg, p1h, p1m, p1l)
            hh = __builtin_bit_cast(tb_s8, tb_u4{p0h[0], p0h[1], p1h[0], p1h[1]});
            hm = __builtin_bit_cast(tb_s8, tb_u4{p0m[0], p0m[1], p1m[0], p1m[1]});
            hl = __builtin_bit_cast(tb_s8, tb_u4{p0l[0], p0l[1], p1l[0], p1l[1]});
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            TB_SB();
            asm volatile("" : "+v"(f[t & 1][0]), "+v"(f[t & 1][1]), "+v"(f[t & 1][2]));
            TB_SB();
            if (t < 15) {
                f[(t + 1) & 1][0] = SP_RD(sw, (t + 1) * 3 + 0); f[(t + 1) & 1][1] = SP_RD(sw, (t + 1) * 3 + 1);
                f[(t + 1) & 1][2] = SP_RD(sw, (t + 1) * 3 + 2);
            }
            TB_SB();
            SP_MM6(y[t], f[t & 1][0], f[t & 1][1], f[t & 1][2], hh, hm, hl)
            if ((t & 1) && (t >> 1) < SP_NPIECE) stream_piece(NP + 2 * c + 3, t >> 1);
        }
        TB_SB();
        SP_END_SLOT()
    }
    // ---- epilogue: + b2 + residual (x = xh + xm + xl exactly, in the accumulator layout), LayerNorm, store
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        // (opaque here: otherwise the unpacked halves computed by the split at the tile's top are kept alive across the
        // whole tile -- 80 spilled registers -- instead of being re-derived by two shifts)
        asm volatile("" : "+v"(xh[s]), "+v"(xm[s]), "+v"(xl[s]));
        const tb_u4 uh = __builtin_bit_cast(tb_u4, xh[s]), um = __builtin_bit_cast(tb_u4, xm[s]), ul = __builtin_bit_cast(tb_u4, xl[s]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {           // pair e: elements 2 e, 2 e + 1 of the step = (tile 2 s + e / 2, r = 2 (e % 2) ..)
            const float x0 = (tb_lo(uh[e]) + tb_lo(um[e])) + tb_lo(ul[e]);
            const float x1 = (tb_hi(uh[e]) + tb_hi(um[e])) + tb_hi(ul[e]);
            y[2 * s + (e >> 1)][2 * (e & 1)] += x0;
            y[2 * s + (e >> 1)][2 * (e & 1) + 1] += x1;
        }
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] += *reinterpret_cast<const tb_f4*>(prm + PRM_B2 + 16 * t + 4 * lg);
    TB_SB();
    // the operand pieces are dead: the next tile's rows travel under the LayerNorm and the stores (after the last tile a
    // valid tile is simply re-read, so that the register tile has one definition per iteration)
    load_rows(tile + (int)gridDim.x < n_tiles ? tile + (int)gridDim.x : tile);
    TB_SB();
    TB_LN_MOMENTS(y, true, mean, rstd)
    if (my_row < M) {
        float* op = p.OUT + (size_t)my_row * p.ldo + 4 * lg;
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
    if (QKV) {
        // ---- the next layer's q | k | v projection of these rows, straight from the registers: split once more, then
        // NQ slots of 32 output channels each, stored from the accumulators
#pragma unroll
        for (int s = 0; s < 8; ++s) sp_split8(y[2 * s], y[2 * s + 1], xh[s], xm[s], xl[s]);
        float* qrow = p.QKV + (size_t)my_row * p.ldq + 4 * lg;
        for (int g = 0; g < NQ; ++g) {
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            SP_W1_SLOT(NP + 2 * nc + g, a0, a1, )
            if (my_row < M) TB_STORE_SLOT(qrow, qbs, g, a0, a1)
            SP_END_SLOT()
        }
    }
    sb = (sb + G) % SP_NSLOT;
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------------------------
// C = X W^T + bias for K = 256 and any N % 32 == 0 (the q | k | v projection of the later encoder layers) with the same
// split operands: the projection phase of the kernel above on its own -- a wave's 16 x 256 rows stay in registers as bf16
// pieces, W streams as N / 32 W1-form slots, every slot's 32 output channels are stored straight from the accumulators
// (lane = token, 16 B = 4 consecutive channels).
__global__ __launch_bounds__(512, 2) void rows256_split_kernel(RowsSplitArgs p) {
    extern __shared__ __attribute__((aligned(16))) char sp_smem[];
    float* bs = reinterpret_cast<float*>(sp_smem + SP_NSLOT * SP_SLOT);
    TB_PROLOGUE(p);
    const int G = p.N >> 5;                         // ring slots per tile
    TB_STAGE_BIAS(bs, p.bias, p.N);
    int sb = 0;
    const char* wimg = reinterpret_cast<const char*>(p.Wimg);
    auto stream_piece = [&](int g, int i) {
        int gg = g;
        while (gg >= G) gg -= G;                    // the next tile's first slots (G may be 1 or 2)
        char* dstp = sp_smem + ((sb + g) % SP_NSLOT) * SP_SLOT + (wave * SP_NPIECE + i) * 1024;
        const char* ub = wimg + (size_t)gg * SP_SLOT + (size_t)(wave * SP_NPIECE + i) * 1024;
        asm volatile("" : "+s"(ub));
        TB_GLDS16(ub + (unsigned)(lane * 16), dstp);
    };
#pragma unroll
    for (int i = 0; i < SP_NPIECE; ++i) stream_piece(0, i);
#pragma unroll
    for (int i = 0; i < SP_NPIECE; ++i) stream_piece(1, i);
    bool first = true;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int my_row = TB_ROW_OF(tile);
        tb_s8 xh[8], xm[8], xl[8];
        {
            tb_f4 xr[16];
            TB_LOAD_ROW(xr, p.X + TB_LD_ROW(my_row) * p.ldx + 4 * lg)
#pragma unroll
            for (int s = 0; s < 8; ++s) sp_split8(xr[2 * s], xr[2 * s + 1], xh[s], xm[s], xl[s]);
        }
        if (first) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(SP_NPIECE) : "memory");
            __syncthreads();
            first = false;
        }
        float* crow = p.C + (size_t)my_row * p.ldc + 4 * lg;
        tb_s8 f[2][3];
        for (int g = 0; g < G; ++g) {
            tb_f4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            SP_W1_SLOT(g, a0, a1, )
            if (my_row < M) TB_STORE_SLOT(crow, bs, g, a0, a1)
            SP_END_SLOT()
        }
        sb = (sb + G) % SP_NSLOT;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#undef SP_MM6
#undef SP_BIAS_RELU_SPLIT
#undef SP_W1_SLOT
#undef SP_END_SLOT
#undef SP_RD
#undef SP_SLOT_OF

struct SplitMode {
    using FfnArgs = FfnSplitArgs;
    using RowsArgs = RowsSplitArgs;
    static constexpr int IMG = TAIL_IMG_SPLIT, SLOT = SP_SLOT, NSLOT = SP_NSLOT, PIECES = 3;
    static constexpr const char* NAME = "split-bf16";
    static constexpr bool HAS_PRE = false;
    template <bool PROJ, bool QKV, bool PRE> static constexpr auto ffn_kernel() { return &ffn_split_kernel<PROJ, QKV>; }
    static constexpr auto rows_kernel() { return &rows256_split_kernel; }
};
extern const TailMode TAIL_MODE_SPLIT = tail_mode<SplitMode>();

}  // namespace cone
