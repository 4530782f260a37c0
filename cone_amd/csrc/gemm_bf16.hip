// The general path's opt-in bf16 row GEMM (option general_bf16): launch_gemm's computation for the GemmArgs subset that
// forward_general uses, with BOTH operands rounded once to bf16 (round to nearest even), one v_mfma_f32_16x16x32_bf16 per
// operand pair, fp32 accumulation; bias, ReLU and the residual (never rounded) in fp32.  Plain bf16 matrix arithmetic: NOT
// fp32-accurate.
//
//   C[m][n] = sum_k bf16(A[m][k] (+ A2[a2_mod ? m % a2_mod : m][k], added in fp32 first)) * bf16(W[n][k])
//             + bias[n],  then ReLU (EPI_RELU),  then + R[r_mod ? m % r_mod : m][n] (EPI_RESIDUAL)
//
// Any N % 16 == 0, any K % 32 == 0 up to 2048, any ldc / lda / ldr % 4 == 0, a device-side row count.  No LayerNorm
// epilogue, no second output, no row offset: refused by name.
//
// ONE tile form, whatever the shape (so a row's bits never depend on M or on the batch it rides in): a workgroup of four
// waves owns 128 token rows x 128 output channels, wave (wm, wn) the 64 x 64 quadrant as 4 x 4 MFMA tiles (64 accumulator
// registers).  Orientation and operand maps are those of tail_bf16_common.h: the MFMA's A operand is the WEIGHT fragment
// (row = output channel), its B operand the activation fragment (column = token li = lane % 16), k slot (lg = lane / 16, j)
// <-> channel 32 t + 8 lg + j, so a lane's fragment is one 16-byte access and its four accumulator registers are four
// consecutive output channels 4 lg + r of token li: one float4 store.
//
// Per k step of 32 channels the workgroup stages, through registers, into a double-buffered LDS pair (2 x 16 KiB):
//   the activations: 128 rows x 32 fp32 channels (+ the A2 rows), summed in fp32, rounded IN FLIGHT (v_cvt_pk_bf16_f32) and
//     written as eight lane-linear 1-KiB slabs (one per 16 tokens) -- no bf16 copy of an activation ever reaches memory;
//   the weights: eight 1-KiB slabs (one per 16 output channels) copied as they lie in the weight image.
// The next step's global loads are issued ahead of the current step's 16 MFMAs and written to the other buffer behind them:
// one barrier per step.  Every LDS access is a lane-linear 16-byte one (conflict-free).  Rows past the row count re-read
// its last row and are never stored; weight rows past N are zeros in the image and never stored.
//
// Weight image (gemm_bf16_image_bytes(N, K) = roundup(N, 128) * K * 2 bytes; built once per model): slab ((nb * K / 32 + t) * 8
// + nt) holds, at lane l = 16 lg + li, the 8 bf16 of W[128 nb + 16 nt + li][32 t + 8 lg .. + 8] -- a workgroup's 8 KiB of a
// k step are contiguous.
#include "tail_bf16_common.h"

namespace cone {

constexpr int GB_BM = 128, GB_BN = 128, GB_BK = 32;
constexpr int GB_STEP_SLABS = GB_BN / 16;                   // weight slabs of one (channel block, k step)
constexpr int GB_MAX_K = 2048;
static_assert(GB_BM / 16 == 8 && GB_STEP_SLABS == 8 && TB_SLAB == 16 * GB_BK * 2, "eight 1-KiB slabs per operand and k step");

struct GemmBf16Args {
    const float* A; int lda;
    const float* A2; int lda2; int a2_mod;
    const void* Wimg;
    const float* bias;
    const float* R; int ldr; int r_mod;
    float* C; int ldc;
    int M; const int* M_dev;
    int N, K;
    int relu;
};

size_t gemm_bf16_image_bytes(int N, int K) {
    if (N < 16 || N % 16 || K < GB_BK || K % GB_BK || K > GB_MAX_K) return 0;
    return (size_t)((N + GB_BN - 1) / GB_BN) * (K / GB_BK) * GB_STEP_SLABS * TB_SLAB;
}

// one thread per 16-byte fragment of the image
__global__ __launch_bounds__(256) void gemm_bf16_pack_kernel(const float* __restrict__ W, int ldw, int N, int K,
                                                             unsigned* __restrict__ img) {
    const int KT = K / GB_BK;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)((N + GB_BN - 1) / GB_BN) * KT * GB_STEP_SLABS * 64;
    if (idx >= total) return;
    const int l = (int)(idx & 63), li = l & 15, lg = l >> 4;
    const size_t slab = idx >> 6;
    const int nt = (int)(slab % GB_STEP_SLABS);
    const int t = (int)((slab / GB_STEP_SLABS) % KT);
    const int nb = (int)(slab / ((size_t)GB_STEP_SLABS * KT));
    const int n = GB_BN * nb + 16 * nt + li;
    tb_u4 v = {0u, 0u, 0u, 0u};
    if (n < N) {
        const float* src = W + (size_t)n * ldw + GB_BK * t + 8 * lg;
        for (int e = 0; e < 4; ++e) v[e] = tb_pk(src[2 * e], src[2 * e + 1]);
    }
    reinterpret_cast<tb_u4*>(img)[idx] = v;
}

template <bool HAS_A2>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const GemmBf16Args p) {
    __shared__ __attribute__((aligned(16))) char lds[2][2][GB_STEP_SLABS * TB_SLAB];     // [buffer][activations, weights]
    int M = p.M;
    if (p.M_dev) { const int md = *p.M_dev; M = md < M ? md : M; }
    const int NB = (p.N + GB_BN - 1) / GB_BN, nb = blockIdx.x % NB;
    const int m0 = (blockIdx.x / NB) * GB_BM, n0 = nb * GB_BN;
    if (m0 >= M) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 15, lg = lane >> 4;
    const int KT = p.K / GB_BK;

    // staging: item i = tid + 256 h (h < 2) is (row i / 4 of the tile, channels 8 (i % 4) .. + 8 of the k step)
    const float* ap[2]; const float* a2p[2]; int sdst[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = tid + 256 * h, r = i >> 2, g = i & 3;
        const int row = m0 + r < M ? m0 + r : M - 1;
        ap[h] = p.A + (size_t)row * p.lda + 8 * g;
        if (HAS_A2) a2p[h] = p.A2 + (size_t)(p.a2_mod ? row % p.a2_mod : row) * p.lda2 + 8 * g;
        sdst[h] = (r >> 4) * TB_SLAB + (16 * g + (r & 15)) * 16;
    }
    const char* wsrc = (const char*)p.Wimg + (size_t)nb * KT * (GB_STEP_SLABS * TB_SLAB) + tid * 16;

    tb_f4 xa[2][2]; tb_u4 xw[2];
    auto load_step = [&](int t) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* s = ap[h] + GB_BK * t;
            xa[h][0] = *reinterpret_cast<const tb_f4*>(s);
            xa[h][1] = *reinterpret_cast<const tb_f4*>(s + 4);
            if (HAS_A2) {
                const float* s2 = a2p[h] + GB_BK * t;
                xa[h][0] += *reinterpret_cast<const tb_f4*>(s2);
                xa[h][1] += *reinterpret_cast<const tb_f4*>(s2 + 4);
            }
            xw[h] = *reinterpret_cast<const tb_u4*>(wsrc + (size_t)t * (GB_STEP_SLABS * TB_SLAB) + 4096 * h);
        }
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const tb_u4 v = {tb_pk(xa[h][0][0], xa[h][0][1]), tb_pk(xa[h][0][2], xa[h][0][3]),
                             tb_pk(xa[h][1][0], xa[h][1][1]), tb_pk(xa[h][1][2], xa[h][1][3])};
            *reinterpret_cast<tb_u4*>(lds[buf][0] + sdst[h]) = v;
            *reinterpret_cast<tb_u4*>(lds[buf][1] + tid * 16 + 4096 * h) = xw[h];
        }
    };

    tb_f4 acc[4][4];                        // [channel tile][token tile]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = tb_f4{0.f, 0.f, 0.f, 0.f};
    const bool live = n0 + 64 * wn < p.N;   // (wave-uniform) the quadrant has channels below N

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int t = 0; t < KT; ++t) {
        const int buf = t & 1;
        if (t + 1 < KT) load_step(t + 1);   // in flight under this step's MFMAs
        if (live) {
            tb_s8 wf[4], xf[4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
                wf[a] = *reinterpret_cast<const tb_s8*>(lds[buf][1] + (4 * wn + a) * TB_SLAB + lane * 16);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                xf[b] = *reinterpret_cast<const tb_s8*>(lds[buf][0] + (4 * wm + b) * TB_SLAB + lane * 16);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) TB_MFMA(acc[a][b], wf[a], xf[b]);
        }
        if (t + 1 < KT) store_step(buf ^ 1);    // (its last readers passed the barrier that ended step t - 1)
        __syncthreads();
    }
    if (!live) return;

    // acc[a][b][r] = C[token m0 + 64 wm + 16 b + li][channel n0 + 64 wn + 16 a + 4 lg + r]
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n = n0 + 64 * wn + 16 * a + 4 * lg;
        if (n >= p.N) continue;             // (N % 16 == 0: the whole 16-channel tile)
        const tb_f4 bv = p.bias ? *reinterpret_cast<const tb_f4*>(p.bias + n) : tb_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int m = m0 + 64 * wm + 16 * b + li;
            if (m >= M) continue;
            tb_f4 v = acc[a][b] + bv;
            if (p.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            if (p.R) v += *reinterpret_cast<const tb_f4*>(p.R + (size_t)(p.r_mod ? m % p.r_mod : m) * p.ldr + n);
            *reinterpret_cast<tb_f4*>(p.C + (size_t)m * p.ldc + n) = v;
        }
    }
}

int launch_gemm_bf16_pack(const float* W, int ldw, int N, int K, void* img, hipStream_t s) {
    const size_t bytes = gemm_bf16_image_bytes(N, K);
    CONE_REQUIRE(bytes, "bf16 gemm weight image: N=%d must be a multiple of 16 and K=%d a multiple of %d up to %d", N, K, GB_BK,
                 GB_MAX_K);
    CONE_REQUIRE(W && img && ldw >= K, "bf16 gemm weight image: bad argument");
    hipLaunchKernelGGL(gemm_bf16_pack_kernel, dim3((unsigned)((bytes / 16 + 255) / 256)), dim3(256), 0, s, W, ldw, N, K,
                       reinterpret_cast<unsigned*>(img));
    CONE_LAUNCH_CHECK();
    return 0;
}

int launch_gemm_bf16(const GemmArgs& a, const void* w_img, hipStream_t s) {
    CONE_REQUIRE(!(a.flags & EPI_LN) && !a.ln_g && !a.ln_b, "bf16 gemm: the LayerNorm epilogue (EPI_LN) is not supported");
    CONE_REQUIRE(!a.C2 && !a.ADD, "bf16 gemm: a second output (C2 / ADD) is not supported");
    CONE_REQUIRE(a.m_off == 0, "bf16 gemm: a row offset (m_off) is not supported");
    CONE_REQUIRE(gemm_bf16_image_bytes(a.N, a.K), "bf16 gemm: N=%d must be a multiple of 16 and K=%d a multiple of %d up to %d",
                 a.N, a.K, GB_BK, GB_MAX_K);
    CONE_REQUIRE(a.A && a.C && w_img, "bf16 gemm: null argument");
    CONE_REQUIRE(a.lda % 4 == 0 && a.ldc % 4 == 0 && a.lda >= a.K && a.ldc >= a.N, "bf16 gemm: lda / ldc must be multiples of 4");
    CONE_REQUIRE(!a.A2 || (a.lda2 % 4 == 0 && a.lda2 >= a.K && a.a2_mod >= 0), "bf16 gemm: bad A2 operand");
    CONE_REQUIRE(!(a.flags & EPI_RESIDUAL) || (a.R && a.ldr % 4 == 0 && a.ldr >= a.N && a.r_mod >= 0),
                 "bf16 gemm: residual flag without R");
    CONE_REQUIRE((((uintptr_t)a.A | (uintptr_t)a.A2 | (uintptr_t)a.C | (uintptr_t)a.bias | (uintptr_t)a.R | (uintptr_t)w_img) & 15) == 0,
                 "bf16 gemm: operands must be 16-byte aligned");
    if (a.M <= 0) return 0;
    GemmBf16Args p{};
    p.A = a.A; p.lda = a.lda; p.A2 = a.A2; p.lda2 = a.lda2; p.a2_mod = a.a2_mod; p.Wimg = w_img; p.bias = a.bias;
    p.R = (a.flags & EPI_RESIDUAL) ? a.R : nullptr; p.ldr = a.ldr; p.r_mod = a.r_mod;
    p.C = a.C; p.ldc = a.ldc; p.M = a.M; p.M_dev = a.M_dev; p.N = a.N; p.K = a.K; p.relu = (a.flags & EPI_RELU) != 0;
    // channel blocks fastest: the workgroups that share a tile's activation rows are dispatched together
    const dim3 grid((unsigned)((a.N + GB_BN - 1) / GB_BN) * (unsigned)((a.M + GB_BM - 1) / GB_BM));
    if (a.A2) hipLaunchKernelGGL(gemm_bf16_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gemm_bf16_kernel<false>, grid, dim3(256), 0, s, p);
    CONE_LAUNCH_CHECK();
    return 0;
}

}  // namespace cone
