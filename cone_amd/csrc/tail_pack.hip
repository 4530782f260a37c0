// Packed fp32 weight streams of the two weight-ring kernels (ffn.hip's row kernel, gemm_tall.hip), built once per model handle.
//
// The ring consumes 32-KiB chunks: 32 slabs of [16 rows][16 floats], each fetched as ONE LDS-DMA piece in which lane l brings
// the 16 B of (row = l / 4, chunk = (l % 4) ^ tf_swz16(l / 4)) of the slab.  From the row-major matrices that is a gather of
// 16 row segments 1 KiB (W1, Wo, Wq) or 4 ff B (W2) apart with the swizzle applied on the source address, redone for every
// piece of every tile on every CU although the weights never change.  The image resolves both once:
//     image[chunk g][slab s][lane l][4 floats] = the 16 B that piece s of chunk g brings to lane l,
// so that a piece's source is image + g * 32 KiB + s * 1 KiB + l * 16 -- one linear run per tile, in the order it is walked:
//     projection format (Wo, Wq, the tall GEMM's W; 32 output channels per chunk):
//         slab s of chunk c = W[32 c + 16 (s / 16) + row][16 (s % 16) + 4 ch ..]
//     feed-forward format (16 hidden units per chunk):
//         slab s < 16  = W1[16 c + row][16 s + 4 ch ..]            slab 16 + t = W2[16 t + row][16 c + 4 ch ..]
// The LDS contents are byte for byte what the gathering stream leaves, so the kernels' results do not depend on the stream form.
#include <atomic>

#include "tail_f32_common.h"

namespace cone {

// one thread per 16 B of the image; n16 = its size in 16-B units.  np / nf / nq = chunks of Wo, of the feed-forward block, of Wq
__global__ __launch_bounds__(256) void f32_pack_kernel(const float* __restrict__ Wo, const float* __restrict__ W1,
                                                       const float* __restrict__ W2, const float* __restrict__ Wq, int np, int nf,
                                                       int nq, int ff, f32x4* __restrict__ img, int n16) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n16) return;
    const int l = idx & 63, s = (idx >> 6) & 31, g = idx >> 11;
    const int row = l >> 2, ch = (l & 3) ^ tf_swz16(row);
    const float* src;
    if (g < np || g >= np + nf) {
        const float* W = g < np ? Wo : Wq;
        const int c = g < np ? g : g - np - nf;
        src = W + (size_t)(32 * c + 16 * (s >> 4) + row) * 256 + 16 * (s & 15) + 4 * ch;
    } else {
        const int c = g - np;
        src = s < 16 ? W1 + (size_t)(16 * c + row) * 256 + 16 * s + 4 * ch
                     : W2 + (size_t)(16 * (s - 16) + row) * ff + 16 * c + 4 * ch;
    }
    img[idx] = *reinterpret_cast<const f32x4*>(src);
}

static std::atomic<long> g_packed_launches[2];
void f32_packed_note(int which) { g_packed_launches[which & 1].fetch_add(1, std::memory_order_relaxed); }
long f32_packed_launches(int which) { return g_packed_launches[which & 1].load(std::memory_order_relaxed); }

size_t f32_pack_tail_bytes(int ff, bool proj, int n_qkv) {
    if (!ffn_fused_supported(ff) || n_qkv < 0 || n_qkv % 32 != 0) return 0;
    return (size_t)((proj ? 8 : 0) + ff / 16 + n_qkv / 32) * F32_PACK_CHUNK_BYTES;
}
size_t f32_pack_rows_bytes(int N) { return N >= 32 && N % 32 == 0 ? (size_t)(N / 32) * F32_PACK_CHUNK_BYTES : 0; }

static int pack_launch(const float* Wo, const float* W1, const float* W2, const float* Wq, int np, int nf, int nq, int ff,
                       void* img, hipStream_t s) {
    const int n16 = (np + nf + nq) * (int)(F32_PACK_CHUNK_BYTES / 16);
    hipLaunchKernelGGL(f32_pack_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, Wo, W1, W2, Wq, np, nf, nq, ff,
                       (f32x4*)img, n16);
    CONE_LAUNCH_CHECK();
    return 0;
}

int launch_f32_pack_tail(const float* Wo, const float* W1, const float* W2, int ff, const float* Wq, int n_qkv, void* img,
                         hipStream_t s) {
    CONE_REQUIRE(ffn_fused_supported(ff), "fp32 tail image: dim_feedforward=%d unsupported", ff);
    CONE_REQUIRE(W1 && W2 && img, "fp32 tail image: null argument");
    CONE_REQUIRE(!Wq || (n_qkv >= 32 && n_qkv % 32 == 0 && n_qkv <= 8192), "fp32 tail image: q|k|v width %d not a multiple of 32", n_qkv);
    return pack_launch(Wo, W1, W2, Wq, Wo ? 8 : 0, ff / 16, Wq ? n_qkv / 32 : 0, ff, img, s);
}

int launch_f32_pack_rows(const float* W, int N, void* img, hipStream_t s) {
    CONE_REQUIRE(W && img, "fp32 row image: null argument");
    CONE_REQUIRE(N >= 32 && N % 32 == 0 && N <= 8192, "fp32 row image: N=%d must be a multiple of 32 up to 8192", N);
    return pack_launch(W, nullptr, nullptr, nullptr, N / 32, 0, 0, 0, img, s);
}

}  // namespace cone
