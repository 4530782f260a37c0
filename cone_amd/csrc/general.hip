// The general-shape path: the window model at any supported (hidden_dim, nheads) -- hidden_dim a multiple of 64 in
// [64, 512], head_dim = hidden_dim / nheads in {16, 32, 64} (cone/config.py:107,116 take both from opt.json).
//
// The shipped kernels (fused layer tails, folded cross-attention, enc_attn16, rows_chain, the row kernels of window_ops.hip)
// are specialised to d = 256 with 8 heads of 32 and stay as they are.  The general path is built from plain blocks instead:
// LayerNorm launches, row GEMMs with residual / ReLU epilogues (gemm.hip: any N, K % 32 == 0), the attention core below and
// d-wide forms of the row kernels.  Everything is exact fp32 (VALU fma chains); no reduced-precision products.
#include "common.h"

namespace cone {

// ------------------------------------------------------------------------------ attention core
// One workgroup (four waves) per (window, head).  Query rows q0 .. q0 + nqr, key / value rows k0 .. k0 + nk, where a side
// with an offset array takes window b's packed rows off[b] .. off[b + 1] and a side without one the nq slot rows b * nq ..
// (encoder self-attention: both packed; decoder self-attention: both slots; decoder cross-attention: slot queries, packed
// keys).  The window's K (row stride HD + 1: the lane-per-key reads are bank-conflict free) and V rows of the head are staged
// in LDS once; each wave then walks its queries: scores for keys lane + 64 t (t < 4: at most 256 keys) as HD-long fma chains
// on q * sqrt(1 / HD) (nn.MultiheadAttention scales q after the in-projection and its bias), max-subtracted softmax with
// wave reductions, and P V with the 64 / HD lane groups taking every (64 / HD)-th key, summed by shuffles.  Padded keys do
// not exist; a window with no query or no key writes nothing.
constexpr int kGenMaxKeys = 256;

template <int HD>
__global__ __launch_bounds__(256) void gen_attn_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                       const float* __restrict__ V, int ldv, float* __restrict__ OUT, int ldo,
                                                       const int* __restrict__ qoff, const int* __restrict__ koff, int nq,
                                                       int kcap, float scale) {
    constexpr int KS = HD + 1;
    constexpr int G = 64 / HD;              // lane groups of the P V product
    extern __shared__ float sm[];
    float* Ks = sm;                         // (kcap, KS)
    float* Vs = sm + (size_t)kcap * KS;     // (kcap, HD)
    const int b = blockIdx.x, h = blockIdx.y;
    const int q0 = qoff ? qoff[b] : b * nq, nqr = qoff ? qoff[b + 1] - q0 : nq;
    const int k0 = koff ? koff[b] : b * nq, nk = koff ? koff[b + 1] - k0 : nq;
    if (nqr <= 0 || nk <= 0 || nk > kcap) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nk * (HD / 4); i += 256) {
        const int j = i / (HD / 4), c = (i % (HD / 4)) * 4;
        const float4 kv = *reinterpret_cast<const float4*>(K + (size_t)(k0 + j) * ldk + h * HD + c);
        const float4 vv = *reinterpret_cast<const float4*>(V + (size_t)(k0 + j) * ldv + h * HD + c);
        float* kd = Ks + j * KS + c;
        kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
        *reinterpret_cast<float4*>(Vs + j * HD + c) = vv;
    }
    __syncthreads();
    const int c = lane % HD, g = lane / HD;
    for (int i = wave; i < nqr; i += 4) {
        float q[HD];
        const float* qp = Q + (size_t)(q0 + i) * ldq + h * HD;
#pragma unroll
        for (int u = 0; u < HD / 4; ++u) {
            const float4 x = reinterpret_cast<const float4*>(qp)[u];
            q[4 * u] = x.x * scale; q[4 * u + 1] = x.y * scale; q[4 * u + 2] = x.z * scale; q[4 * u + 3] = x.w * scale;
        }
        float e[4];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = lane + 64 * t;
            e[t] = -INFINITY;
            if (j < nk) {
                const float* kr = Ks + j * KS;
                float a = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) a = fmaf(q[d], kr[d], a);
                e[t] = a;
                mx = fmaxf(mx, a);
            }
        }
        mx = wave_max(mx);
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            e[t] = lane + 64 * t < nk ? expf(e[t] - mx) : 0.f;
            l += e[t];
        }
        const float inv = 1.0f / wave_sum(l);
        float o = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (64 * t >= nk) break;
            const int jn = nk - 64 * t < 64 ? nk - 64 * t : 64;
            for (int jj = 0; jj < jn; jj += G) {
                const float p = __shfl(e[t], jj + g, 64);
                if (jj + g < jn) o = fmaf(p, Vs[(64 * t + jj + g) * HD + c], o);
            }
        }
#pragma unroll
        for (int s = HD; s < 64; s <<= 1) o += __shfl_xor(o, s, 64);
        if (g == 0) OUT[(size_t)(q0 + i) * ldo + h * HD + c] = o * inv;
    }
}

// ------------------------------------------------------------------------------ streaming attention core (> 256 keys)
// The same (Q, K, V, OUT, ld*, qoff, koff, nq) addressing, for windows of up to kGenMaxStreamKeys keys, in exact fp32 on the
// matrix cores (v_mfma_f32_16x16x4_f32) in the orientation of enc_attn16_kernel: S^T = K Q^T with the key on accumulator rows
// (4 lg + r, lg = lane / 16) and the query on lanes (li = lane % 16), so a query's softmax is an in-register reduction plus two
// cross-group exchanges and the score registers are directly the A operand of P V (k slot lg <-> key 4 lg + r of a 16-key tile).
// One workgroup (four waves) per (window, head); it walks the window's queries in passes of 64 (one 16-query tile per wave) and,
// inside a pass, the window's keys in blocks of kGenStreamBlock = 64 through LDS:
//   K block d-major [HD][LDK], LDK = 64 + 64 / HD: lane group lg reads channel (HD / 4) lg + st, (HD / 4) LDK = 16 mod 64 banks;
//   V block key-major [64][LDV], LDV = HD + 4: lane group lg reads key 4 lg + r, 4 LDV = 16 mod 64 banks.
// 16.3 + 17.0 KiB at head_dim 64 (8.3 + 9.0 at 32, 4.3 + 5.0 at 16), whatever the window length: four workgroups fit a CU's LDS.
// The next block's rows are requested into registers before the current block's MFMAs and written to LDS behind them.
// Online softmax per query: running maximum m, running sum l (a lane's partial over its own 16 keys of every block, reduced
// across the four lane groups once at the end), output accumulators rescaled by exp(m_old - m_new) every block; 1 / l once at
// the end.  Rows of the last block past the window's end re-read its last row (finite) and have their scores masked to -inf
// (probability exactly 0): no per-tile branch.  exp(-inf - (-inf)) cannot arise: the subtrahend is 0 while the maximum is -inf.
// The decomposition and the block order depend on the window's own lengths only: a window's bits do not depend on the batch
// or on kcap.  A window with no query or no key writes nothing.
constexpr int kGenMaxStreamKeys = 1024;
constexpr int kGenStreamBlock = 64;

typedef float gen_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gen_lane_read(float v, int src_lane) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

template <int HD>
__global__ __launch_bounds__(256) void gen_attn_stream_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K,
                                                              int ldk, const float* __restrict__ V, int ldv,
                                                              float* __restrict__ OUT, int ldo, const int* __restrict__ qoff,
                                                              const int* __restrict__ koff, int nq, int kcap, float scale) {
    constexpr int KB = kGenStreamBlock, LDK = KB + 64 / HD, LDV = HD + 4;
    constexpr int CS = HD / 4;              // channel steps of S^T: lane group lg owns channels CS lg .. CS lg + CS - 1
    constexpr int DT = HD / 16;             // 16-channel output tiles
    constexpr int NLD = HD / 16;            // float4 rows per thread and operand of one block (64 HD / 4 float4 over 256 threads)
    __shared__ float KsT[HD * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[KB * LDV];
    const int b = blockIdx.x, h = blockIdx.y;
    const int q0 = qoff ? qoff[b] : b * nq, nqr = qoff ? qoff[b + 1] - q0 : nq;
    const int k0 = koff ? koff[b] : b * nq, nk = koff ? koff[b + 1] - k0 : nq;
    if (nqr <= 0 || nk <= 0 || nk > kcap) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int nblk = (nk + KB - 1) / KB;
    const float* Kb = K + (size_t)k0 * ldk + h * HD;
    const float* Vb = V + (size_t)k0 * ldv + h * HD;
    gen_f32x4 kreg[NLD], vreg[NLD];
    auto load_block = [&](int blk) {        // rows past the window's end: its last row (masked below)
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int idx = tid + 256 * it;
            const int row = min(blk * KB + idx / CS, nk - 1), c4 = (idx % CS) * 4;
            kreg[it] = *reinterpret_cast<const gen_f32x4*>(Kb + (size_t)row * ldk + c4);
            vreg[it] = *reinterpret_cast<const gen_f32x4*>(Vb + (size_t)row * ldv + c4);
        }
    };
    auto store_block = [&]() {
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            const int idx = tid + 256 * it;
            const int key = idx / CS, c4 = (idx % CS) * 4;
            float* kd = KsT + c4 * LDK + key;
            kd[0] = kreg[it][0]; kd[LDK] = kreg[it][1]; kd[2 * LDK] = kreg[it][2]; kd[3 * LDK] = kreg[it][3];
            *reinterpret_cast<gen_f32x4*>(Vs + key * LDV + c4) = vreg[it];
        }
    };
    for (int qp = 0; qp < nqr; qp += 64) {              // (workgroup-uniform: every wave meets every barrier)
        const int qt = qp + 16 * wave;
        const bool active = qt < nqr;                   // wave-uniform
        float qv[CS];
        {
            const float* qr = Q + (size_t)(q0 + min(qt + li, nqr - 1)) * ldq + h * HD + CS * lg;
#pragma unroll
            for (int u = 0; u < CS / 4; ++u) {
                const gen_f32x4 x = reinterpret_cast<const gen_f32x4*>(qr)[u];
#pragma unroll
                for (int j = 0; j < 4; ++j) qv[4 * u + j] = x[j] * scale;
            }
        }
        float m = -INFINITY, l = 0.f;
        gen_f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = gen_f32x4{0.f, 0.f, 0.f, 0.f};
        load_block(0);
        for (int blk = 0; blk < nblk; ++blk) {
            __syncthreads();                            // the previous block's reads are done
            store_block();
            __syncthreads();
            if (blk + 1 < nblk) load_block(blk + 1);    // in flight under this block's MFMAs
            if (!active) continue;
            gen_f32x4 sc[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) sc[kt] = gen_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < CS; ++st) {
                const float* kp = KsT + (CS * lg + st) * LDK + li;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[16 * kt], qv[st], sc[kt], 0, 0, 0);
            }
            // sc[kt][r] = score of key blk KB + 16 kt + 4 lg + r against query li
            const int lim = nk - blk * KB - 4 * lg;     // that key is real iff 16 kt + r < lim
            if ((blk + 1) * KB > nk) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[kt][r] = 16 * kt + r < lim ? sc[kt][r] : -INFINITY;
            }
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) bm = fmaxf(bm, sc[kt][r]);
            bm = fmaxf(bm, gen_lane_read(bm, lane ^ 16));
            bm = fmaxf(bm, gen_lane_read(bm, lane ^ 32));
            const float mn = fmaxf(m, bm);
            const float ms = mn == -INFINITY ? 0.f : mn;    // (a block with no real key: every exponential below is exp(-inf) = 0)
            const float alpha = expf(m - ms);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[kt][r] = expf(sc[kt][r] - ms);
                    ps += sc[kt][r];
                }
            l = fmaf(l, alpha, ps);
            // o[dt][r] = output row (query) 4 lg + r: its rescale factor sits in the lanes whose li is that row
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = gen_lane_read(alpha, (lane & 48) + 4 * lg + r);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt][r] *= a;
            }
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const float* vp = Vs + (16 * kt + 4 * lg) * LDV + li;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[kt][r], vp[r * LDV + 16 * dt], o[dt], 0, 0, 0);
            }
        }
        if (!active) continue;
        l += gen_lane_read(l, lane ^ 16);
        l += gen_lane_read(l, lane ^ 32);
        const float inv = 1.0f / l;
        float* ob = OUT + (size_t)(q0 + qt + 4 * lg) * ldo + h * HD + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = gen_lane_read(inv, (lane & 48) + 4 * lg + r);
            if (qt + 4 * lg + r < nqr) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) ob[(size_t)r * ldo + 16 * dt] = o[dt][r] * s;
            }
        }
    }
}

bool gen_shape_supported(int d, int heads) {
    if (d < 64 || d > 512 || d % 64 != 0 || heads < 1 || d % heads != 0) return false;
    const int hd = d / heads;
    return hd == 16 || hd == 32 || hd == 64;
}

static size_t gen_attn_lds(int hd, int kcap) { return (size_t)kcap * (2 * hd + 1) * sizeof(float); }

int launch_gen_attn(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* OUT, int ldo,
                    const int* qoff, const int* koff, int B, int nq, int heads, int hd, int kcap, hipStream_t s) {
    CONE_REQUIRE(hd == 16 || hd == 32 || hd == 64, "attention: head_dim %d not in {16, 32, 64}", hd);
    CONE_REQUIRE(kcap >= 1 && kcap <= kGenMaxStreamKeys, "attention: %d keys not in [1, %d]", kcap, kGenMaxStreamKeys);
    CONE_REQUIRE(koff || kcap >= nq, "attention: slot keys need kcap >= nq");
    CONE_REQUIRE((ldq | ldk | ldv) % 4 == 0 && Q && K && V && OUT && heads >= 1, "attention: bad operands");
    if (B <= 0) return 0;
    const float scale = (float)(1.0 / sqrt((double)hd));
    const dim3 grid((unsigned)B, (unsigned)heads);
    if (kcap > kGenMaxKeys) {   // the streaming core: static LDS, the same for every window length
        if (hd == 16)
            hipLaunchKernelGGL(gen_attn_stream_kernel<16>, grid, dim3(256), 0, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
        else if (hd == 32)
            hipLaunchKernelGGL(gen_attn_stream_kernel<32>, grid, dim3(256), 0, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
        else
            hipLaunchKernelGGL(gen_attn_stream_kernel<64>, grid, dim3(256), 0, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
        CONE_LAUNCH_CHECK();
        return 0;
    }
    static DeviceOnce once;     // the opt-in to > 64 KiB of LDS (head_dim 64, 256 keys: 129 KiB), once per device
    CONE_CHECK_HIP(device_once(once, [] {
        hipError_t rc = hipFuncSetAttribute((const void*)gen_attn_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)gen_attn_lds(16, kGenMaxKeys));
        if (rc == hipSuccess)
            rc = hipFuncSetAttribute((const void*)gen_attn_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)gen_attn_lds(32, kGenMaxKeys));
        if (rc == hipSuccess)
            rc = hipFuncSetAttribute((const void*)gen_attn_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)gen_attn_lds(64, kGenMaxKeys));
        return rc;
    }));
    const size_t lds = gen_attn_lds(hd, kcap);
    if (hd == 16)
        hipLaunchKernelGGL(gen_attn_kernel<16>, grid, dim3(256), lds, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
    else if (hd == 32)
        hipLaunchKernelGGL(gen_attn_kernel<32>, grid, dim3(256), lds, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
    else
        hipLaunchKernelGGL(gen_attn_kernel<64>, grid, dim3(256), lds, s, Q, ldq, K, ldk, V, ldv, OUT, ldo, qoff, koff, nq, kcap, scale);
    CONE_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------ d-wide row kernels
// One wavefront per row, float4 lanes: lane l holds channels 4 l .. and 4 (l + 64) .. (d <= 512: two float4 per lane).
// The arithmetic of the 256-wide kernels of window_ops.hip / rowops.hip, over d channels.
constexpr int kGenMaxF4 = 2;

__device__ __forceinline__ void gen_sine(const float* __restrict__ dim_t, int p, int lv, int c4, float4& ps) {
    // PositionEmbeddingSine(normalize=True), cone/position_encoding.py:51-72 (see pack_pos_kernel)
    const float xe = __fmul_rn(__fdiv_rn((float)(p + 1), __fadd_rn((float)lv, 1e-6f)), 6.283185307179586f);
    const float4 dt = reinterpret_cast<const float4*>(dim_t)[c4];
    ps.x = sinf(__fdiv_rn(xe, dt.x));
    ps.y = cosf(__fdiv_rn(xe, dt.y));
    ps.z = sinf(__fdiv_rn(xe, dt.z));
    ps.w = cosf(__fdiv_rn(xe, dt.w));
}

// LayerNorm(x + e) of a d-wide row held as float4 lanes (TrainablePositionalEncoding, cone/position_encoding.py:21-31)
__device__ __forceinline__ void gen_txt_pos(const float* __restrict__ xrow, const float* __restrict__ erow,
                                            const float* __restrict__ tpg, const float* __restrict__ tpb, int d, int lane,
                                            float4* out) {
    const int nf = d / 4;
    float4 v[kGenMaxF4];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k) {
        const int c4 = lane + 64 * k;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < nf) {
            const float4 x = reinterpret_cast<const float4*>(xrow)[c4], e = reinterpret_cast<const float4*>(erow)[c4];
            v[k] = make_float4(x.x + e.x, x.y + e.y, x.z + e.z, x.w + e.w);
        }
        sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k)
        if (lane + 64 * k < nf) {
            v[k].x -= mean; v[k].y -= mean; v[k].z -= mean; v[k].w -= mean;
            sq += (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + 1e-5f);
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k) {
        const int c4 = lane + 64 * k;
        if (c4 < nf) {
            const float4 gg = reinterpret_cast<const float4*>(tpg)[c4], bb = reinterpret_cast<const float4*>(tpb)[c4];
            out[k] = make_float4(v[k].x * rstd * gg.x + bb.x, v[k].y * rstd * gg.y + bb.y, v[k].z * rstd * gg.z + bb.z,
                                 v[k].w * rstd * gg.w + bb.w);
        }
    }
}

// pack_pos_kernel over d channels: X = the window's clip rows then text rows at off[b], POS = their position rows
__global__ __launch_bounds__(256) void gen_pack_pos_kernel(const float* __restrict__ vproj, const int* __restrict__ vrow0,
                                                           const int* __restrict__ vlen, const float* __restrict__ tproj,
                                                           const int* __restrict__ trow0, const int* __restrict__ qlen,
                                                           const int* __restrict__ off, const float* __restrict__ dim_t, float* X,
                                                           float* POS, int d, const float* __restrict__ tpe,
                                                           const float* __restrict__ tpg, const float* __restrict__ tpb) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int lv = vlen[b], lq = qlen[b], nf = d / 4;
    if (p >= lv + lq) return;
    const size_t dst = (size_t)(off[b] + p) * d;
    const float* src = p < lv ? vproj + (size_t)(vrow0[b] + p) * d : tproj + (size_t)(trow0[b] + p - lv) * d;
    float4 ps[kGenMaxF4];
    if (p >= lv && tpe) gen_txt_pos(src, tpe + (size_t)(p - lv) * d, tpg, tpb, d, lane, ps);
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k) {
        const int c4 = lane + 64 * k;
        if (c4 >= nf) continue;
        if (p < lv) gen_sine(dim_t, p, lv, c4, ps[k]);
        else if (!tpe) ps[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(X + dst)[c4] = reinterpret_cast<const float4*>(src)[c4];
        reinterpret_cast<float4*>(POS + dst)[c4] = ps[k];
    }
}

int launch_gen_pack_pos(const float* vproj, const int* vrow0, const int* vlen, const float* tproj, const int* trow0,
                        const int* qlen, const int* off, const float* dim_t, float* X, float* POS, int d, int B, int Lmax,
                        hipStream_t s, const float* tpe, const float* tpg, const float* tpb) {
    CONE_REQUIRE(d % 4 == 0 && d <= 256 * kGenMaxF4, "pack: d=%d", d);
    if (B <= 0 || Lmax <= 0) return 0;
    hipLaunchKernelGGL(gen_pack_pos_kernel, dim3((Lmax + 3) / 4, B), dim3(256), 0, s, vproj, vrow0, vlen, tproj, trow0, qlen, off,
                       dim_t, X, POS, d, tpe, tpg, tpb);
    CONE_LAUNCH_CHECK();
    return 0;
}

// pos_rows_kernel over d channels: row lv (lv - 1) / 2 + p of the sine table
__global__ __launch_bounds__(256) void gen_pos_rows_kernel(const float* __restrict__ dim_t, int max_v_l, int d, float* out) {
    const int lv = blockIdx.y + 1;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= lv) return;
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k) {
        const int c4 = lane + 64 * k;
        if (c4 >= d / 4) continue;
        float4 ps;
        gen_sine(dim_t, p, lv, c4, ps);
        reinterpret_cast<float4*>(out + ((size_t)(lv * (lv - 1) / 2 + p)) * d)[c4] = ps;
    }
}

int launch_gen_pos_rows(const float* dim_t, int max_v_l, int d, float* out, hipStream_t s) {
    CONE_REQUIRE(d % 4 == 0 && d <= 256 * kGenMaxF4, "pos rows: d=%d", d);
    hipLaunchKernelGGL(gen_pos_rows_kernel, dim3((max_v_l + 3) / 4, max_v_l), dim3(256), 0, s, dim_t, max_v_l, d, out);
    CONE_LAUNCH_CHECK();
    return 0;
}

// txt_pos_rows_kernel over d channels (cone_layer0_text_positions)
__global__ __launch_bounds__(256) void gen_txt_pos_rows_kernel(const float* __restrict__ tproj, const int* __restrict__ tok_index,
                                                               const int* __restrict__ src_row, int mod, int n_emb,
                                                               const float* __restrict__ tpe, const float* __restrict__ tpg,
                                                               const float* __restrict__ tpb, int n, const int* __restrict__ n_dev,
                                                               int d, float* __restrict__ out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= (n_dev ? min(*n_dev, n) : n)) return;
    int j = tok_index ? tok_index[i] : src_row[i] % mod;
    j = min(max(j, 0), n_emb - 1);
    float4 r[kGenMaxF4];
    gen_txt_pos(tproj + (size_t)i * d, tpe + (size_t)j * d, tpg, tpb, d, lane, r);
#pragma unroll
    for (int k = 0; k < kGenMaxF4; ++k)
        if (lane + 64 * k < d / 4) reinterpret_cast<float4*>(out + (size_t)i * d)[lane + 64 * k] = r[k];
}

int launch_gen_txt_pos_rows(const float* tproj, const int* tok_index, const int* src_row, int mod, int n_emb, const float* tpe,
                            const float* tpg, const float* tpb, int n, const int* n_dev, int d, float* out, hipStream_t s) {
    CONE_REQUIRE(d % 4 == 0 && d <= 256 * kGenMaxF4, "text positions: d=%d", d);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gen_txt_pos_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, s, tproj, tok_index, src_row, mod, n_emb, tpe, tpg,
                       tpb, n, n_dev, d, out);
    CONE_LAUNCH_CHECK();
    return 0;
}

// rowdot_kernel over d channels: out[m][n] = act(<X[m], W[n]> + b[n]), n < nout <= 2 (class head, last span layer)
__global__ __launch_bounds__(256) void gen_rowdot_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W,
                                                         const float* __restrict__ b, float* out, int ldo, int64_t n_rows,
                                                         int nout, int act, int d) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    for (int n = 0; n < nout; ++n) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kGenMaxF4; ++k) {
            const int c4 = lane + 64 * k;
            if (c4 < d / 4) {
                const float4 xv = reinterpret_cast<const float4*>(X + row * ldx)[c4];
                const float4 wv = reinterpret_cast<const float4*>(W + (size_t)n * d)[c4];
                s += __builtin_fmaf(xv.x, wv.x, xv.y * wv.y) + __builtin_fmaf(xv.z, wv.z, xv.w * wv.w);
            }
        }
        s = wave_sum(s) + b[n];
        if (act == 1) s = 1.0f / (1.0f + expf(-s));
        if (lane == 0) out[row * ldo + n] = s;
    }
}

int launch_gen_rowdot(const float* X, int ldx, const float* W, const float* b, float* out, int ldo, int64_t n_rows, int nout,
                      int act, int d, hipStream_t s) {
    CONE_REQUIRE(d % 4 == 0 && d <= 256 * kGenMaxF4 && ldx % 4 == 0, "rowdot: d=%d", d);
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(gen_rowdot_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, X, ldx, W, b, out, ldo, n_rows,
                       nout, act, d);
    CONE_LAUNCH_CHECK();
    return 0;
}

// saliency_kernel over d channels: the saliency head on the clip rows of memory, scattered to (B, Lv_out); optional copy
// of the packed memory into the padded (B, Lv_out + Lq_out, d) tap
__global__ __launch_bounds__(256) void gen_saliency_kernel(const float* __restrict__ MEM, const int* __restrict__ off,
                                                           const int* __restrict__ vlen, const int* __restrict__ qlen,
                                                           const float* __restrict__ w, const float* __restrict__ bias, float* sal,
                                                           int Lv_out, float* mem_tap, int Lq_out, int d) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int lv = vlen[b], lq = qlen[b], nf = d / 4;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < Lv_out) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kGenMaxF4; ++k) {
            const int c4 = lane + 64 * k;
            if (c4 >= nf) continue;
            const float4 x = p < lv ? reinterpret_cast<const float4*>(MEM + (size_t)(off[b] + p) * d)[c4] : z;
            const float4 wv = reinterpret_cast<const float4*>(w)[c4];
            s += (x.x * wv.x + x.y * wv.y) + (x.z * wv.z + x.w * wv.w);
            if (mem_tap) reinterpret_cast<float4*>(mem_tap + ((size_t)b * (Lv_out + Lq_out) + p) * d)[c4] = x;
        }
        s = p < lv ? wave_sum(s) + bias[0] : 0.f;
        if (lane == 0 && sal) sal[(size_t)b * Lv_out + p] = s;
    } else if (mem_tap && p < Lv_out + Lq_out) {
        const int t = p - Lv_out;
#pragma unroll
        for (int k = 0; k < kGenMaxF4; ++k) {
            const int c4 = lane + 64 * k;
            if (c4 >= nf) continue;
            const float4 x = t < lq ? reinterpret_cast<const float4*>(MEM + (size_t)(off[b] + lv + t) * d)[c4] : z;
            reinterpret_cast<float4*>(mem_tap + ((size_t)b * (Lv_out + Lq_out) + p) * d)[c4] = x;
        }
    }
}

int launch_gen_saliency(const float* MEM, const int* off, const int* vlen, const int* qlen, const float* w, const float* bias,
                        float* sal, int Lv_out, float* mem_tap, int Lq_out, int B, int d, hipStream_t s) {
    CONE_REQUIRE(d % 4 == 0 && d <= 256 * kGenMaxF4, "saliency: d=%d", d);
    if (B <= 0) return 0;
    const int span = mem_tap ? Lv_out + Lq_out : Lv_out;
    hipLaunchKernelGGL(gen_saliency_kernel, dim3((span + 3) / 4, B), dim3(256), 0, s, MEM, off, vlen, qlen, w, bias, sal, Lv_out,
                       mem_tap, Lq_out, d);
    CONE_LAUNCH_CHECK();
    return 0;
}

}  // namespace cone
