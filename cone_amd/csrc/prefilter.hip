// Stage A: sliding-window pre-filter (cone/inference.py:276-299).
//
//   frame_score_kernel : frame_scores[q][f] = <vid[f], txt[q]>  -- the HBM-bound stream over the
//                        pre-extracted clip features (12.7 GB for the MAD-scale stress video).
//                        One wavefront streams whole rows with coalesced 16-B lane loads (1 KiB per
//                        wave-instruction), RPW rows in flight per wave, QG query vectors held in
//                        registers; per-(row,query) partial sums are combined with wave shuffles.
//                        The wave keeps the running max of each half-block (S frames) it streams: the window max is
//                        fused (window_combine_kernel), the frame scores are written only on request.
//   topk_kernel        : first k entries of the stable descending sort of each score row.
// The file, in order: the streaming skeleton (PF_LANE_SLOT, pf_slot_max, pf_store_half_max) and its exact-fp32 kernels; the
// stable top-k family (TK_LOAD_CHUNK, tk_load_list, tk_pass_pick around tk_block_select); the many-query skeleton (PfMqCursor,
// pf_mq_tile_end, pf_mq_grid) and its three kernels -- exact fp32, split bf16, plain bf16 --, which differ in operand staging
// and inner product only; the segmented (whole-split) forms; the bf16 streaming forms; the certified pipeline; the library
// search's scan over many videos (library_scan_kernel, library_topk_kernel: DESIGN.md 4c); the C entries and what they share
// (pf_with_vpl, PfPlanes, launch_window_combine, the CONE_PF_REQUIRE_* checks).  DESIGN.md 3b - 3d.
#include <mutex>
#include <type_traits>

#include "common.h"

namespace cone {

// The clip rows are read exactly once per launch: the stream's loads are NON-TEMPORAL (global_load_dwordx4 ... nt).  Measured
// on one box (tools/ab_variants.sh prefilter.hip, the 12.7 GB MAD-scale video, 1 query): 2.11 ms = 6.0 TB/s with ordinary loads,
// 1.89 - 1.96 ms = 6.5 - 6.7 TB/s with nt (0.75 -> 0.81 - 0.84 of the 8 TB/s peak): lines that will not be read again no longer
// displace each other through the L2 / Infinity Cache.  CONE_PF_NT = 0 restores ordinary loads for an A/B.  The matrix-core
// kernels for >= 8 queries (CONE_PF_NT_MQ) keep ordinary loads: there a lane-row's 128-B line is fetched by two consecutive
// instructions (64 B each: the MFMA operand layout), and with nt the second half loses its L1 hit -- measured 8 queries
// 2.38 -> 2.45 ms, the three-piece bf16 form 3.42 -> 3.70 ms, 64 queries unchanged.
#ifndef CONE_PF_NT
#define CONE_PF_NT 1
#endif
#ifndef CONE_PF_MQ_MIN
#define CONE_PF_MQ_MIN 5            // queries per video from which the matrix-core kernel takes over (A/B: 8 = round 5)
#endif
#ifndef CONE_PF_NT_MQ
#define CONE_PF_NT_MQ 0
#endif
__device__ __forceinline__ float4 pf_stream_ld(const float4* p) {
#if CONE_PF_NT
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
#else
    return *p;
#endif
}

// Fused frame scores + window max.  S = int(W/2), so window i = half-blocks i-1 and i (block h = frames [hS, (h+1)S)) plus,
// when W is odd, the first frame of block i+1: a wave keeps the running max of the half-block it streams in registers and
// writes ONE value per (query, half-block) -- hm -- and the block's first frame score -- fr; window_combine_kernel takes
// win[i] = max(hm[i-1], hm[i], fr[i+1]) from those (max is order-free: bit-identical to the max over the stored frame
// scores).  The (nq, ctx_l) frame-score matrix is written only when the caller asks for it (fs != nullptr): the
// reference needs it for nothing but this max (cone/inference.py:284-295).
//   WPH = 1: one wave per half-block, grid-stride (long videos: every wave streams contiguous 4-row groups of its blocks);
//   WPH = 4: the four waves of a workgroup share one half-block and combine through LDS (short videos: 4x the waves).
// <x, q> over one float4 of channels, the arithmetic PINNED: each pair sum is fma(first factors, second product), the two
// pair sums are added -- what hipcc's contraction made of (x.x q.x + x.y q.y) + (x.z q.z + x.w q.w) in the streaming kernels
// since round 1.  Left to -ffp-contract=fast the choice is the backend's, per kernel: the per-video kernel and the batched
// one (frame_score_groups_kernel) must produce the same bits (test_prefilter_batched_equals_per_video_path).
__device__ __forceinline__ float pf_dot4(const float4& x, const float4& q) {
#pragma clang fp contract(off)
    const float m1 = x.y * q.y, m3 = x.w * q.w;
    const float p01 = __builtin_fmaf(x.x, q.x, m1);
    const float p23 = __builtin_fmaf(x.z, q.z, m3);
    return p01 + p23;
}

// Sum of N per-lane values over the 64 lanes at once: the totals of wave_sum() -- the same butterfly (lane l adds its
// partner l ^ 32, then l ^ 16, ... l ^ 1: the same pairs, so the same bits) -- but a lane keeps only HALF of its values at
// each of the first log2(N) steps (the partner keeps the other half), so N totals cost N - 1 + (6 - log2 N) shuffles
// instead of 6 N.  The lane's result is the total of value index J(l) = the top log2(N) bits of l (bit 5 = the index's
// top bit); the 64 / N lanes that share those bits all hold it.  (Recursion on the array size: every index is static.)
template <int N, int O = 32>
__device__ __forceinline__ float wave_sum_multi(const float (&v)[N], int lane) {
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "a power of two");
    if constexpr (N == 1) {
        float x = v[0];
#pragma unroll
        for (int o = O; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    } else {
        constexpr int H = N / 2;
        const bool up = (lane & O) != 0;                // this lane keeps the upper half of its values, its partner the lower
        float w[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float send = up ? v[j] : v[j + H];
            const float keep = up ? v[j + H] : v[j];
            w[j] = keep + __shfl_xor(send, O, 64);
        }
        return wave_sum_multi<H, O / 2>(w, lane);
    }
}

// A lane's share of <row, query>: the pf_dot4 chain over its VPL float4, in channel order.  With the butterfly of
// wave_sum_multi this IS the per-frame arithmetic of the streaming form: frame_score_kernel and pf_rescore_kernel (the
// certified top-k's rescoring of single windows) both call it, so a frame's score has the same bits in either.
template <int VPL>
__device__ __forceinline__ float pf_lane_dot(const float4 (&x)[VPL], const float4 (&q)[VPL]) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) s += pf_dot4(x[v], q[v]);
    return s;
}

// ---- the streaming skeleton (fp32 and bf16, per-video and grouped) ------------------------------------------------------
// Which (row slot, query) total a lane ends up with after wave_sum_multi<RPW * QG>: value index r * QG + g = the lane's top
// bits -- row slot my_r, query slot my_g.  `writer` = one of the 64 / NV lanes that hold the same total; `out_lane` = lane
// g * (64 / NV), the one that stores query g's half-window results.  (A macro, not a struct: with a struct hipcc allocates
// the registers of frame_score_bf16_kernel<1, 2, 4, 4> differently and it loses a wave per SIMD.)
#define PF_LANE_SLOT(RPW, QG, lane)                                                                                        \
    static_assert(((RPW) & ((RPW) - 1)) == 0 && ((QG) & ((QG) - 1)) == 0 && (RPW) * (QG) <= 64, "row / query counts: powers of two"); \
    const int my_j = (lane) / (64 / ((RPW) * (QG))), my_r = my_j / (QG), my_g = my_j % (QG);                                \
    [[maybe_unused]] const bool writer = ((lane) & (64 / ((RPW) * (QG)) - 1)) == 0, out_lane = writer && my_r == 0

// A wave's max over its rows of a half window (every lane of a (row slot, query) group holds that slot's): over the RPW row
// slots of a query -- the lanes that differ in the index's top log2(RPW) bits (lane bits 5, 4, ...).
template <int RPW>
__device__ __forceinline__ float pf_slot_max(float m) {
#pragma unroll
    for (int o = 32; o > 32 / RPW; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

// hm[q0 + g][h] = the half window's max: the wave's own (WPH = 1) or that of the workgroup's four waves through `red` in LDS
// (WPH = 4: h is uniform over the workgroup, so the barriers are too).
template <int QG, int WPH>
__device__ __forceinline__ void pf_store_half_max(float m, int my_g, bool out_lane, int lane, int wave, float (*red)[QG], int q0, int nq,
                                                  int64_t nh, int64_t h, float* __restrict__ hm) {
    if (WPH == 1) {
        if (out_lane && q0 + my_g < nq) hm[(size_t)(q0 + my_g) * nh + h] = m;
    } else {
        if (out_lane) red[wave][my_g] = m;
        __syncthreads();
        if (wave == 0 && lane < QG && q0 + lane < nq)
            hm[(size_t)(q0 + lane) * nh + h] = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
        __syncthreads();
    }
}

// GATED (the certified top-k's fallback, cone_prefilter_topk_certified): gate[q] != 0 says that query q needs no scan; a
// launch group all of whose queries are gated off returns after reading the flags and touches no arena row.  The ungated
// instantiation is the kernel as it always was (frame_score_kernel below: same arguments, same code).
template <int VPL /* float4 per lane per row: dv = 256*VPL */, int QG, int RPW, int WPH, bool GATED>
__device__ __forceinline__ void frame_score_body(const float* __restrict__ vid, int64_t ctx_l, int S, int64_t nh,
                                                 const float* __restrict__ txt, int q0, int nq,
                                                 float* __restrict__ fs, float* __restrict__ hm,
                                                 float* __restrict__ fr, const int* __restrict__ gate) {
    constexpr int DV = 256 * VPL, UPB = 4 / WPH, NV = RPW * QG;
    if constexpr (GATED) {                                           // (uniform over the grid: the flags of this launch's queries)
        bool any = false;
#pragma unroll
        for (int g = 0; g < QG; ++g) any |= gate[min(q0 + g, nq - 1)] == 0;
        if (!any) return;
    }
    __shared__ float red[4][QG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = wave % WPH;
    PF_LANE_SLOT(RPW, QG, lane);
    float4 q[QG][VPL];
#pragma unroll
    for (int g = 0; g < QG; ++g)
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            const int qi = min(q0 + g, nq - 1);
            q[g][v] = reinterpret_cast<const float4*>(txt + (size_t)qi * DV)[lane + 64 * v];
        }
    for (int64_t h = (int64_t)blockIdx.x * UPB + wave / WPH; h < nh; h += (int64_t)gridDim.x * UPB) {
        const int64_t r_lo = h * S;
        const int n = (int)min((int64_t)S, ctx_l - r_lo);            // frames of this half-block
        const float* base = vid + r_lo * DV;
        float m = -INFINITY;                                         // running max of this lane's (row slot, query)
        // (the row loop of pf16_half_block, with the frame-score and first-frame stores inside: as a function of its own it
        // costs every instantiation 4 - 10 VGPRs and <2, 1, 4, 1>, the one-query stream, a wave per SIMD)
        for (int j0 = sub * RPW; j0 < n; j0 += WPH * RPW) {
            float4 x[RPW][VPL];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int row = min(j0 + r, n - 1);
#pragma unroll
                for (int v = 0; v < VPL; ++v)
                    x[r][v] = pf_stream_ld(reinterpret_cast<const float4*>(base + (size_t)row * DV) + lane + 64 * v);
            }
            float part[NV];
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int g = 0; g < QG; ++g) part[r * QG + g] = pf_lane_dot<VPL>(x[r], q[g]);
            const float s = wave_sum_multi<NV>(part, lane);            // = wave_sum of (row j0 + my_r, query q0 + my_g)
            if (j0 + my_r < n) {
                m = fmaxf(m, s);
                if (writer && q0 + my_g < nq) {
                    if (fs) fs[(size_t)(q0 + my_g) * ctx_l + r_lo + j0 + my_r] = s;
                    if (my_r == 0 && j0 == 0) fr[(size_t)(q0 + my_g) * nh + h] = s;      // the block's first frame
                }
            }
        }
        m = pf_slot_max<RPW>(m);
        pf_store_half_max<QG, WPH>(m, my_g, out_lane, lane, wave, red, q0, nq, nh, h, hm);
    }
}

template <int VPL, int QG, int RPW, int WPH>
__global__ __launch_bounds__(256) void frame_score_kernel(const float* __restrict__ vid, int64_t ctx_l, int S, int64_t nh,
                                                          const float* __restrict__ txt, int q0, int nq,
                                                          float* __restrict__ fs, float* __restrict__ hm,
                                                          float* __restrict__ fr) {
    frame_score_body<VPL, QG, RPW, WPH, false>(vid, ctx_l, S, nh, txt, q0, nq, fs, hm, fr, nullptr);
}

// (one launch for every group of 4 queries: blockIdx.y = the group; a last group of fewer repeats its last query and stores nothing for the spare slots)
template <int VPL, int RPW, int WPH>
__global__ __launch_bounds__(256) void frame_score_gated_kernel(const float* __restrict__ vid, int64_t ctx_l, int S, int64_t nh,
                                                                const float* __restrict__ txt, int nq,
                                                                float* __restrict__ hm, float* __restrict__ fr,
                                                                const int* __restrict__ gate) {
    frame_score_body<VPL, 4, RPW, WPH, true>(vid, ctx_l, S, nh, txt, 4 * (int)blockIdx.y, nq, nullptr, hm, fr, gate);
}

// win[i] = max(hm[i-1], hm[i], W odd ? fr[i+1] : -inf) over the half-blocks that exist (0 <= h < nh), a / f = one query's
// rows of the two planes: window i covers frames [max((i-1)S, 0), min((i-1)S + W, ctx_l)), cone/inference.py:286-292.
__device__ __forceinline__ float pf_window_of_halves(const float* __restrict__ a, const float* __restrict__ f, int64_t nh,
                                                     int odd, int64_t i) {
    float m = -INFINITY;
    if (i >= 1) m = a[i - 1];
    if (i < nh) m = fmaxf(m, a[i]);
    if (odd && i + 1 < nh) m = fmaxf(m, f[i + 1]);
    return m;
}

__global__ __launch_bounds__(256) void window_combine_kernel(const float* __restrict__ hm, const float* __restrict__ fr,
                                                             int64_t nh, int odd, float* __restrict__ win) {
    const int q = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nh) return;                                                  // num_window = nh + 1
    win[(size_t)q * (nh + 1) + i] = pf_window_of_halves(hm + (size_t)q * nh, fr + (size_t)q * nh, nh, odd, i);
}

// Two-level stable top-k for long rows: level 1 -- one workgroup per chunk of TK_CH scores extracts the chunk's own
// stable top-k; level 2 -- topk_merge_kernel picks the k best of the (chunks x k) candidates with the same (score desc,
// index asc) order.  Chunks cover ascending index ranges and every list is (score desc, index asc), so the merged list is
// the row's stable descending order (the argument of parallel.merge_topk).
//
// Both levels run the same barrier-free selection (tk_select): every thread holds its share of the values in registers,
// each WAVE extracts the top-k of its own quarter by k passes of (register scan, 6-step shuffle arg-max) -- no LDS traffic,
// no workgroup barrier inside the passes -- and wave 0 merges the four sorted lists (4 k candidates, again in registers)
// behind ONE barrier.  (Round 2 re-read the chunk from LDS in every pass behind three barriers: 156 us for 64 rows of
// 100 001 windows; this form: see profiles/README.md.)
constexpr int TK_CH = 4096;
constexpr int TK_PT = TK_CH / 256;      // values per thread
constexpr int TK_KMAX = 256;            // candidates per wave list held in LDS (4 lists)

// order of the selection: a precedes b iff a.v > b.v or (a.v == b.v and a.i < b.i); "after last" = strictly later
__device__ __forceinline__ bool tk_after(float v, int i, float lv, int li_) { return (v < lv) || (v == lv && i > li_); }
__device__ __forceinline__ bool tk_better(float v, int i, float bv, int bi) { return (v > bv) || (v == bv && i < bi); }

// One wave: k passes over PT (value, index) pairs per lane (index 0x7fffffff = empty slot); pass p's winner goes to
// out_v[p] / out_i[p] (lane 0 writes); returns nothing -- lists shorter than k are padded with (-inf, 0x7fffffff).
template <int PT>
__device__ __forceinline__ void tk_wave_select(const float (&v)[PT], const int (&ix)[PT], int k, float* out_v, int* out_i,
                                               int used = PT /* slots that can hold a value (wave-uniform) */) {
    const int lane = threadIdx.x & 63;
    float last_v = INFINITY;
    int last_i = -1;
    for (int p = 0; p < k; ++p) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < PT; ++u)
            if (u < used && ix[u] != 0x7fffffff && tk_after(v[u], ix[u], last_v, last_i) && tk_better(v[u], ix[u], bv, bi)) { bv = v[u]; bi = ix[u]; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { out_v[p] = bi == 0x7fffffff ? -INFINITY : bv; out_i[p] = bi; }
        if (bi == 0x7fffffff) {                       // (wave-uniform) nothing left: pad the rest of the list
            for (int r = p + 1 + lane; r < k; r += 64) { out_v[r] = -INFINITY; out_i[r] = 0x7fffffff; }
            break;
        }
        last_v = bv; last_i = bi;
    }
}

// Bitonic sort of one (value, index) pair per lane over the 64 lanes of a wave, best first (lane 0 = largest value, ties
// to the lower index); empty slots (index 0x7fffffff, value -inf) sink to the end.
__device__ __forceinline__ void tk_wave_sort(float& v, int& i) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const float pv = __shfl_xor(v, j, 64);
            const int pi = __shfl_xor(i, j, 64);
            const bool take_better = ((lane & j) == 0) == ((lane & k2) == 0);
            const bool p_better = tk_better(pv, pi, v, i), p_worse = tk_better(v, i, pv, pi);
            if (take_better ? p_better : p_worse) { v = pv; i = pi; }
        }
}

// Threshold selection for k <= 64 (the pre-filter's top-k is 20 - 30): sort the 64 per-lane bests; the k-th of them, T,
// cannot precede the k-th best of ALL values (the k best lane-bests are k distinct values at or ahead of T), so every
// member of the top-k is at or ahead of T; typically ~1.3 k values are (40 of 1 024 at k = 30).  They are compacted into
// `scr` (64 slots of this wave), sorted once more, and lanes 0 .. k-1 hold the answer: ~700 instructions instead of k
// passes over all PT values (5 100 at k = 30, PT = 16).  More than 64 survivors (values clustered in few lanes) -> false:
// the caller falls back to the pass-based selection.  Same total order, hence the same list, bit for bit.
template <int PT>
__device__ __forceinline__ bool tk_wave_select_fast(const float (&v)[PT], const int (&ix)[PT], int k, float* out_v, int* out_i,
                                                    float* scr_v, int* scr_i, int used = PT) {
    const int lane = threadIdx.x & 63;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < PT; ++u)
        if (u < used && ix[u] != 0x7fffffff && tk_better(v[u], ix[u], bv, bi)) { bv = v[u]; bi = ix[u]; }
    tk_wave_sort(bv, bi);
    const float tv = __shfl(bv, k - 1, 64);
    const int ti = __shfl(bi, k - 1, 64);           // 0x7fffffff: fewer than k lanes hold anything -> everything survives
    int c = 0;
#pragma unroll
    for (int u = 0; u < PT; ++u)
        c += (u < used && ix[u] != 0x7fffffff && !tk_better(tv, ti, v[u], ix[u])) ? 1 : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    if (total > 64) return false;
    int pos = incl - c;
#pragma unroll
    for (int u = 0; u < PT; ++u)
        if (u < used && ix[u] != 0x7fffffff && !tk_better(tv, ti, v[u], ix[u])) { scr_v[pos] = v[u]; scr_i[pos] = ix[u]; ++pos; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // this wave's ds_writes ahead of its ds_reads
    float cv = lane < total ? scr_v[lane] : -INFINITY;
    int ci = lane < total ? scr_i[lane] : 0x7fffffff;
    tk_wave_sort(cv, ci);
    if (lane < k) { out_v[lane] = ci == 0x7fffffff ? -INFINITY : cv; out_i[lane] = ci; }
    return true;
}

// Workgroup of 256: per-wave lists into LDS, then wave 0 merges the four lists into (gv, gi)[0 .. k) in global memory.
template <int PT>
__device__ __forceinline__ void tk_block_select(const float (&v)[PT], const int (&ix)[PT], int k, float* gv, int* gi,
                                                int idx_none) {
    __shared__ float l_v[4 * TK_KMAX];
    __shared__ int l_i[4 * TK_KMAX];
    __shared__ float s_v[4 * 64];
    __shared__ int s_i[4 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (!(k <= 64 && tk_wave_select_fast<PT>(v, ix, k, l_v + wave * k, l_i + wave * k, s_v + wave * 64, s_i + wave * 64)))
        tk_wave_select<PT>(v, ix, k, l_v + wave * k, l_i + wave * k);
    __syncthreads();
    if (wave != 0) return;
    constexpr int MT = 4 * TK_KMAX / 64;            // merge slots per lane
    float mv[MT];
    int mi[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int e = lane + 64 * t;
        const bool ok = e < 4 * k;
        mv[t] = ok ? l_v[e] : -INFINITY;
        mi[t] = ok ? l_i[e] : 0x7fffffff;
    }
    // the merged list goes through the (now free) first list's LDS slots, then out with the caller's "none" index
    const int used = (4 * k + 63) / 64;
    if (!(k <= 64 && tk_wave_select_fast<MT>(mv, mi, k, l_v, l_i, s_v, s_i, used)))
        tk_wave_select<MT>(mv, mi, k, l_v, l_i, used);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the list's ds_writes before the wave reads it back
    for (int r = lane; r < k; r += 64) {
        const int i = l_i[r];
        gv[r] = l_v[r];
        gi[r] = i == 0x7fffffff ? idx_none : i;
    }
}

// The two register loaders of the chunked selections (thread tid's slot u = element u * 256 + tid; index 0x7fffffff = empty).
// A chunk: windows base .. base + m - 1 of a row into v[] / ix[], SCORE = the score of window base + j as an expression in j
// (a row's element, or the two planes through pf_window_of_halves); a NaN score is never chosen (as in the one-level kernel);
// global window indices, ascending with j.  (A macro: as a function taking the score as a callable it costs topk_chunk_kernel
// and pf_fallback_chunk_kernel 9 VGPRs and with them a wave per SIMD.)
#define TK_LOAD_CHUNK(v, ix, base, m, SCORE)                        \
    float v[TK_PT];                                                 \
    int ix[TK_PT];                                                  \
    _Pragma("unroll") for (int u = 0; u < TK_PT; ++u) {             \
        const int j = u * 256 + (int)threadIdx.x;                   \
        const float x = j < (m) ? (SCORE) : -INFINITY;              \
        const bool ok = j < (m) && x == x;                          \
        v[u] = ok ? x : -INFINITY;                                  \
        ix[u] = ok ? (int)((base) + j) : 0x7fffffff;                \
    }
// A list of n <= 256 * TK_PT (value, index) pairs, as a selection left them.
__device__ __forceinline__ void tk_load_list(const float* __restrict__ cv, const int* __restrict__ ci, int n, float (&v)[TK_PT],
                                             int (&ix)[TK_PT]) {
#pragma unroll
    for (int u = 0; u < TK_PT; ++u) {
        const int j = u * 256 + threadIdx.x;
        v[u] = j < n ? cv[j] : -INFINITY;
        ix[u] = j < n ? ci[j] : 0x7fffffff;
    }
}

__global__ __launch_bounds__(256) void topk_chunk_kernel(const float* __restrict__ sc, int64_t n, int k,
                                                         float* __restrict__ cval, int* __restrict__ cidx, int n_chunks) {
    const int q = blockIdx.y, ch = blockIdx.x;
    const int64_t base = (int64_t)ch * TK_CH;
    const int m = (int)min((int64_t)TK_CH, n - base);
    const float* row = sc + (size_t)q * n + base;
    TK_LOAD_CHUNK(v, ix, base, m, row[j]);
    tk_block_select<TK_PT>(v, ix, k, cval + ((size_t)q * n_chunks + ch) * k, cidx + ((size_t)q * n_chunks + ch) * k, 0x7fffffff);
}

// level 2: up to 256 * TK_PT candidates per row in registers
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ cval, const int* __restrict__ cidx,
                                                         int n_cand, int k, int32_t* __restrict__ idx,
                                                         float* __restrict__ val) {
    __shared__ float o_v[TK_KMAX];
    const int q = blockIdx.x;
    float v[TK_PT];
    int ix[TK_PT];
    tk_load_list(cval + (size_t)q * n_cand, cidx + (size_t)q * n_cand, n_cand, v, ix);
    float* ov = val ? val + (size_t)q * k : o_v;
    tk_block_select<TK_PT>(v, ix, k, ov, idx + (size_t)q * k, -1);
}

// The end of one pass of the pass-based kernels (topk_kernel, topk_seg_kernel's long rows): every thread brings the best
// (bv, bi) of its share; the wave arg-max by shuffles, the NW wave winners through LDS, thread 0 picks the pass's winner
// and stores it (index 0x7fffffff = nothing left: -1), and every thread leaves with it in (last_v, last_i).
template <int NW>
__device__ __forceinline__ void tk_pass_pick(float bv, int bi, int32_t* __restrict__ idx_out, float* __restrict__ val_out,
                                             float& last_v, int& last_i) {
    __shared__ float s_v[NW];
    __shared__ int s_i[NW];
    __shared__ float best_v;
    __shared__ int best_i;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = s_v[0];
        int i = s_i[0];
        for (int w = 1; w < NW; ++w)
            if (tk_better(s_v[w], s_i[w], v, i)) { v = s_v[w]; i = s_i[w]; }
        best_v = v; best_i = i;
        *idx_out = i == 0x7fffffff ? -1 : i;
        if (val_out) *val_out = v;
    }
    __syncthreads();
    last_v = best_v;
    last_i = best_i;
    __syncthreads();
}

// Stable descending top-k: pass p picks the largest (score, then lowest index) strictly after the
// previous pick in that order.  One workgroup per score row.
template <int NT>
__global__ __launch_bounds__(NT) void topk_kernel(const float* __restrict__ sc, int64_t n, int k,
                                                  int32_t* __restrict__ idx, float* __restrict__ val) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* row = sc + (size_t)q * n;
    float last_v = INFINITY;
    int last_i = -1;
    for (int p = 0; p < k; ++p) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        // 4 independent loads in flight per thread: a pass over a 100k-window row is latency-, not bandwidth-bound
        for (int64_t j0 = tid; j0 < n; j0 += 4 * NT) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t j = j0 + (int64_t)u * NT;
                v[u] = j < n ? row[j] : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t j = j0 + (int64_t)u * NT;
                if (j < n && tk_after(v[u], (int)j, last_v, last_i) && tk_better(v[u], (int)j, bv, bi)) { bv = v[u]; bi = (int)j; }
            }
        }
        tk_pass_pick<NT / 64>(bv, bi, idx + (size_t)q * k + p, val ? val + (size_t)q * k + p : nullptr, last_v, last_i);
    }
}

// ---- many queries over one video: frame scores on the fp32 matrix cores --------------------------------------------
// fs[q][f] = <vid[f], txt[q]> for up to 64 queries at once is a skinny GEMM whose big operand is the clip arena itself
// (read ONCE for all queries): arithmetic intensity 0.5 * Q flop/B -- at Q = 64 the MFMA time (2.7 ms for the 12.7 GB
// MAD-scale video) and the HBM time (2.3 ms) are about equal.  A general GEMM tile wastes half of its 128 rows on 64
// queries and re-stages the arena through LDS; here
//   * D[query][frame] tiles of v_mfma_f32_16x16x4_f32: A = the query vectors from LDS (operand slabs [16 queries][16
//     channels], 16-B chunks XOR-swizzled: conflict-free ds_read_b128; 128 KiB for 64 x 512), B = the frames straight
//     from global memory into registers (lane = frame, float4 = channels 16 s + 4 lg .. : k slot lg of step (s, r) <->
//     channel 16 s + 4 lg + r on both operands), 128 channels (8 float4) at a time, the next 128 in flight meanwhile;
//   * a wave owns 16 frames per step of a grid-stride loop; accumulator register r of lane (li, lg) = fs[query 4 lg + r
//     of the tile][frame li]: 64-B row segments per store.
// Exact fp32 products and sums (another summation order than the streaming kernel: ~1e-7 relative).
typedef float pf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int pf_swz16(int row) { return (0x1230 >> (((row >> 2) & 3) * 4)) & 3; }
__device__ __forceinline__ pf4 pf_mq_ld(const float* p) {       // a frame's 16-B piece of the once-read stream
#if CONE_PF_NT_MQ
    return __builtin_nontemporal_load(reinterpret_cast<const pf4*>(p));
#else
    return *reinterpret_cast<const pf4*>(p);
#endif
}

constexpr int MQ_NT = 768;     // 12 waves: the one workgroup a CU holds (128 KiB of LDS) runs three waves per SIMD

// ---- the many-query skeleton: what frame_score_mq_kernel, frame_score_mq3_kernel and frame_score_mq_bf16_kernel share ----
// A wave owns whole half windows (frames [hS, (h+1)S)): ceil(S / 16) tiles of 16 frames, the last one partial (its spare
// lanes re-read the half window's last frame and are masked), running max per (query, lane) in registers, one value per
// (query, half window) out.  The waves of a workgroup take consecutive half windows, so their 4-B results of one query fall
// into one cache line; a wave's next half window is h_step = 12 x gridDim.x further on.  The stream is software-pipelined
// across tiles AND half windows: the kernels differ in their operand staging and inner product only.
//
// The cursor: this tile (half window h, frames f0 .. f0 + 15 of [r_lo, r_hi), fp = lane (li, lg)'s row at its channel
// offset) and, after look_ahead(), the tile after it (h2 ..., fp2; more = there is one; fp2 = fp when there is none, so a
// prefetch stays in bounds).  A wave that is not live (frame_score_mq3_kernel's: no half window at all, or none left) points
// at frame 0 and has no next tile.
template <class T /* the arena's element */>
struct PfMqCursor {
    const T* vid;
    int64_t ctx_l, nh, h_step;
    int dv, S, li, off;
    int64_t h, f0, r_lo, r_hi, h2, f2, lo2, hi2;
    const T *fp, *fp2;
    bool more;
    __device__ __forceinline__ PfMqCursor(const T* vid_, int64_t ctx_l_, int dv_, int S_, int64_t nh_, int64_t h_step_, int li_, int off_,
                                          int64_t h_, bool live = true)
        : vid(vid_), ctx_l(ctx_l_), nh(nh_), h_step(h_step_), dv(dv_), S(S_), li(li_), off(off_), h(h_) {
        r_lo = live ? h * S : 0;
        r_hi = live ? min(r_lo + S, ctx_l) : 1;
        f0 = r_lo;
        fp = vid + min(f0 + li, r_hi - 1) * dv + off;
    }
    __device__ __forceinline__ void look_ahead(bool live = true) {       // where the stream goes after this tile
        h2 = h; f2 = f0 + 16; lo2 = r_lo; hi2 = r_hi;
        if (f2 >= r_hi) { h2 = h + h_step; lo2 = h2 * S; hi2 = min(lo2 + S, ctx_l); f2 = lo2; }
        more = live && h2 < nh;
        fp2 = more ? vid + min(f2 + li, hi2 - 1) * dv + off : fp;
    }
    __device__ __forceinline__ void advance() { h = h2; f0 = f2; r_lo = lo2; r_hi = hi2; fp = fp2; }
};

// The end of a tile.  Accumulator register r of lane (li, lg) = the score of (query q0 + 16 qt + 4 lg + r, frame f0 + li):
// into the running max, the frame-score matrix (FS) and -- frame hS, i.e. lane li = 0 of the half window's first tile -- the
// first-frame plane; on the half window's last tile the max over the 16 frame lanes, one hm store per query, and the
// running max starts over.  (The cursor comes BY VALUE: by reference hipcc does not split the struct before it inlines, and the
// four-tile forms of all three kernels spill.)
template <int QT, bool FS, class T>
__device__ __forceinline__ void pf_mq_tile_end(const PfMqCursor<T> cu, const pf4 (&acc)[QT], pf4 (&mx)[QT], int lg, int q0, int nq,
                                               float* __restrict__ fs, float* __restrict__ hm, float* __restrict__ fr) {
    const bool valid = cu.f0 + cu.li < cu.r_hi;
    const bool first = cu.f0 == cu.r_lo && cu.li == 0;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (valid) mx[qt][r] = fmaxf(mx[qt][r], acc[qt][r]);
            const int qg = q0 + qt * 16 + 4 * lg + r;
            if (FS && valid && qg < nq) fs[(size_t)qg * cu.ctx_l + cu.f0 + cu.li] = acc[qt][r];
            if (first && qg < nq) fr[(size_t)qg * cu.nh + cu.h] = acc[qt][r];
        }
    }
    if (cu.f0 + 16 >= cu.r_hi) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = mx[qt][r];
                v = fmaxf(v, __shfl_xor(v, 1, 64));
                v = fmaxf(v, __shfl_xor(v, 2, 64));
                v = fmaxf(v, __shfl_xor(v, 4, 64));
                v = fmaxf(v, __shfl_xor(v, 8, 64));
                const int qg = q0 + qt * 16 + 4 * lg + r;
                if (cu.li == 0 && qg < nq) hm[(size_t)qg * cu.nh + cu.h] = v;
                mx[qt][r] = -INFINITY;
            }
    }
}

template <int QT /* query tiles of 16 */, bool FS /* also write the frame scores */>
__global__ __launch_bounds__(MQ_NT, 3) void frame_score_mq_kernel(const float* __restrict__ vid, int64_t ctx_l, int dv,
                                                                int S, int64_t nh, const float* __restrict__ txt, int q0,
                                                                int nq, float* __restrict__ fs, float* __restrict__ hm,
                                                                float* __restrict__ fr) {
    extern __shared__ __attribute__((aligned(16))) float qs[];          // [QT][dv / 16] slabs of [16 queries][16 floats]
    const int tid = threadIdx.x, lane = tid & 63;
    const int li = lane & 15, lg = lane >> 4;
    const int ns = dv >> 4;                                              // slabs per query tile
    for (int i = tid; i < QT * 16 * (dv >> 2); i += MQ_NT) {             // (query, float4 of its vector)
        const int qi = i / (dv >> 2), c4 = i % (dv >> 2);
        const int qg = q0 + qi;
        pf4 v = pf4{0.f, 0.f, 0.f, 0.f};
        if (qg < nq) v = *reinterpret_cast<const pf4*>(txt + (size_t)qg * dv + c4 * 4);
        const int row = qi & 15, s = c4 >> 2, ch = c4 & 3;
        *reinterpret_cast<pf4*>(qs + ((qi >> 4) * ns + s) * 256 + row * 16 + ((ch ^ pf_swz16(row)) << 2)) = v;
    }
    __syncthreads();
    const int rd = li * 16 + ((lg ^ pf_swz16(li)) << 2);
    const int nchunk = dv >> 7;                                          // 128-channel chunks (8 slabs)
    constexpr int NW = MQ_NT / 64;
    const int64_t h0 = (int64_t)blockIdx.x * NW + (tid >> 6);
    if (h0 >= nh) return;
    PfMqCursor<float> cu(vid, ctx_l, dv, S, nh, (int64_t)gridDim.x * NW, li, 4 * lg, h0);
    pf4 cur[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) cur[s] = pf_mq_ld(cu.fp + 16 * s);
    pf4 mx[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) mx[qt] = pf4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    while (true) {
        cu.look_ahead();
        pf4 acc[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = pf4{0.f, 0.f, 0.f, 0.f};
        // Burst loads (the 8 x 64 B of a row's next 128 channels back to back: whole 128-B lines), compiler-scheduled MFMAs.
        // Measured on one box at 64 queries (round 3, tools/ab_variants.sh): this loop 3.76 - 3.79 ms; the same with the query
        // fragments software-pipelined and the MFMA order pinned 3.97; with a rolling per-slab prefetch instead of the bursts
        // 4.07 - 4.10.  PMC: 84 % MFMA-busy at an effective 1.85 GHz -- the exact-fp32 matrix pipe under a 3.4 TB/s stream
        // is power-limited, three waves per SIMD already cover each other's LDS and memory waits.
        for (int c = 0; c < nchunk; ++c) {
            const float* np = c + 1 < nchunk ? cu.fp + 128 * (c + 1) : cu.fp2;
            pf4 nxt[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) nxt[s] = pf_mq_ld(np + 16 * s);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const pf4 aa = *reinterpret_cast<const pf4*>(qs + (qt * ns + c * 8 + s) * 256 + rd);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[r], cur[s][r], acc[qt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) cur[s] = nxt[s];
        }
        pf_mq_tile_end<QT, FS>(cu, acc, mx, lg, q0, nq, fs, hm, fr);
        if (!cu.more) break;
        cu.advance();
    }
}

// The many-query launchers' common part: opt the listed kernels into `lds_bytes` of dynamic LDS (past the 64 KiB default:
// once per device) and size the grid -- the one workgroup a CU holds, grid-stride over the half windows, twelve per step.
template <size_t N>
static int pf_mq_grid(DeviceOnce& once, const void* const (&fns)[N], int lds_bytes, int64_t nh, const char* what, unsigned* blocks) {
    int n_cu = 0;
    if (device_once(once, [&] {
            hipError_t e = hipSuccess;
            for (size_t i = 0; i < N && e == hipSuccess; ++i)
                e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
            return e;
        }, &n_cu) != hipSuccess) {
        set_error("%s: raising the LDS limit of the many-query kernel failed", what);
        return CONE_E_HIP;
    }
    const int64_t b = (nh + MQ_NT / 64 - 1) / (MQ_NT / 64);
    *blocks = (unsigned)(b < n_cu ? b : n_cu);
    return 0;
}
// query tiles of 16 for a pass over `rem` remaining queries: 4 (where the form has room for 64 queries), 2, or 1 for <= 16 --
// half the matrix work of two, and the stream is HBM-bound.  A pass takes 16 x tiles queries.
static int pf_mq_tiles(int rem, int max_tiles) { return max_tiles == 4 && rem > 32 ? 4 : (rem > 16 ? 2 : 1); }

static int launch_frame_scores_mq(const float* vid, int64_t ctx_l, int dv, int S, int64_t nh, const float* txt, int nq,
                                  float* fs, float* hm, float* fr, hipStream_t s) {
    static DeviceOnce once;
    const void* const fns[6] = {(const void*)frame_score_mq_kernel<4, false>, (const void*)frame_score_mq_kernel<4, true>,
                                (const void*)frame_score_mq_kernel<2, false>, (const void*)frame_score_mq_kernel<2, true>,
                                (const void*)frame_score_mq_kernel<1, false>, (const void*)frame_score_mq_kernel<1, true>};
    unsigned blocks = 0;
    if (int rc = pf_mq_grid(once, fns, 128 * 1024, nh, "prefilter", &blocks)) return rc;
    // 64 queries per launch while their vectors fit the LDS next to nothing else (64 x 512 x 4 B = 128 KiB), else 32
    const int max_tiles = dv <= 512 ? 4 : 2;
    for (int q0 = 0; q0 < nq;) {
        const int rem = nq - q0, qt = pf_mq_tiles(rem, max_tiles);
        ProfScope ps(PK_FRAME_SCORE, ctx_l, dv, rem < 16 * qt ? rem : 16 * qt, nullptr, s);
#define CONE_MQ_LAUNCH(QT, FS)                                                                                             \
    hipLaunchKernelGGL((frame_score_mq_kernel<QT, FS>), dim3(blocks), dim3(MQ_NT), (size_t)(QT) * 16 * dv * 4, s, vid, ctx_l, dv, S, \
                       nh, txt, q0, nq, fs, hm, fr)
        if (qt == 4) { if (fs) CONE_MQ_LAUNCH(4, true); else CONE_MQ_LAUNCH(4, false); }
        else if (qt == 2) { if (fs) CONE_MQ_LAUNCH(2, true); else CONE_MQ_LAUNCH(2, false); }
        else { if (fs) CONE_MQ_LAUNCH(1, true); else CONE_MQ_LAUNCH(1, false); }
#undef CONE_MQ_LAUNCH
        CONE_LAUNCH_CHECK();
        q0 += 16 * qt;
    }
    return 0;
}

// ---- OPT-IN: many queries on the bf16 matrix cores, every fp32 product as six partial products of three-piece operands --
// At 64 queries the exact-fp32 kernel above is bound by the matrix pipe, not by the stream (32 FLOP per byte is past the
// ridge of 19.7: 3.7 ms where HBM needs 2.1).  gfx950's bf16 MFMA runs 16 x faster, and an fp32 product can ride on it without
// giving up fp32 accuracy (ffn_split.hip; tools/probe/split_bf16_probe.hip: the error of the six-product form equals the
// fp32 chain's): x = xh + xm + xl exactly (three bf16 pieces, 24 bits), x w ~= xl wh + xh wl + xm wm + xh wm + xm wh + xh wh.
//   * D[query][frame] tiles of v_mfma_f32_16x16x32_bf16: B = the frame's 32 channels of a k-step = the two float4 a lane
//     already streams (k slot (lg, j) <-> channel 32 t + 16 (j / 4) + 4 lg + j % 4), split into pieces in registers ONCE per
//     frame tile and used for all four query tiles; A = the query pieces as 1-KiB slabs [16 queries][4 lg][8 bf16] (a
//     lane's ds_read_b128: conflict-free).
//   * The query pieces of 64 queries x 512 channels are 192 KiB -- more than the LDS.  They are split ONCE per launch into an
//     image in the caller's workspace (pf_split_queries_kernel; L2-resident from then on), laid out [128-channel chunk][piece]
//     [query tile][k-step] in exactly the byte order of the LDS slabs, and the workgroup's twelve waves walk their frame tiles
//     in LOCK-STEP on the chunk index: the 48 KiB of chunk c + 2 stream in by LDS-DMA (four 1-KiB pieces per wave: no VGPRs,
//     no addressing) into a three-stage ring while chunk c is multiplied -- one raw barrier per chunk step.  (First cut: 32
//     queries per workgroup and two workgroups on one XCD per frame range, hoping for L2 hits on the second read: FETCH_SIZE
//     1.49 x the arena, 3.78 ms -- the waves' positions are megabytes apart and a 4 MB L2 cannot bridge that.)
// The running max per half window, the first-frame scores and the output format are those of the fp32 kernel.
typedef short pf_s8 __attribute__((ext_vector_type(8)));
typedef unsigned pf_u4 __attribute__((ext_vector_type(4)));
typedef unsigned pf_u2 __attribute__((ext_vector_type(2)));
typedef float pf_f2 __attribute__((ext_vector_type(2)));
typedef __bf16 pf_b2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pf_pk(float a, float b) {       // two floats -> packed bf16 pair, round to nearest even
    return __builtin_bit_cast(unsigned, __builtin_convertvector(pf_f2{a, b}, pf_b2));
}
__device__ __forceinline__ void pf_split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = pf_pk(a, b);
    const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = pf_pk(ra, rb);
    l = pf_pk(ra - __uint_as_float(m << 16), rb - __uint_as_float(m & 0xffff0000u));
}
__device__ __forceinline__ void pf_split8(const pf4& v0, const pf4& v1, pf_s8& h, pf_s8& m, pf_s8& l) {
    unsigned a[4], b[4], c[4];
    pf_split2(v0[0], v0[1], a[0], b[0], c[0]);
    pf_split2(v0[2], v0[3], a[1], b[1], c[1]);
    pf_split2(v1[0], v1[1], a[2], b[2], c[2]);
    pf_split2(v1[2], v1[3], a[3], b[3], c[3]);
    h = __builtin_bit_cast(pf_s8, pf_u4{a[0], a[1], a[2], a[3]});
    m = __builtin_bit_cast(pf_s8, pf_u4{b[0], b[1], b[2], b[3]});
    l = __builtin_bit_cast(pf_s8, pf_u4{c[0], c[1], c[2], c[3]});
}
#define PF_MFMA(acc, a, b) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0)
#define PF_GLDS16(src, dst) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src), \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)

constexpr int MQ3_QT = 4;                           // query tiles of 16 per launch
constexpr int MQ3_CHUNK = 3 * MQ3_QT * 4 * 1024;    // bytes of one 128-channel chunk of the image: [piece][query tile][k-step] slabs
constexpr int MQ3_NBUF = 3;
size_t frame_scores_split_image_bytes(int dv) { return (size_t)(dv >> 7) * MQ3_CHUNK; }

// queries q0 .. q0 + 63 (zeros past nq) -> the image: chunk c = channels [128 c, 128 c + 128), slab (piece, qt, tt), inside a
// slab query row r, lane group lg, half u: 8 B = channels 32 t + 16 u + 4 lg + 0 .. 3 of step t = 4 c + tt
__global__ __launch_bounds__(256) void pf_split_queries_kernel(const float* __restrict__ txt, int dv, int q0, int nq,
                                                               char* __restrict__ img) {
    const int i = blockIdx.x * 256 + threadIdx.x;           // (query, float4 of its vector)
    if (i >= MQ3_QT * 16 * (dv >> 2)) return;
    const int qi = i / (dv >> 2), c4 = i % (dv >> 2);
    const int qg = q0 + qi;
    pf4 v = pf4{0.f, 0.f, 0.f, 0.f};
    if (qg < nq) v = *reinterpret_cast<const pf4*>(txt + (size_t)qg * dv + c4 * 4);
    unsigned h0, m0, l0, h1, m1, l1;
    pf_split2(v[0], v[1], h0, m0, l0);
    pf_split2(v[2], v[3], h1, m1, l1);
    const int t = c4 >> 3, u = (c4 >> 2) & 1, lgq = c4 & 3, row = qi & 15;
    const int c = t >> 2, tt = t & 3, qt = qi >> 4;
    char* base = img + (size_t)c * MQ3_CHUNK + ((qt * 4 + tt) << 10) + row * 64 + lgq * 16 + u * 8;
    constexpr int pstride = MQ3_QT * 4 * 1024;
    *reinterpret_cast<pf_u2*>(base) = pf_u2{h0, h1};
    *reinterpret_cast<pf_u2*>(base + pstride) = pf_u2{m0, m1};
    *reinterpret_cast<pf_u2*>(base + 2 * pstride) = pf_u2{l0, l1};
}

__global__ __launch_bounds__(MQ_NT, 3) void frame_score_mq3_kernel(const float* __restrict__ vid, int64_t ctx_l, int dv, int S,
                                                                 int64_t nh, const char* __restrict__ img, int q0, int nq,
                                                                 float* __restrict__ hm, float* __restrict__ fr) {
    constexpr int QT = MQ3_QT;
    extern __shared__ __attribute__((aligned(16))) char ring[];         // MQ3_NBUF stages of MQ3_CHUNK bytes
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int nchunk = dv >> 7;
    constexpr int NW = MQ_NT / 64;
    constexpr int pstride = QT * 4 * 1024;
    const int rd = li * 64 + lg * 16;
    // tile slots of this workgroup = the tiles of its busiest wave (every wave takes every barrier; a wave out of tiles only
    // keeps the ring fed).  Half-blocks have ceil(S / 16) tiles, the video's last one possibly fewer.
    const int64_t h_step = (int64_t)gridDim.x * NW;
    const int tps = (S + 15) >> 4;
    const int tps_last = (int)((ctx_l - (nh - 1) * S + 15) >> 4);
    auto tiles_of = [&](int w) -> int64_t {
        const int64_t h0 = (int64_t)blockIdx.x * NW + w;
        if (h0 >= nh) return 0;
        const int64_t n = (nh - 1 - h0) / h_step + 1;
        const bool owns_last = (nh - 1 - h0) % h_step == 0;
        return n * tps - (owns_last ? tps - tps_last : 0);
    };
    int64_t slots = 0;
    for (int w = 0; w < NW; ++w) { const int64_t t = tiles_of(w); slots = t > slots ? t : slots; }
    if (slots == 0) return;
    const int64_t n_steps = slots * nchunk;
    // ring: the wave's four 1-KiB pieces of a chunk
    auto stream = [&](int64_t g) {                                      // chunk of global step g -> stage g % MQ3_NBUF
        const char* src = img + (size_t)(g % nchunk) * MQ3_CHUNK + (wave * 4 << 10) + lane * 16;
        char* dst = ring + (int)(g % MQ3_NBUF) * MQ3_CHUNK + (wave * 4 << 10);
#pragma unroll
        for (int i = 0; i < 4; ++i) PF_GLDS16(src + (i << 10), dst + (i << 10));
    };
    stream(0);
    if (n_steps > 1) stream(1);

    const int64_t h0 = (int64_t)blockIdx.x * NW + wave;
    bool live = h0 < nh;
    PfMqCursor<float> cu(vid, ctx_l, dv, S, nh, h_step, li, 4 * lg, h0, live);
    pf4 cur[8];
    if (live) {
#pragma unroll
        for (int s = 0; s < 8; ++s) cur[s] = pf_mq_ld(cu.fp + 16 * s);
    }
    pf4 mx[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) mx[qt] = pf4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int64_t g = 0;
    for (int64_t slot = 0; slot < slots; ++slot) {
        cu.look_ahead(live);
        pf4 acc[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = pf4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunk; ++c, ++g) {
            // stage g has landed (this wave's pieces: everything but the 4 pieces of stage g + 1 and, with the loads of the
            // previous step consumed by the compiler's own waits, nothing else); the barrier makes all twelve shares visible
            // and tells that everybody is done with stage g - 1, which the pieces of stage g + 2 overwrite.  The count is pieces x
            // stages left in flight: 4 while stage g + 1 follows, 0 on the workgroup's last step -- there nothing younger covers
            // the four pieces of stage g in a wave that is out of tiles (it issues no frame loads either), and vmcnt(4) would let
            // it through the barrier with its share of the stage still in the air.  (A live wave needs its frame loads of the
            // previous step right here anyway: the exact wait costs it nothing.)
            if (g + 1 < n_steps) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            pf4 nxt[8];
            if (live) {
                const float* np = c + 1 < nchunk ? cu.fp + 128 * (c + 1) : cu.fp2;
#pragma unroll
                for (int s = 0; s < 8; ++s) nxt[s] = pf_mq_ld(np + 16 * s);
            }
            if (g + 2 < n_steps) stream(g + 2);
            if (live) {
                const char* st = ring + (int)(g % MQ3_NBUF) * MQ3_CHUNK + rd;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    pf_s8 fh, fm, fl;
                    pf_split8(cur[2 * tt], cur[2 * tt + 1], fh, fm, fl);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        const char* sl = st + ((qt * 4 + tt) << 10);
                        const pf_s8 ah = *reinterpret_cast<const pf_s8*>(sl);
                        const pf_s8 am = *reinterpret_cast<const pf_s8*>(sl + pstride);
                        const pf_s8 al = *reinterpret_cast<const pf_s8*>(sl + 2 * pstride);
                        PF_MFMA(acc[qt], al, fh);                       // small terms first
                        PF_MFMA(acc[qt], ah, fl);
                        PF_MFMA(acc[qt], am, fm);
                        PF_MFMA(acc[qt], am, fh);
                        PF_MFMA(acc[qt], ah, fm);
                        PF_MFMA(acc[qt], ah, fh);
                    }
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) cur[s] = nxt[s];
            }
        }
        if (!live) continue;
        pf_mq_tile_end<QT, false>(cu, acc, mx, lg, q0, nq, nullptr, hm, fr);
        if (!cu.more) { live = false; continue; }
        cu.advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no LDS-DMA may outlive the workgroup's LDS
}

bool frame_scores_split_supported(int dv, int nq) { return nq >= 8 && dv % 128 == 0; }

static int launch_frame_scores_mq3(const float* vid, int64_t ctx_l, int dv, int S, int64_t nh, const float* txt, int nq, float* hm,
                                   float* fr, char* img, hipStream_t s) {
    static DeviceOnce once;
    const void* const fns[1] = {(const void*)frame_score_mq3_kernel};
    unsigned blocks = 0;
    if (int rc = pf_mq_grid(once, fns, MQ3_NBUF * MQ3_CHUNK, nh, "prefilter (split)", &blocks)) return rc;
    for (int q0 = 0; q0 < nq; q0 += 64) {
        const int rem = nq - q0;
        hipLaunchKernelGGL(pf_split_queries_kernel, dim3((unsigned)((MQ3_QT * 16 * (dv >> 2) + 255) / 256)), dim3(256), 0, s, txt, dv,
                           q0, nq, img);
        CONE_LAUNCH_CHECK();
        ProfScope ps(PK_FRAME_SCORE, ctx_l, dv, rem < 64 ? rem : 64, nullptr, s);
        hipLaunchKernelGGL(frame_score_mq3_kernel, dim3(blocks), dim3(MQ_NT), MQ3_NBUF * MQ3_CHUNK, s, vid, ctx_l, dv, S, nh,
                           (const char*)img, q0, nq, hm, fr);
        CONE_LAUNCH_CHECK();
    }
    return 0;
}

// ---- segmented forms: all queries of a split in three launches --------------------------------
// A group = one video and up to 4 of its queries (the clip rows are read once per group).
template <int VPL>
__global__ __launch_bounds__(256) void frame_score_groups_kernel(const float* __restrict__ arena,
                                                                 const float* __restrict__ cls,
                                                                 const int64_t* __restrict__ g_row0,
                                                                 const int* __restrict__ g_ctx_l,
                                                                 const int* __restrict__ g_q,
                                                                 const int64_t* __restrict__ q_fs_off,
                                                                 float* __restrict__ fs) {
    constexpr int DV = 256 * VPL, RPW = 4;
    const int g = blockIdx.y;
    const int ctx_l = g_ctx_l[g];
    const int lane = threadIdx.x & 63;
    const int wave_id = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * 4;
    if (wave_id * RPW >= ctx_l) return;
    const float* vid = arena + g_row0[g] * DV;
    int qi[4];
    float4 q[4][VPL];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qi[j] = g_q[g * 4 + j];
        const int src = qi[j] >= 0 ? qi[j] : g_q[g * 4];
#pragma unroll
        for (int v = 0; v < VPL; ++v) q[j][v] = reinterpret_cast<const float4*>(cls + (size_t)src * DV)[lane + 64 * v];
    }
    for (int r0 = wave_id * RPW; r0 < ctx_l; r0 += n_waves * RPW) {
        float4 x[RPW][VPL];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int row = min(r0 + r, ctx_l - 1);
#pragma unroll
            // (ordinary loads: the other groups of this video read the same rows again -- a split's arena sits in the caches)
            for (int v = 0; v < VPL; ++v) x[r][v] = reinterpret_cast<const float4*>(vid + (size_t)row * DV)[lane + 64 * v];
        }
        float part[RPW * 4];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[r * 4 + j] = pf_lane_dot<VPL>(x[r], q[j]);
        // the 16 sums by one butterfly (wave_sum_multi): lane l ends up with the total of (row l / 16, query (l / 4) % 4)
        const float s = wave_sum_multi<RPW * 4>(part, lane);
        PF_LANE_SLOT(RPW, 4, lane);
        int my_qi = qi[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) my_qi = my_g == j ? qi[j] : my_qi;
        if (writer && r0 + my_r < ctx_l && my_qi >= 0) fs[q_fs_off[my_qi] + r0 + my_r] = s;
    }
}

__global__ __launch_bounds__(256) void window_max_seg_kernel(const float* __restrict__ fs,
                                                             const int64_t* __restrict__ q_fs_off,
                                                             const int64_t* __restrict__ q_win_off,
                                                             const int* __restrict__ q_ctx_l, int W, int S,
                                                             float* __restrict__ win) {
    const int q = blockIdx.y;
    const int ctx_l = q_ctx_l[q];
    const int nw = (ctx_l + S - 1) / S + 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nw) return;
    const int s = max((i - 1) * S, 0), e = min((i - 1) * S + W, ctx_l);
    const float* f = fs + q_fs_off[q];
    float m = -INFINITY;
    for (int t = s; t < e; ++t) m = fmaxf(m, f[t]);
    win[q_win_off[q] + i] = m;
}

__global__ __launch_bounds__(256) void topk_seg_kernel(const float* __restrict__ win,
                                                       const int64_t* __restrict__ q_win_off,
                                                       const int* __restrict__ q_ctx_l, int S, int k,
                                                       int32_t* __restrict__ idx) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = (q_ctx_l[q] + S - 1) / S + 1;
    const float* row = win + q_win_off[q];
    if (n <= 1024) {
        // a short row (an Ego4D video: ~22 windows): the stable descending RANK of every window by counting -- rank = #{greater}
        // + #{equal with a lower index}, window j goes to slot rank if rank < k -- one pass and one barrier instead of k selection
        // passes with three barriers each (23 -> 5 us for one query; the same list: the order is a total one).  NaN scores
        // (an all-zero adapted clip row: cone/inference.py:258 divides by an un-eps'd norm) are ordered like torch.sort orders
        // them -- ahead of every number, equal among themselves -- so the ranks stay a permutation and every slot is written
        __shared__ float s_row[1024];
        for (int j = tid; j < n; j += 256) s_row[j] = row[j];
        for (int p = n + tid; p < k; p += 256) idx[(size_t)q * k + p] = -1;        // fewer windows than k: pad with -1
        __syncthreads();
        for (int j = tid; j < n; j += 256) {
            const float v = s_row[j];
            const bool v_nan = v != v;
            int rank = 0;
            for (int i = 0; i < n; ++i) {           // (every thread reads the same address: LDS broadcast)
                const float x = s_row[i];
                const bool x_nan = x != x;
                rank += (x > v) || (x_nan && !v_nan) || ((x == v || (x_nan && v_nan)) && i < j);
            }
            if (rank < k) idx[(size_t)q * k + rank] = j;
        }
        return;
    }
    float last_v = INFINITY;
    int last_i = -1;
    for (int p = 0; p < k; ++p) {
        if (p >= n) {   // fewer windows than k: pad with -1 (uniform branch)
            if (tid == 0) idx[(size_t)q * k + p] = -1;
            continue;
        }
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < n; j += 256) {
            const float v = row[j];
            if (tk_after(v, j, last_v, last_i) && tk_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
        tk_pass_pick<4>(bv, bi, idx + (size_t)q * k + p, nullptr, last_v, last_i);
    }
}

#ifndef CONE_PF_RPW
#define CONE_PF_RPW 4
#endif
#ifndef CONE_PF_WGS_PER_CU
#define CONE_PF_WGS_PER_CU 8
#endif
template <int N> using pf_int = std::integral_constant<int, N>;

// The streaming forms' grid, both element types.  Long videos: one wave per half window (WPH = 1), 8 workgroups per CU
// grid-striding; short ones (`wide`): a workgroup per half window (WPH = 4).
struct PfStreamGrid {
    bool wide;
    unsigned blocks;
    explicit PfStreamGrid(int64_t nh) : wide(nh < 4096) {
        const int64_t b = wide ? nh : (nh + 3) / 4;
        blocks = (unsigned)(b > 256 * CONE_PF_WGS_PER_CU ? 256 * CONE_PF_WGS_PER_CU : b);
    }
};
// ... and their passes over the video: 4, 2 or 1 queries each.  3 remaining queries ride a 4-query launch (the fourth slot
// repeats the last query and stores nothing): one pass instead of two; a query's bits do not depend on the launch it shares
// (pf_dot4, wave_sum_multi).  launch(QG, WPH, blocks, q0) with QG, WPH as pf_int<> enqueues the kernel instantiation.
template <class L>
static int pf_stream_passes(int64_t ctx_l, int dv, int64_t nh, int nq, hipStream_t s, L launch) {
    const PfStreamGrid g(nh);
    for (int q0 = 0; q0 < nq;) {
        const int rem = nq - q0;
        const int qg = rem >= 3 ? 4 : (rem >= 2 ? 2 : 1);
        ProfScope ps(PK_FRAME_SCORE, ctx_l, dv, qg, nullptr, s);
        auto go = [&](auto QG) { if (g.wide) launch(QG, pf_int<4>{}, g.blocks, q0); else launch(QG, pf_int<1>{}, g.blocks, q0); };
        if (qg == 4) go(pf_int<4>{}); else if (qg == 2) go(pf_int<2>{}); else go(pf_int<1>{});
        q0 += qg;
        CONE_LAUNCH_CHECK();
    }
    return 0;
}

template <int VPL>
static int launch_frame_scores(const float* vid, int64_t ctx_l, int S, int64_t nh, const float* txt, int nq, float* fs,
                               float* hm, float* fr, hipStream_t s) {
    return pf_stream_passes(ctx_l, 256 * VPL, nh, nq, s, [&](auto QG, auto WPH, unsigned blocks, int q0) {
        hipLaunchKernelGGL((frame_score_kernel<VPL, decltype(QG)::value, CONE_PF_RPW, decltype(WPH)::value>), dim3(blocks), dim3(256), 0,
                           s, vid, ctx_l, S, nh, txt, q0, nq, fs, hm, fr);
    });
}

// the gated form: every group of 4 queries in ONE launch (a query's bits do not depend on its group); no frame scores
template <int VPL>
static int launch_frame_scores_gated(const float* vid, int64_t ctx_l, int S, int64_t nh, const float* txt, int nq, float* hm,
                                     float* fr, const int* gate, hipStream_t s) {
    const PfStreamGrid g(nh);
    ProfScope ps(PK_FRAME_SCORE, ctx_l, 256 * VPL, 4, nullptr, s);
    const dim3 grid(g.blocks, (unsigned)((nq + 3) / 4));
    if (g.wide) hipLaunchKernelGGL((frame_score_gated_kernel<VPL, CONE_PF_RPW, 4>), grid, dim3(256), 0, s, vid, ctx_l, S, nh, txt, nq, hm, fr, gate);
    else hipLaunchKernelGGL((frame_score_gated_kernel<VPL, CONE_PF_RPW, 1>), grid, dim3(256), 0, s, vid, ctx_l, S, nh, txt, nq, hm, fr, gate);
    CONE_LAUNCH_CHECK();
    return 0;
}

// ---- OPT-IN: the bf16 pre-filter -- bf16 context rows, bf16 operands, fp32 accumulation ------------------------------------
// ONE arithmetic contract for every form: score[q][f] = sum_c bf16(ctx[f][c]) * bf16(cls[q][c]); both operands rounded once
// (round to nearest even: the arena by its producer -- cone_rows_to_bf16 / cone_adapter_norm_bf16 --, the query vectors
// here), every product exact in fp32 (8 x 8 significand bits), the sum in fp32 in the form's own order.  NOT fp32-accurate:
// ~2^-8 relative per operand.  The arena is half the bytes of the fp32 one (the stream is HBM-bound), and the many-query form
// needs 16 x fewer matrix instructions per score than v_mfma_f32_16x16x4_f32.  Window scores: the half-window running max,
// the first-frame term and window_combine_kernel's rule, as above; no frame-score matrix in this mode.
//   frame_score_bf16_kernel        : the streaming form (frame_score_kernel's shape): a row arrives as 16-B non-temporal lane loads
//                                    (8 bf16 = lane's channels 8 c .. 8 c + 7, c = lane + 64 v), widened to fp32 by a shift; dv is
//                                    any multiple of 32 up to 1024 (lanes past dv / 8 hold zeros and load nothing)
//   frame_score_mq_bf16_kernel     : 16 / 32 / 64 queries per pass on v_mfma_f32_16x16x32_bf16
//   frame_score_groups_bf16_kernel : the streaming form for a whole split (one video x up to 4 queries per group)
// From how many queries the matrix-core form takes over: CONE_PF16_MQ_MIN (A/B: compile with another value).  The streaming
// form costs one pass per 4 queries, the matrix-core form one pass per 64, so 5 is the first count at which the latter saves a
// whole pass over the arena; below 5 both are one HBM-bound pass and the streaming form (no LDS prologue, 8 workgroups per
// CU) is kept.  (tools/prefilter_bf16_bench.py measures both sides of it: profiles/prefilter_bf16.txt.)
#ifndef CONE_PF16_MQ_MIN
#define CONE_PF16_MQ_MIN 5
#endif

__device__ __forceinline__ pf_u4 pf16_ld(const uint16_t* p, bool nt) {
    if (nt) return __builtin_nontemporal_load(reinterpret_cast<const pf_u4*>(p));
    return *reinterpret_cast<const pf_u4*>(p);
}
__device__ __forceinline__ float pf16_rne(float a) { return __uint_as_float(pf_pk(a, 0.f) << 16); }    // fp32 -> bf16 -> fp32

// <x, q> over a lane's 8 channels: two pf_dot4 (the pinned fma chain of the fp32 kernels) on the widened values, added
__device__ __forceinline__ float pf16_dot8(const pf_u4& x, const float (&q)[8]) {
#pragma clang fp contract(off)
    const float4 a = make_float4(__uint_as_float(x[0] << 16), __uint_as_float(x[0] & 0xffff0000u),
                                 __uint_as_float(x[1] << 16), __uint_as_float(x[1] & 0xffff0000u));
    const float4 b = make_float4(__uint_as_float(x[2] << 16), __uint_as_float(x[2] & 0xffff0000u),
                                 __uint_as_float(x[3] << 16), __uint_as_float(x[3] & 0xffff0000u));
    const float d0 = pf_dot4(a, make_float4(q[0], q[1], q[2], q[3]));
    const float d1 = pf_dot4(b, make_float4(q[4], q[5], q[6], q[7]));
    return d0 + d1;
}

// a query vector's share of this lane, rounded ONCE to bf16 and held widened (zeros past dv)
template <int VPL>
__device__ __forceinline__ void pf16_load_query(const float* __restrict__ row, int dv, int lane, float (&q)[VPL][8]) {
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        const int c = lane + 64 * v;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (c * 8 < dv) {
            a = reinterpret_cast<const float4*>(row)[2 * c];
            b = reinterpret_cast<const float4*>(row)[2 * c + 1];
        }
        q[v][0] = pf16_rne(a.x); q[v][1] = pf16_rne(a.y); q[v][2] = pf16_rne(a.z); q[v][3] = pf16_rne(a.w);
        q[v][4] = pf16_rne(b.x); q[v][5] = pf16_rne(b.y); q[v][6] = pf16_rne(b.z); q[v][7] = pf16_rne(b.w);
    }
}

// One wave over rows sub * RPW, + step * RPW, ... of a half window of n rows at `base`: RPW rows in flight, the NV = RPW * QG
// (row, query) sums by one butterfly.  Returns the running max of query my_g = (lane / (64 / NV)) % QG over the wave's rows
// (every lane of that query's groups holds it); `first` = the score of row 0 (held by the lanes with row slot 0 of a wave
// with sub == 0).  The per-lane chain and the butterfly's pairs do not depend on QG, so a query's bits do not depend on the
// launch it shares, and the per-video and the grouped kernel produce the same bits.
template <int VPL, int QG, int RPW, bool NT>
__device__ __forceinline__ float pf16_half_block(const uint16_t* __restrict__ base, int n, int dv, const float (&q)[QG][VPL][8],
                                                 int lane, int sub, int step, float& first) {
    constexpr int NV = RPW * QG;
    const int my_r = (lane / (64 / NV)) / QG;
    float m = -INFINITY;
    for (int j0 = sub * RPW; j0 < n; j0 += step * RPW) {
        pf_u4 x[RPW][VPL];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const int row = min(j0 + r, n - 1);
#pragma unroll
            for (int v = 0; v < VPL; ++v) {
                const int c = lane + 64 * v;
                x[r][v] = pf_u4{0u, 0u, 0u, 0u};
                if (c * 8 < dv) x[r][v] = pf16_ld(base + (size_t)row * dv + 8 * c, NT);
            }
        }
        float part[NV];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                float s = 0.f;
#pragma unroll
                for (int v = 0; v < VPL; ++v) s += pf16_dot8(x[r][v], q[g][v]);
                part[r * QG + g] = s;
            }
        const float s = wave_sum_multi<NV>(part, lane);                // = the total of (row j0 + my_r, query my_g)
        if (j0 + my_r < n) {
            m = fmaxf(m, s);
            if (my_r == 0 && j0 == 0) first = s;
        }
    }
    return pf_slot_max<RPW>(m);
}

template <int VPL /* 16-B loads per lane and row: dv <= 512 VPL */, int QG, int RPW, int WPH>
__global__ __launch_bounds__(256) void frame_score_bf16_kernel(const uint16_t* __restrict__ vid, int64_t ctx_l, int dv, int S,
                                                               int64_t nh, const float* __restrict__ txt, int q0, int nq,
                                                               float* __restrict__ hm, float* __restrict__ fr) {
    constexpr int UPB = 4 / WPH;
    __shared__ float red[4][QG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = wave % WPH;
    PF_LANE_SLOT(RPW, QG, lane);
    float q[QG][VPL][8];
#pragma unroll
    for (int g = 0; g < QG; ++g) pf16_load_query<VPL>(txt + (size_t)min(q0 + g, nq - 1) * dv, dv, lane, q[g]);
    for (int64_t h = (int64_t)blockIdx.x * UPB + wave / WPH; h < nh; h += (int64_t)gridDim.x * UPB) {
        const int64_t r_lo = h * S;
        const int n = (int)min((int64_t)S, ctx_l - r_lo);            // frames of this half window
        float first = 0.f;
        const float m = pf16_half_block<VPL, QG, RPW, CONE_PF_NT != 0>(vid + r_lo * dv, n, dv, q, lane, sub, WPH, first);
        if (out_lane && sub == 0 && q0 + my_g < nq) fr[(size_t)(q0 + my_g) * nh + h] = first;     // the block's first frame
        pf_store_half_max<QG, WPH>(m, my_g, out_lane, lane, wave, red, q0, nq, nh, h, hm);
    }
}

template <int VPL>
static int launch_frame_scores_bf16(const uint16_t* vid, int64_t ctx_l, int dv, int S, int64_t nh, const float* txt, int nq,
                                    float* hm, float* fr, hipStream_t s) {
    return pf_stream_passes(ctx_l, dv, nh, nq, s, [&](auto QG, auto WPH, unsigned blocks, int q0) {
        hipLaunchKernelGGL((frame_score_bf16_kernel<VPL, decltype(QG)::value, CONE_PF_RPW, decltype(WPH)::value>), dim3(blocks), dim3(256),
                           0, s, vid, ctx_l, dv, S, nh, txt, q0, nq, hm, fr);
    });
}

// Many queries: D[query][frame] tiles of v_mfma_f32_16x16x32_bf16.  k slot (lg, j) of k-step t <-> channel 32 t + 8 lg + j on both
// operands, so a lane's B fragment (frame li, its 8 k slots) is ONE 16-B load from the arena -- no conversion, no split on the
// frame side -- and its A fragment one ds_read_b128 from the query image: 1-KiB slabs [16 queries][4 lg][8 bf16] per (query
// tile, k-step), rounded and laid out once per launch by the workgroup's prologue (64 queries x 1024 channels = 128 KiB: the
// LDS holds every shape).  A wave owns whole half windows, 16 frames per tile; the loads of the next block of PF16_KS k-steps
// (256 channels: 512 B of each of the tile's 16 rows) are in flight under the MFMAs of the current one, across tiles and half
// windows.  dv / 32 need not be a multiple of PF16_KS: the last block is short (uniform guards).  Ordinary loads, as in the fp32
// kernel (CONE_PF_NT_MQ): a row's 128-B line is fetched by two consecutive instructions.
constexpr int PF16_KS = 8;

template <int QT /* query tiles of 16 */>
__global__ __launch_bounds__(MQ_NT, 3) void frame_score_mq_bf16_kernel(const uint16_t* __restrict__ vid, int64_t ctx_l, int dv,
                                                                     int S, int64_t nh, const float* __restrict__ txt, int q0,
                                                                     int nq, float* __restrict__ hm, float* __restrict__ fr) {
    extern __shared__ __attribute__((aligned(16))) char qb[];           // [QT][dv / 32] slabs of 1 KiB
    const int tid = threadIdx.x, lane = tid & 63;
    const int li = lane & 15, lg = lane >> 4;
    const int nks = dv >> 5;                                             // k-steps of 32 channels
    for (int i = tid; i < QT * 16 * (dv >> 3); i += MQ_NT) {             // (query, 8 channels of its vector)
        const int qi = i / (dv >> 3), c8 = i % (dv >> 3);
        const int qg = q0 + qi;
        pf4 a = pf4{0.f, 0.f, 0.f, 0.f}, b = a;
        if (qg < nq) {
            a = *reinterpret_cast<const pf4*>(txt + (size_t)qg * dv + c8 * 8);
            b = *reinterpret_cast<const pf4*>(txt + (size_t)qg * dv + c8 * 8 + 4);
        }
        *reinterpret_cast<pf_u4*>(qb + (((qi >> 4) * nks + (c8 >> 2)) << 10) + (qi & 15) * 64 + (c8 & 3) * 16) =
            pf_u4{pf_pk(a[0], a[1]), pf_pk(a[2], a[3]), pf_pk(b[0], b[1]), pf_pk(b[2], b[3])};
    }
    __syncthreads();
    const int rd = li * 64 + lg * 16;
    const int nchunk = (nks + PF16_KS - 1) / PF16_KS;
    constexpr int NW = MQ_NT / 64;
    const int64_t h0 = (int64_t)blockIdx.x * NW + (tid >> 6);
    if (h0 >= nh) return;
    PfMqCursor<uint16_t> cu(vid, ctx_l, dv, S, nh, (int64_t)gridDim.x * NW, li, 8 * lg, h0);
    pf_u4 cur[PF16_KS];
#pragma unroll
    for (int s = 0; s < PF16_KS; ++s) {
        cur[s] = pf_u4{0u, 0u, 0u, 0u};
        if (s < nks) cur[s] = pf16_ld(cu.fp + 32 * s, CONE_PF_NT_MQ != 0);
    }
    pf4 mx[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) mx[qt] = pf4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    while (true) {
        cu.look_ahead();
        pf4 acc[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = pf4{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nchunk; ++c) {
            const int kb = c * PF16_KS;
            const bool last = c + 1 == nchunk;
            const uint16_t* np = last ? cu.fp2 : cu.fp + 32 * (kb + PF16_KS);      // the next block's first k-step of this lane
            const int n_nxt = last ? nks : nks - (kb + PF16_KS);              // k-steps it has (>= 1)
            pf_u4 nxt[PF16_KS];
#pragma unroll
            for (int s = 0; s < PF16_KS; ++s) {
                nxt[s] = pf_u4{0u, 0u, 0u, 0u};
                if (s < n_nxt) nxt[s] = pf16_ld(np + 32 * s, CONE_PF_NT_MQ != 0);
            }
#pragma unroll
            for (int s = 0; s < PF16_KS; ++s) {
                if (kb + s < nks) {
                    const pf_s8 bb = __builtin_bit_cast(pf_s8, cur[s]);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        const pf_s8 aa = *reinterpret_cast<const pf_s8*>(qb + ((qt * nks + kb + s) << 10) + rd);
                        PF_MFMA(acc[qt], aa, bb);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PF16_KS; ++s) cur[s] = nxt[s];
        }
        pf_mq_tile_end<QT, false>(cu, acc, mx, lg, q0, nq, nullptr, hm, fr);
        if (!cu.more) break;
        cu.advance();
    }
}

static int launch_frame_scores_mq_bf16(const uint16_t* vid, int64_t ctx_l, int dv, int S, int64_t nh, const float* txt, int nq,
                                       float* hm, float* fr, hipStream_t s) {
    static DeviceOnce once;     // up to 128 KiB of LDS (64 queries x 1024 channels)
    const void* const fns[3] = {(const void*)frame_score_mq_bf16_kernel<4>, (const void*)frame_score_mq_bf16_kernel<2>,
                                (const void*)frame_score_mq_bf16_kernel<1>};
    unsigned blocks = 0;
    if (int rc = pf_mq_grid(once, fns, 128 * 1024, nh, "prefilter (bf16)", &blocks)) return rc;
    for (int q0 = 0; q0 < nq;) {
        const int rem = nq - q0, qt = pf_mq_tiles(rem, 4);             // 64 / 32 / 16 queries: the LDS holds every shape
        ProfScope ps(PK_FRAME_SCORE, ctx_l, dv, rem < 16 * qt ? rem : 16 * qt, nullptr, s);
#define CONE_MQ16_LAUNCH(QT)                                                                                                \
    hipLaunchKernelGGL((frame_score_mq_bf16_kernel<QT>), dim3(blocks), dim3(MQ_NT), (size_t)(QT) * 16 * dv * 2, s, vid, ctx_l, dv, S, \
                       nh, txt, q0, nq, hm, fr)
        if (qt == 4) CONE_MQ16_LAUNCH(4); else if (qt == 2) CONE_MQ16_LAUNCH(2); else CONE_MQ16_LAUNCH(1);
#undef CONE_MQ16_LAUNCH
        CONE_LAUNCH_CHECK();
        q0 += 16 * qt;
    }
    return 0;
}

// The grouped form for a whole split: one video x up to 4 of its queries per group (blockIdx.y), a wave per half window --
// pf16_half_block with four query slots, so the bits of frame_score_bf16_kernel -- and NO intermediate planes: the half-window
// max goes straight into the two windows that contain the half window, the first-frame score (odd W) into the window before,
// by atomic max on the window scores (preset to -inf by win_fill_seg_kernel).  max is order-free, so the result is the one
// window_combine_kernel computes, bit for bit; topk_seg_kernel reads it unchanged.  (Ordinary loads: the video's other groups
// read the same rows again.)
__device__ __forceinline__ void pf_atomic_max(float* p, float v) {      // *p = max(*p, v) on the fp32 order; NaN is dropped (fmaxf)
    if (v != v) return;
    if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

__global__ __launch_bounds__(256) void win_fill_seg_kernel(const int64_t* __restrict__ q_win_off, const int* __restrict__ q_ctx_l,
                                                           int S, float* __restrict__ win) {
    const int q = blockIdx.y;
    const int nw = (q_ctx_l[q] + S - 1) / S + 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nw) win[q_win_off[q] + i] = -INFINITY;
}

template <int VPL>
__global__ __launch_bounds__(256) void frame_score_groups_bf16_kernel(const uint16_t* __restrict__ arena, int dv,
                                                                      const float* __restrict__ cls,
                                                                      const int64_t* __restrict__ g_row0,
                                                                      const int* __restrict__ g_ctx_l,
                                                                      const int* __restrict__ g_q,
                                                                      const int64_t* __restrict__ q_win_off, int S, int odd,
                                                                      float* __restrict__ win) {
    constexpr int RPW = 4, QG = 4;
    const int g = blockIdx.y;
    const int ctx_l = g_ctx_l[g];
    const int nh = (ctx_l + S - 1) / S;
    const int lane = threadIdx.x & 63;
    const int wave_id = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * 4;
    if (wave_id >= nh) return;
    const uint16_t* vid = arena + g_row0[g] * dv;
    int qi[QG];
    float q[QG][VPL][8];
#pragma unroll
    for (int j = 0; j < QG; ++j) {
        qi[j] = g_q[g * 4 + j];
        pf16_load_query<VPL>(cls + (size_t)(qi[j] >= 0 ? qi[j] : g_q[g * 4]) * dv, dv, lane, q[j]);
    }
    PF_LANE_SLOT(RPW, QG, lane);
    int my_qi = qi[0];
#pragma unroll
    for (int j = 1; j < QG; ++j) my_qi = my_g == j ? qi[j] : my_qi;
    for (int h = wave_id; h < nh; h += n_waves) {
        const int n = min(S, ctx_l - h * S);
        float first = 0.f;
        const float m = pf16_half_block<VPL, QG, RPW, false>(vid + (size_t)h * S * dv, n, dv, q, lane, 0, 1, first);
        if (out_lane && my_qi >= 0) {
            float* w = win + q_win_off[my_qi];
            pf_atomic_max(w + h, m);
            pf_atomic_max(w + h + 1, m);
            if (odd && h >= 1) pf_atomic_max(w + h - 1, first);
        }
    }
}

// ---- the certified pre-filter: bf16 scan, fp32 rescore of a few candidates, a proof per query, a gated fp32 fallback ------
// cone_prefilter_topk_certified returns the top-k windows of the exact-fp32 streaming form, bit for bit, and reads the bf16
// shadow (half the bytes) to get there whenever a query's scores are separable:
//   coarse scan                          : the bf16 forms above, unchanged
//   pf_cand_chunk / pf_cand_merge_kernel : the n_cand best coarse windows as an unordered set (bisection on the score bits)
//   pf_rescore_kernel                    : the candidates' window scores in the streaming form's own fp32 arithmetic
//   pf_certify_kernel                    : the k best candidates by (exact score desc, index asc); certified[q] = 1 iff no
//                                          window outside the candidate set can precede the k-th: t - c_last > E(q)
//   frame_score_gated_kernel + pf_fallback_chunk_kernel + pf_fallback_merge_kernel : the full fp32 scan and top-k of the
//                                          queries that are NOT certified; gated on the device, no host read-back
// The bound.  R >= max_f |v_f - bf16(v_f)|, N >= max_f max(|v_f|, |bf16(v_f)|) (2-norms; measured by pf_index_kernel), qh =
// bf16(q), u = 2^-24, g = (dv + 1) u / (1 - (dv + 1) u).  For every frame
//   |coarse_f - exact_f| <= |fl(vh.qh) - vh.qh| + |(vh - v).qh| + |v.(qh - q)| + |v.q - fl(v.q)|
//                        <= g N |qh|         + R |qh|        + N |qh - q|   + g N |q|                (Cauchy-Schwarz)
// in any summation order, and |max_f a_f - max_f b_f| <= max_f |a_f - b_f|, so E = (R |qh| + N |qh - q| + 2 g N max(|q|, |qh|))
// (1 + 2^-10) + PF_CERT_TINY (1 + |qh| + N) bounds |coarse - exact| of every window.  The last term covers operands, products
// and partial sums below 2^-126 (flushed or rounded as subnormals: at most 2^-126 each, 2 dv + 64 of them, and 2^-126 |qh|_1
// resp. 2^-126 |vh|_1 for flushed operands); the factor covers the rounding of E's own evaluation (fp64 here).
constexpr float PF_CERT_INFLATE = 1.0f + 0x1p-10f;      // over the fp32 rounding of a measured norm (pf_index_kernel)
constexpr float PF_INDEX_TINY = 0x1p-55f;               // over the squares too small for fp32 (pf_index_kernel)
constexpr double PF_CERT_TINY = 0x1p-114;               // 2^-126 (2 dv + 64 + 32 |qh| + 32 N) <= this (1 + |qh| + N), dv <= 1024
constexpr int PF_CERT_MAX_CAND = 256 * TK_PT;           // candidates of a query in the selection's registers (topk_merge_kernel's limit)
constexpr int PF_INDEX_MAX_DIM = 16384;

// out = bf16_rne(x) (rows_to_bf16_kernel's bits: the same conversion) and, per row, r = |x - bf16(x)|, n = max(|x|, |bf16(x)|):
// one wave per row, fp32 sums of squares (lane-strided float4, then the butterfly), the maxima over the grid by atomicMax on
// the bit patterns (non-negative floats order like their bits; a NaN is stored as the positive quiet NaN, above +inf, so it
// sticks).  x - bf16(x) is exact in fp32 (the low bits of x).  Inflation: PF_CERT_INFLATE over the sums' rounding ((dim / 64
// + 6) roundings on non-negative terms -- 4 fmas per float4 and lane, then the butterfly --, halved by the square root, plus
// the root and the inflation themselves: about 2^-17 relative at dim = PF_INDEX_MAX_DIM, against 2^-10), and an
// absolute PF_INDEX_TINY over squares too small for fp32 (each loses at most 2^-126, flushed or not: sqrt(dim 2^-126) <= 2^-56).
__global__ __launch_bounds__(256) void pf_index_kernel(const float* __restrict__ x, int64_t n_rows, int dim,
                                                       uint16_t* __restrict__ out, int* __restrict__ err_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int n4 = dim >> 2;
    float mr = 0.f, mn = 0.f;
    for (int64_t row = wave_id; row < n_rows; row += n_waves) {
        const float4* src = reinterpret_cast<const float4*>(x + row * dim);
        uint2* dst = reinterpret_cast<uint2*>(out + row * dim);
        float sr = 0.f, sx = 0.f, sh = 0.f;
        for (int c = lane; c < n4; c += 64) {
            const float4 v = src[c];
            const unsigned lo = pf_pk(v.x, v.y), hi = pf_pk(v.z, v.w);
            dst[c] = make_uint2(lo, hi);
            const float h[4] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                                __uint_as_float(hi & 0xffff0000u)};
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = e[j] - h[j];
                sr = __builtin_fmaf(d, d, sr);
                sx = __builtin_fmaf(e[j], e[j], sx);
                sh = __builtin_fmaf(h[j], h[j], sh);
            }
        }
        sr = wave_sum(sr); sx = wave_sum(sx); sh = wave_sum(sh);
        // (a NaN fails both comparisons: carried over explicitly)
        const float r = sqrtf(sr), n = sqrtf(fmaxf(sx, sh));
        mr = (r != r || mr != mr) ? NAN : fmaxf(mr, r);
        mn = (sx != sx || sh != sh || mn != mn) ? NAN : fmaxf(mn, n);
    }
    if (lane == 0 && wave_id < n_rows) {
        const float R = mr * PF_CERT_INFLATE + PF_INDEX_TINY, N = mn * PF_CERT_INFLATE + PF_INDEX_TINY;
        atomicMax(err_bits, R == R ? __float_as_int(R) : 0x7fc00000);
        atomicMax(err_bits + 1, N == N ? __float_as_int(N) : 0x7fc00000);
    }
}

// One workgroup per (candidate slot, query): window i = cand[q][slot] covers frames [max((i-1)S, 0), min((i-1)S + W, ctx_l));
// its sixteen waves take the frames four at a time each (loads of four rows in flight per wave), every frame's score by pf_lane_dot and the
// butterfly of wave_sum_multi<1> -- the bits frame_score_kernel gives that (frame, query) -- and the max (order-free; fmaxf
// skips a NaN frame score, a window of NaN frames scores -inf) through LDS.  An empty slot (index < 0) scores -inf.
// ---- the candidates: the top-k SET of a row, unordered ------------------------------------------------------------------
// The proof needs the n_cand best coarse windows as a set and the smallest score among them, not their order, and n_cand =
// 128 is past what the sort-based selection of the top-k kernels handles (k <= 64: tk_wave_select_fast): their pass-based
// form is n_cand dependent passes per wave, twice per kernel.  Here the workgroup finds the k-th largest key by bisection
// on the bits -- 32 steps of (one ballot + popcount per register slot, one barrier) -- where key = the score's bit pattern
// mapped to an unsigned that orders like the float (-0 counted as +0), settles ties at that key by a second bisection on
// the window index (lower first: the stable order's set), and compacts the chosen pairs by ballot ranks.  The same total
// order as tk_better, so the same SET as the first k of the stable descending sort.
__device__ __forceinline__ unsigned pf_key(float v) {
    const unsigned b = __float_as_uint(v + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int PT, class F>
__device__ __forceinline__ int pf_block_count(F pred, int (*cnt)[4], int& par) {     // over the PT slots of all 256 threads
    int c = 0;
#pragma unroll
    for (int u = 0; u < PT; ++u) c += __popcll(__ballot(pred(u)));
    if ((threadIdx.x & 63) == 0) cnt[par][threadIdx.x >> 6] = c;
    __syncthreads();
    const int t = cnt[par][0] + cnt[par][1] + cnt[par][2] + cnt[par][3];
    par ^= 1;                           // the next call writes the other set: one barrier per call is enough
    return t;
}

// (gv, gi)[0 .. k) <- the k best of the pairs (index 0x7fffffff = empty slot), in no particular order; fewer than k pairs:
// the tail is (-inf, idx_none).  Every thread of the workgroup calls it (barriers inside).
template <int PT>
__device__ __forceinline__ void pf_block_select_set(const float (&v)[PT], const int (&ix)[PT], int k, float* gv, int* gi,
                                                    int idx_none) {
    __shared__ int cnt[2][4];
    __shared__ int w_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    unsigned key[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) key[u] = ix[u] != 0x7fffffff ? pf_key(v[u]) : 0u;       // (a valid key is >= pf_key(-inf) > 0)
    unsigned T = 0;                     // the k-th largest key: the largest T with #{key >= T} >= k (0: fewer than k pairs)
    for (int b = 31; b >= 0; --b) {
        const unsigned c = T | (1u << b);
        if (pf_block_count<PT>([&](int u) { return key[u] >= c; }, cnt, par) >= k) T = c;
    }
    const int gt = pf_block_count<PT>([&](int u) { return key[u] > T; }, cnt, par);
    const int eq = T ? pf_block_count<PT>([&](int u) { return key[u] == T; }, cnt, par) : 0;
    const int r = k - gt;               // how many of the pairs AT the key are taken: those of the lowest indices
    int J = 0x7fffffff;                 // ... = the indices <= J, J = the r-th smallest index at the key
    if (eq > r) {                       // (uniform)
        J = 0;
        for (int b = 30; b >= 0; --b) {
            const int c = J | (1 << b);
            if (pf_block_count<PT>([&](int u) { return key[u] == T && ix[u] < c; }, cnt, par) < r) J = c;
        }
    }
    auto chosen = [&](int u) { return key[u] > T || (T != 0 && key[u] == T && ix[u] <= J); };
    int mine = 0;
#pragma unroll
    for (int u = 0; u < PT; ++u) mine += __popcll(__ballot(chosen(u)));
    if (lane == 0) w_tot[wave] = mine;
    __syncthreads();
    int pos = 0;
    for (int w2 = 0; w2 < wave; ++w2) pos += w_tot[w2];
    const int total = w_tot[0] + w_tot[1] + w_tot[2] + w_tot[3];       // = min(k, pairs)
#pragma unroll
    for (int u = 0; u < PT; ++u) {
        const bool c = chosen(u);
        const unsigned long long bal = __ballot(c);
        if (c) {
            const int at = pos + __popcll(bal & ((1ull << lane) - 1ull));
            gv[at] = v[u];
            gi[at] = ix[u];
        }
        pos += __popcll(bal);
    }
    for (int e = total + threadIdx.x; e < k; e += 256) { gv[e] = -INFINITY; gi[e] = idx_none; }
}

// level 1: the set of a chunk of TK_CH window scores (TK_LOAD_CHUNK: a NaN is never chosen)
__global__ __launch_bounds__(256) void pf_cand_chunk_kernel(const float* __restrict__ sc, int64_t n, int k, float* __restrict__ cval,
                                                            int* __restrict__ cidx, int n_chunks) {
    const int q = blockIdx.y, ch = blockIdx.x;
    const int64_t base = (int64_t)ch * TK_CH;
    const int m = (int)min((int64_t)TK_CH, n - base);
    const float* row = sc + (size_t)q * n + base;
    TK_LOAD_CHUNK(v, ix, base, m, row[j]);
    pf_block_select_set<TK_PT>(v, ix, k, cval + ((size_t)q * n_chunks + ch) * k, cidx + ((size_t)q * n_chunks + ch) * k, 0x7fffffff);
}

// level 2: the set of the chunk sets' n_in = n_chunks * k <= 256 * TK_PT pairs -> the query's candidates (index -1: none)
__global__ __launch_bounds__(256) void pf_cand_merge_kernel(const float* __restrict__ cval, const int* __restrict__ cidx, int n_in,
                                                            int k, int32_t* __restrict__ cand, float* __restrict__ coarse) {
    const int q = blockIdx.x;
    float v[TK_PT];
    int ix[TK_PT];
    tk_load_list(cval + (size_t)q * n_in, cidx + (size_t)q * n_in, n_in, v, ix);
    pf_block_select_set<TK_PT>(v, ix, k, coarse + (size_t)q * k, cand + (size_t)q * k, -1);
}

constexpr int PF_RS_NT = 1024;      // 16 waves x 4 rows: a 125-frame window in two rounds of loads (n_cand workgroups cannot fill the card: latency counts)
template <int VPL>
__global__ __launch_bounds__(PF_RS_NT) void pf_rescore_kernel(const float* __restrict__ vid, int64_t ctx_l, int W, int S,
                                                         const float* __restrict__ txt, const int32_t* __restrict__ cand,
                                                         int n_cand, float* __restrict__ exact) {
    constexpr int DV = 256 * VPL, RPW = 4;
    constexpr int NW = PF_RS_NT / 64;
    __shared__ float red[NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.y, slot = blockIdx.x;
    const int32_t i = cand[(size_t)q * n_cand + slot];
    float m = -INFINITY;
    if (i >= 0) {                                                   // (uniform over the workgroup)
        const int64_t lo = max(((int64_t)i - 1) * S, (int64_t)0), hi = min(((int64_t)i - 1) * S + W, ctx_l);
        float4 qv[1][VPL];
#pragma unroll
        for (int v = 0; v < VPL; ++v) qv[0][v] = reinterpret_cast<const float4*>(txt + (size_t)q * DV)[lane + 64 * v];
        for (int64_t f0 = lo + wave * RPW; f0 < hi; f0 += NW * RPW) {
            float4 x[RPW][VPL];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int64_t row = min(f0 + r, hi - 1);
#pragma unroll
                for (int v = 0; v < VPL; ++v) x[r][v] = reinterpret_cast<const float4*>(vid + row * DV)[lane + 64 * v];
            }
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float part[1] = {pf_lane_dot<VPL>(x[r], qv[0])};
                const float s = wave_sum_multi<1>(part, lane);
                if (f0 + r < hi) m = fmaxf(m, s);
            }
        }
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) t = fmaxf(t, red[w2]);
        exact[(size_t)q * n_cand + slot] = t;
    }
}

// One workgroup per query.  The k_eff = min(k, num_window) best candidates by (exact score desc, index asc) -> idx / val rows
// of k entries ((-1, -inf) past k_eff and past the row's numbers: cone_topk_windows' padding); certified[q] = 1 iff every
// window is a candidate, or t - c_last > E(q) with everything finite: t = the k_eff-th exact score, c_last = the
// smallest coarse score of the candidate list (in any order) -- every other window's coarse score is <= c_last, its exact score <= c_last
// + E < t, so it cannot precede any of the k listed windows (strictly: ties cannot arise).  E in fp64 from the fp32 inputs.
__global__ __launch_bounds__(256) void pf_certify_kernel(const float* __restrict__ txt, int dv, const float* __restrict__ err,
                                                         const int32_t* __restrict__ cand, const float* __restrict__ coarse,
                                                         const float* __restrict__ exact, int n_cand, int64_t num_window, int k,
                                                         int k_eff, int32_t* __restrict__ idx, float* __restrict__ val,
                                                         int32_t* __restrict__ certified) {
    __shared__ double nrm[4][3];
    __shared__ float c_min[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s_q = 0., s_h = 0., s_d = 0.;                            // |q|^2, |qh|^2, |qh - q|^2
    if (tid * 4 < dv) {
        const float4 a = reinterpret_cast<const float4*>(txt + (size_t)q * dv)[tid];
        const float e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = e[j], h = pf16_rne(e[j]);
            s_q += x * x; s_h += h * h; s_d += (h - x) * (h - x);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s_q += __shfl_xor(s_q, o, 64); s_h += __shfl_xor(s_h, o, 64); s_d += __shfl_xor(s_d, o, 64);
    }
    if (lane == 0) { nrm[wave][0] = s_q; nrm[wave][1] = s_h; nrm[wave][2] = s_d; }
    const float* ex = exact + (size_t)q * n_cand;
    const float* co = coarse + (size_t)q * n_cand;
    const int32_t* ci = cand + (size_t)q * n_cand;
    float v[TK_PT];
    int ix[TK_PT];
    float cm = INFINITY;                                            // the smallest coarse score (an empty slot: -inf, never certified)
#pragma unroll
    for (int u = 0; u < TK_PT; ++u) {
        const int j = u * 256 + tid;
        const int i = j < n_cand ? ci[j] : -1;
        const float x = i >= 0 ? ex[j] : -INFINITY;
        const bool ok = i >= 0 && x == x;
        v[u] = ok ? x : -INFINITY;
        ix[u] = ok ? i : 0x7fffffff;
        if (j < n_cand) cm = fminf(cm, i >= 0 ? co[j] : -INFINITY);
    }
    cm = -wave_max(-cm);
    if (lane == 0) c_min[wave] = cm;
    for (int r = k_eff + tid; r < k; r += 256) { idx[(size_t)q * k + r] = -1; val[(size_t)q * k + r] = -INFINITY; }
    tk_block_select<TK_PT>(v, ix, k_eff, val + (size_t)q * k, idx + (size_t)q * k, -1);
    __syncthreads();                                                // wave 0's list (global memory) and the four norm shares
    if (tid != 0) return;
    const double n_q = sqrt(nrm[0][0] + nrm[1][0] + nrm[2][0] + nrm[3][0]), n_h = sqrt(nrm[0][1] + nrm[1][1] + nrm[2][1] + nrm[3][1]),
                 n_d = sqrt(nrm[0][2] + nrm[1][2] + nrm[2][2] + nrm[3][2]);
    const double R = err[0], N = err[1];
    const double du = (dv + 1) * 0x1p-24, gam = du / (1. - du);
    const double E = (R * n_h + N * n_d + 2. * gam * N * fmax(n_q, n_h)) * (1. + 0x1p-10) + PF_CERT_TINY * (1. + n_h + N);
    const double t = val[(size_t)q * k + k_eff - 1], c_last = fminf(fminf(c_min[0], c_min[1]), fminf(c_min[2], c_min[3]));
    const bool finite = isfinite(E) && isfinite(t) && isfinite(c_last);
    certified[q] = (num_window <= n_cand || (finite && t - c_last > E)) ? 1 : 0;
}

// The fallback's top-k, for the queries with certified[q] == 0 only (the others' workgroups return at once): level 1 = the
// stable top-k of a chunk of TK_CH windows, the window scores taken from the two planes on the fly (pf_window_of_halves:
// window_combine_kernel's values; never NaN), level 2.. = merges of up to `group` lists of k (group * k <= 256 * TK_PT values
// in registers) until one list is left, which goes to the query's rows of idx / val.  topk_chunk_kernel / topk_merge_kernel's
// selection (tk_block_select) and order, so cone_topk_windows' list.
__global__ __launch_bounds__(256) void pf_fallback_chunk_kernel(const float* __restrict__ hm, const float* __restrict__ fr,
                                                                int64_t nh, int odd, int k, float* __restrict__ cval,
                                                                int* __restrict__ cidx, int n_chunks,
                                                                const int32_t* __restrict__ certified) {
    const int q = blockIdx.y, ch = blockIdx.x;
    if (certified[q]) return;
    const int64_t base = (int64_t)ch * TK_CH, n = nh + 1;
    const int m = (int)min((int64_t)TK_CH, n - base);
    TK_LOAD_CHUNK(v, ix, base, m, pf_window_of_halves(hm + (size_t)q * nh, fr + (size_t)q * nh, nh, odd, base + j));
    tk_block_select<TK_PT>(v, ix, k, cval + ((size_t)q * n_chunks + ch) * k, cidx + ((size_t)q * n_chunks + ch) * k, 0x7fffffff);
}

__global__ __launch_bounds__(256) void pf_fallback_merge_kernel(const float* __restrict__ cv_in, const int* __restrict__ ci_in,
                                                                int n_lists, int k, int group, float* __restrict__ cv_out,
                                                                int* __restrict__ ci_out, int32_t* __restrict__ idx,
                                                                float* __restrict__ val, const int32_t* __restrict__ certified) {
    const int q = blockIdx.y, g = blockIdx.x, n_groups = gridDim.x;
    if (certified[q]) return;
    const int l0 = g * group, m = (min(l0 + group, n_lists) - l0) * k;          // this group's candidates: lists are contiguous
    float v[TK_PT];
    int ix[TK_PT];
    tk_load_list(cv_in + ((size_t)q * n_lists + l0) * k, ci_in + ((size_t)q * n_lists + l0) * k, m, v, ix);
    const bool last = n_groups == 1;
    tk_block_select<TK_PT>(v, ix, k, last ? val + (size_t)q * k : cv_out + ((size_t)q * n_groups + g) * k,
                           last ? idx + (size_t)q * k : ci_out + ((size_t)q * n_groups + g) * k, last ? -1 : 0x7fffffff);
}

// ---- library search: stage A over MANY videos of one arena in one pass (cone_library_scan) ---------------------
// The streaming form (frame_score_body: the same loads, pf_lane_dot, wave_sum_multi, so a frame's score has the same bits) over
// a flat list of half-blocks: unit g = half-block h of video v, rows [row0_v + h S, row0_v + min((h + 1) S, ctx_l_v)).  The
// list is not materialised: v is the last video with v_hb_off[v] <= g, found by a binary search over the V + 1 prefix sums --
// wave-uniform (scalar loads of a table that stays in the scalar cache / L2), log2 V dependent loads per 45-row half-block that
// the SIMD's other waves stream through.  (An owner entry per half-block would be one load, but a table as long as the list,
// rebuilt and re-uploaded for every subset.)  Half-blocks restart at every video's first row, so neither a half-block nor a
// window ever holds a row of the next video; rows outside the listed videos are never addressed.  The planes are (nq, total_hb)
// with video v's half-blocks at column v_hb_off[v]; no frame score is written.
//   QG queries a pass, blockIdx.y = the pass (a last pass of fewer repeats its last query and stores nothing for the spares);
//   WPH as in frame_score_kernel (1: a wave per unit; 4: the workgroup's four waves share one, for short lists).
template <int VPL, int QG, int RPW, int WPH>
__global__ __launch_bounds__(256) void library_scan_kernel(const float* __restrict__ arena, int64_t capacity,
                                                           const int64_t* __restrict__ v_row0, const int32_t* __restrict__ v_ctx_l,
                                                           const int64_t* __restrict__ v_hb_off, int n_videos, int64_t total_hb,
                                                           int S, const float* __restrict__ txt, int nq, float* __restrict__ hm,
                                                           float* __restrict__ fr) {
    constexpr int DV = 256 * VPL, UPB = 4 / WPH, NV = RPW * QG;
    __shared__ float red[4][QG];
    const int q0 = QG * (int)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = wave % WPH;
    PF_LANE_SLOT(RPW, QG, lane);
    float4 q[QG][VPL];
#pragma unroll
    for (int g = 0; g < QG; ++g)
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            const int qi = min(q0 + g, nq - 1);
            q[g][v] = reinterpret_cast<const float4*>(txt + (size_t)qi * DV)[lane + 64 * v];
        }
    for (int64_t g = (int64_t)blockIdx.x * UPB + wave / WPH; g < total_hb; g += (int64_t)gridDim.x * UPB) {
        int lo = 0, hi = n_videos - 1;                                   // the last video whose first unit is at or before g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (v_hb_off[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const int64_t h = g - v_hb_off[lo], row0 = v_row0[lo], ctx_l = v_ctx_l[lo], r_lo = h * S;
        int n = (int)min((int64_t)S, ctx_l - r_lo);                      // frames of this half-block
        if (h < 0 || row0 < 0 || ctx_l > capacity - row0) n = 0;         // a video outside the arena is not read: -inf
        const float* base = arena + (row0 + r_lo) * DV;
        float m = -INFINITY;
        for (int j0 = sub * RPW; j0 < n; j0 += WPH * RPW) {              // (frame_score_body's row loop, without the fs store)
            float4 x[RPW][VPL];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int row = min(j0 + r, n - 1);
#pragma unroll
                for (int v = 0; v < VPL; ++v)
                    x[r][v] = pf_stream_ld(reinterpret_cast<const float4*>(base + (size_t)row * DV) + lane + 64 * v);
            }
            float part[NV];
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int g2 = 0; g2 < QG; ++g2) part[r * QG + g2] = pf_lane_dot<VPL>(x[r], q[g2]);
            const float s = wave_sum_multi<NV>(part, lane);
            if (j0 + my_r < n) {
                m = fmaxf(m, s);
                if (writer && q0 + my_g < nq && my_r == 0 && j0 == 0) fr[(size_t)(q0 + my_g) * total_hb + g] = s;
            }
        }
        if (n <= 0 && sub == 0 && out_lane && q0 + my_g < nq) fr[(size_t)(q0 + my_g) * total_hb + g] = -INFINITY;
        m = pf_slot_max<RPW>(m);
        pf_store_half_max<QG, WPH>(m, my_g, out_lane, lane, wave, red, q0, nq, total_hb, g, hm);
    }
}

// Combine + stable top-k of one (query, video): win[i] = pf_window_of_halves over the video's OWN nh half-blocks (the odd-W
// term fr[i + 1] exists only inside the video), then the first K entries of the order of cone_topk_windows_ws -- score
// descending, ties to the lower index -- into widx / wval[(q V + v) K ..], -1 / -inf where the video has fewer than K windows,
// and best[q V + v] = the first value.  Up to 1 024 windows (45 000 clips at W = 90) by counting ranks in LDS, as
// topk_seg_kernel does; above that K selection passes that recompute the window from the planes: the window scores of a scan
// exist nowhere.  (A window score is never NaN: the half-block max starts from -inf and fmaxf drops a NaN frame score, so an
// all-NaN video scores -inf everywhere and lists its windows 0 .. K - 1; the counting order and the selection order agree.)
__global__ __launch_bounds__(256) void library_topk_kernel(const float* __restrict__ hm, const float* __restrict__ fr,
                                                           const int64_t* __restrict__ v_hb_off, int n_videos, int64_t total_hb,
                                                           int odd, int K, int32_t* __restrict__ widx, float* __restrict__ wval,
                                                           float* __restrict__ best) {
    const int v = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t off = v_hb_off[v], nh = v_hb_off[v + 1] - off;
    const float* a = hm + (size_t)q * total_hb + off;
    const float* f = fr + (size_t)q * total_hb + off;
    const size_t pair = (size_t)q * n_videos + v;
    int32_t* oi = widx + pair * K;
    float* ov = wval + pair * K;
    const int n = nh < 1 ? 0 : (int)min(nh + 1, (int64_t)0x7ffffffe);       // windows of this video (nh < 1: a broken table)
    if (n == 0 && tid == 0) best[pair] = -INFINITY;
    if (n <= 1024) {
        __shared__ float s_row[1024];
        for (int j = tid; j < n; j += 256) s_row[j] = pf_window_of_halves(a, f, nh, odd, j);
        for (int p = n + tid; p < K; p += 256) { oi[p] = -1; ov[p] = -INFINITY; }
        __syncthreads();
        for (int j = tid; j < n; j += 256) {
            const float x = s_row[j];
            int rank = 0;
            for (int i = 0; i < n; ++i) {           // (every thread reads the same address: LDS broadcast)
                const float y = s_row[i];
                rank += (y > x) || (y == x && i < j);
            }
            if (rank < K) { oi[rank] = j; ov[rank] = x; }
            if (rank == 0) best[pair] = x;
        }
        return;
    }
    float last_v = INFINITY;
    int last_i = -1;
    for (int p = 0; p < K; ++p) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < n; j += 256) {
            const float x = pf_window_of_halves(a, f, nh, odd, j);
            if (tk_after(x, j, last_v, last_i) && tk_better(x, j, bv, bi)) { bv = x; bi = j; }
        }
        tk_pass_pick<4>(bv, bi, oi + p, ov + p, last_v, last_i);
        if (p == 0 && tid == 0) best[pair] = last_v;
    }
}

// ---- what the C entries share ---------------------------------------------------------------------------------------------
// f(pf_int<VPL>) for the exact-fp32 streaming kernels' VPL = dv / 256 (dv in {256, 512, 768, 1024}: CONE_PF_REQUIRE_DIM)
template <class F>
static int pf_with_vpl(int dv, F f) {
    switch (dv / 256) {
        case 1: return f(pf_int<1>{});
        case 2: return f(pf_int<2>{});
        case 3: return f(pf_int<3>{});
        default: return f(pf_int<4>{});
    }
}

// the two planes of a score workspace of `bytes` (cone_prefilter_scores_workspace): half-window max, first-frame score
struct PfPlanes {
    int64_t nh;
    float *hm, *fr;
    PfPlanes(void* ws, size_t bytes, int64_t ctx_l, int S) : nh((ctx_l + S - 1) / S), hm((float*)ws), fr((float*)((char*)ws + bytes / 2)) {}
};

static int launch_window_combine(const PfPlanes& p, int nq, int W, float* win, hipStream_t s) {
    hipLaunchKernelGGL(window_combine_kernel, dim3((unsigned)((p.nh + 1 + 255) / 256), nq), dim3(256), 0, s, p.hm, p.fr, p.nh, W & 1, win);
    CONE_LAUNCH_CHECK();
    return 0;
}

int launch_frame_scores_gated(const float* vid, int64_t ctx_l, int dv, int S, int64_t nh, const float* txt, int nq, float* hm, float* fr,
                              const int* gate, hipStream_t s) {
    return pf_with_vpl(dv, [&](auto VPL) { return launch_frame_scores_gated<decltype(VPL)::value>(vid, ctx_l, S, nh, txt, nq, hm, fr, gate, s); });
}

// One wording per condition, every entry (`name` = the entry's prefix in the message).
#define CONE_PF_REQUIRE_SIZES(name, ctx_l, nq, W, S)                                                                       \
    CONE_REQUIRE((ctx_l) > 0 && (nq) > 0 && (W) > 0 && (S) > 0 && (S) == (W) / 2, name ": bad sizes ctx_l=%lld nq=%d W=%d S=%d", \
                 (long long)(ctx_l), nq, W, S)
#define CONE_PF_REQUIRE_DIM(name, dv) \
    CONE_REQUIRE((dv) == 256 || (dv) == 512 || (dv) == 768 || (dv) == 1024, name ": feature dim %d not in {256,512,768,1024}", dv)
#define CONE_PF16_REQUIRE_ARENA(name, p, dv)                                                                              \
    CONE_REQUIRE((dv) > 0 && (dv) % 32 == 0 && (dv) <= 1024, name ": feature dim %d must be a multiple of 32 and <= 1024", dv); \
    CONE_REQUIRE(((uintptr_t)(p) & 15) == 0, name ": the bf16 arena must be 16-B aligned (16-B lane loads)")
#define CONE_TK_REQUIRE_SIZES(nq, num_window, k)                                                          \
    CONE_REQUIRE((nq) > 0 && (num_window) > 0 && (k) > 0 && (k) <= (num_window) && (num_window) < 0x7fffffff, \
                 "topk: bad sizes nq=%d num_window=%lld k=%d", nq, (long long)(num_window), k)
#define CONE_PF_REQUIRE_WS(name, ws, ws_bytes, need) \
    CONE_REQUIRE((ws) && (ws_bytes) >= (need), name ": workspace too small (%zu < %zu)", (size_t)(ws_bytes), (size_t)(need))

}  // namespace cone

extern "C" int64_t cone_num_windows(int64_t ctx_l, int W) {
    const int S = W / 2;
    if (S <= 0 || ctx_l <= 0) return 0;
    return (ctx_l + S - 1) / S + 1;
}

extern "C" size_t cone_prefilter_scores_workspace(int64_t ctx_l, int nq, int W) {
    const int S = W / 2;
    if (S <= 0 || ctx_l <= 0 || nq <= 0) return 0;
    const size_t nh = (size_t)((ctx_l + S - 1) / S);
    return 2 * cone::align_up((size_t)nq * nh * sizeof(float), 256);
}

extern "C" size_t cone_prefilter_scores_split_workspace(int64_t ctx_l, int nq, int W, int dv) {
    const size_t base = cone_prefilter_scores_workspace(ctx_l, nq, W);
    return base ? base + cone::frame_scores_split_image_bytes(dv) : 0;
}

static int prefilter_scores_impl(const float* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W, int S,
                                 float* frame_scores, float* win_scores, void* ws, size_t ws_bytes, void* stream, bool split) {
    CONE_REQUIRE(vid && txt && win_scores, "prefilter: null argument");
    CONE_PF_REQUIRE_SIZES("prefilter", ctx_l, nq, W, S);
    CONE_PF_REQUIRE_DIM("prefilter", dv);
    const size_t need = cone_prefilter_scores_workspace(ctx_l, nq, W);
    CONE_PF_REQUIRE_WS("prefilter", ws, ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const cone::PfPlanes p(ws, need, ctx_l, S);
    int rc;
    if (split && !frame_scores && cone::frame_scores_split_supported(dv, nq)) {
        // opt-in: the same stream on the bf16 matrix cores (three-piece operands, six partial products: fp32 accuracy); the
        // split query image lives behind the two score planes of the workspace
        CONE_PF_REQUIRE_WS("prefilter (split)", ws, ws_bytes, need + cone::frame_scores_split_image_bytes(dv));
        rc = cone::launch_frame_scores_mq3(vid, ctx_l, dv, S, p.nh, txt, nq, p.hm, p.fr, (char*)ws + need, s);
    } else if (nq >= CONE_PF_MQ_MIN) {
        // Many queries over one video: the clip arena is read once for up to 64 queries by the fp32-MFMA kernel
        // (BASELINE configs 3 / 5) instead of nq / 4 VALU passes over the features.  From 5 queries on: they would be two
        // passes of the streaming kernel (3.9 ms on the 12.7 GB video), one 16-query tile of this one is a single pass.
        rc = cone::launch_frame_scores_mq(vid, ctx_l, dv, S, p.nh, txt, nq, frame_scores, p.hm, p.fr, s);
    } else {
        rc = cone::pf_with_vpl(dv, [&](auto VPL) {
            return cone::launch_frame_scores<decltype(VPL)::value>(vid, ctx_l, S, p.nh, txt, nq, frame_scores, p.hm, p.fr, s);
        });
    }
    return rc ? rc : cone::launch_window_combine(p, nq, W, win_scores, s);
}

extern "C" int cone_prefilter_scores(const float* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W,
                                     int S, float* frame_scores, float* win_scores, void* ws, size_t ws_bytes,
                                     void* stream) {
    return prefilter_scores_impl(vid, ctx_l, dv, txt, nq, W, S, frame_scores, win_scores, ws, ws_bytes, stream, false);
}

extern "C" int cone_prefilter_scores_split(const float* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W,
                                           int S, float* win_scores, void* ws, size_t ws_bytes, void* stream) {
    return prefilter_scores_impl(vid, ctx_l, dv, txt, nq, W, S, nullptr, win_scores, ws, ws_bytes, stream, true);
}

// ---- the opt-in bf16 pre-filter: entries ----
extern "C" size_t cone_prefilter_scores_bf16_workspace(int64_t ctx_l, int nq, int W) {
    return cone_prefilter_scores_workspace(ctx_l, nq, W);           // the two planes (half-window max, first-frame score)
}

extern "C" int cone_prefilter_scores_bf16(const uint16_t* vid, int64_t ctx_l, int dv, const float* txt, int nq, int W, int S,
                                          float* win_scores, void* ws, size_t ws_bytes, void* stream) {
    CONE_REQUIRE(vid && txt && win_scores, "prefilter (bf16): null argument");
    CONE_PF_REQUIRE_SIZES("prefilter (bf16)", ctx_l, nq, W, S);
    CONE_PF16_REQUIRE_ARENA("prefilter (bf16)", vid, dv);
    CONE_REQUIRE(((uintptr_t)txt & 15) == 0, "prefilter (bf16): the query vectors must be 16-B aligned");
    const size_t need = cone_prefilter_scores_bf16_workspace(ctx_l, nq, W);
    CONE_PF_REQUIRE_WS("prefilter (bf16)", ws, ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const cone::PfPlanes p(ws, need, ctx_l, S);
    int rc;
    if (nq >= CONE_PF16_MQ_MIN) rc = cone::launch_frame_scores_mq_bf16(vid, ctx_l, dv, S, p.nh, txt, nq, p.hm, p.fr, s);
    else if (dv <= 512) rc = cone::launch_frame_scores_bf16<1>(vid, ctx_l, dv, S, p.nh, txt, nq, p.hm, p.fr, s);
    else rc = cone::launch_frame_scores_bf16<2>(vid, ctx_l, dv, S, p.nh, txt, nq, p.hm, p.fr, s);
    return rc ? rc : cone::launch_window_combine(p, nq, W, win_scores, s);
}

// ---- the certified pre-filter: entries ----
extern "C" int cone_prefilter_index_bf16(const float* x, int64_t n_rows, int dim, uint16_t* out, float* err, void* stream) {
    CONE_REQUIRE(x && out && err, "prefilter_index_bf16: null argument");
    CONE_REQUIRE(n_rows > 0, "prefilter_index_bf16: bad row count");
    CONE_REQUIRE(dim > 0 && dim % 4 == 0 && dim <= cone::PF_INDEX_MAX_DIM,
                 "prefilter_index_bf16: dim=%d must be a positive multiple of 4 and <= %d", dim, cone::PF_INDEX_MAX_DIM);
    CONE_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)err & 3) == 0,
                 "prefilter_index_bf16: x must be 16-B aligned, out 8-B aligned");
    hipStream_t s = (hipStream_t)stream;
    CONE_CHECK_HIP(hipMemsetAsync(err, 0, 2 * sizeof(float), s));        // +0.0f: the maxima's neutral element
    int64_t blocks = (n_rows + 3) / 4;                                      // a wave per row, grid-stride past 64 workgroups per CU
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(cone::pf_index_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n_rows, dim, out, (int*)err);
    CONE_LAUNCH_CHECK();
    return 0;
}

namespace {
// the workspace of cone_prefilter_topk_certified: byte offsets of its parts
struct CertLayout {
    int k_eff, n_cand, n_chunks;
    int64_t nh, nw;
    bool fast_cand;     // the candidates by pf_cand_chunk_kernel / pf_cand_merge_kernel (their sets fit one merge workgroup)
    size_t planes, planes_bytes, win, topk, topk_bytes, cand, coarse, exact, lists_a, lists_b, total;
};
bool cert_layout(int64_t ctx_l, int nq, int W, int k, int n_cand, CertLayout* L) {
    const int S = W / 2;
    if (S <= 0 || ctx_l <= 0 || nq <= 0 || k <= 0 || n_cand < 0) return false;
    L->nh = (ctx_l + S - 1) / S;
    L->nw = L->nh + 1;
    L->k_eff = (int)(k < L->nw ? k : L->nw);
    if (n_cand == 0) {                                                  // the default: min(num_window, max(4 k, 128))
        const int64_t d = 4 * (int64_t)k > 128 ? 4 * (int64_t)k : 128;
        n_cand = (int)(d < L->nw ? d : L->nw);
    }
    L->n_cand = n_cand;
    L->n_chunks = (int)((L->nw + cone::TK_CH - 1) / cone::TK_CH);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += cone::align_up(bytes, 256); return at; };
    L->planes_bytes = cone_prefilter_scores_workspace(ctx_l, nq, W);       // (the bf16 entry's workspace has the same size)
    L->planes = take(L->planes_bytes);
    L->win = take((size_t)nq * L->nw * 4);
    L->fast_cand = (int64_t)L->n_chunks * n_cand <= cone::PF_CERT_MAX_CAND;
    L->topk_bytes = L->fast_cand ? (size_t)nq * L->n_chunks * n_cand * 8 : cone_topk_windows_workspace(nq, L->nw, n_cand);
    L->topk = take(L->topk_bytes);
    L->cand = take((size_t)nq * n_cand * 4);
    L->coarse = take((size_t)nq * n_cand * 4);
    L->exact = take((size_t)nq * n_cand * 4);
    const int group = cone::PF_CERT_MAX_CAND / (k < cone::TK_KMAX ? k : cone::TK_KMAX);
    L->lists_a = take((size_t)nq * L->n_chunks * k * 8);                   // values, then indices
    L->lists_b = take((size_t)nq * ((L->n_chunks + group - 1) / group) * k * 8);
    L->total = o;
    return true;
}
}  // namespace

extern "C" size_t cone_prefilter_topk_certified_workspace(int64_t ctx_l, int nq, int W, int k, int n_cand) {
    CertLayout L;
    return cert_layout(ctx_l, nq, W, k, n_cand, &L) ? L.total : 0;
}

extern "C" int cone_prefilter_topk_certified(const float* vid_f32, const uint16_t* vid_bf16, int64_t ctx_l, int dv,
                                             const float* txt, int nq, int W, int S, int k, int n_cand, const float* err,
                                             int32_t* idx, float* val, int32_t* certified, void* ws, size_t ws_bytes,
                                             void* stream) {
    CONE_REQUIRE(vid_f32 && vid_bf16 && txt && err && idx && val && certified, "prefilter_topk_certified: null argument");
    CONE_PF_REQUIRE_SIZES("prefilter_topk_certified", ctx_l, nq, W, S);
    CONE_REQUIRE(k > 0 && n_cand >= 0, "prefilter_topk_certified: bad sizes k=%d n_cand=%d", k, n_cand);
    CONE_PF_REQUIRE_DIM("prefilter_topk_certified", dv);
    CONE_REQUIRE(((uintptr_t)vid_f32 & 15) == 0 && ((uintptr_t)vid_bf16 & 15) == 0 && ((uintptr_t)txt & 15) == 0,
                 "prefilter_topk_certified: the arenas and the query vectors must be 16-B aligned");
    CONE_REQUIRE(k <= cone::TK_KMAX, "prefilter_topk_certified: k=%d exceeds the %d entries of a selection list", k, cone::TK_KMAX);
    CertLayout L;
    cert_layout(ctx_l, nq, W, k, n_cand, &L);
    CONE_REQUIRE(L.nw < 0x7fffffff, "prefilter_topk_certified: %lld windows do not fit an int32 index", (long long)L.nw);
    // what cone_topk_windows_ws supports for the candidate list (n_cand <= num_window), at most the two-level selection's
    // PF_CERT_MAX_CAND candidates per row, and no fewer than the k windows asked for
    CONE_REQUIRE(L.n_cand <= L.nw && L.n_cand <= cone::PF_CERT_MAX_CAND && L.n_cand >= L.k_eff,
                 "prefilter_topk_certified: n_cand=%d must lie in [min(k, num_window)=%d, min(num_window=%lld, %d)]", L.n_cand,
                 L.k_eff, (long long)L.nw, cone::PF_CERT_MAX_CAND);
    CONE_PF_REQUIRE_WS("prefilter_topk_certified", ws, ws_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    float* win = (float*)(w + L.win);
    int32_t* cand = (int32_t*)(w + L.cand);
    float* coarse = (float*)(w + L.coarse);
    float* exact = (float*)(w + L.exact);
    // (a) the coarse window scores off the bf16 shadow (the existing entry, unchanged), (b) the n_cand best of them
    int rc = cone_prefilter_scores_bf16(vid_bf16, ctx_l, dv, txt, nq, W, S, win, w + L.planes, L.planes_bytes, stream);
    if (rc) return rc;
    if (L.fast_cand) {      // as an unordered set (all the proof needs): chunk sets, then the set of their union
        float* cv = (float*)(w + L.topk);
        int* ci = (int*)(cv + (size_t)nq * L.n_chunks * L.n_cand);
        hipLaunchKernelGGL(cone::pf_cand_chunk_kernel, dim3((unsigned)L.n_chunks, (unsigned)nq), dim3(256), 0, s, win, L.nw, L.n_cand, cv,
                           ci, L.n_chunks);
        CONE_LAUNCH_CHECK();
        hipLaunchKernelGGL(cone::pf_cand_merge_kernel, dim3(nq), dim3(256), 0, s, cv, ci, L.n_chunks * L.n_cand, L.n_cand, cand, coarse);
        CONE_LAUNCH_CHECK();
    } else {                // more than 4 096 chunk-set entries (n_cand x ceil(num_window / 4 096)): the top-k entry's own forms
        rc = cone_topk_windows_ws(win, nq, L.nw, L.n_cand, cand, coarse, w + L.topk, L.topk_bytes, stream);
        if (rc) return rc;
    }
    // (c) the candidates' exact scores
    cone::pf_with_vpl(dv, [&](auto VPL) {
        hipLaunchKernelGGL(cone::pf_rescore_kernel<decltype(VPL)::value>, dim3((unsigned)L.n_cand, (unsigned)nq), dim3(cone::PF_RS_NT), 0, s,
                           vid_f32, ctx_l, W, S, txt, cand, L.n_cand, exact);
        return 0;
    });
    CONE_LAUNCH_CHECK();
    // (d) the k best candidates and the proof
    hipLaunchKernelGGL(cone::pf_certify_kernel, dim3(nq), dim3(256), 0, s, txt, dv, err, cand, coarse, exact, L.n_cand, L.nw, k,
                       L.k_eff, idx, val, certified);
    CONE_LAUNCH_CHECK();
    if (L.nw <= L.n_cand) return 0;                     // every window is a candidate: every query is certified
    // (e) the fallback, gated on the device by `certified`: the streaming scan in groups of up to 4 queries (a query's bits
    // do not depend on its group), the planes of the coarse scan reused (dead by now), then the gated top-k (here k <= n_cand
    // < num_window, so the rows' stride k is the list length)
    const cone::PfPlanes p(w + L.planes, L.planes_bytes, ctx_l, S);
    rc = cone::launch_frame_scores_gated(vid_f32, ctx_l, dv, S, p.nh, txt, nq, p.hm, p.fr, certified, s);
    if (rc) return rc;
    float* cv_a = (float*)(w + L.lists_a);
    int* ci_a = (int*)(cv_a + (size_t)nq * L.n_chunks * k);
    hipLaunchKernelGGL(cone::pf_fallback_chunk_kernel, dim3((unsigned)L.n_chunks, (unsigned)nq), dim3(256), 0, s, p.hm, p.fr, p.nh, W & 1, k,
                       cv_a, ci_a, L.n_chunks, certified);
    CONE_LAUNCH_CHECK();
    const int group = cone::PF_CERT_MAX_CAND / k;          // lists per merge workgroup (>= 16)
    char* out_buf = w + L.lists_b;
    char* in_buf = w + L.lists_a;
    for (int n_lists = L.n_chunks;;) {
        const int n_groups = (n_lists + group - 1) / group;
        float* cv_in = (float*)in_buf;
        int* ci_in = (int*)(cv_in + (size_t)nq * n_lists * k);
        float* cv_out = (float*)out_buf;
        int* ci_out = (int*)(cv_out + (size_t)nq * n_groups * k);
        hipLaunchKernelGGL(cone::pf_fallback_merge_kernel, dim3((unsigned)n_groups, (unsigned)nq), dim3(256), 0, s, cv_in, ci_in, n_lists,
                           k, group, cv_out, ci_out, idx, val, certified);
        CONE_LAUNCH_CHECK();
        if (n_groups == 1) break;
        n_lists = n_groups;                                 // (the lists shrink: each buffer holds every later level too)
        char* t = in_buf; in_buf = out_buf; out_buf = t;
    }
    return 0;
}

extern "C" int cone_prefilter_batched_bf16(const uint16_t* arena, int dv, const float* cls, const int64_t* g_row0,
                                           const int32_t* g_ctx_l, const int32_t* g_q, int ng, int max_ctx_l,
                                           const int64_t* q_win_off, const int32_t* q_ctx_l, int nq, int W, int S,
                                           float* win_scores, int k, int32_t* topk_idx, void* stream) {
    CONE_REQUIRE(arena && cls && g_row0 && g_ctx_l && g_q && q_win_off && q_ctx_l && win_scores && topk_idx,
                 "prefilter_batched (bf16): null argument");
    CONE_REQUIRE(ng > 0 && nq > 0 && max_ctx_l > 0 && W > 0 && S > 0 && S == W / 2 && k > 0, "prefilter_batched (bf16): bad sizes");
    CONE_PF16_REQUIRE_ARENA("prefilter_batched (bf16)", arena, dv);
    CONE_REQUIRE(((uintptr_t)cls & 15) == 0, "prefilter_batched (bf16): the query vectors must be 16-B aligned");
    hipStream_t s = (hipStream_t)stream;
    const int max_nh = (max_ctx_l + S - 1) / S, max_nw = max_nh + 1;
    hipLaunchKernelGGL(cone::win_fill_seg_kernel, dim3((max_nw + 255) / 256, nq), dim3(256), 0, s, q_win_off, q_ctx_l, S,
                       win_scores);
    CONE_LAUNCH_CHECK();
    int bx = (max_nh + 3) / 4;                  // a wave per half window of the longest video
    if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, ng);
    {
        cone::ProfScope ps(cone::PK_FRAME_SCORE, max_ctx_l, dv, ng, nullptr, s);
        if (dv <= 512)
            hipLaunchKernelGGL(cone::frame_score_groups_bf16_kernel<1>, grid, dim3(256), 0, s, arena, dv, cls, g_row0, g_ctx_l, g_q,
                               q_win_off, S, W & 1, win_scores);
        else
            hipLaunchKernelGGL(cone::frame_score_groups_bf16_kernel<2>, grid, dim3(256), 0, s, arena, dv, cls, g_row0, g_ctx_l, g_q,
                               q_win_off, S, W & 1, win_scores);
    }
    CONE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cone::topk_seg_kernel, dim3(nq), dim3(256), 0, s, win_scores, q_win_off, q_ctx_l, S, k, topk_idx);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" int cone_prefilter_batched(const float* arena, int dv, const float* cls, const int64_t* g_row0,
                                      const int32_t* g_ctx_l, const int32_t* g_q, int ng, int max_ctx_l,
                                      const int64_t* q_fs_off, const int64_t* q_win_off, const int32_t* q_ctx_l,
                                      int nq, int W, int S, float* frame_scores, float* win_scores, int k,
                                      int32_t* topk_idx, void* stream) {
    CONE_REQUIRE(arena && cls && g_row0 && g_ctx_l && g_q && q_fs_off && q_win_off && q_ctx_l && frame_scores &&
                     win_scores && topk_idx, "prefilter_batched: null argument");
    CONE_REQUIRE(ng > 0 && nq > 0 && max_ctx_l > 0 && W > 0 && S > 0 && k > 0, "prefilter_batched: bad sizes");
    CONE_PF_REQUIRE_DIM("prefilter", dv);
    hipStream_t s = (hipStream_t)stream;
    int64_t bx = ((int64_t)max_ctx_l + 15) / 16;
    if (bx > 2048) bx = 2048;
    dim3 grid((unsigned)bx, ng);
    {
        cone::ProfScope ps(cone::PK_FRAME_SCORE, max_ctx_l, dv, ng, nullptr, s);
        cone::pf_with_vpl(dv, [&](auto VPL) {
            hipLaunchKernelGGL(cone::frame_score_groups_kernel<decltype(VPL)::value>, grid, dim3(256), 0, s, arena, cls, g_row0, g_ctx_l, g_q,
                               q_fs_off, frame_scores);
            return 0;
        });
    }
    CONE_LAUNCH_CHECK();
    const int max_nw = (max_ctx_l + S - 1) / S + 1;
    hipLaunchKernelGGL(cone::window_max_seg_kernel, dim3((max_nw + 255) / 256, nq), dim3(256), 0, s, frame_scores,
                       q_fs_off, q_win_off, q_ctx_l, W, S, win_scores);
    CONE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cone::topk_seg_kernel, dim3(nq), dim3(256), 0, s, win_scores, q_win_off, q_ctx_l, S, k,
                       topk_idx);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t cone_topk_windows_workspace(int nq, int64_t num_window, int k) {
    if (num_window <= 2 * cone::TK_CH) return 0;
    const size_t n_chunks = (size_t)((num_window + cone::TK_CH - 1) / cone::TK_CH);
    return 2 * cone::align_up((size_t)nq * n_chunks * k * 4, 256);
}

extern "C" int cone_topk_windows_ws(const float* win_scores, int nq, int64_t num_window, int k, int32_t* idx, float* val,
                                    void* ws, size_t ws_bytes, void* stream) {
    CONE_TK_REQUIRE_SIZES(nq, num_window, k);
    const size_t need = cone_topk_windows_workspace(nq, num_window, k);
    const int64_t n_chunks = (num_window + cone::TK_CH - 1) / cone::TK_CH;
    // two-level selection: lists of <= TK_KMAX per wave, all candidates of a row in the merge workgroup's registers
    if (need == 0 || k > cone::TK_KMAX || n_chunks * k > 256 * cone::TK_PT)
        return cone_topk_windows(win_scores, nq, num_window, k, idx, val, stream);
    CONE_PF_REQUIRE_WS("topk", ws, ws_bytes, need);
    float* cval = (float*)ws;
    int* cidx = (int*)((char*)ws + need / 2);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cone::topk_chunk_kernel, dim3((unsigned)n_chunks, nq), dim3(256), 0, s, win_scores, num_window, k, cval,
                       cidx, (int)n_chunks);
    CONE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cone::topk_merge_kernel, dim3(nq), dim3(256), 0, s, cval, cidx, (int)(n_chunks * k), k, idx, val);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" int cone_topk_windows(const float* win_scores, int nq, int64_t num_window, int k, int32_t* idx,
                                 float* val, void* stream) {
    CONE_TK_REQUIRE_SIZES(nq, num_window, k);
    if (num_window > 4096)      // long video (MAD scale): 16 waves per row
        hipLaunchKernelGGL(cone::topk_kernel<1024>, dim3(nq), dim3(1024), 0, (hipStream_t)stream, win_scores,
                           num_window, k, idx, val);
    else
        hipLaunchKernelGGL(cone::topk_kernel<256>, dim3(nq), dim3(256), 0, (hipStream_t)stream, win_scores,
                           num_window, k, idx, val);
    CONE_LAUNCH_CHECK();
    return 0;
}

// ---- library search: entries ----
namespace cone {

// the regions of a scan's workspace: the two planes, best, the ranking's scratch (each 256-B aligned)
struct ScanLayout { size_t hm, fr, best, rank_ws, rank_bytes, total; };
static ScanLayout scan_layout(int64_t n_videos, int64_t total_hb, int nq, int n_rank) {
    ScanLayout L{};
    const size_t plane = align_up((size_t)nq * (size_t)total_hb * 4, 256);
    L.hm = 0; L.fr = plane; L.best = 2 * plane;
    L.rank_ws = L.best + align_up((size_t)nq * (size_t)n_videos * 4, 256);
    L.rank_bytes = cone_topk_windows_workspace(nq, n_videos, n_rank);
    L.total = L.rank_ws + align_up(L.rank_bytes, 256);
    return L;
}

// The refusals a scan makes from host values alone, in this order, before any pointer or the handle is looked at.
static int scan_precheck(const cone_library* lib, int64_t n_videos, int64_t total_hb, int nq, int K, int n_rank, int max_v_l,
                         const char* who = "library_scan") {
    CONE_REQUIRE(lib, "%s: null argument", who);
    CONE_REQUIRE(nq >= 1 && nq <= CONE_SESSION_MAX_QUERIES, "%s: nq=%d not in [1, %d]", who, nq, CONE_SESSION_MAX_QUERIES);
    CONE_REQUIRE(n_videos >= 1, "%s: n_videos=%lld < 1", who, (long long)n_videos);
    CONE_REQUIRE(lib->capacity >= 1 && lib->capacity < (1ll << 31), "%s: capacity=%lld not in [1, 2^31)", who, (long long)lib->capacity);
    CONE_REQUIRE(total_hb >= n_videos && total_hb <= lib->capacity,
                 "%s: total_hb=%lld not in [n_videos=%lld, capacity=%lld] (a video has at least one half-block, a half-block at least one row)",
                 who, (long long)total_hb, (long long)n_videos, (long long)lib->capacity);
    CONE_REQUIRE(K >= 1 && K <= 256, "%s: K=%d not in [1, 256]", who, K);
    CONE_REQUIRE(n_rank >= 1 && n_rank <= n_videos, "%s: n_rank=%d not in [1, n_videos=%lld]", who, n_rank, (long long)n_videos);
    CONE_REQUIRE(max_v_l >= 2, "%s: max_v_l=%d", who, max_v_l);
    CONE_REQUIRE(!(lib->flags & CONE_SESSION_CERTIFIED), "%s: CONE_SESSION_CERTIFIED libraries are not supported", who);
    CONE_REQUIRE(!(lib->flags & CONE_SESSION_BF16), "%s: CONE_SESSION_BF16 libraries are not supported", who);
    return 0;
}

template <int VPL>
static int launch_library_scan(const float* arena, int64_t capacity, const int64_t* v_row0, const int32_t* v_ctx_l,
                               const int64_t* v_hb_off, int n_videos, int64_t total_hb, int S, const float* txt, int nq, float* hm,
                               float* fr, hipStream_t s) {
    const PfStreamGrid g(total_hb);
    const int qg = nq >= 3 ? 4 : nq;                        // 3 queries ride a 4-query pass, as in pf_stream_passes
    ProfScope ps(PK_FRAME_SCORE, total_hb * S, 256 * VPL, qg, nullptr, s);
    const dim3 grid(g.blocks, (unsigned)((nq + qg - 1) / qg));
#define CONE_SCAN_LAUNCH(QG, WPH)                                                                                            \
    hipLaunchKernelGGL((library_scan_kernel<VPL, QG, CONE_PF_RPW, WPH>), grid, dim3(256), 0, s, arena, capacity, v_row0, v_ctx_l, \
                       v_hb_off, n_videos, total_hb, S, txt, nq, hm, fr)
    if (g.wide) { if (qg == 4) CONE_SCAN_LAUNCH(4, 4); else if (qg == 2) CONE_SCAN_LAUNCH(2, 4); else CONE_SCAN_LAUNCH(1, 4); }
    else { if (qg == 4) CONE_SCAN_LAUNCH(4, 1); else if (qg == 2) CONE_SCAN_LAUNCH(2, 1); else CONE_SCAN_LAUNCH(1, 1); }
#undef CONE_SCAN_LAUNCH
    CONE_LAUNCH_CHECK();
    return 0;
}

}  // namespace cone

extern "C" size_t cone_library_scan_workspace(const cone_library* lib, int64_t n_videos, int64_t total_hb, int nq, int K, int n_rank) {
    if (cone::scan_precheck(lib, n_videos, total_hb, nq, K, n_rank, 2)) return 0;
    return cone::scan_layout(n_videos, total_hb, nq, n_rank).total;
}

extern "C" int cone_library_scan(const cone_model* m, const cone_library* lib, const int64_t* v_row0, const int32_t* v_ctx_l,
                                 const int64_t* v_hb_off, int64_t n_videos, int64_t total_hb, const float* cls, int nq, int K,
                                 int n_rank, const cone_session_params* params, int32_t* widx, float* wval, int32_t* rank_slot,
                                 float* rank_val, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "library_scan";
    CONE_REQUIRE(lib && params, "%s: null argument", who);
    if (int rc = cone::scan_precheck(lib, n_videos, total_hb, nq, K, n_rank, params->max_v_l)) return rc;
    CONE_REQUIRE(m && v_row0 && v_ctx_l && v_hb_off && cls && widx && wval && rank_slot && rank_val && ws, "%s: null argument", who);
    CONE_REQUIRE(lib->model == m, "%s: the library was opened with another handle", who);
    CONE_PF_REQUIRE_DIM("library_scan", lib->v_dim);
    CONE_REQUIRE(lib->adapted, "%s: the library handle misses a region (not one cone_library_open filled)", who);
    CONE_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-B aligned", who);
    const cone::ScanLayout L = cone::scan_layout(n_videos, total_hb, nq, n_rank);
    if (ws_bytes < L.total) { cone::set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    float *hm = (float*)(w + L.hm), *fr = (float*)(w + L.fr), *best = (float*)(w + L.best);
    const int W = params->max_v_l, S = W / 2, V = (int)n_videos;
    if (int rc = cone::pf_with_vpl(lib->v_dim, [&](auto VPL) {
            return cone::launch_library_scan<decltype(VPL)::value>(lib->adapted, lib->capacity, v_row0, v_ctx_l, v_hb_off, V, total_hb, S,
                                                                   cls, nq, hm, fr, s);
        }))
        return rc;
    hipLaunchKernelGGL(cone::library_topk_kernel, dim3((unsigned)V, (unsigned)nq), dim3(256), 0, s, hm, fr, v_hb_off, V, total_hb, W & 1,
                       K, widx, wval, best);
    CONE_LAUNCH_CHECK();
    // the videos' order: the existing stable top-k on best (nq, V) -- slots, ties to the lower one
    return cone_topk_windows_ws(best, nq, n_videos, n_rank, rank_slot, rank_val, L.rank_bytes ? w + L.rank_ws : nullptr, L.rank_bytes, stream);
}

// ---- certified library budgets (include/cone_hip.h, "certified library budgets") ---------------------------------
// cone_library_scan's lists for a budget of W windows at half the scan's bytes: the library scan's skeleton over a bf16 shadow of
// the adapted rows, the n_cand best coarse windows of the WHOLE table as one set per query, their exact scores in the scan's own
// fp32 arithmetic, and the proof of 3d per query.  Every device function below is the one the per-video certified path uses.
namespace cone {

// One wave per row: pf_index_kernel's arithmetic for that row (the same lane-strided float4 chains, wave_sum, sqrtf, inflation),
// the two measures stored per row instead of maximised over the grid.  max over rows of these = that kernel's err, bit for bit:
// x -> x * PF_CERT_INFLATE + PF_INDEX_TINY is monotone in fp32, and a NaN is the same positive quiet NaN.
__global__ __launch_bounds__(256) void lib_shadow_index_kernel(const float* __restrict__ x, int64_t row0, int64_t n_rows, int dim,
                                                               uint16_t* __restrict__ out, float* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int n4 = dim >> 2;
    for (int64_t i = wave_id; i < n_rows; i += n_waves) {
        const int64_t row = row0 + i;
        const float4* src = reinterpret_cast<const float4*>(x + row * dim);
        uint2* dst = reinterpret_cast<uint2*>(out + row * dim);
        float sr = 0.f, sx = 0.f, sh = 0.f;
        for (int c = lane; c < n4; c += 64) {
            const float4 v = src[c];
            const unsigned lo = pf_pk(v.x, v.y), hi = pf_pk(v.z, v.w);
            dst[c] = make_uint2(lo, hi);
            const float h[4] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                                __uint_as_float(hi & 0xffff0000u)};
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = e[j] - h[j];
                sr = __builtin_fmaf(d, d, sr);
                sx = __builtin_fmaf(e[j], e[j], sx);
                sh = __builtin_fmaf(h[j], h[j], sh);
            }
        }
        sr = wave_sum(sr); sx = wave_sum(sx); sh = wave_sum(sh);
        const float r = sqrtf(sr), n = sqrtf(fmaxf(sx, sh));
        const float mr = (r != r) ? NAN : fmaxf(0.f, r);
        const float mn = (sx != sx || sh != sh) ? NAN : fmaxf(0.f, n);
        if (lane == 0) {
            const float R = mr * PF_CERT_INFLATE + PF_INDEX_TINY, N = mn * PF_CERT_INFLATE + PF_INDEX_TINY;
            reinterpret_cast<float2*>(err)[row] = make_float2(R == R ? R : __int_as_float(0x7fc00000), N == N ? N : __int_as_float(0x7fc00000));
        }
    }
}

// a measure's bits on the order atomicMax keeps: non-negative floats order like their bits, a NaN above +inf (pf_index_kernel)
__device__ __forceinline__ int lib_measure_bits(float x) { return x == x ? __float_as_int(x) : 0x7fc00000; }

// library_scan_kernel over the shadow: the same flat list of half-block units, owner search, restart at every video's first
// row and -inf for a video outside the arena; the rows through pf16_half_block / pf16_load_query (frame_score_bf16_kernel's
// bits for that video).  The pass of the first queries (blockIdx.y == 0) also takes the maxima of the per-row measures over
// exactly the rows it scores -- 8 bytes a row beside a 2 dv-byte stream -- into rn_bits[0..1] (zeroed by the host).
template <int VPL /* 16-B loads per lane and row: dv <= 512 VPL */, int QG, int RPW, int WPH>
__global__ __launch_bounds__(256) void library_scan_bf16_kernel(const uint16_t* __restrict__ arena, const float* __restrict__ err,
                                                                int64_t capacity, int dv, const int64_t* __restrict__ v_row0,
                                                                const int32_t* __restrict__ v_ctx_l, const int64_t* __restrict__ v_hb_off,
                                                                int n_videos, int64_t total_hb, int S, const float* __restrict__ txt,
                                                                int nq, float* __restrict__ hm, float* __restrict__ fr,
                                                                int* __restrict__ rn_bits) {
    constexpr int UPB = 4 / WPH;
    __shared__ float red[4][QG];
    const int q0 = QG * (int)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), sub = wave % WPH;
    PF_LANE_SLOT(RPW, QG, lane);
    float q[QG][VPL][8];
#pragma unroll
    for (int g = 0; g < QG; ++g) pf16_load_query<VPL>(txt + (size_t)min(q0 + g, nq - 1) * dv, dv, lane, q[g]);
    const bool measure = blockIdx.y == 0 && sub == 0;
    int br = 0, bn = 0;
    for (int64_t g = (int64_t)blockIdx.x * UPB + wave / WPH; g < total_hb; g += (int64_t)gridDim.x * UPB) {
        int lo = 0, hi = n_videos - 1;                                   // the last video whose first unit is at or before g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (v_hb_off[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const int64_t h = g - v_hb_off[lo], row0 = v_row0[lo], ctx_l = v_ctx_l[lo], r_lo = h * S;
        int n = (int)max(min((int64_t)S, ctx_l - r_lo), (int64_t)0);     // frames of this half-block
        if (h < 0 || row0 < 0 || ctx_l > capacity - row0) n = 0;         // a video outside the arena is not read: -inf
        float first = -INFINITY;
        const float m = pf16_half_block<VPL, QG, RPW, CONE_PF_NT != 0>(arena + (row0 + r_lo) * dv, n, dv, q, lane, sub, WPH, first);
        if (out_lane && sub == 0 && q0 + my_g < nq) fr[(size_t)(q0 + my_g) * total_hb + g] = first;
        pf_store_half_max<QG, WPH>(m, my_g, out_lane, lane, wave, red, q0, nq, total_hb, g, hm);
        if (measure)
            for (int j = lane; j < n; j += 64) {
                const float2 e = reinterpret_cast<const float2*>(err)[row0 + r_lo + j];
                br = max(br, lib_measure_bits(e.x));
                bn = max(bn, lib_measure_bits(e.y));
            }
    }
    if (measure) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { br = max(br, __shfl_xor(br, o, 64)); bn = max(bn, __shfl_xor(bn, o, 64)); }
        // (a maximum only grows: a wave whose value is not above what it reads -- however stale -- has nothing to add; without the
        // test every wave of the grid queues on one address, 0.1 - 0.2 ms of a 0.26 ms scan at 1 M clips)
        if (lane == 0) {
            if (br > __atomic_load_n(rn_bits, __ATOMIC_RELAXED)) atomicMax(rn_bits, br);
            if (bn > __atomic_load_n(rn_bits + 1, __ATOMIC_RELAXED)) atomicMax(rn_bits + 1, bn);
        }
    }
}

// the slot that owns flat window t: the last v with v_win_off[v] <= t
__device__ __forceinline__ int lib_window_owner(const int64_t* __restrict__ v_win_off, int n_videos, int64_t t) {
    int lo = 0, hi = n_videos - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v_win_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The coarse window row (nq, total_win): window j of slot v at v_win_off[v] + j = pf_window_of_halves over that video's OWN
// half-blocks (library_topk_kernel's rule: the odd-W term exists only inside the video).  A table whose two prefix sums disagree
// scores -inf there and reads nothing outside the planes.
__global__ __launch_bounds__(256) void lib_window_row_kernel(const float* __restrict__ hm, const float* __restrict__ fr,
                                                             const int64_t* __restrict__ v_hb_off, const int64_t* __restrict__ v_win_off,
                                                             int n_videos, int64_t total_hb, int64_t total_win, int odd,
                                                             float* __restrict__ win) {
    const int q = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total_win) return;
    const int v = lib_window_owner(v_win_off, n_videos, t);
    const int64_t i = t - v_win_off[v], off = v_hb_off[v], nh = v_hb_off[v + 1] - off;
    float x = -INFINITY;
    if (i >= 0 && i <= nh && nh >= 1 && off >= 0 && off + nh <= total_hb)
        x = pf_window_of_halves(hm + (size_t)q * total_hb + off, fr + (size_t)q * total_hb + off, nh, odd, i);
    win[(size_t)q * total_win + t] = x;
}

// One level of the candidate sets' merge: group g of a query takes up to `group` consecutive sets of k pairs (group * k <= 256 PT
// values in registers) to one set of k -- pf_cand_merge_kernel's selection, repeated until one set is left: a library's row is
// past one merge workgroup's pairs.  The last level (one group) writes the query's candidates (index -1: none).
template <int PT>
__global__ __launch_bounds__(256) void lib_cand_merge_kernel(const float* __restrict__ cv_in, const int* __restrict__ ci_in,
                                                             int n_lists, int k, int group, float* __restrict__ cv_out,
                                                             int* __restrict__ ci_out, int32_t* __restrict__ cand,
                                                             float* __restrict__ coarse) {
    const int q = blockIdx.y, g = blockIdx.x, n_groups = gridDim.x;
    const int l0 = g * group, m = (min(l0 + group, n_lists) - l0) * k;
    const float* cv = cv_in + ((size_t)q * n_lists + l0) * k;
    const int* ci = ci_in + ((size_t)q * n_lists + l0) * k;
    float v[PT];
    int ix[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) {
        const int j = u * 256 + threadIdx.x;
        v[u] = j < m ? cv[j] : -INFINITY;
        ix[u] = j < m ? ci[j] : 0x7fffffff;
    }
    const bool last = n_groups == 1;
    pf_block_select_set<PT>(v, ix, k, last ? coarse + (size_t)q * k : cv_out + ((size_t)q * n_groups + g) * k,
                            last ? cand + (size_t)q * k : ci_out + ((size_t)q * n_groups + g) * k, last ? -1 : 0x7fffffff);
}

// pf_rescore_kernel for a flat window index: slot v = its owner, window i = the remainder, frames [max((i-1)S, 0), min((i-1)S
// + W, ctx_l_v)) of the video's rows, every frame by pf_lane_dot + wave_sum_multi<1> -- frame_score_kernel's bits, hence
// library_scan_kernel's --, the max by fmaxf (a window of NaN frames scores -inf).  Also leaves (slot, window) per candidate for
// the walk.  A video outside the arena is not read.
template <int VPL>
__global__ __launch_bounds__(PF_RS_NT) void lib_rescore_kernel(const float* __restrict__ arena, int64_t capacity,
                                                               const int64_t* __restrict__ v_row0, const int32_t* __restrict__ v_ctx_l,
                                                               const int64_t* __restrict__ v_win_off, int n_videos, int64_t total_win,
                                                               int W, int S, const float* __restrict__ txt,
                                                               const int32_t* __restrict__ cand, int n_cand, float* __restrict__ exact,
                                                               int32_t* __restrict__ c_slot, int32_t* __restrict__ c_win) {
    constexpr int DV = 256 * VPL, RPW = 4;
    constexpr int NW = PF_RS_NT / 64;
    __shared__ float red[NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.y, slot = blockIdx.x;
    const int32_t t = cand[(size_t)q * n_cand + slot];
    float m = -INFINITY;
    int v = -1, i = -1;
    if (t >= 0 && t < total_win) {                                  // (uniform over the workgroup)
        v = lib_window_owner(v_win_off, n_videos, t);
        i = (int)(t - v_win_off[v]);
        const int64_t row0 = v_row0[v], ctx_l = v_ctx_l[v];
        int64_t lo = max(((int64_t)i - 1) * S, (int64_t)0), hi = min(((int64_t)i - 1) * S + W, ctx_l);
        if (i < 0 || row0 < 0 || ctx_l > capacity - row0) hi = lo;
        const float* vid = arena + row0 * DV;
        float4 qv[1][VPL];
#pragma unroll
        for (int c = 0; c < VPL; ++c) qv[0][c] = reinterpret_cast<const float4*>(txt + (size_t)q * DV)[lane + 64 * c];
        for (int64_t f0 = lo + wave * RPW; f0 < hi; f0 += NW * RPW) {
            float4 x[RPW][VPL];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int64_t row = min(f0 + r, hi - 1);
#pragma unroll
                for (int c = 0; c < VPL; ++c) x[r][c] = reinterpret_cast<const float4*>(vid + row * DV)[lane + 64 * c];
            }
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const float part[1] = {pf_lane_dot<VPL>(x[r], qv[0])};
                const float s = wave_sum_multi<1>(part, lane);
                if (f0 + r < hi) m = fmaxf(m, s);
            }
        }
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float best = red[0];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) best = fmaxf(best, red[w2]);
        exact[(size_t)q * n_cand + slot] = best;
        c_slot[(size_t)q * n_cand + slot] = v;
        c_win[(size_t)q * n_cand + slot] = i;
    }
}

__global__ __launch_bounds__(256) void lib_fill_lists_kernel(int32_t* __restrict__ widx, float* __restrict__ wval, size_t n) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) { widx[e] = -1; wval[e] = -INFINITY; }
}

// One workgroup per query: the walk and the proof.  The candidates (n_cand <= LIB_CERT_MAX_CAND, in LDS) are ranked by (exact
// score desc, flat index asc) by counting: rs = a candidate's rank among those of its own slot, eligible iff rs < cap = min(K, its
// video's windows) -- the walk skips exactly the others --, pos = its rank among the eligible, taken iff pos < W.  A taken
// candidate's list position is rs (every candidate of its slot ahead of it is taken too).  t = the exact score at pos W - 1,
// c_last = the smallest coarse score of the set; E as in pf_certify_kernel, from the measures of the scan.  The lists were
// filled with -1 / -inf by lib_fill_lists_kernel; a taken candidate's element has this one writer.
constexpr int LIB_CERT_MAX_CAND = 4096;
__global__ __launch_bounds__(256) void lib_certify_kernel(const float* __restrict__ txt, int dv, const float* __restrict__ rn,
                                                          const int32_t* __restrict__ cand, const float* __restrict__ coarse,
                                                          const float* __restrict__ exact, const int32_t* __restrict__ c_slot,
                                                          const int32_t* __restrict__ c_win, const int64_t* __restrict__ v_win_off,
                                                          int n_cand, int64_t total_win, int n_videos, int K, int W,
                                                          int32_t* __restrict__ widx, float* __restrict__ wval,
                                                          int32_t* __restrict__ certified) {
    __shared__ float s_ex[LIB_CERT_MAX_CAND];
    __shared__ int s_flat[LIB_CERT_MAX_CAND];
    __shared__ int s_slot[LIB_CERT_MAX_CAND];           // -1: not eligible (after the first pass: an empty or capped candidate)
    __shared__ double nrm[4][3];
    __shared__ float c_min[4];
    __shared__ float s_t;
    __shared__ int s_taken[4];
    constexpr int PT = LIB_CERT_MAX_CAND / 256;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s_q = 0., s_h = 0., s_d = 0.;                            // |q|^2, |qh|^2, |qh - q|^2 (pf_certify_kernel)
    if (tid * 4 < dv) {
        const float4 a = reinterpret_cast<const float4*>(txt + (size_t)q * dv)[tid];
        const float e[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double x = e[j], h = pf16_rne(e[j]);
            s_q += x * x; s_h += h * h; s_d += (h - x) * (h - x);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s_q += __shfl_xor(s_q, o, 64); s_h += __shfl_xor(s_h, o, 64); s_d += __shfl_xor(s_d, o, 64);
    }
    if (lane == 0) { nrm[wave][0] = s_q; nrm[wave][1] = s_h; nrm[wave][2] = s_d; }
    float cm = INFINITY;
    int cap[PT];
    for (int j = tid; j < n_cand; j += 256) {
        const size_t at = (size_t)q * n_cand + j;
        const int flat = cand[at], v = c_slot[at];
        const bool ok = flat >= 0 && v >= 0 && v < n_videos;
        const float x = ok ? exact[at] : -INFINITY;
        s_ex[j] = x == x ? x : -INFINITY;
        s_flat[j] = ok ? flat : 0x7fffffff;
        s_slot[j] = ok ? v : -1;
        cm = fminf(cm, flat >= 0 ? coarse[at] : -INFINITY);
    }
#pragma unroll
    for (int u = 0; u < PT; ++u) {
        const int j = u * 256 + tid;
        cap[u] = 0;
        if (j < n_cand) {
            const int v = c_slot[(size_t)q * n_cand + j];
            if (v >= 0 && v < n_videos) cap[u] = (int)min((int64_t)K, v_win_off[v + 1] - v_win_off[v]);
        }
    }
    cm = -wave_max(-cm);
    if (lane == 0) c_min[wave] = cm;
    __syncthreads();
    int rs[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) {                                   // rank inside the slot
        const int j = u * 256 + tid;
        rs[u] = 0;
        if (j < n_cand && s_slot[j] >= 0) {
            const float x = s_ex[j];
            const int f = s_flat[j], v = s_slot[j];
            int r = 0;
            for (int i = 0; i < n_cand; ++i) {
                const float y = s_ex[i];
                r += (s_slot[i] == v) & ((y > x) | ((y == x) & (s_flat[i] < f)));
            }
            rs[u] = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PT; ++u) {
        const int j = u * 256 + tid;
        if (j < n_cand && s_slot[j] >= 0 && rs[u] >= cap[u]) s_slot[j] = -1;
    }
    __syncthreads();
    int mine = 0;
    float t_mine = 0.f;
    bool have_t = false;
#pragma unroll
    for (int u = 0; u < PT; ++u) {                                   // rank among the eligible
        const int j = u * 256 + tid;
        if (j < n_cand && s_slot[j] >= 0) {
            const float x = s_ex[j];
            const int f = s_flat[j];
            int pos = 0;
            for (int i = 0; i < n_cand; ++i) {
                const float y = s_ex[i];
                pos += (s_slot[i] >= 0) & ((y > x) | ((y == x) & (s_flat[i] < f)));
            }
            if (pos < W) {
                const size_t o = ((size_t)q * n_videos + s_slot[j]) * K + rs[u];
                widx[o] = c_win[(size_t)q * n_cand + j];
                wval[o] = x;
                ++mine;
                if (pos == W - 1) { t_mine = x; have_t = true; }
            }
        }
    }
    if (have_t) s_t = t_mine;                                        // (one candidate holds rank W - 1)
    mine = (int)wave_sum((float)mine);                               // (<= 256: exact in fp32)
    if (lane == 0) s_taken[wave] = mine;
    __syncthreads();
    if (tid != 0) return;
    const int taken = s_taken[0] + s_taken[1] + s_taken[2] + s_taken[3];
    const double n_q = sqrt(nrm[0][0] + nrm[1][0] + nrm[2][0] + nrm[3][0]), n_h = sqrt(nrm[0][1] + nrm[1][1] + nrm[2][1] + nrm[3][1]),
                 n_d = sqrt(nrm[0][2] + nrm[1][2] + nrm[2][2] + nrm[3][2]);
    const double R = rn[0], N = rn[1];
    const double du = (dv + 1) * 0x1p-24, gam = du / (1. - du);
    const double E = (R * n_h + N * n_d + 2. * gam * N * fmax(n_q, n_h)) * (1. + 0x1p-10) + PF_CERT_TINY * (1. + n_h + N);
    bool ok = total_win <= n_cand;
    if (!ok && taken == W) {
        const double t = s_t, c_last = fminf(fminf(c_min[0], c_min[1]), fminf(c_min[2], c_min[3]));
        ok = isfinite(E) && isfinite(t) && isfinite(c_last) && t - c_last > E;
    }
    certified[q] = ok ? 1 : 0;
}

struct LibCertLayout {
    int n_cand, n_chunks, group, pt;
    size_t hm, fr, win, lists_a, lists_b, cand, coarse, exact, c_slot, c_win, rn, total;
};
static LibCertLayout lib_cert_layout(int64_t total_hb, int64_t total_win, int nq, int W, int n_cand) {
    LibCertLayout L{};
    if (n_cand == 0) {
        const int64_t d = 4 * (int64_t)W > 128 ? 4 * (int64_t)W : 128;
        n_cand = (int)(d < total_win ? d : total_win);
    }
    L.n_cand = n_cand;
    L.n_chunks = (int)((total_win + TK_CH - 1) / TK_CH);
    L.pt = 2 * n_cand <= 256 * TK_PT ? TK_PT : 2 * TK_PT;           // a merge of two sets always fits: 2 n_cand <= 8192
    L.group = 256 * L.pt / n_cand;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; };
    L.hm = take((size_t)nq * total_hb * 4);
    L.fr = take((size_t)nq * total_hb * 4);
    L.win = take((size_t)nq * total_win * 4);
    L.lists_a = take((size_t)nq * L.n_chunks * n_cand * 8);         // values, then indices
    L.lists_b = take((size_t)nq * ((L.n_chunks + L.group - 1) / L.group) * n_cand * 8);
    L.cand = take((size_t)nq * n_cand * 4);
    L.coarse = take((size_t)nq * n_cand * 4);
    L.exact = take((size_t)nq * n_cand * 4);
    L.c_slot = take((size_t)nq * n_cand * 4);
    L.c_win = take((size_t)nq * n_cand * 4);
    L.rn = take(8);
    L.total = o;
    return L;
}

// The refusals from host values alone, in this order, before any pointer or the handles are looked at.
static int scan_certified_precheck(const cone_library* lib, int64_t n_videos, int64_t total_hb, int64_t total_win, int nq, int K, int W,
                                   int n_cand, int max_v_l) {
    const char* who = "library_scan_certified";
    if (int rc = scan_precheck(lib, n_videos, total_hb, nq, K, 1, max_v_l, who)) return rc;
    CONE_REQUIRE(W >= 1 && W <= 256, "%s: W=%d not in [1, 256]", who, W);
    CONE_REQUIRE(total_win == total_hb + n_videos && total_win < 0x7fffffff,
                 "%s: total_win=%lld is not total_hb=%lld + n_videos=%lld (a video of nh half-blocks has nh + 1 windows) or does not fit an int32 index",
                 who, (long long)total_win, (long long)total_hb, (long long)n_videos);
    if (n_cand != 0) {
        const int64_t lo = W < total_win ? W : total_win, hi = total_win < LIB_CERT_MAX_CAND ? total_win : LIB_CERT_MAX_CAND;
        CONE_REQUIRE(n_cand >= lo && n_cand <= hi, "%s: n_cand=%d must lie in [min(W, total_win)=%lld, min(total_win, %d)=%lld]", who,
                     n_cand, (long long)lo, LIB_CERT_MAX_CAND, (long long)hi);
    }
    return 0;
}

static int shadow_precheck(const cone_library* lib) {
    const char* who = "library_shadow";
    CONE_REQUIRE(lib, "%s: null argument", who);
    CONE_REQUIRE(lib->flags == 0, "%s: flags=%d: the shadow belongs to a plain fp32 library (flags 0)", who, lib->flags);
    CONE_REQUIRE(lib->capacity >= 1 && lib->capacity < (1ll << 31), "%s: capacity=%lld not in [1, 2^31)", who, (long long)lib->capacity);
    CONE_PF_REQUIRE_DIM("library_shadow", lib->v_dim);
    return 0;
}

static bool shadow_matches(const cone_library* lib, const cone_library_shadow* sh) {
    return sh->model == lib->model && sh->capacity == lib->capacity && sh->v_dim == lib->v_dim && sh->rows_bf16 && sh->err;
}

}  // namespace cone

extern "C" size_t cone_library_shadow_bytes(const cone_library* lib) {
    if (cone::shadow_precheck(lib)) return 0;
    return cone::align_up((size_t)lib->capacity * lib->v_dim * 2, 256) + cone::align_up((size_t)lib->capacity * 8, 256);
}

extern "C" int cone_library_shadow_open(const cone_library* lib, void* arena, size_t arena_bytes, cone_library_shadow* out) {
    const char* who = "library_shadow";
    if (int rc = cone::shadow_precheck(lib)) return rc;
    CONE_REQUIRE(arena && out, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)arena & 255) == 0, "%s: the arena must be 256-B aligned", who);
    const size_t need = cone_library_shadow_bytes(lib);
    CONE_REQUIRE(arena_bytes >= need, "%s: arena too small (%zu < %zu)", who, arena_bytes, need);
    out->model = lib->model;
    out->capacity = lib->capacity;
    out->v_dim = lib->v_dim;
    out->rows_bf16 = (uint16_t*)arena;
    out->err = (float*)((char*)arena + cone::align_up((size_t)lib->capacity * lib->v_dim * 2, 256));
    return 0;
}

extern "C" int cone_library_shadow_index(const cone_model* m, const cone_library* lib, const cone_library_shadow* shadow, int64_t row0,
                                         int64_t n_rows, void* stream) {
    const char* who = "library_shadow";
    if (int rc = cone::shadow_precheck(lib)) return rc;
    CONE_REQUIRE(row0 >= 0 && n_rows >= 1 && n_rows <= lib->capacity && row0 <= lib->capacity - n_rows,
                 "%s: rows [%lld, %lld + %lld) leave the arena of %lld", who, (long long)row0, (long long)row0, (long long)n_rows,
                 (long long)lib->capacity);
    CONE_REQUIRE(m && shadow, "%s: null argument", who);
    CONE_REQUIRE(lib->model == m, "%s: the library was opened with another handle", who);
    CONE_REQUIRE(cone::shadow_matches(lib, shadow), "%s: the shadow belongs to another library (handle, capacity or v_dim)", who);
    CONE_REQUIRE(lib->adapted, "%s: the library handle misses a region (not one cone_library_open filled)", who);
    int64_t blocks = (n_rows + 3) / 4;                                      // a wave per row, grid-stride past 64 workgroups per CU
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(cone::lib_shadow_index_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, lib->adapted, row0, n_rows,
                       lib->v_dim, shadow->rows_bf16, shadow->err);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t cone_library_scan_certified_workspace(const cone_library* lib, int64_t n_videos, int64_t total_hb, int64_t total_win,
                                                        int nq, int K, int W, int n_cand) {
    if (cone::scan_certified_precheck(lib, n_videos, total_hb, total_win, nq, K, W, n_cand, 2)) return 0;
    return cone::lib_cert_layout(total_hb, total_win, nq, W, n_cand).total;
}

extern "C" int cone_library_scan_certified(const cone_model* m, const cone_library* lib, const cone_library_shadow* shadow,
                                           const int64_t* v_row0, const int32_t* v_ctx_l, const int64_t* v_hb_off,
                                           const int64_t* v_win_off, int64_t n_videos, int64_t total_hb, int64_t total_win,
                                           const float* cls, int nq, int K, int W, int n_cand, const cone_session_params* params,
                                           int32_t* widx, float* wval, int32_t* certified, void* ws, size_t ws_bytes, void* stream) {
    using namespace cone;
    const char* who = "library_scan_certified";
    CONE_REQUIRE(lib && params, "%s: null argument", who);
    if (int rc = scan_certified_precheck(lib, n_videos, total_hb, total_win, nq, K, W, n_cand, params->max_v_l)) return rc;
    CONE_REQUIRE(m && shadow && v_row0 && v_ctx_l && v_hb_off && v_win_off && cls && widx && wval && certified && ws, "%s: null argument", who);
    CONE_REQUIRE(lib->model == m, "%s: the library was opened with another handle", who);
    CONE_REQUIRE(shadow_matches(lib, shadow), "%s: the shadow belongs to another library (handle, capacity or v_dim)", who);
    CONE_PF_REQUIRE_DIM("library_scan_certified", lib->v_dim);
    CONE_REQUIRE(lib->adapted, "%s: the library handle misses a region (not one cone_library_open filled)", who);
    CONE_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-B aligned", who);
    const LibCertLayout L = lib_cert_layout(total_hb, total_win, nq, W, n_cand);
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    float *hm = (float*)(w + L.hm), *fr = (float*)(w + L.fr), *win = (float*)(w + L.win);
    int32_t *cand = (int32_t*)(w + L.cand), *c_slot = (int32_t*)(w + L.c_slot), *c_win = (int32_t*)(w + L.c_win);
    float *coarse = (float*)(w + L.coarse), *exact = (float*)(w + L.exact);
    int* rn = (int*)(w + L.rn);
    const int Wl = params->max_v_l, S = Wl / 2, V = (int)n_videos, dv = lib->v_dim;
    // (1) + (2) the coarse scan and the measures of the rows it scores
    CONE_CHECK_HIP(hipMemsetAsync(rn, 0, 8, s));                            // +0.0f: the maxima's neutral element
    {
        const PfStreamGrid g(total_hb);
        const int qg = nq >= 3 ? 4 : nq;                                    // 3 queries ride a 4-query pass, as in pf_stream_passes
        ProfScope ps(PK_FRAME_SCORE, total_hb * S, dv, qg, nullptr, s);
        const dim3 grid(g.blocks, (unsigned)((nq + qg - 1) / qg));
#define CONE_SCAN16_LAUNCH(VPL, QG, WPH)                                                                                         \
    hipLaunchKernelGGL((library_scan_bf16_kernel<VPL, QG, CONE_PF_RPW, WPH>), grid, dim3(256), 0, s, shadow->rows_bf16, shadow->err, \
                       lib->capacity, dv, v_row0, v_ctx_l, v_hb_off, V, total_hb, S, cls, nq, hm, fr, rn)
#define CONE_SCAN16_FORMS(VPL)                                                                                                   \
    if (g.wide) { if (qg == 4) CONE_SCAN16_LAUNCH(VPL, 4, 4); else if (qg == 2) CONE_SCAN16_LAUNCH(VPL, 2, 4); else CONE_SCAN16_LAUNCH(VPL, 1, 4); } \
    else { if (qg == 4) CONE_SCAN16_LAUNCH(VPL, 4, 1); else if (qg == 2) CONE_SCAN16_LAUNCH(VPL, 2, 1); else CONE_SCAN16_LAUNCH(VPL, 1, 1); }
        if (dv <= 512) { CONE_SCAN16_FORMS(1) } else { CONE_SCAN16_FORMS(2) }
#undef CONE_SCAN16_FORMS
#undef CONE_SCAN16_LAUNCH
        CONE_LAUNCH_CHECK();
    }
    // (3) the coarse window row, (4) its n_cand best as a set: chunk sets, then merges until one set is left
    hipLaunchKernelGGL(lib_window_row_kernel, dim3((unsigned)((total_win + 255) / 256), (unsigned)nq), dim3(256), 0, s, hm, fr, v_hb_off,
                       v_win_off, V, total_hb, total_win, Wl & 1, win);
    CONE_LAUNCH_CHECK();
    {
        float* cv = (float*)(w + L.lists_a);
        int* ci = (int*)(cv + (size_t)nq * L.n_chunks * L.n_cand);
        hipLaunchKernelGGL(pf_cand_chunk_kernel, dim3((unsigned)L.n_chunks, (unsigned)nq), dim3(256), 0, s, win, total_win, L.n_cand, cv, ci,
                           L.n_chunks);
        CONE_LAUNCH_CHECK();
        char *in_buf = w + L.lists_a, *out_buf = w + L.lists_b;
        for (int n_lists = L.n_chunks;;) {
            const int n_groups = (n_lists + L.group - 1) / L.group;
            float* cv_in = (float*)in_buf;
            int* ci_in = (int*)(cv_in + (size_t)nq * n_lists * L.n_cand);
            float* cv_out = (float*)out_buf;
            int* ci_out = (int*)(cv_out + (size_t)nq * n_groups * L.n_cand);
            if (L.pt == TK_PT)
                hipLaunchKernelGGL(lib_cand_merge_kernel<TK_PT>, dim3((unsigned)n_groups, (unsigned)nq), dim3(256), 0, s, cv_in, ci_in, n_lists,
                                   L.n_cand, L.group, cv_out, ci_out, cand, coarse);
            else
                hipLaunchKernelGGL(lib_cand_merge_kernel<2 * TK_PT>, dim3((unsigned)n_groups, (unsigned)nq), dim3(256), 0, s, cv_in, ci_in,
                                   n_lists, L.n_cand, L.group, cv_out, ci_out, cand, coarse);
            CONE_LAUNCH_CHECK();
            if (n_groups == 1) break;
            n_lists = n_groups;                                 // (the lists shrink: each buffer holds every later level too)
            char* t = in_buf; in_buf = out_buf; out_buf = t;
        }
    }
    // (5) the candidates' exact scores
    pf_with_vpl(dv, [&](auto VPL) {
        hipLaunchKernelGGL(lib_rescore_kernel<decltype(VPL)::value>, dim3((unsigned)L.n_cand, (unsigned)nq), dim3(PF_RS_NT), 0, s, lib->adapted,
                           lib->capacity, v_row0, v_ctx_l, v_win_off, V, total_win, Wl, S, cls, cand, L.n_cand, exact, c_slot, c_win);
        return 0;
    });
    CONE_LAUNCH_CHECK();
    // (6) the lists' padding everywhere, then the walk and the proof
    {
        const size_t n = (size_t)nq * V * K;
        const size_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(lib_fill_lists_kernel, dim3((unsigned)(blocks > 256 * 8 ? 256 * 8 : blocks)), dim3(256), 0, s, widx, wval, n);
        CONE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lib_certify_kernel, dim3(nq), dim3(256), 0, s, cls, dv, (const float*)rn, cand, coarse, exact, c_slot, c_win, v_win_off,
                       L.n_cand, total_win, V, K, W, widx, wval, certified);
    CONE_LAUNCH_CHECK();
    return 0;
}
