// Standing queries on a live video (include/cone_hip.h, "standing queries"): the two small launches of a poll that sit around
// the query half.  A watcher keeps, per (query, window), the Nq candidate rows the window model produced and the video's ctx_l at
// that time (the stamp).  cone_watch_plan reads a one-video scan's lists and says which listed windows must run (never seen, or
// seen while they were still growing), and lays the segment table of stage C over the cache; cone_watch_store copies the rows the
// query half then wrote into their cache rows and stamps them.
//
// Both are latency-bound: one workgroup of 256 threads per query, a few hundred bytes each.  The compaction of the missing
// entries keeps list order: a wave ballot and the count of the lower lanes inside a wave, the four waves' totals through LDS
// (K <= 256 = one entry per thread).  Every output element has exactly one writer and is written with a plain vector store.
// The validity rule, the store loop, the constants and the shared refusals are watch_common.h's.
#include "watch_common.h"

namespace cone {

__global__ __launch_bounds__(WATCH_T) void watch_plan_kernel(const int32_t* __restrict__ widx, const float* __restrict__ wval,
                                                                 int nq, int K, const int32_t* __restrict__ stamp, int n_win, int ctx_l,
                                                                 int W, int Nq, int32_t* __restrict__ miss_widx,
                                                                 float* __restrict__ miss_wval, int32_t* __restrict__ n_miss,
                                                                 int32_t* __restrict__ seg_off, int64_t* __restrict__ seg_cand,
                                                                 int32_t* __restrict__ seg_n, int32_t* __restrict__ seg_tag) {
    __shared__ int s_wave[WATCH_T / 64];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t row = (size_t)q * K;
    int wi = -1;
    float val = -INFINITY;
    bool listed = false, missing = false;
    if (t < K) {
        wi = widx[row + t];
        val = wval[row + t];
        listed = wi >= 0 && wi < n_win;
        if (listed) missing = !watch_valid(wi, stamp[(size_t)q * n_win + wi], ctx_l, W, W / 2);
        seg_cand[row + t] = listed ? ((int64_t)q * n_win + wi) * Nq : 0;
        seg_n[row + t] = listed ? Nq : 0;
        seg_tag[row + t] = 0;
    }
    const unsigned long long b = __ballot(missing);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (missing) {                                  // base + lower lanes < total <= K
        const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
        miss_widx[row + pos] = wi;
        miss_wval[row + pos] = val;
    }
    if (t >= total && t < K) { miss_widx[row + t] = -1; miss_wval[row + t] = -INFINITY; }
    if (t == 0) {
        n_miss[q] = total;
        seg_off[q] = q * K;
        if (q == nq - 1) seg_off[nq] = nq * K;
    }
}

__global__ __launch_bounds__(WATCH_T) void watch_store_kernel(const float4* __restrict__ cand, const int32_t* __restrict__ miss_widx,
                                                          const int32_t* __restrict__ n_miss, int K, int n_win, int ctx_l, int Nq,
                                                          float4* __restrict__ cache, int32_t* __restrict__ stamp) {
    __shared__ int s_first;         // window rows of the queries before this one
    const int q = blockIdx.x, t = threadIdx.x;
    if (t < 64) {                   // nq <= 64: one lane per earlier query, one wave sum
        int c = t < q ? min(max(n_miss[t], 0), K) : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        if (t == 0) s_first = c;
    }
    __syncthreads();
    const int n = min(max(n_miss[q], 0), K);
    // the one video's slab is the whole axis: windows [0, n_win) of query q
    watch_store_rows(miss_widx + (size_t)q * K, n, cand + (size_t)s_first * Nq, Nq, (size_t)q * n_win, n_win, n_win, ctx_l, cache, stamp);
}

}  // namespace cone

extern "C" int cone_watch_plan(const int32_t* widx, const float* wval, int nq, int K, const int32_t* stamp, int n_win, int ctx_l, int W,
                               int Nq, int32_t* miss_widx, float* miss_wval, int32_t* n_miss, int32_t* seg_off, int64_t* seg_cand,
                               int32_t* seg_n, int32_t* seg_tag, void* stream) {
    using namespace cone;
    const char* who = "watch_plan";     // (the refusals from host values alone, in this order, before any pointer is looked at)
    if (int rc = watch_precheck(who, nq, 1, K)) return rc;
    if (int rc = watch_check_slots(who, Nq)) return rc;
    CONE_REQUIRE(n_win >= 1, "%s: n_win=%d < 1", who, n_win);
    CONE_REQUIRE(ctx_l >= 1, "%s: ctx_l=%d < 1", who, ctx_l);
    CONE_REQUIRE(W >= 2, "%s: W=%d < 2", who, W);
    CONE_REQUIRE(widx && wval && stamp && miss_widx && miss_wval && n_miss && seg_off && seg_cand && seg_n && seg_tag,
                 "%s: null argument", who);
    hipLaunchKernelGGL(watch_plan_kernel, dim3(nq), dim3(WATCH_T), 0, (hipStream_t)stream, widx, wval, nq, K, stamp, n_win, ctx_l, W,
                       Nq, miss_widx, miss_wval, n_miss, seg_off, seg_cand, seg_n, seg_tag);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" int cone_watch_store(const float* cand, const int32_t* miss_widx, const int32_t* n_miss, int nq, int K, int n_win, int ctx_l,
                                int Nq, float* cache, int32_t* stamp, void* stream) {
    using namespace cone;
    const char* who = "watch_store";
    if (int rc = watch_precheck(who, nq, 1, K)) return rc;
    CONE_REQUIRE(n_win >= 1, "%s: n_win=%d < 1", who, n_win);
    CONE_REQUIRE(ctx_l >= 1, "%s: ctx_l=%d < 1", who, ctx_l);
    if (int rc = watch_check_slots(who, Nq)) return rc;
    CONE_REQUIRE(cand && miss_widx && n_miss && cache && stamp, "%s: null argument", who);
    if (int rc = watch_check_rows(who, cand, cache)) return rc;
    hipLaunchKernelGGL(watch_store_kernel, dim3(nq), dim3(WATCH_T), 0, (hipStream_t)stream, (const float4*)cand, miss_widx, n_miss, K,
                       n_win, ctx_l, Nq, (float4*)cache, stamp);
    CONE_LAUNCH_CHECK();
    return 0;
}
