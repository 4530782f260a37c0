// Standing queries over a library (include/cone_hip.h, "standing queries over a library"): the two small launches of a
// LibraryWatcher's poll that sit around the query half.  The watcher keeps ONE cache (nq, n_win_total, Nq, 4) and ONE stamp plane
// (nq, n_win_total) for every watched video: table slot s owns the windows [v_win0[s], v_win0[s] + v_cap[s]) of the axis and its
// stamps are clip counts of ITS video (v_ctx_l[s]).  cone_watch_pool_plan reads a library scan's lists and the budget's pairs, says
// which chosen windows must run -- per pair, in list order -- and lays the segment table of stage C over the cache, one segment
// per chosen window in pool order; cone_watch_pool_store copies the rows the query half then wrote into the cache and stamps them.
//
// Both are latency-bound.  The plan runs one workgroup of 256 threads per query: thread t owns the t-th chosen window.  Two
// workgroup prefix sums, both by wave scans whose four totals go through LDS (library_watch.hip's idiom): pair_k over the pairs
// (which pair owns ordinal t), the missing flags over the ordinals (a wave ballot and the count of the lower lanes); a pair's
// misses are the difference of the second at the pair's two ends, so the compaction is stable and segmented across wave edges.
// The store runs one workgroup per job (a pair that missed something).  Every output element has exactly one writer and is written
// with a plain vector store.  A window is missing by watch_common.h's rule (watch_valid) at ITS video's clip count; the store
// loop, the constants and the shared refusals are that header's too.
#include "watch_common.h"

namespace cone {

// Inclusive prefix sum of v over the 256 threads; s_wave holds the four waves' totals afterwards (the caller syncs before it
// reuses s_wave).
__device__ __forceinline__ int pool_scan_incl(int v, int* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += s_wave[w];
    return v;
}

__global__ __launch_bounds__(WATCH_T) void watch_pool_plan_kernel(
    const int32_t* __restrict__ widx, const float* __restrict__ wval, const int32_t* __restrict__ n_pairs,
    const int32_t* __restrict__ pair_slot, const int32_t* __restrict__ pair_k, const int32_t* __restrict__ v_ctx_l,
    const int32_t* __restrict__ v_win0, const int32_t* __restrict__ v_cap, const int32_t* __restrict__ stamp, int nq, int V, int K,
    int Wb, int n_win_total, int W, int Nq, int32_t* __restrict__ miss_widx, float* __restrict__ miss_wval,
    int32_t* __restrict__ pair_miss, int32_t* __restrict__ seg_off, int64_t* __restrict__ seg_cand, int32_t* __restrict__ seg_n,
    int32_t* __restrict__ seg_tag) {
    __shared__ int s_end[WATCH_T];           // chosen windows up to and including pair p
    __shared__ int s_slot[WATCH_T];
    __shared__ int s_before[WATCH_T + 1];    // missing windows among the ordinals below t; [256] = all of them
    __shared__ int s_wave_k[WATCH_T / 64], s_wave_m[WATCH_T / 64];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const size_t prow = (size_t)q * Wb;
    // ---- the pairs: thread t is pair t
    const int np = min(max(n_pairs[q], 0), Wb);
    int slot = -1, k = 0;
    if (t < np) {
        slot = pair_slot[prow + t];
        k = min(max(pair_k[prow + t], 0), K);
        if (slot < 0 || slot >= V) k = 0;       // an empty pair
    }
    const int end = pool_scan_incl(k, s_wave_k);
    s_end[t] = end;
    s_slot[t] = slot;
    __syncthreads();
    const int total = min(s_end[WATCH_T - 1], Wb);      // chosen windows past the first Wb are neither planned nor listed
    // ---- the chosen windows: thread t is ordinal t
    int p = 0, j = 0, wslot = 0, wi = -1, first = 0;
    float val = -INFINITY;
    bool listed = false, missing = false;
    size_t lrow = 0;
    int64_t cand = 0;
    if (t < total) {
        int lo = 0, hi = WATCH_T - 1;                    // the first pair whose end lies above t (s_end[255] > t)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] > t) hi = mid; else lo = mid + 1;
        }
        p = lo;
        first = p ? s_end[p - 1] : 0;
        j = t - first;
        wslot = s_slot[p];                              // (k > 0: the slot lies in [0, V))
        lrow = ((size_t)q * V + wslot) * K;
        wi = widx[lrow + j];
        val = wval[lrow + j];
        const int win0 = v_win0[wslot];
        listed = wi >= 0 && wi < v_cap[wslot] && win0 >= 0 && (long long)win0 + wi < (long long)n_win_total;
        if (listed) {
            const size_t at = (size_t)q * n_win_total + win0 + wi;
            missing = !watch_valid(wi, stamp[at], v_ctx_l[wslot], W, W / 2);
            cand = (int64_t)at * Nq;
        }
    }
    if (t < Wb) {
        seg_cand[prow + t] = cand;
        seg_n[prow + t] = listed ? Nq : 0;
        seg_tag[prow + t] = t < total ? wslot : 0;
    }
    // ---- the missing windows below every ordinal
    const unsigned long long b = __ballot(missing);
    const int wave_total = __popcll(b);
    if (lane == 0) s_wave_m[t >> 6] = wave_total;
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < (t >> 6); ++w) before += s_wave_m[w];
    s_before[t] = before;
    if (t == 0) s_before[WATCH_T] = s_wave_m[0] + s_wave_m[1] + s_wave_m[2] + s_wave_m[3];
    __syncthreads();
    if (t < total) {        // ordinal t is entry j of pair p: the pair's misses first, in list order, then the padding
        const int last = min(s_end[p], total);
        const int n_miss = s_before[last] - s_before[first];
        if (missing) {
            const int pos = before - s_before[first];   // < n_miss <= last - first <= K
            miss_widx[lrow + pos] = wi;
            miss_wval[lrow + pos] = val;
        }
        if (j >= n_miss) { miss_widx[lrow + j] = -1; miss_wval[lrow + j] = -INFINITY; }
    }
    if (t < Wb) {           // thread t is pair t again
        int n_miss = 0;
        if (t < np) {
            const int lo = min(end - k, total), hi = min(end, total);
            n_miss = s_before[hi] - s_before[lo];
        }
        pair_miss[prow + t] = n_miss;
    }
    if (t == 0) {
        seg_off[q] = q * Wb;
        if (q == nq - 1) seg_off[nq] = nq * Wb;
    }
}

__global__ __launch_bounds__(WATCH_T) void watch_pool_store_kernel(
    const float4* __restrict__ cand, const int32_t* __restrict__ jobs, const int32_t* __restrict__ miss_widx,
    const int32_t* __restrict__ v_ctx_l, const int32_t* __restrict__ v_win0, const int32_t* __restrict__ v_cap, int nq, int V, int K,
    int n_win_total, int Nq, float4* __restrict__ cache, int32_t* __restrict__ stamp) {
    const int32_t* job = jobs + (size_t)blockIdx.x * 4;
    const int q = job[0], slot = job[1], n = min(max(job[2], 0), K), first = job[3];
    if (q < 0 || q >= nq || slot < 0 || slot >= V || first < 0) return;        // (uniform over the workgroup)
    const int win0 = v_win0[slot], cap = v_cap[slot], ctx_l = v_ctx_l[slot];
    if (win0 < 0) return;
    watch_store_rows(miss_widx + ((size_t)q * V + slot) * K, n, cand + (size_t)first, Nq, (size_t)q * n_win_total + win0, cap,
                     (long long)n_win_total - win0, ctx_l, cache, stamp);
}

}  // namespace cone

extern "C" int cone_watch_pool_plan(const int32_t* widx, const float* wval, const int32_t* n_pairs, const int32_t* pair_slot,
                                    const int32_t* pair_k, const int32_t* v_ctx_l, const int32_t* v_win0, const int32_t* v_cap,
                                    const int32_t* stamp, int nq, int V, int K, int Wb, int n_win_total, int W, int Nq,
                                    int32_t* miss_widx, float* miss_wval, int32_t* pair_miss, int32_t* seg_off, int64_t* seg_cand,
                                    int32_t* seg_n, int32_t* seg_tag, void* stream) {
    using namespace cone;
    const char* who = "watch_pool_plan";    // (the refusals from host values alone, in this order, before any pointer is looked at)
    if (int rc = watch_precheck(who, nq, V, K)) return rc;
    CONE_REQUIRE(Wb >= 1 && Wb <= WATCH_T, "%s: Wb=%d not in [1, %d]", who, Wb, WATCH_T);
    if (int rc = watch_check_slots(who, Nq)) return rc;
    CONE_REQUIRE(n_win_total >= 1, "%s: n_win_total=%d < 1", who, n_win_total);
    CONE_REQUIRE(W >= 2, "%s: W=%d < 2", who, W);
    CONE_REQUIRE(widx && wval && n_pairs && pair_slot && pair_k && v_ctx_l && v_win0 && v_cap && stamp && miss_widx && miss_wval &&
                     pair_miss && seg_off && seg_cand && seg_n && seg_tag,
                 "%s: null argument", who);
    hipLaunchKernelGGL(watch_pool_plan_kernel, dim3(nq), dim3(WATCH_T), 0, (hipStream_t)stream, widx, wval, n_pairs, pair_slot, pair_k,
                       v_ctx_l, v_win0, v_cap, stamp, nq, V, K, Wb, n_win_total, W, Nq, miss_widx, miss_wval, pair_miss, seg_off,
                       seg_cand, seg_n, seg_tag);
    CONE_LAUNCH_CHECK();
    return 0;
}

extern "C" int cone_watch_pool_store(const float* cand, const int32_t* jobs, int n_jobs, const int32_t* miss_widx,
                                     const int32_t* v_ctx_l, const int32_t* v_win0, const int32_t* v_cap, int nq, int V, int K,
                                     int n_win_total, int Nq, float* cache, int32_t* stamp, void* stream) {
    using namespace cone;
    const char* who = "watch_pool_store";
    if (int rc = watch_precheck(who, nq, V, K)) return rc;
    if (int rc = watch_check_slots(who, Nq)) return rc;
    CONE_REQUIRE(n_win_total >= 1, "%s: n_win_total=%d < 1", who, n_win_total);
    CONE_REQUIRE(n_jobs >= 1, "%s: n_jobs=%d < 1", who, n_jobs);
    CONE_REQUIRE(cand && jobs && miss_widx && v_ctx_l && v_win0 && v_cap && cache && stamp, "%s: null argument", who);
    if (int rc = watch_check_rows(who, cand, cache)) return rc;
    hipLaunchKernelGGL(watch_pool_store_kernel, dim3(n_jobs), dim3(WATCH_T), 0, (hipStream_t)stream, (const float4*)cand, jobs, miss_widx,
                       v_ctx_l, v_win0, v_cap, nq, V, K, n_win_total, Nq, (float4*)cache, stamp);
    CONE_LAUNCH_CHECK();
    return 0;
}
