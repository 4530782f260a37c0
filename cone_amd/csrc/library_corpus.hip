// Library moment search: stage C over ONE candidate pool per query -- everything that came out of the windows a budgeted
// search chose for the query, whichever videos they lie in (run_on_video/cone_localizator.py:187-221 with the pool in place
// of one video's topk_window windows).  The pool of a query is a list of SEGMENTS of the search's flat candidate buffer, a
// segment = the rows of one (video, query) pair, tagged with its video.  Both score lists are normalised over the whole pool;
// the dict is keyed by (tag, st, ed); a kept moment suppresses a later one only inside its own video.  One workgroup per
// query, fp64 throughout, the exactness rules of postproc.hip (stage_c.h); the fused ranking only.
//
// LDS (static, 61 KiB of 64): what postproc.hip keeps for three score types does not fit beside a tag per candidate, so the
// rounded proposal / matching scores live in registers while the pool is fused (4 candidates a thread) and are rounded again
// from the candidate rows for the few kept moments -- the same operation on the same fp32 value: the same double.
#include "stage_c.h"

namespace cone {

constexpr int kCorpusMaxQueries = 64 * 16;

__global__ __launch_bounds__(256) void corpus_fuse_nms_kernel(const float* __restrict__ cand, const int* __restrict__ seg_off,
                                                              const int64_t* __restrict__ seg_cand,
                                                              const int* __restrict__ seg_n, const int* __restrict__ seg_tag,
                                                              int n_seg, double thd, int max_before, int max_after,
                                                              double* out_rows, int* out_seg, int* out_n) {
    __shared__ double c_st[kMaxCand], c_ed[kMaxCand], c_fused[kMaxCand];
    __shared__ int64_t c_row[kMaxCand];     // the candidate's row in `cand`
    __shared__ int c_tag[kMaxCand];         // its video
    __shared__ int c_seg[kMaxCand];         // its segment's ordinal within the query
    __shared__ int u_first[kMaxCand];       // unique entries in first-insertion order: candidate id of the key
    __shared__ int u_last[kMaxCand];        //   candidate id whose values the dict holds for that key
    __shared__ int sidx[kMaxCand];          // unique-entry ids in score order
    // kept_pos | cidx (NMS scratch) share their 8 KiB with uval (the unique entries' values while they are ranked)
    __shared__ __attribute__((aligned(8))) int ibuf[2 * kMaxCand];
    int* kept_pos = ibuf;
    int* cidx = ibuf + kMaxCand;
    double* uval = reinterpret_cast<double*>(ibuf);
    __shared__ unsigned char flag[kMaxCand];
    __shared__ double red[4][4];
    __shared__ int s_cnt[4][kMaxCand / 256];
    __shared__ int s_wsum[4];
    __shared__ int s_nu, s_kept_n;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 0. the pool: the query's segments in table order, each one's rows in buffer order; candidates are taken until the pool
    // holds kMaxCand (the segment that crosses the cap is truncated, the ones behind it are empty).  A prefix sum of the
    // counts over 256 segments a round; every thread then lists its own segment.
    const int s_lo = max(seg_off[q], 0), s_hi = min(seg_off[q + 1], n_seg);
    int n = 0;
    for (int s0 = s_lo; s0 < s_hi && n < kMaxCand; s0 += 256) {
        const int s = s0 + tid;
        const int cnt = s < s_hi ? min(max(seg_n[s], 0), kMaxCand) : 0;
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int base = n;
        for (int w = 0; w < wave; ++w) base += s_wsum[w];
        const int total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        base += incl - cnt;
        if (cnt > 0 && base < kMaxCand) {
            const int take = min(cnt, kMaxCand - base);
            const int64_t row0 = seg_cand[s];
            const int tg = seg_tag[s];
            for (int r = 0; r < take; ++r) { c_row[base + r] = row0 + r; c_tag[base + r] = tg; c_seg[base + r] = s - s_lo; }
        }
        n = min(n + total, kMaxCand);
        __syncthreads();
    }

    // 1. float(f"{e:.4f}")
    double pr[kMaxCand / 256], ma[kMaxCand / 256];
#pragma unroll
    for (int k = 0; k < kMaxCand / 256; ++k) {
        const int i = k * 256 + tid;
        pr[k] = 0.0; ma[k] = 0.0;
        if (i < n) {
            const float* row = cand + c_row[i] * 4;
            c_st[i] = round4((double)row[0]);
            c_ed[i] = round4((double)row[1]);
            pr[k] = round4((double)row[2]);
            ma[k] = round4((double)row[3]);
        }
    }
    // 2. normalize_score on both lists, each over the whole pool + fused = (0 + a) + b
    double mn0 = INFINITY, mx0 = -INFINITY, mn1 = INFINITY, mx1 = -INFINITY;
#pragma unroll
    for (int k = 0; k < kMaxCand / 256; ++k)
        if (k * 256 + tid < n) {
            mn0 = fmin(mn0, pr[k]); mx0 = fmax(mx0, pr[k]);
            mn1 = fmin(mn1, ma[k]); mx1 = fmax(mx1, ma[k]);
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mn0 = fmin(mn0, __shfl_xor(mn0, o, 64)); mx0 = fmax(mx0, __shfl_xor(mx0, o, 64));
        mn1 = fmin(mn1, __shfl_xor(mn1, o, 64)); mx1 = fmax(mx1, __shfl_xor(mx1, o, 64));
    }
    if (lane == 0) { red[wave][0] = mn0; red[wave][1] = mx0; red[wave][2] = mn1; red[wave][3] = mx1; }
    __syncthreads();
    mn0 = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
    mx0 = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
    mn1 = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    mx1 = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
#pragma unroll
    for (int k = 0; k < kMaxCand / 256; ++k) {
        const int i = k * 256 + tid;
        if (i < n) {
            const double a = (mn0 == mx0) ? pr[k] : (pr[k] - mn0) / (mx0 - mn0);
            const double b = (mn1 == mx1) ? ma[k] : (ma[k] - mn1) / (mx1 - mn1);
            c_fused[i] = (0.0 + a) + b;
        }
    }
    __syncthreads();
    // 3. dict keyed by (tag, st, ed): first occurrence fixes the position, last occurrence the values (postproc.hip's step 3
    // with the tag in the key)
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        bool first = i < n;
        int last = i;
        if (i < n) {
            const double si = c_st[i], ei = c_ed[i];
            const int ti = c_tag[i];
            for (int j = 0; j < n; ++j) {
                const bool same = c_tag[j] == ti && c_st[j] == si && c_ed[j] == ei;
                first = first && !(same && j < i);
                last = same && j > last ? j : last;
            }
        }
        flag[i0 + tid] = first ? 1 : 0;             // (kMaxCand is a multiple of 256: in bounds)
        if (first) kept_pos[i] = last;              // parked: the value-holder of the key whose first occurrence is i
        const unsigned long long b = __ballot(first);
        if (lane == 0) s_cnt[wave][i0 >> 8] = __popcll(b);
    }
    __syncthreads();
    int nu_acc = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int base = nu_acc;
        for (int w = 0; w < wave; ++w) base += s_cnt[w][i0 >> 8];
        const bool first = i < n && flag[i];
        const unsigned long long b = __ballot(first);
        if (first) {
            const int u = base + __popcll(b & ((1ull << lane) - 1ull));
            u_first[u] = i;
            u_last[u] = kept_pos[i];
        }
        nu_acc += s_cnt[0][i0 >> 8] + s_cnt[1][i0 >> 8] + s_cnt[2][i0 >> 8] + s_cnt[3][i0 >> 8];
    }
    if (tid == 0) s_nu = nu_acc;
    __syncthreads();
    const int nu = s_nu;

    // 4. stable descending order of the unique entries by fused, truncate, NMS inside each video
    for (int u = tid; u < nu; u += 256) uval[u] = c_fused[u_last[u]];
    __syncthreads();
    for (int u = tid; u < nu; u += 256) {
        const double v = uval[u];
        int rank = 0;
        for (int w = 0; w < nu; ++w) {
            const double x = uval[w];
            rank += (x > v) || (x == v && w < u);
        }
        sidx[rank] = u;
    }
    __syncthreads();
    int kept;
    if (thd != -1.0) {
        const int m = min(nu, max_before);
        for (int j = tid; j < m; j += 256) cidx[j] = u_first[sidx[j]];
        __syncthreads();
        if (m > 0) {
            block_nms<true>(c_st, c_ed, c_tag, cidx, m, thd, max_after, flag, kept_pos, &s_kept_n);
            kept = s_kept_n;
        } else {
            kept = 0;
        }
    } else {
        kept = min(nu, max_after);
        for (int j = tid; j < kept; j += 256) kept_pos[j] = j;
        __syncthreads();
    }
    double* rows = out_rows + (size_t)q * max_after * 5;
    int* oseg = out_seg + (size_t)q * max_after;
    for (int j = tid; j < kept; j += 256) {
        const int u = sidx[kept_pos[j]];
        const int kf = u_first[u], kl = u_last[u];
        const float* row = cand + c_row[kl] * 4;
        rows[j * 5] = c_st[kf]; rows[j * 5 + 1] = c_ed[kf];
        rows[j * 5 + 2] = round4((double)row[2]); rows[j * 5 + 3] = round4((double)row[3]); rows[j * 5 + 4] = c_fused[kl];
        oseg[j] = c_seg[kf];
    }
    for (int j = kept + tid; j < max_after; j += 256) {     // rows past the kept ones: zeros / -1 (the caller need not pre-fill)
        rows[j * 5] = 0.0; rows[j * 5 + 1] = 0.0; rows[j * 5 + 2] = 0.0; rows[j * 5 + 3] = 0.0; rows[j * 5 + 4] = 0.0;
        oseg[j] = -1;
    }
    if (tid == 0) out_n[q] = kept;
}

}  // namespace cone

extern "C" int cone_corpus_fuse_nms(const float* cand, const int32_t* seg_off, const int64_t* seg_cand, const int32_t* seg_n,
                                    const int32_t* seg_tag, int nq, int n_seg, double nms_thd, int max_before, int max_after,
                                    double* out_rows, int32_t* out_seg, int32_t* out_n, void* stream) {
    CONE_REQUIRE(nq >= 1 && nq <= cone::kCorpusMaxQueries, "corpus_fuse_nms: nq=%d not in [1, %d]", nq, cone::kCorpusMaxQueries);
    CONE_REQUIRE(n_seg >= 0, "corpus_fuse_nms: n_seg=%d < 0", n_seg);
    CONE_REQUIRE(max_after >= 1 && max_after <= cone::kMaxCand, "corpus_fuse_nms: max_after=%d not in [1, %d]", max_after,
                 cone::kMaxCand);
    CONE_REQUIRE(max_before >= 1, "corpus_fuse_nms: max_before=%d < 1", max_before);
    // (a table of no segments has nothing to point at: every query answers 0 moments)
    CONE_REQUIRE(seg_off && out_rows && out_seg && out_n && (n_seg == 0 || (cand && seg_cand && seg_n && seg_tag)),
                 "corpus_fuse_nms: null argument");
    hipLaunchKernelGGL(cone::corpus_fuse_nms_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, cand, seg_off, seg_cand, seg_n,
                       seg_tag, n_seg, nms_thd, max_before, max_after, out_rows, out_seg, out_n);
    CONE_LAUNCH_CHECK();
    return 0;
}
