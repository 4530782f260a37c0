// Stage C's shared arithmetic: what fuse_nms_kernel (postproc.hip: the candidates of one (video, query) pair) and
// corpus_fuse_nms_kernel (library_corpus.hip: the candidates of one query over many videos) both do, in fp64 exactly like the
// reference's Python floats (cone/inference.py:83; utils/temporal_nms.py:6-74).  Files that include this are built with
// -ffp-contract=off (cone_amd/build.py: NO_CONTRACT).
#pragma once
#include "common.h"

namespace cone {

constexpr int kMaxCand = 1024;

// float(f"{x:.4f}") for an fp32 x: x*1e4 is exact in fp64 (24-bit x 14-bit significands), so rint(x*1e4)/1e4 (round-half-even,
// correctly rounded division) is the same double that Python's correctly-rounded format + parse produces.
__device__ __forceinline__ double round4(double x) { return rint(x * 1e4) / 1e4; }

__device__ __forceinline__ double pseudo_iou(double s0, double e0, double s1, double e1) {
    const double lo = fmin(e0, e1) - fmax(s0, s1);
    const double inter = lo > 0.0 ? lo : 0.0;
    const double uni = fmax(e0, e1) - fmin(s0, s1);
    return uni == 0.0 ? 0.0 : inter / uni;
}

// Greedy NMS over `m` candidates already in score order (sidx[j] = candidate id at sorted position j).
// Block-cooperative; writes kept sorted positions.  kTags: a kept candidate suppresses a later one only where tag[] agrees
// (moments of different videos never overlap); without it `tag` is not read.
template <bool kTags>
__device__ void block_nms(const double* st, const double* ed, const int* tag, const int* sidx, int m, double thd,
                          int max_after, unsigned char* alive, int* kept_pos, int* kept_n_out) {
    const int tid = threadIdx.x;
    __shared__ int s_cur;
    __shared__ int s_kept;
    for (int j = tid; j < m; j += blockDim.x) alive[j] = 1;
    if (tid == 0) { s_kept = 0; s_cur = 0; }
    __syncthreads();
    if (m == 1) {  // utils/temporal_nms.py:38-39
        if (tid == 0) { kept_pos[0] = 0; *kept_n_out = 1; }
        __syncthreads();
        return;
    }
    int start = 0;
    while (true) {
        if (tid == 0) {
            int c = start;
            while (c < m && !alive[c]) ++c;
            s_cur = c;
            if (c < m && s_kept < max_after) kept_pos[s_kept++] = c; else s_cur = m;
        }
        __syncthreads();
        const int cur = s_cur;
        if (cur >= m) break;
        const double s0 = st[sidx[cur]], e0 = ed[sidx[cur]];
        const int t0 = kTags ? tag[sidx[cur]] : 0;
        for (int j = cur + 1 + tid; j < m; j += blockDim.x)
            if (alive[j] && (!kTags || tag[sidx[j]] == t0) && pseudo_iou(s0, e0, st[sidx[j]], ed[sidx[j]]) > thd) alive[j] = 0;
        start = cur + 1;
        __syncthreads();
    }
    if (tid == 0) *kept_n_out = s_kept;
    __syncthreads();
}

}  // namespace cone
