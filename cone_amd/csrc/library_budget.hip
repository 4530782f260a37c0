// Library window budgets (include/cone_hip.h, "library window budgets"): the W best windows of a query over EVERY video of a
// cone_library_scan, and how many of them fall to which video.
//
// A scan leaves, per (query, video slot), the stable descending list of that video's window scores: (nq, n_videos, scan_K).
// Viewed as one row of n_videos * scan_K values per query, the order the contract asks for -- value descending, ties to the lower
// slot, then to the lower list position, -0.0 == +0.0 -- IS the order of cone_topk_windows_ws on that row (ties to the lower flat
// index slot * scan_K + j), so the selection is that launcher, in whichever of its forms the row's length picks.  What is new
// here is the step behind it: one workgroup of 256 threads per query turns the min(W, row length) selected flat indices into the
// (slot, count, best score) triples of the videos they fall into, in order of first appearance.
//
// The compaction: thread i < n holds selected entry i (its slot in LDS; entries of -inf, the lists' padding and windows of NaN
// frames alike, are dropped: they sort behind every number, so the kept entries are a prefix).  It walks the n <= 256 slots in
// LDS once: the entries of its slot are its pair's count, an earlier entry of its slot means another thread speaks for the pair.
// A second walk over the "first" flags ranks the pairs.  2 x 256 LDS reads per thread, two barriers, no atomics; every output
// element has one writer and is written with a plain vector store (rows past n_pairs: -1 / 0 / -inf).
#include "common.h"

namespace cone {

constexpr int BUDGET_MAX_W = 256;       // one thread per selected entry
constexpr size_t BUDGET_ALIGN = 256;

__global__ __launch_bounds__(BUDGET_MAX_W) void library_budget_pairs_kernel(const int32_t* __restrict__ sel_idx,
                                                                            const float* __restrict__ sel_val, int n_sel, int scan_K,
                                                                            int W, int32_t* __restrict__ n_pairs,
                                                                            int32_t* __restrict__ pair_slot, int32_t* __restrict__ pair_k,
                                                                            float* __restrict__ pair_best) {
    __shared__ int s_slot[BUDGET_MAX_W];            // slot of selected entry i; -1: not chosen
    __shared__ unsigned char s_first[BUDGET_MAX_W];
    const int q = blockIdx.x, t = threadIdx.x;
    int slot = -1;
    float val = -INFINITY;
    if (t < n_sel) {
        const int idx = sel_idx[(size_t)q * n_sel + t];
        val = sel_val[(size_t)q * n_sel + t];
        if (idx >= 0 && val > -INFINITY) slot = idx / scan_K;
    }
    s_slot[t] = slot;
    __syncthreads();
    int count = 0;
    bool first = slot >= 0;
    for (int j = 0; j < n_sel; ++j) {
        const bool same = s_slot[j] == slot;
        count += same;
        first = first && !(same && j < t);
    }
    s_first[t] = first;
    __syncthreads();
    int rank = 0, total = 0;
    for (int j = 0; j < n_sel; ++j) {
        rank += (j < t) & s_first[j];
        total += s_first[j];
    }
    int32_t* o_slot = pair_slot + (size_t)q * W;
    int32_t* o_k = pair_k + (size_t)q * W;
    float* o_best = pair_best + (size_t)q * W;
    if (first) { o_slot[rank] = slot; o_k[rank] = count; o_best[rank] = val; }      // rank < total <= n_sel <= W
    if (t >= total && t < W) { o_slot[t] = -1; o_k[t] = 0; o_best[t] = -INFINITY; }
    if (t == 0) n_pairs[q] = total;
}

struct BudgetLayout { size_t sel_idx, sel_val, topk_ws, topk_bytes, total; int n_sel; };
static BudgetLayout budget_layout(int nq, int64_t n_videos, int scan_K, int W) {
    BudgetLayout L{};
    const int64_t row = n_videos * scan_K;
    L.n_sel = (int)(W < row ? W : row);
    const size_t list = align_up((size_t)nq * L.n_sel * 4, BUDGET_ALIGN);
    L.sel_idx = 0; L.sel_val = list; L.topk_ws = 2 * list;
    L.topk_bytes = cone_topk_windows_workspace(nq, row, L.n_sel);
    L.total = L.topk_ws + align_up(L.topk_bytes, BUDGET_ALIGN);
    return L;
}

// The refusals from host values alone, in this order, before any pointer is looked at.
static int budget_precheck(int nq, int64_t n_videos, int scan_K, int W) {
    const char* who = "library_budget";
    CONE_REQUIRE(nq >= 1 && nq <= CONE_SESSION_MAX_QUERIES, "%s: nq=%d not in [1, %d]", who, nq, CONE_SESSION_MAX_QUERIES);
    CONE_REQUIRE(n_videos >= 1, "%s: n_videos=%lld < 1", who, (long long)n_videos);
    CONE_REQUIRE(scan_K >= 1 && scan_K <= 256, "%s: scan_K=%d not in [1, 256]", who, scan_K);
    CONE_REQUIRE(W >= 1 && W <= BUDGET_MAX_W, "%s: W=%d not in [1, %d]", who, W, BUDGET_MAX_W);
    CONE_REQUIRE(n_videos < 0x7fffffff / scan_K, "%s: n_videos=%lld x scan_K=%d entries per query do not fit an int32 index", who,
                 (long long)n_videos, scan_K);
    return 0;
}

}  // namespace cone

extern "C" size_t cone_library_budget_workspace(int nq, int64_t n_videos, int scan_K, int W) {
    if (cone::budget_precheck(nq, n_videos, scan_K, W)) return 0;
    return cone::budget_layout(nq, n_videos, scan_K, W).total;
}

extern "C" int cone_library_budget(const float* wval, int nq, int64_t n_videos, int scan_K, int W, int32_t* n_pairs, int32_t* pair_slot,
                                   int32_t* pair_k, float* pair_best, void* ws, size_t ws_bytes, void* stream) {
    using namespace cone;
    const char* who = "library_budget";
    if (int rc = budget_precheck(nq, n_videos, scan_K, W)) return rc;
    CONE_REQUIRE(wval && n_pairs && pair_slot && pair_k && pair_best && ws, "%s: null argument", who);
    CONE_REQUIRE(((uintptr_t)ws & (BUDGET_ALIGN - 1)) == 0, "%s: the workspace must be 256-B aligned", who);
    const BudgetLayout L = budget_layout(nq, n_videos, scan_K, W);
    if (ws_bytes < L.total) { set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, L.total); return CONE_E_WORKSPACE; }
    char* w = (char*)ws;
    int32_t* sel_idx = (int32_t*)(w + L.sel_idx);
    float* sel_val = (float*)(w + L.sel_val);
    if (int rc = cone_topk_windows_ws(wval, nq, n_videos * scan_K, L.n_sel, sel_idx, sel_val, w + L.topk_ws, L.topk_bytes, stream)) return rc;
    hipLaunchKernelGGL(library_budget_pairs_kernel, dim3(nq), dim3(BUDGET_MAX_W), 0, (hipStream_t)stream, sel_idx, sel_val, L.n_sel,
                       scan_K, W, n_pairs, pair_slot, pair_k, pair_best);
    CONE_LAUNCH_CHECK();
    return 0;
}
