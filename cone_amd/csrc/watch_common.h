// What the two watcher files share (library_watch.hip: one video; library_watch_pool.hip: a slab per video of a library): the
// rule that says a cached window is still good, the loop that copies freshly computed rows into the cache and stamps them, the
// two size constants and the host refusals both make.  No asm, no atomics: every element has one writer and is written with a
// plain vector store.
#pragma once
#include "common.h"

namespace cone {

constexpr int WATCH_T = 256;            // threads of a workgroup = the most list entries (K), pairs and chosen windows of a query
constexpr int WATCH_MAX_NQ = 16;        // decoder slots per window

// A cached entry of window wi, computed when its video had `stamp` clips (0: never), is still good at ctx_l clips when the
// video has not grown since, or when (wi - 1) S + W <= stamp: the window's clip range [max((wi - 1) S, 0),
// min((wi - 1) S + W, ctx_l)) was not cut by the video's end when the entry was computed, so it is the range of today (a video
// only grows between two resets of the stamps).
__device__ __forceinline__ bool watch_valid(int wi, int stamp, int ctx_l, int W, int S) {
    return stamp == ctx_l || (stamp > 0 && (long long)(wi - 1) * S + W <= (long long)stamp);
}

// The workgroup copies the Nq rows of each of the n windows list[0 .. n) from src (n x Nq rows, list order) to the cache rows
// of window base + list[m], then stamps those windows (a workgroup of WATCH_T threads).  Two bounds, and an index outside either
// is skipped by both loops: cap = the windows of the video's slab, room = the windows the axis has from the slab's first on (a slab
// that overhangs the axis never reaches past it).  The listed windows are distinct: one writer per row and per stamp.
__device__ __forceinline__ void watch_store_rows(const int32_t* list, int n, const float4* src, int Nq, size_t base, int cap,
                                                 long long room, int stamp_value, float4* cache, int32_t* stamp) {
    const int t = threadIdx.x;
    for (int i = t; i < n * Nq; i += WATCH_T) {
        const int m = i / Nq, r = i - m * Nq;
        const int wi = list[m];
        if (wi >= 0 && wi < cap && (long long)wi < room) cache[(base + wi) * Nq + r] = src[(size_t)m * Nq + r];
    }
    for (int m = t; m < n; m += WATCH_T) {
        const int wi = list[m];
        if (wi >= 0 && wi < cap && (long long)wi < room) stamp[base + wi] = stamp_value;
    }
}

// The refusals the four entries share, from host values alone; each returns 0 or CONE_E_INVALID with the text set.  V = the
// slots of the scan's table (the one-video entries pass 1).
static int watch_precheck(const char* who, int nq, int V, int K) {
    CONE_REQUIRE(nq >= 1 && nq <= CONE_SESSION_MAX_QUERIES, "%s: nq=%d not in [1, %d]", who, nq, CONE_SESSION_MAX_QUERIES);
    CONE_REQUIRE(V >= 1, "%s: V=%d < 1", who, V);
    CONE_REQUIRE(K >= 1 && K <= WATCH_T, "%s: K=%d not in [1, %d]", who, K, WATCH_T);
    return 0;
}
static int watch_check_slots(const char* who, int Nq) {
    CONE_REQUIRE(Nq >= 1 && Nq <= WATCH_MAX_NQ, "%s: Nq=%d not in [1, %d]", who, Nq, WATCH_MAX_NQ);
    return 0;
}
static int watch_check_rows(const char* who, const void* cand, const void* cache) {
    CONE_REQUIRE((((uintptr_t)cand | (uintptr_t)cache) & 15) == 0, "%s: cand and cache must be 16-B aligned", who);
    return 0;
}

}  // namespace cone
