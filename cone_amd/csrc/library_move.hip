// Library maintenance (include/cone_hip.h, "library maintenance"): moving resident rows of a video library, bit for bit.
//
// Everything a library holds per clip is a row in four or five planes (vid_norm, adapted or adapted_bf16, vproj, qkv_vid:
// arena_layout in session.hip), and a row's bits do not depend on where it lives.  Compacting an arena in place and resizing
// into another one are therefore the same pure HBM copy: a list of row ranges ("moves"), given as a DEVICE table, copied in
// every present plane.  One kernel body does it in three forms: table -> table (a direct call), table -> packed (the gather
// of a staged call) and packed -> table (its scatter); a staged call is the last two in stream order, which is what makes it
// correct for any overlap between the rows it reads and the rows it writes.
//
// The tile: a workgroup of 256 threads owns LIBRARY_MOVE_TILE = 16 consecutive rows of the call's flat row list (the moves laid
// end to end).  It finds the move of its first row by binary search in mv_off, walks the moves its rows belong to, and copies
// each (piece of a move, plane) as one contiguous run of 16-B words: rows of a move are contiguous in the source and in the
// destination.  At 6 KiB per clip (v_dim = hidden_dim = 256, fp32) a tile is 96 KiB, 24 words per thread.  A thread loads four
// words -- four wave-wide 1 KiB accesses, i.e. several rows per wave -- before it stores them (plain dwordx4 stores: the line
// stays in L2 for whoever reads the rows next); the loop runs whole rounds of 1 024 words without a per-thread guard, because a
// guard per load makes the compiler wait for each load before the next branch.  Every byte is read once and written once; no LDS, no atomics, no waiting
// between workgroups, nothing allocated, no read-back: both forms can be captured in a graph.
//
// The table is untrusted: a move whose source range leaves [0, src capacity) or whose destination range leaves
// [0, dst capacity) is skipped whole (not read, not written), and a table whose offsets are not the prefix sums they should
// be can make a workgroup skip rows but never leave a listed, checked range or the staging rows of the call.
#include "common.h"

namespace cone {

constexpr int MOVE_TILE = 16;       // flat rows per workgroup (tests/move_refs.py: TILE)
constexpr int MOVE_THREADS = 256;
constexpr int MOVE_UNROLL = 4;      // 16-B words a thread has in flight before its stores
constexpr int MOVE_PLANES = 5;
constexpr size_t MOVE_ALIGN = 256;

struct MovePlanes {
    const char* src[MOVE_PLANES];   // table form: the plane's row 0; packed form: the plane's region of the staging buffer
    char* dst[MOVE_PLANES];
    int32_t row_words[MOVE_PLANES]; // 16-B words per row
    int32_t n;                      // planes present
};

// The planes of a library in arena order, with their row bytes; absent planes are left out.
struct PlaneList {
    char* base[MOVE_PLANES];
    size_t row_bytes[MOVE_PLANES];
    int present[MOVE_PLANES];       // which of the five (vid_norm, adapted, adapted_bf16, vproj, qkv_vid)
    int n;
};
static PlaneList planes_of(const cone_library& B) {
    PlaneList P{};
    const size_t dv = (size_t)B.v_dim, dh = (size_t)B.hidden_dim;
    char* base[MOVE_PLANES] = {(char*)B.vid_norm, (char*)B.adapted, (char*)B.adapted_bf16, (char*)B.vproj, (char*)B.qkv_vid};
    const size_t bytes[MOVE_PLANES] = {dv * 4, dv * 4, dv * 2, dh * 4, dh * 12};
    for (int p = 0; p < MOVE_PLANES; ++p)
        if (base[p]) {
            P.base[P.n] = base[p];
            P.row_bytes[P.n] = bytes[p];
            P.present[P.n] = p;
            ++P.n;
        }
    return P;
}
// The staging buffer of n_rows rows: the present planes packed one behind the other, each MOVE_ALIGN aligned.
static size_t stage_bytes_of(const cone_library& B, int64_t n_rows) {
    const PlaneList P = planes_of(B);
    size_t total = 0;
    for (int p = 0; p < P.n; ++p) total += align_up((size_t)n_rows * P.row_bytes[p], MOVE_ALIGN);
    return total;
}

// SRC_TABLE / DST_TABLE: the side is addressed through the move table (arena rows); otherwise it is packed: flat row r of the
// call lies at row r - row_begin of the plane's staging region.
template <bool SRC_TABLE, bool DST_TABLE>
__global__ __launch_bounds__(MOVE_THREADS) void library_move_kernel(MovePlanes P, int64_t src_cap, int64_t dst_cap,
                                                                    const int64_t* __restrict__ mv_src,
                                                                    const int64_t* __restrict__ mv_dst,
                                                                    const int64_t* __restrict__ mv_off, int64_t n_moves,
                                                                    int64_t row_begin, int64_t row_end) {
    const int64_t tile0 = row_begin + (int64_t)blockIdx.x * MOVE_TILE;
    if (tile0 >= row_end) return;
    const int64_t tile1 = tile0 + MOVE_TILE < row_end ? tile0 + MOVE_TILE : row_end;
    // the last move whose first flat row is <= tile0
    int64_t lo = 0, hi = n_moves - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (mv_off[mid] <= tile0) lo = mid; else hi = mid - 1;
    }
    int64_t at = tile0;
    for (int64_t i = lo; i < n_moves && at < tile1; ++i) {
        const int64_t first = mv_off[i], end = mv_off[i + 1];
        if (end <= at) continue;                                  // (an empty move, or a table that is no prefix sum)
        const int64_t stop = end < tile1 ? end : tile1;
        const int64_t n = (int64_t)((uint64_t)end - (uint64_t)first), s = mv_src[i], d = mv_dst[i];     // (wraps on a hostile table)
        const bool ok = first <= at && n >= 1 && n <= src_cap && n <= dst_cap && s >= 0 && s <= src_cap - n && d >= 0 && d <= dst_cap - n;
        if (ok) {
            const int64_t rows = stop - at;
            const int64_t src_row = SRC_TABLE ? s + (at - first) : at - row_begin;
            const int64_t dst_row = DST_TABLE ? d + (at - first) : at - row_begin;
            for (int p = 0; p < P.n; ++p) {
                const int64_t w = P.row_words[p];
                const uint4* from = (const uint4*)P.src[p] + src_row * w;      // no __restrict__: a direct call inside one arena
                uint4* to = (uint4*)P.dst[p] + dst_row * w;                    // reads and writes the same plane
                const int64_t count = rows * w;
                int64_t k = 0;                                                 // whole rounds: no per-thread guard, so the four
                for (; k + MOVE_THREADS * MOVE_UNROLL <= count; k += MOVE_THREADS * MOVE_UNROLL) {      // loads issue back to back
                    uint4 v[MOVE_UNROLL];
#pragma unroll
                    for (int u = 0; u < MOVE_UNROLL; ++u) v[u] = from[k + u * MOVE_THREADS + threadIdx.x];
#pragma unroll
                    for (int u = 0; u < MOVE_UNROLL; ++u) to[k + u * MOVE_THREADS + threadIdx.x] = v[u];
                }
                if (k + MOVE_THREADS * 2 <= count) {                                                    // a half round
                    const uint4 v0 = from[k + threadIdx.x], v1 = from[k + MOVE_THREADS + threadIdx.x];
                    to[k + threadIdx.x] = v0;
                    to[k + MOVE_THREADS + threadIdx.x] = v1;
                    k += MOVE_THREADS * 2;
                }
                for (k += threadIdx.x; k < count; k += MOVE_THREADS) to[k] = from[k];                   // the rest: short pieces
            }
        }
        at = stop;
    }
}

// The refusals a move makes from host values alone, in this order, before any pointer or the handle is looked at.
static int move_precheck(const char* who, const cone_library* src, const cone_library* dst, int64_t n_moves, int64_t total_rows,
                         int64_t row_begin, int64_t row_end) {
    CONE_REQUIRE(src && dst, "%s: null argument", who);
    CONE_REQUIRE(n_moves >= 1, "%s: n_moves=%lld < 1", who, (long long)n_moves);
    CONE_REQUIRE(total_rows >= n_moves, "%s: total_rows=%lld < n_moves=%lld (a move has at least one row)", who, (long long)total_rows,
                 (long long)n_moves);
    CONE_REQUIRE(row_begin >= 0 && row_begin < row_end && row_end <= total_rows, "%s: rows [%lld, %lld) not in 0 <= begin < end <= total_rows=%lld",
                 who, (long long)row_begin, (long long)row_end, (long long)total_rows);
    CONE_REQUIRE(!((src->flags | dst->flags) & CONE_SESSION_CERTIFIED), "%s: CONE_SESSION_CERTIFIED libraries are not supported", who);
    return 0;
}

template <bool SRC_TABLE, bool DST_TABLE>
static int launch_move(const MovePlanes& P, int64_t src_cap, int64_t dst_cap, const int64_t* mv_src, const int64_t* mv_dst,
                       const int64_t* mv_off, int64_t n_moves, int64_t row_begin, int64_t row_end, hipStream_t s) {
    const int64_t tiles = (row_end - row_begin + MOVE_TILE - 1) / MOVE_TILE;
    hipLaunchKernelGGL((library_move_kernel<SRC_TABLE, DST_TABLE>), dim3((unsigned)tiles), dim3(MOVE_THREADS), 0, s, P, src_cap, dst_cap,
                       mv_src, mv_dst, mv_off, n_moves, row_begin, row_end);
    CONE_LAUNCH_CHECK();
    return 0;
}

}  // namespace cone

extern "C" size_t cone_library_move_stage_bytes(const cone_library* lib, int64_t n_rows) {
    const char* who = "library_move_stage_bytes";
    if (!lib) { cone::set_error("%s: null argument", who); return 0; }
    if (n_rows < 1 || n_rows >= (1ll << 31)) { cone::set_error("%s: n_rows=%lld not in [1, 2^31)", who, (long long)n_rows); return 0; }
    if (lib->flags & CONE_SESSION_CERTIFIED) { cone::set_error("%s: CONE_SESSION_CERTIFIED libraries are not supported", who); return 0; }
    if (!lib->vid_norm || !lib->vproj || !(lib->adapted || lib->adapted_bf16)) {
        cone::set_error("%s: the library handle misses a region (not one cone_library_open filled)", who);
        return 0;
    }
    return cone::stage_bytes_of(*lib, n_rows);
}

extern "C" int cone_library_move_rows(const cone_model* m, const cone_library* src, const cone_library* dst, const int64_t* mv_src,
                                      const int64_t* mv_dst, const int64_t* mv_off, int64_t n_moves, int64_t total_rows,
                                      int64_t row_begin, int64_t row_end, void* stage, size_t stage_bytes, void* stream) {
    using namespace cone;
    const char* who = "library_move";
    if (int rc = move_precheck(who, src, dst, n_moves, total_rows, row_begin, row_end)) return rc;
    CONE_REQUIRE(m && mv_src && mv_dst && mv_off, "%s: null argument", who);
    CONE_REQUIRE(src->capacity >= 1 && src->capacity < (1ll << 31) && dst->capacity >= 1 && dst->capacity < (1ll << 31),
                 "%s: capacity=%lld / %lld not in [1, 2^31)", who, (long long)src->capacity, (long long)dst->capacity);
    CONE_REQUIRE(total_rows <= src->capacity, "%s: total_rows=%lld > capacity=%lld of the source (a row is moved once)", who,
                 (long long)total_rows, (long long)src->capacity);
    CONE_REQUIRE(src->model == dst->model && src->flags == dst->flags && src->v_dim == dst->v_dim && src->hidden_dim == dst->hidden_dim,
                 "%s: src and dst differ in model, flags or row widths (%d / %d, %d / %d, %d / %d)", who, src->flags, dst->flags, src->v_dim,
                 dst->v_dim, src->hidden_dim, dst->hidden_dim);
    CONE_REQUIRE(!src->adapted == !dst->adapted && !src->adapted_bf16 == !dst->adapted_bf16 && !src->qkv_vid == !dst->qkv_vid,
                 "%s: src and dst differ in which planes are present", who);
    CONE_REQUIRE(src->model == m, "%s: the libraries were opened with another handle", who);
    CONE_REQUIRE(src->vid_norm && dst->vid_norm && src->vproj && dst->vproj &&
                     (src->flags & CONE_SESSION_BF16 ? src->adapted_bf16 != nullptr : src->adapted != nullptr),
                 "%s: a library handle misses a region (not one cone_library_open filled)", who);
    CONE_REQUIRE(src->v_dim >= 8 && src->v_dim % 8 == 0 && src->hidden_dim >= 4 && src->hidden_dim % 4 == 0,
                 "%s: row widths %d / %d: every row must be a multiple of 16 bytes", who, src->v_dim, src->hidden_dim);
    const PlaneList S = planes_of(*src), D = planes_of(*dst);
    for (int p = 0; p < S.n; ++p)
        CONE_REQUIRE((((uintptr_t)S.base[p] | (uintptr_t)D.base[p]) & 15) == 0, "%s: a plane of the arena is not 16-B aligned", who);
    const int64_t n_rows = row_end - row_begin;
    if (stage) {
        CONE_REQUIRE(((uintptr_t)stage & (MOVE_ALIGN - 1)) == 0, "%s: the staging buffer must be 256-B aligned", who);
        const size_t need = stage_bytes_of(*src, n_rows);
        if (stage_bytes < need) { set_error("%s: staging buffer too small (%zu < %zu)", who, stage_bytes, need); return CONE_E_WORKSPACE; }
    }
    hipStream_t s = (hipStream_t)stream;
    MovePlanes P{};
    P.n = S.n;
    for (int p = 0; p < S.n; ++p) P.row_words[p] = (int32_t)(S.row_bytes[p] / 16);
    if (!stage) {                                                   // direct: ONE launch, arena rows to arena rows
        for (int p = 0; p < S.n; ++p) { P.src[p] = S.base[p]; P.dst[p] = D.base[p]; }
        return launch_move<true, true>(P, src->capacity, dst->capacity, mv_src, mv_dst, mv_off, n_moves, row_begin, row_end, s);
    }
    char* packed[MOVE_PLANES];                                      // staged: gather, then scatter; stream order is the only sync
    size_t at = 0;
    for (int p = 0; p < S.n; ++p) {
        packed[p] = (char*)stage + at;
        at += align_up((size_t)n_rows * S.row_bytes[p], MOVE_ALIGN);
    }
    for (int p = 0; p < S.n; ++p) { P.src[p] = S.base[p]; P.dst[p] = packed[p]; }
    if (int rc = launch_move<true, false>(P, src->capacity, dst->capacity, mv_src, mv_dst, mv_off, n_moves, row_begin, row_end, s)) return rc;
    for (int p = 0; p < S.n; ++p) { P.src[p] = packed[p]; P.dst[p] = D.base[p]; }
    return launch_move<false, true>(P, src->capacity, dst->capacity, mv_src, mv_dst, mv_off, n_moves, row_begin, row_end, s);
}
