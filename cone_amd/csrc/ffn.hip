// Fused position-wise feed-forward block of the post-norm transformer layers
//     out = LayerNorm(x + W2 relu(W1 x + b1) + b2)          (cone/transformer.py:241-245, 312-316)
// as ONE kernel on the fp32 matrix cores: the (M, ff) hidden activations never leave the CU.
//
// Unfused, the two linear layers are 76 % of the window model's GEMM time and move 4 * ff bytes per token row out
// to HBM and back in between (16 GB per encoder layer at 2 M rows, ff = 1024), through two launches whose
// 128 x 256 output tiles each pay a prologue and a store / LayerNorm epilogue per 16 (linear1) or 64 (linear2)
// k-slabs.  Here a workgroup owns 128 token rows for the whole block and pays them once per 128 slabs' worth of
// MFMAs.
//
// Orientation.  Everything is computed TRANSPOSED so that the hidden tile can be fed back to the matrix core
// straight from its accumulator registers (cdna_hip_programming.md section 3, "An accumulator tile as the next
// MFMA's operand": a following product that sums over the tile's ROW index takes it with no lane movement):
//   a wave owns 16 token rows (the MFMA column index j = lane % 16);
//   GEMM1:  H^T[h][j]  = sum_k  W1[h][k]  x[j][k]    A = W1 rows of a 16-unit hidden chunk (LDS), B = x^T (registers:
//                                                      the wave's 16 x 256 input tile is loaded once, 64 VGPRs);
//           accumulator register r of lane (li, lg) = H^T[h0 + 4 lg + r][token li];
//   GEMM2:  Y^T[n][j] += sum_h  W2[n][h]  H^T[h][j]  A = W2[:, chunk] (LDS), B = the accumulator of GEMM1 after bias +
//                                                      ReLU -- k slot lg of step r <-> hidden unit h0 + 4 lg + r;
//           accumulator (t, r) of lane (li, lg) = Y[token li][channel 16 t + 4 lg + r].
//   The k index of GEMM1 is permuted the same way on both operands (k slot lg of step (q, r) <-> 16 q + 4 lg + r), so
//   a lane's A fragment for four steps is ONE ds_read_b128 and its x fragment is the float4 x[token][16 q + 4 lg ..],
//   which is also exactly the residual that Y's accumulator (t = q, r) needs: the residual add is register-register.
//   Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): results equal the two-GEMM path up to fp32 summation order.
//
// Weight stream.  Per 16-unit hidden chunk the workgroup needs W1[h0 .. h0+15][0..255] (16 KiB) and
// W2[0..255][h0 .. h0+15] (16 KiB).  Both are staged by LDS-DMA (global_load_lds_dwordx4, no VGPRs) as 16 + 16 slabs of
// [16 rows][16 floats] -- the operand-slab format of gemm.hip's row tile: unpadded 64-B rows, 16-B chunk XOR-swizzled
// on the SOURCE address and on the ds_read_b128 address (conflict-free for lane = (row, chunk)) -- into a 4-stage
// ring (128 KiB): chunk c+2 streams in while chunk c is multiplied, one counted s_waitcnt vmcnt + raw s_barrier per
// chunk (128 MFMAs per wave).  b1 is copied to LDS once so that no ordinary global load sits inside the loop (hipcc
// would drain the DMA queue for it, cdna_hip_programming.md section 5 "Three .s-level traps" (b)).
// Where the handle has the layer's packed image (tail_pack.hip: the chunks of a tile in walking order, gather and swizzle
// resolved once) the PK instantiations stream the same bytes from it: scalar base + (chunk, slab) + lane * 16.
//
// One PERSISTENT 8-wave workgroup per CU (132 KiB of LDS, <= 256 VGPRs) walks the 128-row tiles: two waves per SIMD
// keep the matrix pipe fed; GEMM1 of chunk i and GEMM2 of chunk i-1 share the units of one iteration (software
// pipelining across chunks), so bias + ReLU never stall a chunk; the epilogue is bias + residual + LayerNorm in
// registers (a token's 256 channels sit in 4 lanes x 64 registers, two shuffle steps per moment).
//
// What this kernel must do exactly as the wide and spread kernels of ffn_wide.hip do (the same bits for a row in every form)
// is in tail_f32_common.h: the slab primitives, the register LayerNorm and its apply, the gathered residual row, the clamped
// load row, the row count, the kernel-argument layout, the host fill and the argument checks.  This file keeps the ring, the
// MFMA schedule (FFN_CHUNK32: the projection's and the q | k | v ride's chunk), the row-kernel launchers and the form ladder.
#include <mutex>

#include "tail_f32_common.h"

namespace cone {

constexpr int FFN_STAGE = 2 * 16 * 256;           // floats per ring stage: W1 image (16 slabs) + W2 image (16 slabs)
constexpr int FFN_NST = 4;                        // ring depth: a stage is refilled two barriers after its last read
// 1-KiB LDS-DMA pieces per wave per chunk: 32 pieces / NW waves (NW = 8: 4, NW = 4: 8)

// NW = waves per workgroup = 16-row groups per tile.  NW = 8 (128-row tiles, two waves per SIMD) is the throughput form.
// NW = 4 (64-row tiles, ONE wave per SIMD) is the small-M form: a wave runs the very same instruction sequence on its 16
// rows (bit-identical results), but has its SIMD's matrix pipe to itself -- a tile takes half the time -- and the tile
// grid is twice as fine; chosen by the launcher when the 128-row tiles would leave at least half of the CUs idle.
// PK: the weight pieces stream from the packed image p.Wimg (tail_pack.hip) instead of being gathered from the row-major
// matrices: the same bytes at the same LDS addresses, so nothing else in the kernel knows of it.
template <bool PROJ, bool QKV, int NW, bool PRE = false, bool PK = false>
__global__ __launch_bounds__(64 * NW, NW / 4) void ffn_fused_kernel(FfnArgs p) {
    static_assert(!PRE || (PROJ && !QKV), "the pre-norm form is the layer tail");
    constexpr int FFN_ROWS = 16 * NW, FFN_NPIECE = 32 / NW, NT = 64 * NW, HW = NW / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* b1s = smem + FFN_NST * FFN_STAGE;
    TF_LAUNCH_ROWS(M, p, 0)
    // Work items of the persistent loop: full tiles of FFN_ROWS rows, walked round-robin over the grid -- except that the
    // tiles of the LAST round, when they would occupy at most half of the workgroups, are cut into half tiles of 64 rows
    // (waves 0-3; waves 4-7 idle through the item): twice as many CUs finish the ragged end of a launch in 0.18 ms instead of
    // 0.30 (one wave per SIMD has the matrix pipe to itself).  The per-wave instruction sequence on a row group does not
    // change: results are bit-identical.  `act` (wave-uniform) = this wave holds rows of the item; an idle wave takes a
    // short side path (its share of the weight stream + every barrier, no MFMA) instead of the tile body.
    const int n_tiles = (M + FFN_ROWS - 1) / FFN_ROWS;
    if (n_tiles == 0) return;
    const int G_ = (int)gridDim.x;
    const int full_items = ((n_tiles - 1) / G_) * G_;                          // tiles of the complete rounds
    const int rem_rows = M - full_items * FFN_ROWS;                             // rows of the last round (> 0)
    const int rem_half = (rem_rows + 63) >> 6;
    const bool half_mode = NW == 8 && rem_half <= G_ && 2 * ((rem_rows + FFN_ROWS - 1) / FFN_ROWS) <= G_;
    const int n_items = full_items + (half_mode ? rem_half : (rem_rows + FFN_ROWS - 1) / FFN_ROWS);
    if ((int)blockIdx.x >= n_items) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // first row of this wave's 16-row group in work item `it` (M or more: the wave idles)
    auto wave_row0 = [&](int it) -> int {
        if (it < full_items || !half_mode) return it * FFN_ROWS + wave * 16;
        return wave < 4 ? full_items * FFN_ROWS + (it - full_items) * 64 + wave * 16 : M;
    };
    const int li = lane & 15, lg = lane >> 4;
    const int ff = p.ff, nc = ff >> 4;
    constexpr int NP = PROJ ? 8 : 0;              // leading chunks of the output projection (32 channels each)
    const int NQ = QKV ? p.n_qkv >> 5 : 0;        // trailing chunks of the next layer's q | k | v projection (32 channels each)
    const int G = NP + nc + NQ;                   // weight chunks per tile; the ring runs on across tiles

    // every per-channel parameter vector goes to LDS once per workgroup: b1 (ff), then 6 x 256: b2, ln_g, ln_b and
    // (PROJ) bo, pg, pb -- no ordinary global load remains inside the tile loop besides the tile's own rows
    float* prm = b1s + ff;
    for (int i = tid; i < (ff >> 2); i += NT)
        reinterpret_cast<f32x4*>(b1s)[i] = reinterpret_cast<const f32x4*>(p.b1)[i];
    if (tid < 64) {
        reinterpret_cast<f32x4*>(prm)[tid] = reinterpret_cast<const f32x4*>(p.b2)[tid];
        reinterpret_cast<f32x4*>(prm + 256)[tid] = reinterpret_cast<const f32x4*>(p.ln_g)[tid];
        reinterpret_cast<f32x4*>(prm + 512)[tid] = reinterpret_cast<const f32x4*>(p.ln_b)[tid];
        if (PROJ) {
            reinterpret_cast<f32x4*>(prm + 768)[tid] = reinterpret_cast<const f32x4*>(p.bo)[tid];
            reinterpret_cast<f32x4*>(prm + 1024)[tid] = reinterpret_cast<const f32x4*>(p.pg)[tid];
            reinterpret_cast<f32x4*>(prm + 1280)[tid] = reinterpret_cast<const f32x4*>(p.pb)[tid];
        }
    }
    float* qbs = prm + 1536;
    if (QKV)
        for (int i = tid; i < (p.n_qkv >> 2); i += NT)
            reinterpret_cast<f32x4*>(qbs)[i] = reinterpret_cast<const f32x4*>(p.qb)[i];

    // ---- LDS-DMA pieces.  A feed-forward chunk = 32 slabs of [16 rows][16 floats]; wave w issues slabs 4w .. 4w+3
    // (0-15 = W1, 16-31 = W2); lane -> (row = lane / 4, physical chunk = lane % 4), the source chunk is XOR-swizzled.
    // A projection chunk = 32 slabs too: Wo rows [32 g, 32 g + 16) in the first half of the stage, rows [32 g + 16,
    // 32 g + 32) in the second half, both in the W1 slab format -- every chunk of the kernel costs the same 4 pieces
    // per wave and one counted s_waitcnt serves all of it.
    // Addressing: all four pieces of a wave lie on one side (waves 0-3: W1 slabs 4w .. 4w+3, waves 4-7: W2 slabs), so a
    // piece's source is a wave-uniform base (SGPRs) + ONE per-lane offset + scalar multiples of the piece / chunk index.
    const int drow = lane >> 2;
    const int dch = (lane & 3) ^ tf_swz16(drow);
    const bool w2side = wave >= HW;
    const float* fbase = w2side ? p.W2 : p.W1;                         // wave-uniform
    const int foff = w2side ? (16 * FFN_NPIECE * (wave - HW) + drow) * ff + 4 * dch   // W2[16 t + row][h0 + 4 ch ..], t = NPIECE (w - HW) + i
                            : drow * 256 + 16 * FFN_NPIECE * wave + 4 * dch;         // W1[h0 + row][16 q + 4 ch ..],  q = NPIECE w + i
    const int fpiece = w2side ? 16 * ff : 16;                          // + i * fpiece
    const int fchunk = w2side ? 16 : 16 * 256;                         // + c * fchunk
    // projection chunk g: Wo[32 g + 16 (pid / 16) + row][16 (pid % 16) + 4 ch ..], pid = 4 w + i
    const int poff = PROJ ? (16 * (wave / HW) + drow) * 256 + 16 * FFN_NPIECE * (wave % HW) + 4 * dch : 0;
    // piece i of chunk g of the current tile (projection chunks first, then the feed-forward chunks); g >= G = the
    // first chunks of the NEXT tile this workgroup will run -- the same weights, so the ring simply runs on (after
    // the last tile they land in stages nobody reads again).  sb = (chunks consumed before this tile) % FFN_NST.
    int sb = 0;
    unsigned pkvo = (unsigned)(lane * 16);        // PK: the lane's offset inside every piece
    unsigned poff4 = (unsigned)(poff * 4), foff4 = (unsigned)(foff * 4);      // row-major: the lane's byte offsets
    auto stream_piece = [&](int g, int i) {
        float* dstp = smem + ((sb + g) % FFN_NST) * FFN_STAGE + (wave * FFN_NPIECE + i) * 256;
        const int gg = g < G ? g : g - G;
        if (PK) {
            // the image holds a tile's chunks in walking order, every lane's 16 B in place: scalar base + one 32-bit offset of
            // (chunk, slab), and lane * 16 -- no select, no swizzle, no per-side stride (the pin: as below)
            const char* ub = reinterpret_cast<const char*>(p.Wimg) + (((unsigned)gg << 15) + (unsigned)(wave * FFN_NPIECE + i) * 1024u);
            asm volatile("" : "+s"(ub));
            // the lane offset is pinned HERE too: hoisted, its zero-extension lands in another block than the load, and the
            // load then takes a 64-bit VGPR address (one v_lshl_add_u64 per piece in the MFMA stream) instead of saddr + voffset
            // (in place, on ONE variable that lives across the kernel: a pinned copy would cost a v_mov per piece)
            asm volatile("" : "+v"(pkvo));
            TF_GLDS16(ub + pkvo, dstp);
            return;
        }
        // wave-uniform pointer + zero-extended 32-bit lane offset: the saddr + voffset form of global_load_lds -- which the
        // load takes only with BOTH pins below (the base's and the lane offsets')
        // ONE scalar base (selected, not branched on) + ONE 32-bit lane offset; the empty asm pins the base in SGPRs at
        // this point: hoisted out of the tile loop, base + lane offset becomes a 64-bit VGPR pair per piece, spilled,
        // and every reload drains the DMA queue with a vmcnt(0)
        const bool qk = QKV && gg >= NP + nc;         // a q | k | v chunk: 32 rows of Wq in the projection's slab format
        const bool pj = (PROJ && gg < NP) || qk;
        const char* ub = reinterpret_cast<const char*>(
            qk ? p.Wq + ((size_t)(gg - NP - nc) * (32 * 256) + 16 * i)
               : (pj ? p.Wo + ((size_t)gg * (32 * 256) + 16 * i) : fbase + ((size_t)(gg - NP) * fchunk + (size_t)i * fpiece)));
        asm volatile("" : "+s"(ub));
        // the lane offsets are pinned next to the load as well (in place, on the two variables that live across the kernel):
        // hoisted, the zero-extension of the offset lands in another block than the load, and the load then takes a 64-bit
        // VGPR address -- one v_lshl_add_u64 per piece in the MFMA stream -- instead of saddr + voffset
        asm volatile("" : "+v"(poff4), "+v"(foff4));
        const unsigned vo = pj ? poff4 : foff4;
        TF_GLDS16(ub + vo, dstp);
    };

    const int rd = li * 16 + ((lg ^ tf_swz16(li)) << 2);          // this lane's 16-B chunk inside a slab
#define FFN_RD(stg, off) (*reinterpret_cast<const f32x4*>((stg) + (off) + rd))
#define FFN_STAGE_OF(g) (smem + ((sb + (g)) % FFN_NST) * FFN_STAGE)
#define FFN_SB() __builtin_amdgcn_sched_barrier(0)
    // unit u of a chunk (8 units) issues the wave's share of the next-but-one chunk: every other unit at 4 pieces per wave,
    // every unit at 8
#define FFN_STREAM(g, u) { if (FFN_NPIECE == 8) stream_piece(g, u); else if ((u) & 1) stream_piece(g, (u) >> 1); }
    // a counted wait + barrier ends every chunk: the next chunk has landed (all but the 4 pieces issued last, which
    // belong to the chunk after it), and every wave is done reading the stage that the next pieces will overwrite
#define FFN_END_CHUNK()                                                           \
    {                                                                             \
        FFN_SB();                                                                 \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FFN_NPIECE) : "memory");         \
        __builtin_amdgcn_s_barrier();                                             \
        FFN_SB();                                                                 \
    }
    // MFMA issue order is pinned (a sched_barrier after every MFMA): hipcc otherwise regroups the MFMAs of a unit by
    // accumulator, and back-to-back MFMAs on one accumulator wait out the 40-cycle dependent latency of the 32-cycle
    // v_mfma_f32_16x16x4_f32 (measured: 139 -> 131 TFLOP/s).  In every sequence below an accumulator is reused at the
    // earliest two MFMAs (64 cycles) later.
#define FFN_MFMA(acc, a, b) { acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); FFN_SB(); }
    // 8 MFMAs of a weight-slab pair against a register tile: four independent partial chains acc[0..3]
#define FFN_MM_A(acc, w0, w1, B, q)                                                   \
    {                                                                                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) FFN_MFMA(acc[r], w0[r], B[q][r])         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) FFN_MFMA(acc[r], w1[r], B[(q) + 1][r])   \
    }
    // 8 MFMAs of GEMM2: two output tiles, alternating accumulators
#define FFN_MM_Y(w0, w1, hh, t)                                                       \
    {                                                                                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                               \
            FFN_MFMA(y[t], w0[r], hh[r])                                              \
            FFN_MFMA(y[(t) + 1], w1[r], hh[r])                                        \
        }                                                                             \
    }
    // 16 MFMAs: GEMM1 slab pair and GEMM2 tile pair interleaved (accumulator reuse distance 4)
#define FFN_MM_AY(acc, w0, w1, B, q, v0, v1, hh, t)                                   \
    {                                                                                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                               \
            FFN_MFMA(acc[r], w0[r], B[q][r])                                          \
            FFN_MFMA(y[(t) + (r & 1)], ((r & 1) ? v1 : v0)[r >> 1], hh[r >> 1])       \
        }                                                                             \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                               \
            FFN_MFMA(acc[r], w1[r], B[(q) + 1][r])                                    \
            FFN_MFMA(y[(t) + (r & 1)], ((r & 1) ? v1 : v0)[2 + (r >> 1)], hh[2 + (r >> 1)]) \
        }                                                                             \
    }

    // One chunk of 32 output channels in the projection's slab format (pair g of the output projection, a chunk of the q | k | v
    // ride) against the register tile B: declares st and ha / hb = two partial chains for each of the chunk's two 16-channel
    // tiles -- with both tiles interleaved, four MFMAs apart; fully unrolled: B[] is indexed statically
#define FFN_CHUNK32(gi, B)                                                                                                 \
    const float* st = FFN_STAGE_OF(gi);                                                                                    \
    f32x4 ha[2], hb[2];                                                                                                    \
    ha[0] = f32x4{0.f, 0.f, 0.f, 0.f}; hb[0] = ha[0];                                                                      \
    ha[1] = ha[0]; hb[1] = ha[0];                                                                                          \
    wa = FFN_RD(st, 0); wb = FFN_RD(st, 256); va = FFN_RD(st, 4096); vb = FFN_RD(st, 4096 + 256);                          \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                                        \
        FFN_SB();                                                                                                          \
        asm volatile("" : "+v"(wa), "+v"(wb), "+v"(va), "+v"(vb));                                                         \
        FFN_SB();                                                                                                          \
        if (u < 7) {                                                                                                       \
            na = FFN_RD(st, (2 * u + 2) * 256); nb = FFN_RD(st, (2 * u + 3) * 256);                                        \
            nva = FFN_RD(st, 4096 + (2 * u + 2) * 256); nvb = FFN_RD(st, 4096 + (2 * u + 3) * 256);                        \
        }                                                                                                                  \
        FFN_SB();                                                                                                          \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                    \
            FFN_MFMA(ha[r & 1], wa[r], B[2 * u][r])                                                                        \
            FFN_MFMA(hb[r & 1], va[r], B[2 * u][r])                                                                        \
        }                                                                                                                  \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                    \
            FFN_MFMA(ha[r & 1], wb[r], B[2 * u + 1][r])                                                                    \
            FFN_MFMA(hb[r & 1], vb[r], B[2 * u + 1][r])                                                                    \
        }                                                                                                                  \
        FFN_STREAM((gi) + 2, u)                 /* the next-but-one chunk's pieces ride behind MFMAs */                    \
        if (u < 7) { wa = na; wb = nb; va = nva; vb = nvb; }                                                               \
    }

#pragma unroll
    for (int i = 0; i < FFN_NPIECE; ++i) stream_piece(0, i);
#pragma unroll
    for (int i = 0; i < FFN_NPIECE; ++i) stream_piece(1 < G ? 1 : 0, i);

    // Schedule.  Every chunk is walked as 8 units of 16 MFMAs (two slabs of each half of the stage).  The ds_read_b128
    // of unit u+1 are issued right ahead of the MFMAs of unit u and consumed (the empty asm at the top of unit u+1 is
    // where hipcc puts its lgkmcnt wait -- BEFORE the next reads are issued, so it never covers a read that was only
    // just issued) after them: LDS latency hides under 512 matrix-pipe cycles.  Loop bodies are straight-line code: the
    // ring is refilled unconditionally (the last iterations re-stream the final chunk into stages nobody reads again).
    f32x4 wa, wb, na, nb;      // W1-format fragments (current / next unit)
    f32x4 va, vb, nva, nvb;    // second-half fragments

    // Persistent workgroup: one per CU, walking tiles blockIdx.x, + gridDim.x, ...  A tile's fixed costs -- its
    // input rows (16 KiB per wave, 64-B row segments per load), the output stores, the dispatch of a fresh workgroup --
    // are not covered by another workgroup at this occupancy (measured 18 us per 128-row tile against 3.7 us per
    // chunk = 7 % at ff = 1024); here the next tile's rows are requested while the previous tile's stores drain and
    // the weight ring never restarts.
    // register tiles: v[q][r] = row[token li][16 q + 4 lg + r], q = 0 .. 15.  xr = block input: B operand of GEMM1 and
    // the residual of the block (PROJ: starts as the residual of the projection, becomes the block input); ar (PROJ) =
    // attention rows, B operand of the projection.  The NEXT tile's rows are requested from the epilogue, ahead of
    // this tile's stores (vmcnt retires in order: loads queued behind stores would wait for the stores' acks).
    f32x4 xr[16];
    f32x4 ar[PROJ ? 16 : 1];
    auto load_tile = [&](int tile) {
        const int row = wave_row0(tile) + li;
        const size_t ld_row = TF_LD_ROW(row, M);
        if (PROJ) {     // the attention rows; the residual rows follow at the top of the tile (load_res)
            const float* ap = p.A + ld_row * p.lda + 4 * lg;
#pragma unroll
            for (int q = 0; q < 16; ++q) ar[q] = *reinterpret_cast<const f32x4*>(ap + 16 * q);
        } else {
            const float* xp = p.X + ld_row * p.ldx + 4 * lg;
#pragma unroll
            for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const f32x4*>(xp + 16 * q);
        }
    };
    // PROJ: the residual rows of a tile are requested at its top and consumed at the end of each projection chunk (they
    // land under the first chunk's MFMAs): at no point are the next tile's rows, this tile's outputs and both input
    // tiles live together
    auto load_res = [&](int tile) {
        const int row = wave_row0(tile) + li;
        const size_t ld_row = TF_LD_ROW(row, M);
        TF_RES_ROW(rp, p, ld_row, 4 * lg)
#pragma unroll
        for (int q = 0; q < 16; ++q) xr[q] = *reinterpret_cast<const f32x4*>(rp + 16 * q);
    };
    load_tile(blockIdx.x);
    bool first = true;
    for (int tile = blockIdx.x; tile < n_items; tile += gridDim.x) {
    const int my_row0 = wave_row0(tile);
    const int my_row = my_row0 + li;
    const bool act = my_row0 < M;                   // wave-uniform
    if (first) {        // chunk 0 and the b1 image are in LDS (later tiles: the previous tile's last barrier covers chunk 0)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FFN_NPIECE) : "memory");
        __syncthreads();
        first = false;
    }
    if (!act) {
        // this wave holds no row of the item (the upper waves of a half tile, the waves past a launch's last row): it keeps
        // its part of the protocol -- per chunk its pieces of the next-but-one chunk, the counted wait, the barrier: G of
        // each per item, exactly what a computing wave does -- and issues no MFMA, so that the waves that do compute have
        // the matrix pipes to themselves.  Only the last item of a workgroup can be short.
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int i = 0; i < FFN_NPIECE; ++i) stream_piece(g + 2, i);
            FFN_END_CHUNK()
        }
        break;
    }

    f32x4 y[16];
    if (PROJ) {
        load_res(tile);
        // ---- attention output projection + residual + LayerNorm: pair g computes channels [32 g, 32 g + 32) of
        // A Wo^T and adds them to xr[2 g], xr[2 g + 1] (the residual rows); fully unrolled: xr[] is indexed statically
#pragma unroll
        for (int g = 0; g < NP; ++g) {
            FFN_CHUNK32(g, ar)
            xr[2 * g] += ha[0] + ha[1];
            xr[2 * g + 1] += hb[0] + hb[1];
            FFN_END_CHUNK()
        }
        FFN_SB();
#pragma unroll
        for (int t = 0; t < 16; ++t) xr[t] += *reinterpret_cast<const f32x4*>(prm + 768 + 16 * t + 4 * lg);       // + bo
        if (PRE) {      // the un-normalised stream x1 is the block's residual: the output accumulators START from x1 + b2
                        // (no second copy of the tile in registers), then xr becomes the normalised block input
#pragma unroll
            for (int t = 0; t < 16; ++t) y[t] = xr[t] + *reinterpret_cast<const f32x4*>(prm + 16 * t + 4 * lg);
        }
        float rstd;
        tf_layernorm_regs(xr, rstd);
        TF_LN_APPLY(xr, rstd, prm + 1024, prm + 1280)
        FFN_SB();
    }

    // ---- feed-forward block, software-pipelined across chunks: iteration i multiplies GEMM1 of chunk i (W1 half of
    // stage i) and GEMM2 of chunk i-1 (W2 half of stage i-1, hidden tile h of the previous iteration) in the same
    // units, so the GEMM1 -> bias/ReLU -> GEMM2 dependency spans a whole iteration instead of stalling every chunk.
    if (!PRE) {
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 h, hp[4];
    {   // iteration 0: GEMM1 of chunk 0 alone
        const float* st = FFN_STAGE_OF(NP);
#pragma unroll
        for (int r = 0; r < 4; ++r) hp[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        wa = FFN_RD(st, 0); wb = FFN_RD(st, 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            FFN_SB();
            asm volatile("" : "+v"(wa), "+v"(wb));
            FFN_SB();
            if (u < 7) { na = FFN_RD(st, (2 * u + 2) * 256); nb = FFN_RD(st, (2 * u + 3) * 256); }
            else { va = FFN_RD(st, 4096); vb = FFN_RD(st, 4096 + 256); }       // unit 0 of GEMM2(0), next iteration
            FFN_SB();
            FFN_MM_A(hp, wa, wb, xr, 2 * u)
            FFN_STREAM(NP + 2, u)
            if (u < 7) { wa = na; wb = nb; }
        }
        FFN_SB();
        h = (hp[0] + hp[1]) + (hp[2] + hp[3]) + *reinterpret_cast<const f32x4*>(b1s + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = fmaxf(h[r], 0.f);
        FFN_END_CHUNK()
    }
    for (int i = 1; i < nc; ++i) {
        const float* s1 = FFN_STAGE_OF(NP + i);             // W1 half: chunk i
        const float* s2 = FFN_STAGE_OF(NP + i - 1);         // W2 half: chunk i - 1
#pragma unroll
        for (int r = 0; r < 4; ++r) hp[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        wa = FFN_RD(s1, 0); wb = FFN_RD(s1, 256);           // only now visible (the barrier above); GEMM2's first
#pragma unroll                                              // fragments were requested before it
        for (int u = 0; u < 8; ++u) {
            FFN_SB();
            if (u == 0) {
                // the first unit runs GEMM2 ahead of GEMM1: its fragments are already here, GEMM1's are in flight
                asm volatile("" : "+v"(va), "+v"(vb));
                FFN_SB();
                nva = FFN_RD(s2, 4096 + 2 * 256); nvb = FFN_RD(s2, 4096 + 3 * 256);
                FFN_SB();
                FFN_MM_Y(va, vb, h, 0)
                FFN_SB();
                asm volatile("" : "+v"(wa), "+v"(wb));
                FFN_SB();
                na = FFN_RD(s1, 2 * 256); nb = FFN_RD(s1, 3 * 256);
                FFN_SB();
                FFN_MM_A(hp, wa, wb, xr, 0)
            } else {
                asm volatile("" : "+v"(wa), "+v"(wb), "+v"(va), "+v"(vb));
                FFN_SB();
                if (u < 7) {
                    na = FFN_RD(s1, (2 * u + 2) * 256); nb = FFN_RD(s1, (2 * u + 3) * 256);
                    nva = FFN_RD(s2, 4096 + (2 * u + 2) * 256); nvb = FFN_RD(s2, 4096 + (2 * u + 3) * 256);
                } else {    // GEMM2's first fragments of the next iteration: W2 half of THIS chunk's stage
                    nva = FFN_RD(s1, 4096); nvb = FFN_RD(s1, 4096 + 256);
                }
                FFN_SB();
                FFN_MM_AY(hp, wa, wb, xr, 2 * u, va, vb, h, 2 * u)
            }
            FFN_STREAM(NP + i + 2, u)
            if (u < 7) { wa = na; wb = nb; }
            va = nva; vb = nvb;
        }
        FFN_SB();
        // hidden tile of chunk i for the next iteration (the last GEMM1 MFMAs finished under the last GEMM2 ones)
        h = (hp[0] + hp[1]) + (hp[2] + hp[3]) + *reinterpret_cast<const f32x4*>(b1s + 16 * i + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = fmaxf(h[r], 0.f);
        FFN_END_CHUNK()
    }
    {   // last iteration: GEMM2 of chunk nc - 1 alone
        const float* st = FFN_STAGE_OF(NP + nc - 1);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            FFN_SB();
            asm volatile("" : "+v"(va), "+v"(vb));
            FFN_SB();
            if (u < 7) { nva = FFN_RD(st, 4096 + (2 * u + 2) * 256); nvb = FFN_RD(st, 4096 + (2 * u + 3) * 256); }
            FFN_SB();
            FFN_MM_Y(va, vb, h, 2 * u)
            if (u < 7) { va = nva; vb = nvb; }
        }
    }
    // ---- epilogue: + b2 + residual, LayerNorm over the token's 256 channels (4 lanes x 64 registers), store
    FFN_SB();
    if (!PRE) {
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = y[t] + *reinterpret_cast<const f32x4*>(prm + 16 * t + 4 * lg) + xr[t];
    }
    FFN_SB();
    // in flight under the LayerNorm + stores (unconditional -- after the last tile a valid tile is simply re-read --
    // so that the register tiles have ONE definition per iteration)
    load_tile(tile + (int)gridDim.x < n_items ? tile + (int)gridDim.x : tile);
    FFN_SB();
    if (PRE && my_row < M) {        // the un-normalised stream
        float* op = p.OUT + (size_t)my_row * p.ldo + 4 * lg;
#pragma unroll
        for (int t = 0; t < 16; ++t) *reinterpret_cast<f32x4*>(op + 16 * t) = y[t];
    }
    float rstd;
    if (!PRE || p.OUT2) tf_layernorm_regs(y, rstd);
    if (PRE) {
        if (p.OUT2 && my_row < M) {
            float* op = p.OUT2 + (size_t)my_row * p.ldo2 + 4 * lg;
            TF_LN_STORE(op, y, rstd, prm + 256, prm + 512, true, false)
        }
    } else if (my_row < M) {
        float* op = p.OUT + (size_t)my_row * p.ldo + 4 * lg;
        TF_LN_STORE(op, y, rstd, prm + 256, prm + 512, true, QKV)
    } else if (QKV) {       // rows past M feed unstored outputs: any finite values
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (QKV) {
        // ---- the next layer's q | k | v projection of the tile's output rows (still in registers, in the B-operand
        // layout): NQ chunks of 32 output channels in the projection phase's format, stored from the accumulators
        float* qrow = p.QKV + (size_t)my_row * p.ldq + 4 * lg;
        for (int g = 0; g < NQ; ++g) {
            FFN_CHUNK32(NP + nc + g, y)
            FFN_SB();
            if (my_row < M) {
                *reinterpret_cast<f32x4*>(qrow + 32 * g) = (ha[0] + ha[1]) + *reinterpret_cast<const f32x4*>(qbs + 32 * g + 4 * lg);
                *reinterpret_cast<f32x4*>(qrow + 32 * g + 16) = (hb[0] + hb[1]) + *reinterpret_cast<const f32x4*>(qbs + 32 * g + 16 + 4 * lg);
            }
            FFN_END_CHUNK()
        }
    }
    sb = (sb + G) % FFN_NST;
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // no LDS-DMA may outlive the workgroup's LDS
}

#undef FFN_CHUNK32
#undef FFN_MM_A
#undef FFN_MM_Y
#undef FFN_MM_AY
#undef FFN_MFMA
#undef FFN_END_CHUNK
#undef FFN_SB
#undef FFN_STREAM
#undef FFN_STAGE_OF
#undef FFN_RD

bool ffn_fused_supported(int ff) { return ff >= 32 && ff % 16 == 0 && ff <= 4096; }

bool ffn_fused_qkv_fits(int ff, int n_qkv) {
    return ffn_fused_supported(ff) && n_qkv >= 32 && n_qkv % 32 == 0 &&
           (size_t)(FFN_NST * FFN_STAGE + ff + 6 * 256 + n_qkv) * sizeof(float) <= 160 * 1024;
}

// The CU count: it sizes the persistent grids and picks the form.
static int ffn_cu_count(int* n_cu) {
    static DeviceOnce once;
    CONE_CHECK_HIP(device_once(once, [] { return hipSuccess; }, n_cu));
    return 0;
}

// n_cu: the CU count that sizes the grid (0: the device's)
template <bool PROJ, bool QKV, int NW, bool PRE = false, bool PK = false>
static int launch_ffn_nw(const TailF32Args& a, int n_cu, hipStream_t s) {
    const size_t lds = (size_t)(FFN_NST * FFN_STAGE + a.ff + 6 * 256 + (QKV ? a.n_qkv : 0)) * sizeof(float);
    CONE_REQUIRE(lds <= 160 * 1024, "fused layer tail: %zu bytes of LDS (ff %d, q|k|v %d) exceed 160 KiB", lds, a.ff, a.n_qkv);
    // once per device: the opt-in to > 64 KiB of LDS (a property of the code object) and the CU count that sizes
    // the persistent grid (one workgroup per CU: 132 KiB of LDS, 64 NW threads at <= 256 VGPRs)
    static DeviceOnce once;
    int dev_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        return hipFuncSetAttribute((const void*)ffn_fused_kernel<PROJ, QKV, NW, PRE, PK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024);
    }, &dev_cu));
    if (!n_cu) n_cu = dev_cu;
    const int tiles = (a.M + 16 * NW - 1) / (16 * NW);
    const int grid = tiles < n_cu ? tiles : n_cu;
    // FLOPs of a record: 4 * M * ff * 256 for the block, + 2 * M * 256 * 256 with the projection
    // (+ 2 * M * n_qkv * 256 with the fused q | k | v projection: booked as n_qkv / 2 extra hidden units)
    ProfScope ps(NW == 8 ? (PROJ ? PK_FFN_PROJ : PK_FFN_FUSED) : (PROJ ? PK_FFN_PROJ_NW4 : PK_FFN_FUSED_NW4), a.M,
                 a.ff + (QKV ? a.n_qkv / 2 : 0), 256, a.M_dev, s);
    FfnArgs k;
    static_cast<TailF32Args&>(k) = a;
    hipLaunchKernelGGL((ffn_fused_kernel<PROJ, QKV, NW, PRE, PK>), dim3((unsigned)grid), dim3(64 * NW), lds, s, k);
    CONE_LAUNCH_CHECK();
    if (PK) f32_packed_note(0);
    return 0;
}

// The row kernel on filled arguments: nw = 8 (128-row tiles) or 4 (64-row tiles); the ride (a.Wq) and the pre-norm form exist
// on 8 waves only.
template <bool PK>
static int launch_ffn_rows_pk(const TailF32Args& a, bool proj, bool pre, int nw, int n_cu, hipStream_t s) {
    if (pre) return launch_ffn_nw<true, false, 8, true, PK>(a, n_cu, s);
    if (a.Wq) return launch_ffn_nw<true, true, 8, false, PK>(a, n_cu, s);
    if (nw == 4) return proj ? launch_ffn_nw<true, false, 4, false, PK>(a, n_cu, s) : launch_ffn_nw<false, false, 4, false, PK>(a, n_cu, s);
    return proj ? launch_ffn_nw<true, false, 8, false, PK>(a, n_cu, s) : launch_ffn_nw<false, false, 8, false, PK>(a, n_cu, s);
}
// a.Wimg (the packed stream, from its Wo chunks when it has them) picks the stream form; the block alone starts behind them
static int launch_ffn_rows(const TailF32Args& a, bool proj, bool pre, int nw, int n_cu, hipStream_t s) {
    return a.Wimg ? launch_ffn_rows_pk<true>(a, proj, pre, nw, n_cu, s) : launch_ffn_rows_pk<false>(a, proj, pre, nw, n_cu, s);
}

// Rows past the last FULL round of the persistent grid (n_cu tiles of 128 rows) cost the row forms a partial round -- half
// a round or more (0.15 - 0.29 ms) whatever their number; up to FFN_SPLIT_GROUPS groups of them are handed to the wide form
// instead (52 / 124 us for <= 4 096 / 8 192 rows; same bits).  Returns the row count of the full rounds, or M (no split).
#ifndef CONE_FFN_SPLIT_GROUPS
#define CONE_FFN_SPLIT_GROUPS 512
#endif
static int ffn_full_round_rows(int M, int n_cu, int ff) {
    const int tiles = (M + 127) / 128;
    if (tiles <= n_cu || !ffn_wide_supported(ff)) return M;
    const int64_t full = (int64_t)(tiles / n_cu) * n_cu * 128;
    const int64_t rem = M - full;
    return rem > 0 && (rem + 15) / 16 <= CONE_FFN_SPLIT_GROUPS ? (int)full : M;
}

// The form ladder of the post-norm launches (proj: the projecting tail, else the block on a.X), by the HOST-known row bound
// a.M, never by the device-side count; the rows' results do not depend on the choice (the same fma chains in every form):
//   at most wide_groups groups of 16 rows, an ff the wide form takes, no ride   the wide form (ffn_wide.hip)
//   otherwise the row kernel on the full rounds of n_cu 128-row tiles and the wide form on the rows past them
//   (ffn_full_round_rows), or the row kernel on all rows: 64-row tiles (one wave per SIMD) when the 128-row tiles would
//   occupy at most half of the CUs -- every 64-row tile then has a CU to itself and finishes in half the time.
// n_cu = 0: the device's CU count.
static int launch_ffn_ladder(TailF32Args a, bool proj, int n_cu, int wide_groups, hipStream_t s) {
    const int M = a.M;
    const bool ride = a.Wq != nullptr;
    if (!ride && (M + 15) / 16 <= wide_groups && ffn_wide_supported(a.ff)) return launch_tail_f32_wide(a, proj, false, s);
    if (!n_cu)
        if (int rc = ffn_cu_count(&n_cu)) return rc;
    const int m1 = ride ? M : ffn_full_round_rows(M, n_cu, a.ff);
    a.M = m1;
    if (int rc = launch_ffn_rows(a, proj, false, !ride && 2 * ((m1 + 127) / 128) <= n_cu ? 4 : 8, n_cu, s)) return rc;
    if (m1 == M) return 0;
    // the rows past the last full round: the wide form on offset pointers
    a.M = M - m1; a.m_off = m1; a.OUT += (size_t)m1 * a.ldo;
    if (!proj) a.X += (size_t)m1 * a.ldx;
    else {
        a.A += (size_t)m1 * a.lda;
        if (a.r_idx) a.r_idx += m1; else a.R += (size_t)m1 * a.ldr;
    }
    return launch_tail_f32_wide(a, proj, false, s);
}

int launch_ffn_fused(const float* X, int ldx, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* ln_g, const float* ln_b, float* OUT, int ldo, int M, const int* M_dev, int ff,
                     hipStream_t s) {
    CONE_REQUIRE(ffn_fused_supported(ff), "fused FFN: dim_feedforward=%d unsupported", ff);
    CONE_REQUIRE(X && W1 && b1 && W2 && b2 && ln_g && ln_b && OUT, "fused FFN: null argument");
    CONE_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0, "fused FFN: row strides must be multiples of 4");
    if (M <= 0) return 0;
    TailF32Args a{};
    a.X = X; a.ldx = ldx; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.ln_g = ln_g; a.ln_b = ln_b;
    a.OUT = OUT; a.ldo = ldo; a.M = M; a.M_dev = M_dev; a.ff = ff;
    return launch_ffn_ladder(a, false, 0, FFN_WIDE_GROUPS, s);
}

int launch_proj_ffn_fused(const TailArgs& t, hipStream_t s) {
    if (int rc = tail_f32_check(t, TF_FORM_ROWS, "fused layer tail")) return rc;
    if (t.M <= 0) return 0;
    return launch_ffn_ladder(tail_f32_args(t), true, 0, FFN_WIDE_GROUPS, s);
}

// The pre-norm layer tail (--pre_norm, t.pre): OUT = x1 + FFN(LN(x1; in_g, in_b)), x1 = R + A Wo^T + bo; OUT2 (may be null) =
// LN(OUT; out_g, out_b).  The persistent 128-row kernel for every row count (the option is off in every shipped configuration:
// no 64-row form; api.hip picks the wide and spread forms).  OUT may be R (in place).
int launch_proj_ffn_prenorm(const TailArgs& t, hipStream_t s) {
    if (int rc = tail_f32_check(t, TF_FORM_ROWS, "pre-norm layer tail")) return rc;
    if (t.M <= 0) return 0;
    return launch_ffn_rows(tail_f32_args(t), true, true, 8, 0, s);
}

// Test hook (cone_test_tail_form): the projecting tail t (post-norm or t.pre) in ONE forced form, or -- CONE_TAIL_FORM_LADDER,
// post-norm -- by the ladder's row rules for an assumed CU count, so that the full rounds + wide remainder split is reached
// with a few hundred rows (the few-groups rule is off: such a launch would always go wide).  No production path calls it.
int launch_tail_f32_form(const TailArgs& t, int form, int n_cu, hipStream_t s) {
    if (form == CONE_TAIL_FORM_SPREAD) return launch_proj_ffn_spread(t, s);
    CONE_REQUIRE(form >= CONE_TAIL_FORM_ROWS128 && form <= CONE_TAIL_FORM_LADDER, "tail form hook: unknown form %d", form);
    CONE_REQUIRE(!t.pre || (form != CONE_TAIL_FORM_ROWS64 && form != CONE_TAIL_FORM_LADDER), "tail form hook: no such pre-norm form");
    CONE_REQUIRE(form != CONE_TAIL_FORM_LADDER || n_cu > 0, "tail form hook: the ladder needs a CU count");
    if (int rc = tail_f32_check(t, form == CONE_TAIL_FORM_WIDE ? TF_FORM_WIDE : TF_FORM_ROWS, "tail form hook")) return rc;
    if (t.M <= 0) return 0;
    const TailF32Args a = tail_f32_args(t);
    if (form == CONE_TAIL_FORM_WIDE) return launch_tail_f32_wide(a, true, t.pre, s);
    if (form == CONE_TAIL_FORM_LADDER) return launch_ffn_ladder(a, true, n_cu, 0, s);
    return launch_ffn_rows(a, true, t.pre, form == CONE_TAIL_FORM_ROWS64 ? 4 : 8, 0, s);
}

// Test hook (cone_test_tail_packed): the row kernel itself -- t.A == null: the block alone on t.R as its input -- on nw waves
// (8 | 4), a persistent grid sized for n_cu CUs (0: the device's), streaming the packed image img (null: the row-major
// matrices).  img is what launch_f32_pack_tail built from these weights: with the Wo chunks exactly when t.A is given.
int launch_tail_f32_rows_hook(const TailArgs& t, const void* img, int nw, int n_cu, hipStream_t s) {
    CONE_REQUIRE(nw == 8 || nw == 4, "tail rows hook: %d waves", nw);
    CONE_REQUIRE(n_cu >= 0, "tail rows hook: negative CU count");
    const bool proj = t.A != nullptr;
    CONE_REQUIRE(proj || (!t.pre && !t.next), "tail rows hook: the block alone has no pre-norm form and no ride");
    CONE_REQUIRE(nw == 8 || (!t.pre && !t.next), "tail rows hook: the ride and the pre-norm form run on 8 waves");
    TailF32Args a;
    if (proj) {
        if (int rc = tail_f32_check(t, TF_FORM_ROWS, "tail rows hook")) return rc;
        a = tail_f32_args(t);
    } else {
        const TailWeights& w = *t.w;
        CONE_REQUIRE(ffn_fused_supported(t.ff) && t.R && w.W1 && w.b1 && w.W2 && w.b2 && w.out_g && w.out_b && t.OUT,
                     "tail rows hook: bad block arguments");
        a = TailF32Args{};
        a.X = t.R; a.ldx = t.ldr; a.W1 = w.W1; a.b1 = w.b1; a.W2 = w.W2; a.b2 = w.b2; a.ln_g = w.out_g; a.ln_b = w.out_b;
        a.OUT = t.OUT; a.ldo = t.ldo; a.M = t.M; a.M_dev = t.M_dev; a.ff = t.ff;
    }
    a.Wimg = img;
    if (t.M <= 0) return 0;
    return launch_ffn_rows(a, proj, t.pre, nw, n_cu, s);
}
}  // namespace cone
