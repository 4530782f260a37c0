// Tall form of the row GEMM  C = epi(A W^T + bias)  for K = 256 and many rows: the layer tail's projection loop (ffn.hip,
// FFN_CHUNK32) run as a GEMM of its own.
//
// gemm_rows16_kernel streams A and W k-slab by k-slab through LDS (3 LDS-DMA pieces and a barrier per 64 MFMAs per wave, A read
// N / 256 times) and parks its 64 accumulators in LDS for the epilogue.  Here the orientation is the tail's: a wave owns 16
// rows, loads their 256 values ONCE per tile into 64 VGPRs (x[q][r] = A[row li][16 q + 4 lg + r]) as the B operand, and only
// the weights go through LDS, in chunks of 32 output channels in the projection's slab format (tail_f32_common.h: [16 rows][16
// floats] slabs, the 16-B chunk XOR-swizzled on the source and on the ds_read_b128 address; W rows [32 g, 32 g + 16) in the
// first half of a 32-KiB stage, [32 g + 16, 32 g + 32) in the second).  One persistent 8-wave workgroup per CU walks the
// 128-row tiles round-robin; the ring is ffn.hip's: 4 stages, chunk c + 2 streams while chunk c is multiplied, 4 pieces per
// wave and ONE counted s_waitcnt vmcnt + ONE s_barrier per chunk (128 MFMAs per wave), and it runs on across tiles -- the
// weights of every tile are the same.  The next tile's rows are requested into a second register tile at the top of a tile.
// The epilogue of a chunk goes straight from the accumulators: accumulator r of lane (li, lg) = C[row li][c0 + 4 lg + r], four
// consecutive channels of the lane's row, one 16-B store per 16-channel tile; bias sits in LDS.
//
// Bits.  gemm_rows16_kernel computes an output element as ONE chain  for kt, for j: acc = mfma(a[j], b[j], acc)  in which lane
// group lg supplies k = 16 kt + 4 lg + j.  The chain here -- for q, for r: acc = mfma(Wfrag[q][r], x[q][r], acc), k = 16 q +
// 4 lg + r -- walks the same k in the same order with the operand roles swapped, and an exact-fp32 MFMA is a k-ordered fma
// chain per element whichever operand comes first (what the spread form and the layer tail's forms rely on too).  The epilogue
// is the same arithmetic in the same order: (acc + bias), ReLU, + R.  So a row's bits are the 8-wave row tile's, and the choice
// between the two is made by shape and host-known row bound alone.
//
// vmcnt.  Vector-memory operations retire in issue order, and the chunk's wait is counted, so what a wave issues between two
// waits is fixed by construction: per chunk g, in this order,
//     [after the barrier that ended chunk g - 1]  the stores of chunk g - 1 (0 or 2), RES: the residual loads of chunk g (2),
//                                                 ahead of a tile's chunk 0 the next tile's 16 row loads;
//     [under the MFMAs of chunk g]                the wave's GT_NPIECE pieces of chunk g + 2 -- the LAST operations issued;
//     s_waitcnt vmcnt(GT_NPIECE), s_barrier.
// The wait therefore leaves exactly the pieces of chunk g + 2 in flight whatever the number of stores and loads ahead of them
// (a wave with rows past M issues the same count; an idle wave issues pieces only): the pieces of chunk g + 1, issued a chunk
// earlier, have landed, and so have the stores of chunk g - 1 and the row loads, which had a whole chunk (3.7 us) to do so.
// The stores of chunk g are issued BEHIND the barrier, so no wait ever covers a store younger than a chunk.
//
// Weight stream.  gemm_tall_kernel<RES, false> gathers a piece's 16 row segments from the row-major W; <RES, true> reads the
// same bytes from W's packed image (tail_pack.hip, a.Wimg), where every lane's 16 B already sits in place.
#include "gemm_tall.h"
#include "tail_f32_common.h"

namespace cone {

constexpr int GT_ROWS = 128;                      // rows per tile: 8 waves x 16
constexpr int GT_STAGE = 32 * 256;                // floats per ring stage: 32 W rows x K = 256
constexpr int GT_NST = 4;                         // ring depth (ffn.hip's FFN_NST): a stage is refilled two barriers after its last read
constexpr int GT_NPIECE = 4;                      // 1-KiB LDS-DMA pieces per wave per chunk
static_assert(GT_NPIECE * 8 * 256 == GT_STAGE, "8 waves x GT_NPIECE pieces of 256 floats fill a stage");
static_assert(GT_NST == 4, "the stage index is advanced with & 3, and chunk c + 2 must not land in a stage still being read");

// PK: the weight pieces stream from W's packed image p.Wimg (tail_pack.hip: the chunks in walking order, every lane's 16 B in
// place) instead of being gathered from the row-major matrix -- the same bytes at the same LDS addresses.
template <bool RES, bool PK = false>
__global__ __launch_bounds__(512, 2) void gemm_tall_kernel(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bs = smem + GT_NST * GT_STAGE;         // bias (N floats; zeros without one)
    int M = p.M;
    if (p.M_dev) { const int md = *p.M_dev; M = md < M ? md : M; }
    const int n_tiles = M > 0 ? (M + GT_ROWS - 1) / GT_ROWS : 0;
    if ((int)blockIdx.x >= n_tiles) return;       // (the whole workgroup: nothing has been issued)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int NC = p.N >> 5;                      // weight chunks per tile
    const bool relu = (p.flags & EPI_RELU) != 0;

    for (int i = tid; i < (p.N >> 2); i += 512)
        reinterpret_cast<f32x4*>(bs)[i] = p.bias ? reinterpret_cast<const f32x4*>(p.bias)[i] : f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- LDS-DMA pieces (ffn.hip's projection chunk): a chunk = 32 slabs of [16 rows][16 floats], slab pid = 4 w + i holds
    // W[32 g + 16 (pid / 16) + row][16 (pid % 16) + 4 ch ..]; lane -> (row = lane / 4, physical chunk = lane % 4), the source
    // chunk XOR-swizzled.  A piece's source = a wave-uniform base (SGPRs) + ONE 32-bit lane offset.
    const int drow = lane >> 2;
    const int dch = (lane & 3) ^ tf_swz16(drow);
    unsigned vo = PK ? (unsigned)(lane * 16)
                           : (unsigned)(((16 * (wave >> 2) + drow) * 256 + 16 * GT_NPIECE * (wave & 3) + 4 * dch) * 4);
    int stg = 0;                                  // ring stage of the chunk being multiplied
    int ws = 0;                                   // weight chunk (< NC) that streams next
    auto stream_piece = [&](int stage, int wchunk, int i) {
        float* dstp = smem + stage * GT_STAGE + (wave * GT_NPIECE + i) * 256;
        // the empty asm pins the base in SGPRs at this point: hoisted out of the loops, base + lane offset becomes a 64-bit
        // VGPR pair per piece
        // (PK: one 32-bit offset of (chunk, slab); an image is far below 4 GiB)
        const char* ub = PK ? reinterpret_cast<const char*>(p.Wimg) + (((unsigned)wchunk << 15) + (unsigned)(wave * GT_NPIECE + i) * 1024u)
                            : reinterpret_cast<const char*>(p.W + ((size_t)wchunk * (32 * 256) + 16 * i));
        asm volatile("" : "+s"(ub));
        // the lane offset is pinned here too -- hoisted, its zero-extension lands in another block than the load, which then
        // takes a 64-bit VGPR address (one v_lshl_add_u64 per piece in the MFMA stream) instead of saddr + voffset
        // (in place, on the one variable: a pinned copy would cost a v_mov per piece)
        asm volatile("" : "+v"(vo));
        TF_GLDS16(ub + vo, dstp);
    };
    auto next_chunk = [&]() { ws = ws + 1 < NC ? ws + 1 : 0; stg = (stg + 1) & 3; };

    const int rd = li * 16 + ((lg ^ tf_swz16(li)) << 2);          // this lane's 16-B chunk inside a slab
#define GT_RD(stp, off) (*reinterpret_cast<const f32x4*>((stp) + (off) + rd))
#define GT_SB() __builtin_amdgcn_sched_barrier(0)
    // the counted wait + barrier that ends every chunk (see "vmcnt" in the header): the next chunk has landed -- all but the
    // GT_NPIECE pieces issued last, which belong to the chunk after it -- and every wave is done with the stage they overwrite
#define GT_END_CHUNK()                                                            \
    {                                                                             \
        GT_SB();                                                                  \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GT_NPIECE) : "memory");          \
        __builtin_amdgcn_s_barrier();                                             \
        GT_SB();                                                                  \
    }
    // MFMA issue order is pinned as in ffn.hip (FFN_MFMA): the two chains of a chunk alternate, so an accumulator is reused two
    // MFMAs (64 cycles) later, beyond the 40-cycle dependent latency
#define GT_MFMA(acc, a, b) { acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); GT_SB(); }

    // The rows of a tile (rows past M re-read row M - 1: they feed unstored outputs).  The loads are asm statements, which
    // hipcc does not count: for a load it counts it drains vmcnt -- the pieces in flight with it -- ahead of the first use of
    // the registers, once per tile (measured 6.07 -> 6.05 ms at 2 M x 768: inside the noise, kept for the ISA).  Their completion is the
    // protocol's (header, "vmcnt"): issued ahead of the pieces of their chunk, they have landed at that chunk's counted wait;
    // GT_ROWS_LANDED behind that wait is the first point at which the program reads the registers.
    f32x4 x[16], xn[16];
    auto load_rows = [&](int tile) {
        const float* ap = p.A + TF_LD_ROW(tile * GT_ROWS + wave * 16 + li, M) * p.lda + 4 * lg;
#pragma unroll
        for (int q = 0; q < 16; ++q)
            asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(xn[q]) : "v"(ap), "n"(64 * q) : "memory");
    };
#define GT_ROWS_LANDED()                                                                                         \
    asm volatile("" : "+v"(xn[0]), "+v"(xn[1]), "+v"(xn[2]), "+v"(xn[3]), "+v"(xn[4]), "+v"(xn[5]), "+v"(xn[6]),  \
                      "+v"(xn[7]), "+v"(xn[8]), "+v"(xn[9]), "+v"(xn[10]), "+v"(xn[11]), "+v"(xn[12]),           \
                      "+v"(xn[13]), "+v"(xn[14]), "+v"(xn[15]))
    load_rows(blockIdx.x);                        // ahead of the pieces: the first wait below covers them
    {
        const int w1 = NC > 1 ? 1 : 0;
#pragma unroll
        for (int i = 0; i < GT_NPIECE; ++i) stream_piece(0, 0, i);
#pragma unroll
        for (int i = 0; i < GT_NPIECE; ++i) stream_piece(1, w1, i);
        ws = w1 + 1 < NC ? w1 + 1 : 0;
    }

    f32x4 wa, wb, na, nb;      // first-half fragments (current / next unit)
    f32x4 va, vb, nva, nvb;    // second-half fragments
    // chunk 0, the first tile's rows and the bias image are in place (later tiles: the previous tile's last barrier covers
    // chunk 0).  Ahead of the tile loop, not under a first-iteration flag in it: hipcc must see the rows waited for on every
    // path into the chunk loop, or it drains vmcnt -- the next tile's rows with it -- before the first MFMA of every tile.
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GT_NPIECE) : "memory");
    GT_ROWS_LANDED();
    __syncthreads();
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int my_row0 = tile * GT_ROWS + wave * 16;
        const int my_row = my_row0 + li;
        const bool act = my_row0 < M;             // wave-uniform
        if (!act) {
            // this wave holds no row of the tile (only a launch's last tile can be short): it keeps its part of the protocol
            // -- per chunk its pieces of the next-but-one chunk, the counted wait, the barrier -- and issues no MFMA
            for (int g = 0; g < NC; ++g) {
#pragma unroll
                for (int i = 0; i < GT_NPIECE; ++i) stream_piece((stg + 2) & 3, ws, i);
                GT_END_CHUNK()
                next_chunk();
            }
            break;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = xn[q];
        GT_SB();
        float* cp = p.C + (size_t)my_row * p.ldc + 4 * lg;
        const float* rp = RES ? p.R + TF_LD_ROW(my_row, M) * p.ldr + 4 * lg : nullptr;
        f32x4 r0, r1;
        if (RES) { r0 = *reinterpret_cast<const f32x4*>(rp); r1 = *reinterpret_cast<const f32x4*>(rp + 16); }
        GT_SB();

        for (int g = 0; g < NC; ++g) {
            // ---- one chunk of 32 output channels: two 16-channel tiles, ONE chain each (ha, hb), interleaved; 8 units of 16
            // MFMAs, the ds_read_b128 of unit u + 1 issued right ahead of the MFMAs of unit u (the empty asm at the top of a
            // unit is where hipcc puts its lgkmcnt wait: before the next reads are issued)
            // the next tile's rows, in flight under chunk 0 (after the last tile a valid tile is re-read, so that the register
            // tile has ONE definition per tile)
            if (g == 0) load_rows(tile + (int)gridDim.x < n_tiles ? tile + (int)gridDim.x : tile);
            const float* st = smem + stg * GT_STAGE;
            const int sn = (stg + 2) & 3;
            f32x4 ha = f32x4{0.f, 0.f, 0.f, 0.f}, hb = ha;
            wa = GT_RD(st, 0); wb = GT_RD(st, 256); va = GT_RD(st, 4096); vb = GT_RD(st, 4096 + 256);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                GT_SB();
                asm volatile("" : "+v"(wa), "+v"(wb), "+v"(va), "+v"(vb));
                GT_SB();
                if (u < 7) {
                    na = GT_RD(st, (2 * u + 2) * 256); nb = GT_RD(st, (2 * u + 3) * 256);
                    nva = GT_RD(st, 4096 + (2 * u + 2) * 256); nvb = GT_RD(st, 4096 + (2 * u + 3) * 256);
                }
                GT_SB();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    GT_MFMA(ha, wa[r], x[2 * u][r])
                    GT_MFMA(hb, va[r], x[2 * u][r])
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    GT_MFMA(ha, wb[r], x[2 * u + 1][r])
                    GT_MFMA(hb, vb[r], x[2 * u + 1][r])
                }
                if (u & 1) stream_piece(sn, ws, u >> 1);        // the next-but-one chunk's pieces ride behind MFMAs
                if (u < 7) { wa = na; wb = nb; va = nva; vb = nvb; }
            }
            GT_SB();
            // ---- epilogue, gemm_rows16_kernel's arithmetic: (acc + bias), ReLU, + R
            f32x4 o0 = ha + *reinterpret_cast<const f32x4*>(bs + 32 * g + 4 * lg);
            f32x4 o1 = hb + *reinterpret_cast<const f32x4*>(bs + 32 * g + 16 + 4 * lg);
            if (relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { o0[r] = fmaxf(o0[r], 0.f); o1[r] = fmaxf(o1[r], 0.f); }
            }
            if (RES) { o0 += r0; o1 += r1; }
            // the outputs are complete HERE: hipcc otherwise sinks this arithmetic behind the barrier into the store's branch,
            // where its wait for the residual drains the pieces and the stores
            asm volatile("" : "+v"(o0), "+v"(o1));
            GT_END_CHUNK()
            GT_ROWS_LANDED();
            // behind the barrier, ahead of the next chunk's pieces: this chunk's stores, the next chunk's residual
            if (my_row < M) {
                *reinterpret_cast<f32x4*>(cp + 32 * g) = o0;
                *reinterpret_cast<f32x4*>(cp + 32 * g + 16) = o1;
            }
            if (RES) {
                const int gn = g + 1 < NC ? g + 1 : g;
                r0 = *reinterpret_cast<const f32x4*>(rp + 32 * gn);
                r1 = *reinterpret_cast<const f32x4*>(rp + 32 * gn + 16);
            }
            GT_SB();
            next_chunk();
        }
    }   // tile loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // no LDS-DMA may outlive the workgroup's LDS
}

#undef GT_ROWS_LANDED
#undef GT_MFMA
#undef GT_END_CHUNK
#undef GT_SB
#undef GT_RD

static size_t gt_lds_bytes(int N) { return (size_t)(GT_NST * GT_STAGE + N) * sizeof(float); }

const char* gemm_tall_refusal(const GemmArgs& a) {
    if (a.K != 256) return "K must be 256";
    if (a.N < 32 || a.N % 32 != 0 || gt_lds_bytes(a.N) > 160 * 1024) return "N must be a multiple of 32 up to 8192";
    if (a.ldw != 256) return "the weight rows must be contiguous (ldw == 256)";
    if (a.A2) return "no fused addend (A2)";
    if (a.C2 || a.ADD) return "no second output (C2 / ADD)";
    if (a.flags & EPI_LN) return "no LayerNorm epilogue";
    if (a.r_mod) return "no row-periodic residual (r_mod)";
    if (a.m_off) return "no row offset (m_off)";
    if (a.lda % 4 != 0 || a.ldc % 4 != 0 || ((a.flags & EPI_RESIDUAL) && a.ldr % 4 != 0)) return "row strides must be multiples of 4";
    return nullptr;
}

int launch_gemm_tall(const GemmArgs& a, int n_cu, hipStream_t s) {
    const char* why = gemm_tall_refusal(a);
    CONE_REQUIRE(!why, "gemm: the tall form (variant %d) cannot run this launch: %s (M=%d N=%d K=%d flags=%d)", GEMM_TALL, why,
                 a.M, a.N, a.K, a.flags);
    CONE_REQUIRE(a.A && a.W && a.C && (!(a.flags & EPI_RESIDUAL) || a.R), "gemm: the tall form: null argument");
    if (a.M <= 0) return 0;
    // once per device: the opt-in to > 64 KiB of LDS and the CU count that sizes the persistent grid (one workgroup per CU)
    static DeviceOnce once;
    int dev_cu = 0;
    CONE_CHECK_HIP(device_once(once, [] {
        const void* const kernels[4] = {(const void*)gemm_tall_kernel<false, false>, (const void*)gemm_tall_kernel<true, false>,
                                        (const void*)gemm_tall_kernel<false, true>, (const void*)gemm_tall_kernel<true, true>};
        hipError_t rc = hipSuccess;
        for (int i = 0; i < 4 && rc == hipSuccess; ++i)
            rc = hipFuncSetAttribute(kernels[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        return rc;
    }, &dev_cu));
    if (n_cu <= 0) n_cu = dev_cu;
    const int tiles = (a.M + GT_ROWS - 1) / GT_ROWS;
    const int grid = tiles < n_cu ? tiles : n_cu;
    // booked as the 8-wave row tile's kind: the same computation, and the FLOP accounting by shape stays complete
    ProfScope ps(PK_GEMM_ROWS16, a.M, a.N, a.K, a.M_dev, s);
    // a.Wimg (W's packed image) picks the stream form
    const bool res = (a.flags & EPI_RESIDUAL) != 0;
    auto* const kernel = a.Wimg ? (res ? gemm_tall_kernel<true, true> : gemm_tall_kernel<false, true>)
                                : (res ? gemm_tall_kernel<true, false> : gemm_tall_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(512), gt_lds_bytes(a.N), s, a);
    CONE_LAUNCH_CHECK();
    if (a.Wimg) f32_packed_note(1);
    return 0;
}

}  // namespace cone
