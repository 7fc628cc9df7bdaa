// Input projections of the two BiLSTM layers (fast recogniser modes): x [rows_pad, 256] -> [rows_pad, 2048] 16-bit gate pre-activations.
//
// conv1x1_dma_kernel gives this GEMM one 256-row x 256-cout tile per workgroup and K = 256 is only 8 k-steps: a prologue, ~4 us of MFMA and
// a 128 KB store burst with nothing beside it on the CU.  Here the operands swap roles: the WEIGHTS stay in registers and the rows stream.
//   - A workgroup of 8 waves owns 512 output channels (two 256-cout tiles `nt` of the plan's packed image) and one contiguous chunk of rows.
//     Wave w owns the 64 channels (nt = 2 cg + (w >> 2), wn = w & 3) and loads its 8 k-steps x 4 fragments -- 128 VGPRs -- ONCE, straight from
//     the packed image pack_conv_weights wrote for the tile kernel ([nt][ks][wn 4][j 4][lane 64] x 16 B).
//   - Rows enter LDS by lds_dma16 in slots of 64 rows x 256 channels (32 KB: [ks 8][64 rows][4 groups] x 16 B, the pixel-major swizzled image
//     of conv1x1_dma_kernel per k-step) through a ring of 4 slots: 3 measured 598 us per launch at 518,400 rows, 4 574 us (the DMAs of a slot
//     retire behind two slots' stores instead of one).  One workgroup fits per CU (128 KB of LDS, two waves per SIMD).
//   - Per 16-row block a wave reads its 8 B fragments, runs the tile kernel's 32 MFMAs in the tile kernel's order (acc[j] = mfma(w[ks][j],
//     x[ks], acc[j]), ks = 0..7, from zero), applies conv_epilogue's value path (fma(acc, acc_scale, bias), round, the DPP regroup into whole
//     128-byte lines) and issues its two 1 KB stores WITHOUT waiting for them: the result is bit-identical to the tile kernel's.
//   - vmcnt retires in order and counts stores as well as DMAs.  Every store of a slot is unconditional (the launcher hands out whole
//     slots), so the number of operations younger than a slot's DMAs is a compile-time constant and the one wait per slot is counted.
//   - The 4 column groups of a row chunk are consecutive logical block ids of one XCD (xcd_remap): the chunk comes from HBM once.
#include "common.h"
#include "kernels.h"

namespace {
constexpr int SP_K = 256, SP_N = 2048;
constexpr int SP_WAVES = 8, SP_COLS = SP_WAVES * 64, SP_CG = SP_N / SP_COLS;      // 512 couts per workgroup, 4 column groups
constexpr int SP_RING = 4, SP_SLOT_ROWS = 64, SP_SLOT = SP_SLOT_ROWS * SP_K * 2;  // 32 KB
constexpr int SP_DMAS = SP_SLOT / 1024 / SP_WAVES;                                 // 1 KB DMAs a wave issues per slot: 4
constexpr int SP_STORES = (SP_SLOT_ROWS / 16) * 2;                                 // 1 KB stores a wave issues per slot: 8
constexpr size_t SP_LDS = (size_t)SP_RING * SP_SLOT;
static_assert(SP_DMAS * SP_WAVES * 1024 == SP_SLOT && SP_DMAS == SP_SLOT_ROWS / 16 && SP_WAVES == SP_K / 32, "wave w fetches k-step w of the slot's four 16-row blocks");
static_assert((SP_RING - 1) * SP_STORES + (SP_RING - 2) * SP_DMAS < 64, "the counted wait must fit vmcnt's 6 bits");

template <int EL>
__global__ void __launch_bounds__(SP_WAVES * 64, 2) seq_proj_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wpk, const float* __restrict__ bias,
                                                                    uint16_t* __restrict__ out, float acc_scale, int nslots, int chunk_slots) {
    typedef typename El<EL>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [SP_RING][ks 8][64 rows][4 slots] x 16 B
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int cg = bid % SP_CG, chunk = bid / SP_CG;
    const int s0 = chunk * chunk_slots;                                    // the chunk's first slot; (the launcher keeps chunks * chunk_slots in an int)
    const int n = nslots - s0 < chunk_slots ? nslots - s0 : chunk_slots;   // the last chunk is shorter, the ones behind it are empty
    if (n <= 0) return;                                                    // (the whole workgroup, before any barrier)
    const int nt = cg * 2 + (wave >> 2), wn = wave & 3;
    const int g = lane >> 4, pl = lane & 15;
    const int cout0 = nt * 256 + wn * 64 + g * 8;                          // first cout of the lane's run 0; run 1 starts 32 further (conv_epilogue)

    // ---- the wave's weights and biases, once
    typedef const __attribute__((address_space(1))) v8* gfrag_ptr;         // global_load (vmcnt only), never flat_load
    const gfrag_ptr wg = (gfrag_ptr)((const v8*)wpk + ((size_t)nt * 8 * 16 + wn * 4) * 64 + lane);   // 16 fragments of 64 lanes per (nt, ks)
    v8 w[8][4];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) w[ks][j] = wg[(ks * 16 + j) * 64];
    f32x4 bs[4];                                                           // bs[j][r]: bias of v[j * 4 + r], run j >> 1, position (j & 1) * 4 + r
#pragma unroll
    for (int j = 0; j < 4; ++j) bs[j] = *(const __attribute__((address_space(1))) f32x4*)(bias + cout0 + (j >> 1) * 32 + (j & 1) * 4);

    // ---- row slots: wave w fetches k-step w (channels 32 w .. 32 w + 31) of the slot's four 16-row blocks; lane L the 16 bytes of channel
    // group (L & 3) ^ swizzle of row L >> 2, landing linearly
    const uint16_t* src = x + ((size_t)s0 * SP_SLOT_ROWS + (lane >> 2)) * SP_K + wave * 32 + ((lane & 3) ^ (((lane >> 4) & 1) * 2)) * 8;
    auto issue = [&](int s, int ring) {
        unsigned char* sb = smem + ring * SP_SLOT + wave * 4096;
#pragma unroll
        for (int i = 0; i < SP_DMAS; ++i) lds_dma16(src + ((size_t)s * SP_SLOT_ROWS + i * 16) * SP_K, sb + i * 1024);
    };
#pragma unroll
    for (int i = 0; i < SP_RING - 1; ++i)
        if (i < n) issue(i, i);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // Everything loaded above is in its registers from here on: hipcc's waitcnt pass does not see through the asm, and would otherwise wait
    // for "its" weight loads at their first use INSIDE the row loop -- with a count that drains the stores of the slot before.
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(w[ks][j]));
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(bs[j]));

    const int lane_p_off = pl * 64 + (g ^ (((pl >> 2) & 1) * 2)) * 16;
    // lanes pl < 8 store rows 0..7 of a block (their run 0 + the run 1 of lane pl + 8), lanes pl >= 8 rows 8..15: whole 128-byte lines
    uint16_t* op = out + ((size_t)s0 * SP_SLOT_ROWS + (pl & 7)) * SP_N + cout0 + (pl >> 3) * 32;
    int ring = 0;
    for (int s = 0; s < n; ++s) {
        const bool ahead = s + SP_RING - 1 < n;
        if (ahead) {
            int r2 = ring + SP_RING - 1;
            if (r2 >= SP_RING) r2 -= SP_RING;
            issue(s + SP_RING - 1, r2);         // the slot read one iteration ago: every wave has passed that iteration's barrier
        }
        const unsigned char* sb = smem + ring * SP_SLOT + lane_p_off;
#pragma unroll
        for (int b = 0; b < SP_SLOT_ROWS / 16; ++b) {
            v8 bq[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) bq[ks] = *(const v8*)(sb + ks * 4096 + b * 1024);
            f32x4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = El<EL>::mfma(w[ks][j], bq[ks], acc[j]);
            // conv_epilogue's value path (pool_mode 0, no ReLU, fullw)
            float v[16];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[j * 4 + r] = fmaf(acc[j][r], acc_scale, bs[j][r]);
            const u32x4 lo = {El<EL>::pack2(v[0], v[1]), El<EL>::pack2(v[2], v[3]), El<EL>::pack2(v[4], v[5]), El<EL>::pack2(v[6], v[7])};
            const u32x4 hi = {El<EL>::pack2(v[8], v[9]), El<EL>::pack2(v[10], v[11]), El<EL>::pack2(v[12], v[13]), El<EL>::pack2(v[14], v[15])};
            u32x4 dA, dB;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dA[i] = (unsigned)__builtin_amdgcn_update_dpp((int)lo[i], (int)hi[i], 0x118 /*row_shr:8*/, 0xF, 0xC, false);
                dB[i] = (unsigned)__builtin_amdgcn_update_dpp((int)hi[i], (int)lo[i], 0x108 /*row_shl:8*/, 0xF, 0x3, false);
            }
            *(u32x4*)op = dA;
            *(u32x4*)(op + 8 * SP_N) = dB;
            op += 16 * SP_N;
        }
        // Slot s + 1 was issued SP_RING - 2 iterations ago (or in the prologue, which drained).  Younger than its DMAs are the stores of
        // SP_RING - 1 iterations, this one included, and -- while the pipeline is full -- the DMAs of the SP_RING - 2 slots behind it; all
        // of them unconditional, so the count is exact.  Draining out, fewer DMAs follow: counting the stores alone waits for no less.
        // lgkmcnt(0) is part of the barrier: the next iteration's DMAs overwrite the slot just read (see conv3x3_up4_kernel's barrier).
        if (ahead) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((SP_RING - 1) * SP_STORES + (SP_RING - 2) * SP_DMAS) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((SP_RING - 1) * SP_STORES) : "memory");
        ring = ring + 1 == SP_RING ? 0 : ring + 1;
    }
}
}  // namespace

// Row chunks of a launch: one residency of workgroups (one per compute unit), SP_CG column groups per chunk, whole chunks per XCD.  A chunk
// is chunk_slots slots of 64 rows; the last one may be shorter and the ones behind it empty.
SeqProjPlan seq_proj_plan(size_t rows_pad, int ncu) {
    SeqProjPlan p{};
    int chunks = ncu / SP_CG / 8 * 8;            // xcd_remap deals each XCD grid / 8 consecutive ids: a multiple of SP_CG when chunks % 8 == 0
    if (chunks < 8) chunks = 8;
    const size_t nslots = rows_pad / SP_SLOT_ROWS;
    p.chunks = chunks;
    p.ring = SP_RING;
    p.grid = chunks * SP_CG;
    p.nslots = (long long)nslots;
    p.chunk_slots = (long long)((nslots + chunks - 1) / chunks);
    return p;
}

hipError_t launch_seq_proj(const ConvPlan& p, const uint16_t* x, size_t rows_pad, uint16_t* out, hipStream_t s) {
    if (p.KH != 1 || p.KW != 1 || p.Cin != SP_K || p.Cin_pad != SP_K || p.Cout != SP_N || p.Cout_pad != SP_N || p.BN != 256 || p.split || !p.d_w || !p.d_b)
        return hipErrorNotSupported;
    if (!x || !out || rows_pad == 0 || rows_pad % 256 != 0) return hipErrorNotSupported;
    const SeqProjPlan g = seq_proj_plan(rows_pad, device_cus());
    if (g.nslots + g.chunks > 0x7fffffffLL) return hipErrorNotSupported;      // chunk * chunk_slots stays in an int
    static LdsOptIn attr[2];
    const void* k = p.el ? (const void*)seq_proj_kernel<1> : (const void*)seq_proj_kernel<0>;
    if (hipError_t e = lds_opt_in(attr[p.el ? 1 : 0], k, SP_LDS); e != hipSuccess) return e;
    if (p.el) hipLaunchKernelGGL(seq_proj_kernel<1>, dim3(g.grid), dim3(SP_WAVES * 64), SP_LDS, s, x, p.d_w, p.d_b, out, p.acc_scale, (int)g.nslots, (int)g.chunk_slots);
    else hipLaunchKernelGGL(seq_proj_kernel<0>, dim3(g.grid), dim3(SP_WAVES * 64), SP_LDS, s, x, p.d_w, p.d_b, out, p.acc_scale, (int)g.nslots, (int)g.chunk_slots);
    return hipGetLastError();
}
