// Microbenchmark (diagnostic, not part of the library): landing rate of global_load_lds_dwordx4 (LDS-DMA, 16 B per lane, 1 KiB per
// wave-instruction) by the SHAPE of the per-lane source addresses, from an NHWC tensor of C 16-bit channels that stays inside L2.
// A workgroup of four waves fetches, per step, the 32-channel chunk (64 B) of 64 consecutive pixels -- the activation operand of
// conv3x3_dma_kernel / conv1x1_dma_kernel -- as four wave-instructions:
//   (a) 64 pixels x 16 B per instruction   wave w = channel group w of the 64 pixels              (the kernels' gather today)
//   (b) 32 pixels x 32 B per instruction   lane pairs; wave w = half (w & 1) of the pixels, channel groups 2 (w >> 1) + {0, 1}
//   (c) 16 pixels x 64 B per instruction   lane quads; wave w = pixels 16 w .. 16 w + 15, all four groups
//   (d) 1 KiB contiguous per instruction   (the weight operand's shape; the same bytes read as a flat buffer)
// Every wave keeps 6 instructions in flight into an LDS ring (never read) behind `s_waitcnt vmcnt(5)`.  256-thread workgroups sized
// (LDS) for two per CU.  Two modes: `idle` = one gathering workgroup per CU and nothing else; `mfma` = two workgroups per CU, the
// first to arrive on a CU gathers, the second runs a bare v_mfma_f32_16x16x32_bf16 loop (the other wave of every SIMD) that outlasts it.
// Rates come from the gathering workgroups' own s_memrealtime stamps (100 MHz).
//   hipcc -O3 --offload-arch=gfx950 -o tools/micro/gather_shapes tools/micro/gather_shapes.hip && tools/micro/gather_shapes
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int FOOT = 1 << 20;          // bytes of the source tensor (every XCD's L2 holds its own copy)
constexpr int INFLIGHT = 6;
constexpr int CU_KEYS = 4096;

// lane l's 16 bytes land at lds + 16 l; `lds` wave-uniform
__device__ __forceinline__ void lds_dma16(const void* gptr, unsigned la) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(la) : "memory");
}

// (XCC, SE, SH, CU) of the wave: HW_REG_HW_ID bits 8..15 and HW_REG_XCC_ID bits 0..3
__device__ __forceinline__ int cu_key() {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
    return (int)(((xcc & 15u) << 8) | ((hw >> 8) & 255u));
}

struct Result { unsigned long long ticks; int role; int key; };

template <int SHAPE>
__global__ void __launch_bounds__(256, 2) gather(const unsigned char* __restrict__ src, int C, int steps, int mfma_iters, int pair, int* arrivals,
                                                 Result* res, float* sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ring[];
    __shared__ int s_role;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int key = cu_key();
    if (threadIdx.x == 0) s_role = atomicAdd(&arrivals[key], 1);
    __syncthreads();
    const int role = pair ? (s_role & 1) : 0;          // 0: gather, 1: MFMA loop
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    if (role == 0) {
        const int ps = C * 2;                          // bytes per pixel
        const int nblk = FOOT / (64 * ps), nchunk = C / 32;
        unsigned lane_off;                             // per-lane byte offset inside (64-pixel block, chunk)
        if (SHAPE == 0) lane_off = lane * ps + wave * 16;
        else if (SHAPE == 1) lane_off = ((wave & 1) * 32 + (lane >> 1)) * ps + ((wave >> 1) * 2 + (lane & 1)) * 16;
        else if (SHAPE == 2) lane_off = (wave * 16 + (lane >> 2)) * ps + (lane & 3) * 16;
        else lane_off = wave * 1024 + lane * 16;
        const unsigned char* lp = src + lane_off;
        int blk = (blockIdx.x * 5) % nblk, chunk = blockIdx.x % nchunk;
        int flat = (blockIdx.x * 5) % (FOOT / 4096);
        const unsigned la0 = (unsigned)(size_t)(const __attribute__((address_space(3))) void*)ring + wave * (INFLIGHT * 1024);
        auto next = [&]() -> const unsigned char* {    // wave-uniform walk: all pixel blocks of a chunk, then the next chunk
            size_t uo;
            if (SHAPE == 3) {
                uo = (size_t)flat * 4096;
                flat = flat + 1 == FOOT / 4096 ? 0 : flat + 1;
            } else {
                uo = (size_t)blk * 64 * ps + chunk * 64;
                if (++blk == nblk) { blk = 0; chunk = chunk + 1 == nchunk ? 0 : chunk + 1; }
            }
            return lp + uo;
        };
#pragma unroll
        for (int s = 0; s < INFLIGHT; ++s) lds_dma16(next(), la0 + s * 1024);
        for (int it = 1; it < steps / INFLIGHT; ++it) {
#pragma unroll
            for (int s = 0; s < INFLIGHT; ++s) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(INFLIGHT - 1) : "memory");
                lds_dma16(next(), la0 + s * 1024);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        bf16x8 a[4], b[8];
        const bf16x8* frag = (const bf16x8*)src;
        for (int i = 0; i < 4; ++i) a[i] = frag[i * 64 + lane];
        for (int i = 0; i < 8; ++i) b[i] = frag[(4 + i) * 64 + lane];
        f32x4 acc[8][4];
        for (int f = 0; f < 8; ++f)
            for (int j = 0; j < 4; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < mfma_iters; ++it) {
#pragma unroll
            for (int f = 0; f < 8; ++f)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], b[f], acc[f][j], 0, 0, 0);
        }
        float t = 0.f;
        for (int f = 0; f < 8; ++f)
            for (int j = 0; j < 4; ++j) t += acc[f][j][0] + acc[f][j][3];
        if (t == 123.456f) sink[0] = t;
    }
    __syncthreads();
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) res[blockIdx.x] = Result{t1 - t0, role, key};
}

struct Row { double per_cu, chip, mfma_over_gather; int gatherers, crowded; };

template <int SHAPE>
static Row run(const unsigned char* src, int C, int ncu, bool pair, int* arrivals, Result* res, float* sink) {
    const int steps = 6144, mfma_iters = 60000;       // 6 MiB per gathering wave; the MFMA loop is ~8 ms, longer than any gather here
    const int grid = pair ? 2 * ncu : ncu;
    const size_t lds = pair ? 64 * 1024 : 128 * 1024; // two / one workgroup per CU
    CK(hipFuncSetAttribute((const void*)gather<SHAPE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CK(hipMemset(arrivals, 0, CU_KEYS * sizeof(int)));
    hipLaunchKernelGGL(gather<SHAPE>, dim3(grid), dim3(256), lds, 0, src, C, steps, mfma_iters, pair ? 1 : 0, arrivals, res, sink);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<Result> h(grid);
    CK(hipMemcpy(h.data(), res, grid * sizeof(Result), hipMemcpyDeviceToHost));
    std::vector<int> per_key(CU_KEYS, 0);
    const double bytes = 4.0 * steps * 1024;           // per gathering workgroup
    Row r{0, 0, 0, 0, 0};
    double tg = 0, tm = 0;
    int nm = 0;
    for (auto& x : h) {
        if (x.role == 0) {
            const double s = (double)x.ticks / 100e6;
            r.chip += bytes / s / 1e9;
            tg += s;
            ++r.gatherers;
            if (++per_key[x.key] > 1) ++r.crowded;     // a second gatherer on one CU: the placement assumption failed there
        } else { tm += (double)x.ticks / 100e6; ++nm; }
    }
    r.per_cu = r.gatherers ? r.chip / r.gatherers : 0;
    r.mfma_over_gather = (nm && tg > 0) ? (tm / nm) / (tg / r.gatherers) : 0;
    return r;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int ncu = prop.multiProcessorCount;
    unsigned char* src; int* arrivals; Result* res; float* sink;
    CK(hipMalloc((void**)&src, FOOT + (1 << 16)));
    CK(hipMalloc((void**)&arrivals, CU_KEYS * sizeof(int)));
    CK(hipMalloc((void**)&res, 2 * ncu * sizeof(Result)));
    CK(hipMalloc((void**)&sink, 64));
    std::vector<unsigned short> h((FOOT + (1 << 16)) / 2);
    srand(1);
    for (auto& v : h) v = (unsigned short)(0x3c00 + (rand() & 0x3ff));     // 16-bit values in [1, 2)
    CK(hipMemcpy(src, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    printf("LDS-DMA landing rate by source shape, %d CUs, source footprint %d KiB, %d instructions in flight per wave, 3 repetitions each\n", ncu,
           FOOT >> 10, INFLIGHT);
    printf("%-5s %-6s %-24s %-46s %-30s %s\n", "mode", "C", "shape", "GB/s per CU (3 reps)", "chip-wide TB/s (3 reps)", "gatherers / crowded CUs / MFMA-time : gather-time");
    const char* names[4] = {"(a) 64 px x 16 B", "(b) 32 px x 32 B", "(c) 16 px x 64 B", "(d) 1 KiB contiguous"};
    const int Cs[4] = {64, 256, 512, 1024};
    for (int pair = 0; pair < 2; ++pair)
        for (int ci = 0; ci < 4; ++ci)
            for (int shape = 0; shape < 4; ++shape) {
                Row r[4];
                for (int rep = 0; rep < 4; ++rep) {    // rep 0 warms L2 and the clocks, not reported
                    if (shape == 0) r[rep] = run<0>(src, Cs[ci], ncu, pair, arrivals, res, sink);
                    else if (shape == 1) r[rep] = run<1>(src, Cs[ci], ncu, pair, arrivals, res, sink);
                    else if (shape == 2) r[rep] = run<2>(src, Cs[ci], ncu, pair, arrivals, res, sink);
                    else r[rep] = run<3>(src, Cs[ci], ncu, pair, arrivals, res, sink);
                }
                printf("%-5s %-6d %-24s %7.1f %7.1f %7.1f  (spread %4.1f %%)          %6.2f %6.2f %6.2f            %d / %d / %.1f\n", pair ? "mfma" : "idle",
                       Cs[ci], names[shape], r[1].per_cu, r[2].per_cu, r[3].per_cu,
                       100.0 * (std::max({r[1].per_cu, r[2].per_cu, r[3].per_cu}) - std::min({r[1].per_cu, r[2].per_cu, r[3].per_cu})) / r[1].per_cu,
                       r[1].chip / 1e3, r[2].chip / 1e3, r[3].chip / 1e3, r[3].gatherers, r[3].crowded, r[3].mfma_over_gather);
                fflush(stdout);
            }
    return 0;
}
