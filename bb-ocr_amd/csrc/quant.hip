// rec_quant: the sequence half of the recogniser in torch's x86 / fbgemm DYNAMIC int8 arithmetic (what easyocr's quantize=True runs on a CPU
// device: torch.quantization.quantize_dynamic over both nn.LSTMs, the two nn.Linears behind them and Prediction), per crop.
//
// One quantised matrix product over a tensor X (a crop's [T, K] rows, or the 256 values of h of one direction at one step):
//   mn = min(min X, 0), mx = max(max X, 0); scale = (double(mx) - mn) / 127, replaced by 0.1 where float(scale) == 0 or 1 / float(scale) is inf;
//   zero point = fbgemm ChooseQuantizationParams(qmin 0, qmax 127) in double; inv = 1.0f / float(scale);
//   code = clamp(nearbyint(fmaf(x, inv, zp)), 0, 255) (fbgemm clamps to uint8; 128 is the largest code that occurs, code - zp fits a byte);  acc = sum (code - zp) * q_w  (int32, v_mfma_i32_16x16x64_i8);
//   out = fmaf(float(acc), float(scale) * scale_w, bias).
// Weights: symmetric qint8 per tensor (weights.cpp::quantize_weight_q8), packed as B fragments of the MFMA: lane l of fragment (n-block nf,
// k-block kc) holds q[nf * 16 + (l & 15)][kc * 64 + 16 * (l >> 4) + j], j = 0..15 (16 B).  A fragments use the same k map (lane l: row l & 15),
// so the sum over k does not depend on how the instruction orders k inside a lane group.
#include "common.h"
#include "kernels.h"
#include <math.h>

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {

struct Q8Params { float scale, inv, zp; };

// ChooseQuantizationParams(min, max, 0, 127) of fbgemm, and the float inverse its Quantize uses
__device__ __forceinline__ Q8Params q8_choose(float mn, float mx) {
    mn = fminf(mn, 0.f);
    mx = fmaxf(mx, 0.f);
    double scale = ((double)mx - (double)mn) / 127.0;
    if ((float)scale == 0.0f || isinf(1.0f / (float)scale)) scale = 0.1;
    const double zmin = 0.0 - (double)mn / scale, zmax = 127.0 - (double)mx / scale;
    const double emin = fabs((double)mn / scale), emax = 127.0 + fabs((double)mx / scale);
    const double z = emin < emax ? zmin : zmax;
    const double zp = z < 0.0 ? 0.0 : (z > 127.0 ? 127.0 : nearbyint(z));
    Q8Params p;
    p.scale = (float)scale;
    p.inv = 1.0f / p.scale;
    p.zp = (float)zp;
    return p;
}
__device__ __forceinline__ float q8_code(float x, const Q8Params& p) { return fminf(fmaxf(rintf(fmaf(x, p.inv, p.zp)), 0.f), 255.f); }

// SRC 0: fp32 [rows, K]; SRC 1: the exact mode's pair [rows, K hi | K lo] fp16 with value = hi + lo / SPLIT_LO_SCALE
template <int SRC> __device__ __forceinline__ f32x4 q8_load4(const void* x, size_t row, int K, int k) {
    if constexpr (SRC == 0) {
        return *(const f32x4*)((const float*)x + row * K + k);
    } else {
        const uint16_t* p = (const uint16_t*)x + row * 2 * K + k;
        const u32x2 h = *(const u32x2*)p, l = *(const u32x2*)(p + K);
        const f32x2_t h0 = El<1>::unpack2(h[0]), h1 = El<1>::unpack2(h[1]), l0 = El<1>::unpack2(l[0]), l1 = El<1>::unpack2(l[1]);
        const float inv = 1.0f / SPLIT_LO_SCALE;
        return (f32x4){h0[0] + l0[0] * inv, h0[1] + l0[1] * inv, h1[0] + l1[0] * inv, h1[1] + l1[1] * inv};
    }
}

// ---- parameter pass: one workgroup per segment (crop) {first row, T}: min / max over its T x K values -> rowp[row] = {scale, inv, zp, 0} for
// each of its rows, segp[seg] = {scale, zp} (optional)
template <int SRC>
__global__ void __launch_bounds__(256) q8_params_kernel(const void* __restrict__ x, int K, const int2* __restrict__ seqs, float4* __restrict__ rowp,
                                                        float2* __restrict__ segp) {
    __shared__ float smn[4], smx[4];
    __shared__ Q8Params sp;
    const int2 sq = seqs[blockIdx.x];
    const int k4 = K >> 2, total = sq.y * k4;
    float mn = 0.f, mx = 0.f;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int t = i / k4, k = (i - t * k4) * 4;
        const f32x4 v = q8_load4<SRC>(x, (size_t)sq.x + t, K, k);
        mn = fminf(mn, fminf(fminf(v[0], v[1]), fminf(v[2], v[3])));
        mx = fmaxf(mx, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sp = q8_choose(fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3])), fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3])));
        if (segp) segp[blockIdx.x] = make_float2(sp.scale, sp.zp);
    }
    __syncthreads();
    const Q8Params p = sp;
    for (int t = threadIdx.x; t < sq.y; t += 256) rowp[(size_t)sq.x + t] = make_float4(p.scale, p.inv, p.zp, 0.f);
}

// ---- coding pass: a8[row][k] = code - zp (signed byte, the MFMA's A operand), codes[row][k] = code (optional); rows in [rows, rows_pad) are
// cleared and get scale 0
template <int SRC>
__global__ void __launch_bounds__(256) q8_code_kernel(const void* __restrict__ x, int K, size_t rows, size_t rows_pad, float4* __restrict__ rowp,
                                                      int8_t* __restrict__ a8, uint8_t* __restrict__ codes) {
    const int k4 = K >> 2;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_pad * k4) return;
    const size_t row = i / k4;
    const int k = (int)(i - row * k4) * 4;
    unsigned int packed = 0;
    if (row < rows) {
        const float4 rp = rowp[row];
        const Q8Params p{rp.x, rp.y, rp.z};
        const f32x4 v = q8_load4<SRC>(x, row, K, k);
        unsigned int cd = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (int)q8_code(v[j], p);
            cd |= (unsigned int)c << (8 * j);
            packed |= (unsigned int)((c - (int)p.zp) & 0xff) << (8 * j);
        }
        if (codes) *(unsigned int*)(codes + row * K + k) = cd;
    } else if (k == 0) {
        rowp[row] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    *(unsigned int*)(a8 + row * K + k) = packed;
}

// ---- int8 GEMM: out[row][col] = fmaf(float(sum_k a8[row][k] q[col][k]), rowp[row].scale * wscale[col / 16], bias[col]).
// Workgroup = 4 waves = 64 rows x NF 16-column fragments; the NF x K/64 weight fragments of the column block are staged in LDS once (they
// are contiguous in the packed image) and shared by the four waves; every wave owns 16 rows, whose A fragments it reads straight from the
// row-major int8 tensor (16 B per lane).  rows_pad % 64 == 0; K % 64 == 0, K <= 512.
constexpr int Q8_LDS = 4 * 8 * 1024;          // NF 4 x K 512, or NF 7 x K 256 (28 KB)
template <int NF>
__global__ void __launch_bounds__(256) q8_gemm_kernel(const int8_t* __restrict__ a8, int K, const int8_t* __restrict__ wpk, const float4* __restrict__ rowp,
                                                      const float* __restrict__ wscale, const float* __restrict__ bias, float* __restrict__ out, int ldo,
                                                      int ncols) {
    __shared__ __attribute__((aligned(16))) unsigned char wl[Q8_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KC = K >> 6, nf0 = blockIdx.y * NF;
    const u32x4* src = (const u32x4*)(wpk + (size_t)nf0 * KC * 1024);
    for (int i = tid; i < NF * KC * 64; i += 256) ((u32x4*)wl)[i] = src[i];
    __syncthreads();
    const size_t row0 = (size_t)blockIdx.x * 64 + wave * 16;
    const int8_t* ap = a8 + (row0 + (lane & 15)) * K + 16 * (lane >> 4);
    i32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = (i32x4){0, 0, 0, 0};
    for (int kc = 0; kc < KC; ++kc) {
        const i32x4 a = *(const i32x4*)(ap + kc * 64);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const i32x4 b = ((const i32x4*)wl)[(f * KC + kc) * 64 + lane];
            acc[f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[f], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t row = row0 + 4 * (lane >> 4) + r;
        const float rs = rowp[row].x;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int col = (nf0 + f) * 16 + (lane & 15);
            if (col < ncols) out[row * ldo + col] = fmaf((float)acc[f][r], rs * wscale[nf0 + f], bias[col]);
        }
    }
}

// ---- the recurrence.  One workgroup = up to 16 sequences (each with its own T) x one direction, 8 waves; wave w owns hidden units
// [32w, 32w + 32) and all four of their gates (fragment (a, gate): lane l holds unit 32w + 16a + (l & 15) for sequences 4 (l >> 4) + r), and
// keeps its 32 W_hh fragments (4 k-blocks x 2 x 4, 128 registers) for all T steps.  c and h stay in fp32 registers.  Per step:
//   min / max of h per sequence (16-lane butterflies, then across the waves through LDS) | barrier | parameters (every wave, for sequence
//   lane & 15; the lanes fetch those of their four sequences by shuffle) and h's codes - zp into LDS [sequence][256 B] | barrier |
//   32 MFMAs | fmaf(acc, scale_h * scale_w, b_hh) + G[t] | gates (expf / tanhf, IEEE division, as lstm_exact_kernel).
// G: fp32 [rows, 2048], column dir * 1024 + gate * 256 + unit (torch's own row order of weight_ih).  Every loop is bounded by the tile's
// longest T; a sequence past its own T neither loads nor stores.
constexpr int LQ_STRIDE = 272;                 // bytes per sequence row of the code image: 256 + 16 (conflict-free 16-byte fragment reads)
__global__ void __launch_bounds__(512, 1) lstm_q8_kernel(const float* __restrict__ G, const int8_t* __restrict__ whh, const float* __restrict__ whh_scale,
                                                         const float* __restrict__ bhh, float* __restrict__ out, const int2* __restrict__ seqs,
                                                         const int4* __restrict__ tiles, float* __restrict__ c_out, uint8_t* __restrict__ hcodes,
                                                         float2* __restrict__ hparams) {
    __shared__ __attribute__((aligned(16))) unsigned char hq[16 * LQ_STRIDE];
    __shared__ float red[2][8][16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dir = blockIdx.y;
    const int4 tile = tiles[blockIdx.x];
    const int s0 = tile.x, n = tile.y;
    const int g = lane >> 4, u = lane & 15;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) Tmax = max(Tmax, seqs[s0 + i].y);
    int Ts[4], row0[4];                            // Ts = 0: no such sequence in this tile (its lanes compute on zeros and never store)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int s = g * 4 + r;
        const int2 sq = seqs[s0 + (s < n ? s : n - 1)];
        row0[r] = sq.x;
        Ts[r] = s < n ? sq.y : 0;
    }
    i32x4 w[4][2][4];
    {
        const i32x4* wp = (const i32x4*)whh + ((size_t)(dir * 8 + wave) * 32) * 64 + lane;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) w[kk][a][q] = wp[(size_t)((kk * 2 + a) * 4 + q) * 64];
    }
    const float ws = whh_scale[dir];
    float bh[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) bh[a][q] = bhh[dir * 1024 + q * 256 + wave * 32 + a * 16 + u];
    float h[2][4], c[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[a][r] = c[a][r] = 0.f;
    for (int step = 0; step < Tmax; ++step) {
        // 1. min / max of h over the 256 units of each sequence
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mn = fminf(h[0][r], h[1][r]), mx = fmaxf(h[0][r], h[1][r]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                mn = fminf(mn, __shfl_xor(mn, o));
                mx = fmaxf(mx, __shfl_xor(mx, o));
            }
            if (u == 0) { red[0][wave][g * 4 + r] = mn; red[1][wave][g * 4 + r] = mx; }
        }
        __syncthreads();
        // 2. parameters of sequence lane & 15, then those of the lane's own four sequences
        float mn = red[0][0][u], mx = red[1][0][u];
#pragma unroll
        for (int k = 1; k < 8; ++k) { mn = fminf(mn, red[0][k][u]); mx = fmaxf(mx, red[1][k][u]); }
        const Q8Params mine = q8_choose(mn, mx);
        Q8Params p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r].scale = __shfl(mine.scale, g * 4 + r);
            p[r].inv = __shfl(mine.inv, g * 4 + r);
            p[r].zp = __shfl(mine.zp, g * 4 + r);
        }
        // 3. codes of h
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = step < Ts[r];
            const size_t row = (size_t)(row0[r] + (dir ? Ts[r] - 1 - step : step));
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int unit = wave * 32 + a * 16 + u;
                const int cd = (int)q8_code(h[a][r], p[r]);
                hq[(g * 4 + r) * LQ_STRIDE + unit] = (unsigned char)((cd - (int)p[r].zp) & 0xff);
                if (hcodes && on) hcodes[row * 512 + dir * 256 + unit] = (uint8_t)cd;
            }
            if (hparams && on && wave == 0 && u == 0) hparams[row * 2 + dir] = make_float2(p[r].scale, p[r].zp);
        }
        __syncthreads();
        // 4. acc = (codes - zp) W_hh^T
        i32x4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[a][q] = (i32x4){0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const i32x4 af = *(const i32x4*)(hq + u * LQ_STRIDE + kk * 64 + 16 * g);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, w[kk][a][q], acc[a][q], 0, 0, 0);
        }
        // 5.-7. gates
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (step >= Ts[r]) continue;
            const size_t row = (size_t)(row0[r] + (dir ? Ts[r] - 1 - step : step));
            const float mult = p[r].scale * ws;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int unit = wave * 32 + a * 16 + u;
                const float* gp = G + row * 2048 + dir * 1024 + unit;
                auto pre = [&](int q) { return gp[q * 256] + fmaf((float)acc[a][q][r], mult, bh[a][q]); };
                const float gi = 1.0f / (1.0f + expf(-pre(0)));
                const float gf = 1.0f / (1.0f + expf(-pre(1)));
                const float gg = tanhf(pre(2));
                const float go = 1.0f / (1.0f + expf(-pre(3)));
                const float cn = gf * c[a][r] + gi * gg;
                c[a][r] = cn;
                const float hv = go * tanhf(cn);
                h[a][r] = hv;
                out[row * 512 + dir * 256 + unit] = hv;
                if (c_out) c_out[row * 512 + dir * 256 + unit] = cn;
            }
        }
    }
}

}  // namespace

size_t q8_packed_bytes(int N, int K) { return (size_t)((N + 15) / 16) * (K / 64) * 1024; }

// q: int8 [N][K] (row n = output column n) -> B fragments [ceil(N / 16)][K / 64][lane 64][16]; rows past N are zero
void pack_q8_weights(const int8_t* q, int N, int K, int8_t* out) {
    const int NFt = (N + 15) / 16, KC = K / 64;
    for (int nf = 0; nf < NFt; ++nf)
        for (int kc = 0; kc < KC; ++kc)
            for (int l = 0; l < 64; ++l) {
                const int nrow = nf * 16 + (l & 15);
                for (int j = 0; j < 16; ++j)
                    out[(((size_t)nf * KC + kc) * 64 + l) * 16 + j] = nrow < N ? q[(size_t)nrow * K + kc * 64 + 16 * (l >> 4) + j] : (int8_t)0;
            }
}

// W_hh of both directions, int8 [1024][256] each -> [dir][wave 8][k-block 4][a 2][gate 4][lane 64][16] (lstm_q8_kernel)
void pack_q8_whh(const int8_t* q_fwd, const int8_t* q_bwd, int8_t* out) {
    size_t o = 0;
    for (int d = 0; d < 2; ++d) {
        const int8_t* q = d ? q_bwd : q_fwd;
        for (int w = 0; w < 8; ++w)
            for (int kk = 0; kk < 4; ++kk)
                for (int a = 0; a < 2; ++a)
                    for (int gate = 0; gate < 4; ++gate)
                        for (int l = 0; l < 64; ++l) {
                            const int row = gate * 256 + w * 32 + a * 16 + (l & 15);
                            for (int j = 0; j < 16; ++j) out[o++] = q[(size_t)row * 256 + kk * 64 + 16 * (l >> 4) + j];
                        }
    }
}

hipError_t launch_q8_quantize(const void* x, int src_pair, int K, size_t rows, size_t rows_pad, const int* seqs_dev, int nseq, float* rowp, int8_t* a8,
                              uint8_t* codes, float* segp, hipStream_t s) {
    if (nseq <= 0 || rows == 0) return hipSuccess;
    if ((K & 63) || K > 512 || rows > rows_pad || (rows_pad & 63)) return hipErrorInvalidValue;
    const unsigned int blocks = (unsigned int)((rows_pad * (size_t)(K / 4) + 255) / 256);
    if (src_pair) {
        hipLaunchKernelGGL(q8_params_kernel<1>, dim3(nseq), dim3(256), 0, s, x, K, (const int2*)seqs_dev, (float4*)rowp, (float2*)segp);
        hipLaunchKernelGGL(q8_code_kernel<1>, dim3(blocks), dim3(256), 0, s, x, K, rows, rows_pad, (float4*)rowp, a8, codes);
    } else {
        hipLaunchKernelGGL(q8_params_kernel<0>, dim3(nseq), dim3(256), 0, s, x, K, (const int2*)seqs_dev, (float4*)rowp, (float2*)segp);
        hipLaunchKernelGGL(q8_code_kernel<0>, dim3(blocks), dim3(256), 0, s, x, K, rows, rows_pad, (float4*)rowp, a8, codes);
    }
    return hipGetLastError();
}

hipError_t launch_q8_gemm(const int8_t* a8, size_t rows_pad, int K, const int8_t* wpk, int N, const float* rowp, const float* wscale, const float* bias,
                          float* out, int ldo, hipStream_t s) {
    if (rows_pad == 0) return hipSuccess;
    const int NFt = (N + 15) / 16;
    if ((K & 63) || K > 512 || (rows_pad & 63) || ldo < N) return hipErrorInvalidValue;
    if (NFt % 4 == 0) {
        hipLaunchKernelGGL(q8_gemm_kernel<4>, dim3((unsigned int)(rows_pad / 64), NFt / 4), dim3(256), 0, s, a8, K, wpk, (const float4*)rowp, wscale, bias,
                           out, ldo, N);
    } else if (NFt == 7 && K <= 256) {
        hipLaunchKernelGGL(q8_gemm_kernel<7>, dim3((unsigned int)(rows_pad / 64), 1), dim3(256), 0, s, a8, K, wpk, (const float4*)rowp, wscale, bias, out,
                           ldo, N);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_lstm_q8(const float* G, const int8_t* whh_pk, const float* whh_scale, const float* bhh, float* out, const int* seqs_dev,
                          const int* tiles_dev, int ntiles, float* c_out, uint8_t* hcodes, float* hparams, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(lstm_q8_kernel, dim3(ntiles, 2), dim3(512), 0, s, G, whh_pk, whh_scale, bhh, out, (const int2*)seqs_dev, (const int4*)tiles_dev,
                       c_out, hcodes, (float2*)hparams);
    return hipGetLastError();
}
