// Prediction (Linear 256 -> C) + softmax + ignore mask + renormalisation + arg-max of a greedy recognition pass as ONE kernel, for recognisers
// of more than 128 classes (latin_g2 352 ... zh_sim_g2 6,719).
//
// Why: the unfused route (crnn_seq_pred + ctc_rows_wide_kernel) writes and re-reads C fp32 logits per time step -- 54 KB per row at 6,719
// classes, 40 GB for a full sequence pass of 1.5 M rows -- for a stage whose result is 8 bytes per row.  Here no logit and no probability
// reaches memory.
//
// Shape.  A workgroup of 4 waves owns kPredCtcRows = 64 rows of x [rows, 256] and keeps them in registers for the whole kernel, as the B
// operands of v_mfma_f32_16x16x32_{f16,bf16}: 4 row fragments x 8 k-steps x 4 VGPRs = 128 VGPRs per lane, the same in every wave.  The class axis
// is cut into fragments of 16 classes (the MFMA's M); wave w takes fragments w, w + 4, ...  One fragment = 8 A operands of 1 KB each, packed
// at load so that a lane's 16 bytes are contiguous (pack_pred_ctc_weights), double-buffered in 2 x 32 VGPRs, and 32 MFMAs.  The D fragment of
// (class fragment f, row fragment t) holds, in lane l, row 16 t + (l & 15) and classes 16 f + 4 (l >> 4) + {0, 1, 2, 3}: a lane only ever sees
// ONE row per row fragment, so the running softmax state lives in registers per lane -- 4 x {max, sum over all classes, sum over the
// unmasked ones, best unmasked logit, its class} = 20 VGPRs -- and nothing crosses lanes until the end: two xor steps (16, 32) merge the
// four class groups of a wave, 5 KB of LDS merge the four waves.  Budget: ~250 of the 512 VGPRs a 256-thread workgroup may use, 5 KB of the
// 160 KB of LDS; the packed matrix (3.4 MB at 6,719 classes) is just inside an XCD's 4 MiB of L2, from which every workgroup streams it once.
//
// Arithmetic.  logit = acc + bias with acc the fp32 MFMA accumulation over k = 0 .. 255 in ascending k-steps from a zero accumulator (the
// order of the conv plan the unfused route runs).  The sums are rescaled sums: whenever a lane's maximum grows, both are multiplied by
// expf(old - new).  Classes >= C never take part; masked classes take part in the maximum and in the sum over all classes only.  Among equal
// logits the lowest class wins: a lane meets its classes in ascending order and takes a strictly larger one only, and every merge prefers the
// lower class on equality.  pmax = (e_best / sum_all) / (sum_unmasked / sum_all), e_best = expf(best - max), in that order of operations.
#include "bbocr.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int MT = kPredCtcRows / 16;      // row fragments per workgroup
constexpr int KS = 256 / 32;               // k-steps of a fragment

struct SoftState {
    float m, s_all, s_un, bv;
    int bi;
};

// b folded into a: both describe disjoint class sets of the same row
__device__ __forceinline__ void soft_merge(SoftState& a, const SoftState& b) {
    const float M = fmaxf(a.m, b.m);
    const float fa = a.m == M ? 1.f : expf(a.m - M), fb = b.m == M ? 1.f : expf(b.m - M);     // an empty set has m = -inf and sums 0
    a.s_all = a.s_all * fa + b.s_all * fb;
    a.s_un = a.s_un * fa + b.s_un * fb;
    a.m = M;
    if (b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi)) { a.bv = b.bv; a.bi = b.bi; }
}

template <int EL>
__global__ void __launch_bounds__(256) pred_ctc_kernel(const uint16_t* __restrict__ x, size_t rows, const uint16_t* __restrict__ wpk,
                                                       const float* __restrict__ bias, int C, int NF, const unsigned int* __restrict__ mask,
                                                       int* __restrict__ idx, float* __restrict__ pmax) {
    typedef typename El<EL>::v8 v8;
    __shared__ SoftState merge[4][kPredCtcRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)blockIdx.x * kPredCtcRows;

    v8 xf[MT][KS];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const size_t row = row0 + t * 16 + n;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            u32x4 q = {0u, 0u, 0u, 0u};
            if (row < rows) q = *(const u32x4*)(x + row * 256 + k * 32 + g * 8);
            xf[t][k] = __builtin_bit_cast(v8, q);
        }
    }

    SoftState st[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) st[t] = SoftState{-INFINITY, 0.f, 0.f, -INFINITY, 0x7fffffff};

    auto load_a = [&](int f, v8 (&a)[KS]) {
        const u32x4* src = (const u32x4*)(wpk + ((size_t)f * KS * 64 + lane) * 8);
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = __builtin_bit_cast(v8, src[k * 64]);
    };
    v8 a_cur[KS], a_nxt[KS];
    if (wave < NF) load_a(wave, a_cur);
    for (int f = wave; f < NF; f += 4) {
        const bool more = f + 4 < NF;                    // wave-uniform
        if (more) load_a(f + 4, a_nxt);
        f32x4 acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = El<EL>::mfma(a_cur[k], xf[t][k], acc[t]);
        const int c0 = f * 16 + g * 4;                   // this lane's four classes: c0 .. c0 + 3, inside one mask word
        const f32x4 b4 = *(const f32x4*)(bias + c0);     // padded to NF * 16
        const unsigned int mw = (mask && c0 < C) ? (mask[c0 >> 5] >> (c0 & 31)) : 0u;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            float v[4];
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = c0 + r < C ? acc[t][r] + b4[r] : -INFINITY;
                tm = fmaxf(tm, v[r]);
            }
            SoftState& s = st[t];
            if (tm > s.m) {                              // (never with tm = -inf: nothing to add then)
                const float sc = expf(s.m - tm);         // first time: expf(-inf) = 0 on sums that are 0
                s.s_all *= sc;
                s.s_un *= sc;
                s.m = tm;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!(v[r] > -INFINITY)) continue;       // a class behind C, or a logit of -inf: contributes exactly 0
                const float e = expf(v[r] - s.m);
                s.s_all += e;
                if (!((mw >> r) & 1u)) {
                    s.s_un += e;
                    if (v[r] > s.bv) { s.bv = v[r]; s.bi = c0 + r; }
                }
            }
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < KS; ++k) a_cur[k] = a_nxt[k];
        }
    }

    // the four class groups of a wave (lanes n, n + 16, n + 32, n + 48), then the four waves
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            SoftState b;
            b.m = __shfl_xor(st[t].m, o);
            b.s_all = __shfl_xor(st[t].s_all, o);
            b.s_un = __shfl_xor(st[t].s_un, o);
            b.bv = __shfl_xor(st[t].bv, o);
            b.bi = __shfl_xor(st[t].bi, o);
            soft_merge(st[t], b);                        // symmetric in its operands (no contraction): both partners hold the same floats
        }
        if (g == 0) merge[wave][t * 16 + n] = st[t];
    }
    __syncthreads();
    if (threadIdx.x < kPredCtcRows) {
        const size_t row = row0 + threadIdx.x;
        SoftState a = merge[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) soft_merge(a, merge[w][threadIdx.x]);
        if (row < rows) {
            const float e_best = expf(a.bv - a.m);
            idx[row] = a.bi < C ? a.bi : 0;              // a row of NaNs compares to nothing: the blank, never a class outside the table
            pmax[row] = (e_best / a.s_all) / (a.s_un / a.s_all);
        }
    }
}

}  // namespace

size_t pred_ctc_packed_elems(int C) { return (size_t)((C + 15) / 16) * KS * 64 * 8; }
size_t pred_ctc_bias_elems(int C) { return (size_t)((C + 15) / 16) * 16; }

// A operand of v_mfma_f32_16x16x32: lane l holds A[row l & 15][k = 8 (l >> 4) + j], j = 0 .. 7; fragment f, k-step ks at ((f * 8 + ks) * 64 + l) * 8
void pack_pred_ctc_weights(int el, const float* w, const float* b, int C, uint16_t* wpk, float* bias) {
    const int NF = (C + 15) / 16;
    size_t o = 0;
    for (int f = 0; f < NF; ++f)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int c = f * 16 + (l & 15);
                for (int j = 0; j < 8; ++j) {
                    const int k = ks * 32 + 8 * (l >> 4) + j;
                    wpk[o++] = f32_to_el_host(el, c < C ? w[(size_t)c * 256 + k] : 0.f);
                }
            }
    for (int c = 0; c < NF * 16; ++c) bias[c] = c < C ? b[c] : 0.f;
}

hipError_t launch_pred_ctc(int el, const uint16_t* x, size_t rows, const uint16_t* wpk, const float* bias, int C, const unsigned int* mask_dev,
                           int* idx, float* pmax, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if (!x || !wpk || !bias || !idx || !pmax || C < 2 || C > BBOCR_REC_CLASSES_MAX) return hipErrorInvalidValue;
    const size_t blocks = (rows + kPredCtcRows - 1) / kPredCtcRows;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const int NF = (C + 15) / 16;
    if (el) hipLaunchKernelGGL(pred_ctc_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, wpk, bias, C, NF, mask_dev, idx, pmax);
    else hipLaunchKernelGGL(pred_ctc_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, x, rows, wpk, bias, C, NF, mask_dev, idx, pmax);
    return hipGetLastError();
}
