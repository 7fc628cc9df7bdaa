// CRAFT's slice5 is MaxPool -> Conv(512 -> 1024, 3x3, dilation 6) -> Conv(1024 -> 1024, 1x1) with no activation and no BatchNorm between or
// behind the two convs, and upconv1 opens with a 1x1 over cat[fc7, relu5_3], linear in fc7 up to its BatchNorm + ReLU: three linear maps in a
// row, which the fast modes run as ONE dilated 3x3 plus the skip half of the 1x1 (detector.cpp::craft_fc_stage):
//
//   u1a = ReLU(Wc (*)dil p5 + Ws s4 + b')      Wc[o][i][tap] = sum_m sum_k Wy[o][m] W7[m][k] W6[k][i][tap]
//                                              b'            = Wy (W7 b6 + b7) + bu
//
// [Wy | Ws] are the two column blocks of upconv1.conv.0 with its BatchNorm folded in (what weights.cpp::fold_conv returns).  fc6's zero padding
// applies to p5 and b6 is added at EVERY pixel, so the identity also holds at the page borders.
// Plain host C++ (no HIP): weights.cpp forms the product once per weight load; tools/fc_fold_hostcheck.cpp checks it against the layer-by-layer
// chain.  Accumulation is in double, A = Wy W7 first and then A W6 (2.9 G multiply-adds at CRAFT's sizes); the column strips fan out over the
// caller's HostPool (sized from the process's CPU share), and every sum runs over k in order, whatever the number of threads.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "hostpool.h"

struct FcFoldDims {
    int Cin, M6, M7, Cout, Cs, taps;      // fc6: Cin -> M6 (taps), fc7: M6 -> M7, the 1x1: [M7 | Cs] -> Cout
};

namespace fc_fold_detail {
constexpr int RB = 4, CB = 8;             // register tile: 4 rows x 8 columns of double accumulators (16 SSE2 registers; measured against
                                          // 4 x 4, 2 x 8, 2 x 16, 8 x 4 and 4 x 16 at the baseline x86-64 target the library is built for)
inline int pad_rows(int M) { return (M + RB - 1) / RB * RB; }

// C [M][N] = A B in double, A given transposed and row-padded: At [K][pad_rows(M)] (zero beyond M), B [K][N] of T.  A task owns a strip of CB
// columns for all M rows: it converts the strip of B to double once (K x CB, 64 KB at K = 1024: it stays in L2 while the rows pass over it)
// and keeps the RB x CB accumulators of a row block in registers over the whole k loop, so that neither C nor B is streamed per row.
template <typename T, typename F>
void gemm(int M, int K, int N, const double* At, const T* B, double* C, F&& parallel) {
    const int Mp = pad_rows(M);
    parallel((N + CB - 1) / CB, [&, M, K, N, Mp](int t) {
        const int c0 = t * CB, nc = std::min(CB, N - c0);
        std::vector<double> strip((size_t)K * CB, 0.0);
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < nc; ++j) strip[(size_t)k * CB + j] = (double)B[(size_t)k * N + c0 + j];
        for (int o0 = 0; o0 < M; o0 += RB) {
            double acc[RB][CB] = {};
            for (int k = 0; k < K; ++k) {
                const double* a = At + (size_t)k * Mp + o0;
                const double* w = strip.data() + (size_t)k * CB;
                for (int r = 0; r < RB; ++r)
                    for (int j = 0; j < CB; ++j) acc[r][j] += a[r] * w[j];
            }
            for (int r = 0; r < RB && o0 + r < M; ++r)
                for (int j = 0; j < nc; ++j) C[(size_t)(o0 + r) * N + c0 + j] = acc[r][j];
        }
    });
}
}  // namespace fc_fold_detail

// w6 [M6][Cin][taps], b6 [M6];  w7 [M7][M6], b7 [M7];  wu [Cout][M7 + Cs], bu [Cout]   ->   wc [Cout][Cin][taps], ws [Cout][Cs], bp [Cout]
// T: float (the library: fp32 tensors in, fp32 tensors out, rounded once from the double sums) or double (the host check: nothing rounded)
template <typename T>
void fc_fold(const FcFoldDims& d, const T* w6, const T* b6, const T* w7, const T* b7, const T* wu, const T* bu, std::vector<T>& wc, std::vector<T>& ws,
             std::vector<T>& bp, HostPool* pool = nullptr) {
    using namespace fc_fold_detail;
    const size_t per = (size_t)d.Cin * d.taps, cu = (size_t)d.M7 + d.Cs;
    const int Mp = pad_rows(d.Cout);
    auto parallel = [&](int n, const std::function<void(int)>& fn) {
        if (pool) pool->parallel_for(n, fn);
        else for (int i = 0; i < n; ++i) fn(i);
    };
    // A = Wy W7 [Cout][M6]
    std::vector<double> Yt((size_t)d.M7 * Mp, 0.0), A((size_t)d.Cout * d.M6, 0.0);
    for (int o = 0; o < d.Cout; ++o)
        for (int m = 0; m < d.M7; ++m) Yt[(size_t)m * Mp + o] = (double)wu[o * cu + m];
    gemm(d.Cout, d.M7, d.M6, Yt.data(), w7, A.data(), parallel);
    // b' = Wy b7 + A b6 + bu, and Ws as it stands
    ws.assign((size_t)d.Cout * d.Cs, T(0));
    bp.assign(d.Cout, T(0));
    for (int o = 0; o < d.Cout; ++o) {
        double s = (double)bu[o];
        for (int m = 0; m < d.M7; ++m) s += (double)wu[o * cu + m] * (double)b7[m];
        for (int k = 0; k < d.M6; ++k) s += A[(size_t)o * d.M6 + k] * (double)b6[k];
        bp[o] = (T)s;
        for (int i = 0; i < d.Cs; ++i) ws[(size_t)o * d.Cs + i] = wu[o * cu + d.M7 + i];
    }
    // Wc = A W6 [Cout][Cin * taps]
    std::vector<double> At((size_t)d.M6 * Mp, 0.0), C((size_t)d.Cout * per, 0.0);
    for (int o = 0; o < d.Cout; ++o)
        for (int k = 0; k < d.M6; ++k) At[(size_t)k * Mp + o] = A[(size_t)o * d.M6 + k];
    gemm(d.Cout, d.M6, (int)per, At.data(), w6, C.data(), parallel);
    wc.resize(C.size());
    for (size_t i = 0; i < C.size(); ++i) wc[i] = (T)C[i];
}
