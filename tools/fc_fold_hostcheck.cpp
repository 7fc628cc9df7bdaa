// The fold of fc6 -> fc7 -> upconv1's 1x1 (csrc/fc_fold.h) as a stand-alone host program: small random chains (Cin 8, mids 12 and 10, Cout 6,
// 5 skip channels, a BatchNorm with non-trivial running statistics behind the 1x1, dilation 2) on a 7 x 9 and a 3 x 2 image (width below the
// dilation).  The folded stage -- ONE dilated 3x3 with Wc, plus Ws s4 + b' -- must equal the layer-by-layer chain in double within 1e-12 of
// the largest pre-activation, with the fold's rows fanned out over a HostPool and without one; and each of four mistakes must be SEEN by
// that same comparison (> 1e-6) on both images:
//     W7 b6 left out of b';  the BatchNorm scale applied to the Ws block only;  the Wy and Ws columns swapped;  the taps transposed.
// Last, the float instantiation the library runs: its outputs are the double fold's, rounded once.
// One line per check, "ok" / "FAIL" first; exit status 1 when any failed.  tests/test_fc_fold_cpu.py builds it twice (plain, and with
// -fsanitize=address,undefined) and runs both.  No GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../bb-ocr_amd/csrc/fc_fold.h"

namespace {
using Vec = std::vector<double>;
constexpr int CIN = 8, M6 = 12, M7 = 10, COUT = 6, CS = 5, DIL = 2;

uint64_t g_state = 0x9e3779b97f4a7c15ULL;
double rnd() {      // xorshift64*, uniform in [-1, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1DULL) >> 11) / (double)(1ULL << 52) - 1.0;
}
Vec randv(size_t n, double scale = 1.0) { Vec v(n); for (double& x : v) x = rnd() * scale; return v; }

struct Chain {
    Vec w6, b6, w7, b7, wu, bu, g, be, mu, var;      // wu [COUT][M7 + CS], bu: the 1x1 BEFORE its BatchNorm
};
Chain make_chain() {
    Chain c;
    c.w6 = randv((size_t)M6 * CIN * 9, 0.3); c.b6 = randv(M6, 0.5);
    c.w7 = randv((size_t)M7 * M6, 0.4); c.b7 = randv(M7, 0.5);
    c.wu = randv((size_t)COUT * (M7 + CS), 0.4); c.bu = randv(COUT, 0.5);
    c.g = randv(COUT); c.be = randv(COUT); c.mu = randv(COUT, 0.7); c.var = randv(COUT);
    for (int o = 0; o < COUT; ++o) { c.g[o] = 0.6 + 0.5 * std::fabs(c.g[o]) * (o & 1 ? -1.0 : 1.0); c.var[o] = 0.3 + 1.5 * std::fabs(c.var[o]); }
    return c;
}

// x [C][H][W] -> [Cout][H][W]: 3x3, dilation and zero padding DIL, w [Cout][C][9] (tap = ky * 3 + kx), b may be null
Vec dilconv(const Vec& x, int C, int H, int W, const Vec& w, int Cout, const double* b) {
    Vec y((size_t)Cout * H * W, 0.0);
    for (int o = 0; o < Cout; ++o)
        for (int yy = 0; yy < H; ++yy)
            for (int xx = 0; xx < W; ++xx) {
                double s = b ? b[o] : 0.0;
                for (int i = 0; i < C; ++i)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int sy = yy + (ky - 1) * DIL, sx = xx + (kx - 1) * DIL;
                            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
                            s += w[((size_t)o * C + i) * 9 + ky * 3 + kx] * x[((size_t)i * H + sy) * W + sx];
                        }
                y[((size_t)o * H + yy) * W + xx] = s;
            }
    return y;
}
// y[o] = sum_i w[o][off + i] x[i] (+ b[o]) per pixel; w rows are `stride` long
Vec conv1x1(const Vec& x, int C, int HW, const Vec& w, int stride, int off, int Cout, const double* b) {
    Vec y((size_t)Cout * HW, 0.0);
    for (int o = 0; o < Cout; ++o)
        for (int p = 0; p < HW; ++p) {
            double s = b ? b[o] : 0.0;
            for (int i = 0; i < C; ++i) s += w[(size_t)o * stride + off + i] * x[(size_t)i * HW + p];
            y[(size_t)o * HW + p] = s;
        }
    return y;
}

// the pre-activation of upconv1's first block, layer by layer: fc6, fc7, the 1x1 over cat[f7, s4], its BatchNorm (eval mode)
Vec chain_ref(const Chain& c, const Vec& p5, const Vec& s4, int H, int W) {
    const Vec f6 = dilconv(p5, CIN, H, W, c.w6, M6, c.b6.data());
    const Vec f7 = conv1x1(f6, M6, H * W, c.w7, M6, 0, M7, c.b7.data());
    Vec y = conv1x1(f7, M7, H * W, c.wu, M7 + CS, 0, COUT, c.bu.data());
    const Vec ys = conv1x1(s4, CS, H * W, c.wu, M7 + CS, M7, COUT, nullptr);
    for (int o = 0; o < COUT; ++o)
        for (int p = 0; p < H * W; ++p) {
            double& v = y[(size_t)o * H * W + p];
            v = (v + ys[(size_t)o * H * W + p] - c.mu[o]) / std::sqrt(c.var[o] + 1e-5) * c.g[o] + c.be[o];
        }
    return y;
}

enum Mistake { NONE, NO_W7B6, BN_WS_ONLY, COLS_SWAPPED, TAPS_TRANSPOSED, N_MISTAKES };
const char* kNames[] = {"the fold", "W7 b6 left out of b'", "BN scale on the Ws block only", "Wy and Ws columns swapped", "taps transposed"};

struct Folded { Vec wc, ws, bp; };
Folded fold(const Chain& c, Mistake m, HostPool* pool) {
    // BatchNorm folded into the 1x1, as weights.cpp::fold_conv does
    Vec wu = c.wu, bu(COUT);
    for (int o = 0; o < COUT; ++o) {
        const double sc = c.g[o] / std::sqrt(c.var[o] + 1e-5);
        for (int i = 0; i < M7 + CS; ++i)
            if (m != BN_WS_ONLY || i >= M7) wu[(size_t)o * (M7 + CS) + i] *= sc;
        bu[o] = (c.bu[o] - c.mu[o]) * sc + c.be[o];
    }
    if (m == COLS_SWAPPED) {        // the row handed over as [Ws | Wy]
        for (int o = 0; o < COUT; ++o) {
            double* r = wu.data() + (size_t)o * (M7 + CS);
            Vec t(r, r + M7 + CS);
            for (int i = 0; i < CS; ++i) r[i] = t[M7 + i];
            for (int i = 0; i < M7; ++i) r[CS + i] = t[i];
        }
    }
    const Vec zero(M6, 0.0);
    Folded f;
    const FcFoldDims d{CIN, M6, M7, COUT, CS, 9};
    fc_fold<double>(d, c.w6.data(), (m == NO_W7B6 ? zero : c.b6).data(), c.w7.data(), c.b7.data(), wu.data(), bu.data(), f.wc, f.ws, f.bp, pool);
    if (m == TAPS_TRANSPOSED) {
        const Vec t = f.wc;
        for (size_t oi = 0; oi < (size_t)COUT * CIN; ++oi)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) f.wc[oi * 9 + ky * 3 + kx] = t[oi * 9 + kx * 3 + ky];
    }
    return f;
}
// what craft_fc_stage computes before its ReLU: z = Wc (*) p5, then z + Ws s4 + b'
Vec folded_out(const Folded& f, const Vec& p5, const Vec& s4, int H, int W) {
    Vec z = dilconv(p5, CIN, H, W, f.wc, COUT, nullptr);
    const Vec ys = conv1x1(s4, CS, H * W, f.ws, CS, 0, COUT, f.bp.data());
    for (size_t i = 0; i < z.size(); ++i) z[i] += ys[i];
    return z;
}
double rel_err(const Vec& a, const Vec& ref) {
    double e = 0, m = 0;
    for (size_t i = 0; i < a.size(); ++i) { e = std::max(e, std::fabs(a[i] - ref[i])); m = std::max(m, std::fabs(ref[i])); }
    return e / m;
}
}  // namespace

int main() {
    int failures = 0;
    auto report = [&](bool ok, const char* what, const char* where, double v) {
        std::printf("%s %s, %s: %.3e\n", ok ? "ok" : "FAIL", what, where, v);
        failures += !ok;
    };
    HostPool pool(3);
    const Chain c = make_chain();
    const int shapes[2][2] = {{7, 9}, {3, 2}};
    for (const auto& s : shapes) {
        const int H = s[0], W = s[1];
        char where[32];
        std::snprintf(where, sizeof where, "%d x %d", H, W);
        const Vec p5 = randv((size_t)CIN * H * W), s4 = randv((size_t)CS * H * W);
        const Vec ref = chain_ref(c, p5, s4, H, W);
        const double e_pool = rel_err(folded_out(fold(c, NONE, &pool), p5, s4, H, W), ref);
        const double e_serial = rel_err(folded_out(fold(c, NONE, nullptr), p5, s4, H, W), ref);
        report(e_pool <= 1e-12, "the fold over a pool against the chain in double (<= 1e-12)", where, e_pool);
        report(e_serial <= 1e-12, "the fold on one thread against the chain in double (<= 1e-12)", where, e_serial);
        for (int m = NONE + 1; m < N_MISTAKES; ++m) {
            const double e = rel_err(folded_out(fold(c, (Mistake)m, &pool), p5, s4, H, W), ref);
            char what[96];
            std::snprintf(what, sizeof what, "mistake seen (> 1e-6): %s", kNames[m]);
            report(e > 1e-6, what, where, e);
        }
    }
    {   // the float instantiation: every output is the double fold's value of the float inputs, rounded once
        auto tof = [](const Vec& v) { return std::vector<float>(v.begin(), v.end()); };
        auto tod = [](const std::vector<float>& v) { return Vec(v.begin(), v.end()); };
        const std::vector<float> w6 = tof(c.w6), b6 = tof(c.b6), w7 = tof(c.w7), b7 = tof(c.b7), wu = tof(c.wu), bu = tof(c.bu);
        const Vec w6d = tod(w6), b6d = tod(b6), w7d = tod(w7), b7d = tod(b7), wud = tod(wu), bud = tod(bu);
        const FcFoldDims d{CIN, M6, M7, COUT, CS, 9};
        std::vector<float> wc, ws, bp;
        Vec wcd, wsd, bpd;
        fc_fold<float>(d, w6.data(), b6.data(), w7.data(), b7.data(), wu.data(), bu.data(), wc, ws, bp, &pool);
        fc_fold<double>(d, w6d.data(), b6d.data(), w7d.data(), b7d.data(), wud.data(), bud.data(), wcd, wsd, bpd, nullptr);
        size_t bad = 0;
        for (size_t i = 0; i < wc.size(); ++i) bad += wc[i] != (float)wcd[i];
        for (size_t i = 0; i < ws.size(); ++i) bad += ws[i] != (float)wsd[i];
        for (size_t i = 0; i < bp.size(); ++i) bad += bp[i] != (float)bpd[i];
        report(bad == 0 && wc.size() == (size_t)COUT * CIN * 9 && ws.size() == (size_t)COUT * CS && bp.size() == (size_t)COUT,
               "float fold == double fold rounded once (values that differ)", "all outputs", (double)bad);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
