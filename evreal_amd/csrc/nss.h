// The scaffold under the no-reference metrics of nriqa.hip (NIQE, BRISQUE, PIQE): natural-scene statistics, one definition of
// each step.  The metrics are held to a float64 oracle at 1e-9 .. 1e-10 and to bitwise batch independence: the order of the
// operations below is part of the contract (no contraction into fused multiply-adds: build.py).  The four-wave hand-off of fp64
// sums is metric_tiles.h's.  A metric's formulas, staging, border rule, feature order and finisher stay in nriqa.hip.
// Host side: Carve (a workspace's regions, stated once), Model (a handle's device storage), check_run (a run's refusals).
#pragma once
#include "metric_tiles.h"
#include <cmath>
#include <vector>

namespace evr_nss {

using evr_tiles::NT;
constexpr int NGRID = 9801;            // alpha = 0.2 + 0.001 k, k = 0 .. 9800

struct Taps { double g[49]; };         // the 7x7 Gaussian, row-major

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// symmetric (half-sample) reflection, repeated for an index more than one length outside (a side shorter than 4)
__device__ __forceinline__ int mirror(int i, int n) {
    i %= 2 * n;
    if (i < 0) i += 2 * n;
    return i < n ? i : 2 * n - 1 - i;
}

__device__ __forceinline__ float quant(float v, int clip) {
    if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
    return rintf(255.f * v);
}

struct Mscn { double m, sigma; };

// the closing step: from a pixel, its local mean and its local second moment
__device__ __forceinline__ Mscn mscn_close(double centre, double mu, double s2) {
    const double sigma = sqrt(fabs(s2 - mu * mu));
    return Mscn{(centre - mu) / (sigma + 1.0), sigma};
}

// M (and sigma) at one pixel from its 7x7 neighbourhood get(dy, dx), taps accumulated row by row (the oracles' order)
template <typename Get>
__device__ __forceinline__ Mscn mscn_at(const Taps& taps, double centre, Get get) {
    double mu = 0.0, s2 = 0.0;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
            const double v = get(dy, dx), g = taps.g[dy * 7 + dx];
            mu = mu + g * v;
            s2 = s2 + g * (v * v);
        }
    }
    return mscn_close(centre, mu, s2);
}

// one value into an AGGD's five running sums: sum v^2 | v<0, n<0, sum v^2 | v>0, n>0, sum |v|
__device__ __forceinline__ void aggd_add(double v, double* s) {
    const double q = v * v;
    if (v < 0.0) { s[0] += q; s[1] += 1.0; }
    if (v > 0.0) { s[2] += q; s[3] += 1.0; }
    s[4] += fabs(v);
}

struct Aggd { double ls, rs, rn; };    // the side deviations and the normalised ratio the alpha grid is searched for

// estimateaggdparam.m up to the search, from the five sums, the sum of squares (each metric's own) and the pixel count
__device__ __forceinline__ Aggd aggd_ratio(const double* s, double sumsq, double N) {
    const double ls = sqrt(s[0] / s[1]), rs = sqrt(s[2] / s[3]);     // an empty side: 0/0 = NaN
    const double g = ls / rs;
    const double ma = s[4] / N;
    const double rhat = (ma * ma) / (sumsq / N);
    return Aggd{ls, rs, (rhat * (g * g * g + 1.0) * (g + 1.0)) / ((g * g + 1.0) * (g * g + 1.0))};
}

__device__ __forceinline__ bool better(double d, int k, double bd, int bk) { return d < bd || (d == bd && k < bk); }

// The grid point k minimising dist(k), by one wave, in every lane: the first on ties, k = 0 for a NaN ratio (numpy's argmin)
template <typename Dist>
__device__ __forceinline__ int alpha_argmin(double rn, Dist dist) {
    const int lane = threadIdx.x & 63;
    int bk = 0;
    if (!isnan(rn)) {
        double bd = dist(lane);
        bk = lane;
        for (int k = lane + 64; k < NGRID; k += 64) {
            const double d = dist(k);
            if (d < bd) { bd = d; bk = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int ok = __shfl_xor(bk, o, 64);
            if (better(od, ok, bd, bk)) { bd = od; bk = ok; }
        }
    }
    return bk;
}

// Counting in a block: a wave counts its lanes that hold `pred` by a ballot (one scalar population count, the same in every
// lane; a lane that has left the loop counts as none), and block_count adds the four waves' counts, in every thread.
// Contract: block_count stores the wave's lane 0's running count, so the caller adds wave_votes up in a loop that lane 0 runs
// at least as long as any lane of its wave -- `for (i = threadIdx.x; i < n; i += NT)` is one.
__device__ __forceinline__ int wave_votes(bool pred) { return __popcll(__ballot(pred)); }
__device__ __forceinline__ int block_count(int wave_c, int (&cnt)[NT / 64]) {
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = wave_c;
    __syncthreads();
    return ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
}

inline Taps gaussian_taps() {
    // fspecial('gaussian', 7, 7/6); tests/nriqa_ref.py gaussian_window() evaluates the same expressions in the same order
    Taps t;
    const double sig = 7.0 / 6.0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) {
            const int y = i - 3, x = j - 3;
            t.g[i * 7 + j] = std::exp(-(double)(x * x + y * y) / (2.0 * sig * sig));
        }
    double s = 0.0;
    for (int k = 0; k < 49; ++k) s += t.g[k];
    for (int k = 0; k < 49; ++k) t.g[k] = t.g[k] / s;
    return t;
}

// The alpha grid's columns, Gamma evaluated once on the host: r(alpha) = G(2/a)^2/(G(1/a)G(3/a)) (the AGGD ratio), alpha,
// sqrt(G(1/a)/G(3/a)), G(2/a)/G(1/a), and with cols = 5 the GGD ratio G(1/a)G(3/a)/G(2/a)^2.  [cols][NGRID]
inline std::vector<double> alpha_table(int cols) {
    std::vector<double> table((size_t)cols * NGRID);
    for (int k = 0; k < NGRID; ++k) {
        const double a = 0.2 + 0.001 * (double)k;
        const double g1 = std::tgamma(1.0 / a), g2 = std::tgamma(2.0 / a), g3 = std::tgamma(3.0 / a);
        table[k] = (g2 * g2) / (g1 * g3);
        table[NGRID + k] = a;
        table[2 * NGRID + k] = std::sqrt(g1 / g3);
        table[3 * NGRID + k] = g2 / g1;
        if (cols > 4) table[4 * NGRID + k] = (g1 * g3) / (g2 * g2);
    }
    return table;
}

// A workspace's regions, stated once and in order: take<T>(count) is the next one, 256-B aligned from the base.  Over a null
// base it only counts and hands out nulls, so a metric's size function and its run function go through the same statement.
class Carve {
    char* base;
    size_t off = 0;
public:
    explicit Carve(void* ws) : base((char*)ws) {}
    template <typename T> T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += evr::align_up(count * sizeof(T), 256);
        return p;
    }
    size_t bytes() const { return off + 256; }
};

// What a handle keeps on the device.  The handle structs derive from it.
struct Model {
    double* d_model = nullptr;
    double* d_table = nullptr;   // alpha_table(cols)
    Taps taps;
};

// the one release: both allocations freed, the handle deleted, the first failure reported
template <typename H>
int destroy(H* h) {
    if (!h) return EVR_OK;
    const hipError_t e1 = h->d_model ? hipFree(h->d_model) : hipSuccess;
    const hipError_t e2 = h->d_table ? hipFree(h->d_table) : hipSuccess;
    delete h;
    EVR_HIP(e1);
    EVR_HIP(e2);
    return EVR_OK;
}

// the end of a *_create: the taps, the model and the table onto the device (evr::upload pads each allocation by 64 B);
// *out = h, or h destroyed.  The code returned is the upload's; a failing hipFree in destroy would replace its message.
template <typename H>
int finish_create(H* h, const std::vector<double>& model, int table_cols, H** out) {
    h->taps = gaussian_taps();
    int rc = evr::upload(model, &h->d_model);
    if (rc == EVR_OK) rc = evr::upload(alpha_table(table_cols), &h->d_table);
    if (rc == EVR_OK) *out = h;
    else (void)destroy(h);
    return rc;
}

// What a run function refuses first, in this order: a shape with n < n_min or a side < 1, (n == 0: nothing to do, EVR_OK),
// a null pointer.  The caller returns on anything but EVR_OK and on n == 0; a limit of its own and the workspace follow.
inline int check_run(const char* what, int n_min, int n, int H, int W, bool pointers) {
    EVR_REQUIRE(n >= n_min && H >= 1 && W >= 1, "%s: bad shape n=%d H=%d W=%d", what, n, H, W);
    if (n == 0) return EVR_OK;
    EVR_REQUIRE(pointers, "%s: null pointer", what);
    return EVR_OK;
}

}  // namespace evr_nss
