// NIQE (Mittal, Soundararajan, Bovik 2013) on gfx950: the no-reference score of the reference's `-qm niqe`
// (utils/eval_metrics.py:100-156 -> pyiqa), following the published MATLAB release (computequality.m,
// computefeature.m, estimateaggdparam.m, estimatemodelparam.m).  Conventions (tests/nriqa_ref.py restates them):
//   input   u = rint(255 * clip(v)) in fp32 (half to even), fp64 from here on; cropped to whole 96 x 96 blocks
//   scale s mu = G*I, sigma = sqrt(|G*(I.I) - mu^2|), MSCN = (I - mu)/(sigma + 1); G: 7x7 Gaussian, sigma 7/6, sum 1,
//           correlation with replicate padding, the 49 taps accumulated row by row; blocks of 96/s
//   resize  MATLAB imresize(I, 0.5): bicubic (a = -0.5) with antialiasing = 8 taps of 0.5 * cubic(0.5 d), symmetric
//           borders, rows first.  The taps are multiples of 2^-8 and the inputs integers <= 255: both passes are exact.
//   fit     AGGD per block on the MSCN values and on four in-block circular pair products (shifts (0,1) (1,0) (1,1)
//           (1,-1)); alpha = the grid point 0.2 + 0.001 k minimising (r(alpha) - r_hat_norm)^2, first on ties (NaN ->
//           k = 0, as numpy's argmin).  Gamma is never evaluated here: the handle's table (built on the host) holds
//           r(alpha), sqrt(G(1/a)/G(3/a)) and G(2/a)/G(1/a).
//   score   sqrt(d' ((Sp + Sd)/2)^-1 d), d = mu_p - nanmean(rows), Sd = unbiased covariance of the NaN-free rows,
//           by a Cholesky solve (Sp is SPD: checked at creation).
// Launches per batch, whatever n: resize, block kernel at scale 1, block kernel at scale 2, score (features: three).
// Every frame's arithmetic runs in work-groups of its own, each sum in a fixed order, no atomics: the results are
// bitwise independent of the batch size and of a frame's position in the batch.
// What the three metrics share -- MSCN, the AGGD fit, the hand-offs, the workspace carve, the handles' storage and the run
// functions' refusals -- is csrc/nss.h.  More than 65535 frames: the kernels that carry the frame on gridDim.y are launched per
// chunk of 65535 on offset pointers (every frame owns its part of every workspace region); the finishers ride gridDim.x.
#include "nss.h"
#include <new>

namespace {

using namespace evr_nss;
using evr_tiles::block_total, evr_tiles::block_totals, evr_tiles::for_frame_chunks;

constexpr int BLK = 96;
constexpr int NF = 36;                 // features per block: 18 per scale
constexpr int MAX_BLOCKS = 8192;       // blocks per frame the score kernel takes (its NaN-row flags live in LDS)

// imresize(u, 0.5) of the cropped (NIQE) or whole (BRISQUE) quantised frame: out [n, ceil(Hc/2), ceil(Wc/2)]
__global__ __launch_bounds__(NT) void niqe_resize_kernel(const float* __restrict__ img, int H, int W, int Hc, int Wc,
                                                         int clip, double* __restrict__ out) {
    // 0.5 * cubic(0.5 * d) at d = 3.5, 2.5, 1.5, 0.5, -0.5, ... (they sum to 1 exactly: the per-output normalisation is a no-op)
    const double w[8] = {-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875};
    const int Hh = (Hc + 1) / 2, Wh = (Wc + 1) / 2, f = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)Hh * Wh) return;
    const int y = (int)(i / Wh), x = (int)(i % Wh);
    const float* src = img + (int64_t)f * H * W;
    int rows[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) rows[t] = mirror(2 * y - 3 + t, Hc);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = mirror(2 * x - 3 + j, Wc);
        double col = 0.0;                       // the row pass at column c
#pragma unroll
        for (int t = 0; t < 8; ++t) col = col + w[t] * (double)quant(src[(int64_t)rows[t] * W + c], clip);
        acc = acc + w[j] * col;
    }
    out[(int64_t)f * Hh * Wh + i] = acc;
}

// One work-group per (block, frame) at one scale: MSCN on chip, the 26 block sums (5 vectors x {sum x^2 | x<0, n<0,
// sum x^2 | x>0, n>0, sum |x|} + the sigma sum), then the five AGGD fits -> feat[f][b][scale*18 .. +18].
// S = 96 reads the fp32 frame (quantised on load, exact in fp32); S = 48 reads the fp64 half-size image.
template <int S, typename T>
__global__ __launch_bounds__(NT) void niqe_block_kernel(const float* __restrict__ img, const double* __restrict__ half, int H,
                                                        int W, int Hs, int Ws, int clip, int nbx, Taps taps,
                                                        const double* __restrict__ table, double* __restrict__ feat,
                                                        double* __restrict__ sharp) {
    constexpr int TS = S + 6;
    constexpr int NS = 26;
    __shared__ T tile[TS][TS + 1];
    __shared__ double m[S][S + 1];
    __shared__ double red[NT / 64][NS];
    __shared__ double st[NS];
    const int b = blockIdx.x, f = blockIdx.y, nb = gridDim.x, tid = threadIdx.x;
    const int y0 = (b / nbx) * S, x0 = (b % nbx) * S;

    for (int i = tid; i < TS * TS; i += NT) {
        const int r = i / TS, c = i % TS;
        const int yy = clampi(y0 + r - 3, Hs), xx = clampi(x0 + c - 3, Ws);
        if constexpr (S == BLK) tile[r][c] = quant(img[(int64_t)f * H * W + (int64_t)yy * W + xx], clip);
        else tile[r][c] = half[(int64_t)f * Hs * Ws + (int64_t)yy * Ws + xx];
    }
    __syncthreads();

    double ssig = 0.0;
    for (int i = tid; i < S * S; i += NT) {
        const int r = i / S, c = i % S;
        const Mscn p = mscn_at(taps, (double)tile[r + 3][c + 3], [&](int dy, int dx) { return (double)tile[r + dy][c + dx]; });
        m[r][c] = p.m;
        ssig += p.sigma;
    }
    __syncthreads();

    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    a[25] = ssig;
    for (int i = tid; i < S * S; i += NT) {
        const int r = i / S, c = i % S;
        const double x = m[r][c];
        double v[5];
        v[0] = x;
        v[1] = x * m[r][(c + S - 1) % S];                      // np.roll by (0, 1): m[r][c - 1]
        v[2] = x * m[(r + S - 1) % S][c];                      // (1, 0)
        v[3] = x * m[(r + S - 1) % S][(c + S - 1) % S];        // (1, 1)
        v[4] = x * m[(r + S - 1) % S][(c + 1) % S];            // (1, -1)
#pragma unroll
        for (int k = 0; k < 5; ++k) aggd_add(v[k], a + 5 * k);
    }
    block_totals(a, red, st);
    __syncthreads();

    const double* R = table;
    const double* ALPHA = table + NGRID;
    const double* F1 = table + 2 * NGRID;
    const double* F2 = table + 3 * NGRID;
    const double N = (double)(S * S);
    const int lane = tid & 63, wave = tid >> 6;
    double* out = feat + ((int64_t)f * nb + b) * NF + (S == BLK ? 0 : 18);
    for (int v = wave; v < 5; v += NT / 64) {      // one wave per fit
        const double* s = st + v * 5;
        const Aggd fit = aggd_ratio(s, s[0] + s[2], N);
        const double ls = fit.ls, rs = fit.rs;
        const int bk = alpha_argmin(fit.rn, [&](int k) { return (R[k] - fit.rn) * (R[k] - fit.rn); });
        if (lane == 0) {
            const double bl = ls * F1[bk], br = rs * F1[bk];
            if (v == 0) {
                out[0] = ALPHA[bk];
                out[1] = (bl + br) / 2.0;
            } else {
                double* o = out + 2 + 4 * (v - 1);
                o[0] = ALPHA[bk];
                o[1] = (br - bl) * F2[bk];
                o[2] = bl;
                o[3] = br;
            }
        }
    }
    if (S == BLK && tid == 0 && sharp) sharp[(int64_t)f * nb + b] = st[25] / N;
}

// One work-group per frame: NaN-aware mean, covariance of the NaN-free rows, Cholesky of (Sp + Sd)/2, solve, sqrt.
__global__ __launch_bounds__(NT) void niqe_score_kernel(const double* __restrict__ feat, int nb, const double* __restrict__ model,
                                                        double* __restrict__ scores) {
    __shared__ double A[NF][NF + 1];
    __shared__ double mud[NF], muc[NF], y[NF];
    __shared__ unsigned char ok[MAX_BLOCKS];
    __shared__ int cnt[NT / 64];
    __shared__ int bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    const double* F = feat + (int64_t)f * nb * NF;
    const double* mup = model;
    const double* covp = model + NF;
    int c = 0;
    for (int r = tid; r < nb; r += NT) {
        bool full = true;
        for (int k = 0; k < NF; ++k) full = full && !isnan(F[(int64_t)r * NF + k]);
        ok[r] = full ? 1 : 0;
        c += wave_votes(full);
    }
    if (tid == 0) bad = 0;
    const int m = block_count(c, cnt);
    if (tid < NF) {
        double s = 0.0, sc = 0.0;
        int k = 0;
        for (int r = 0; r < nb; ++r) {
            const double v = F[(int64_t)r * NF + tid];
            if (!isnan(v)) { s += v; ++k; }
            if (ok[r]) sc += v;
        }
        mud[tid] = s / (double)k;               // no value: 0/0 = NaN
        muc[tid] = sc / (double)m;
    }
    __syncthreads();
    for (int e = tid; e < NF * NF; e += NT) {
        const int i = e / NF, j = e % NF;
        if (j > i) continue;
        double s = 0.0;
        for (int r = 0; r < nb; ++r)
            if (ok[r]) s += (F[(int64_t)r * NF + i] - muc[i]) * (F[(int64_t)r * NF + j] - muc[j]);
        A[i][j] = (covp[i * NF + j] + s / (double)(m - 1)) / 2.0;
    }
    __syncthreads();
    // right-looking Cholesky of the lower triangle, in place
    for (int k = 0; k < NF; ++k) {
        if (tid == 0) {
            const double d = A[k][k];
            if (!(d > 0.0)) bad = 1;
            A[k][k] = sqrt(d);
        }
        __syncthreads();
        if (tid > k && tid < NF) A[tid][k] = A[tid][k] / A[k][k];
        __syncthreads();
        for (int e = tid; e < NF * NF; e += NT) {
            const int i = e / NF, j = e % NF;
            if (j > k && j <= i) A[i][j] = A[i][j] - A[i][k] * A[j][k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double q = 0.0;
        for (int i = 0; i < NF; ++i) {
            double s = mup[i] - mud[i];
            for (int j = 0; j < i; ++j) s = s - A[i][j] * y[j];
            y[i] = s / A[i][i];
            q += y[i] * y[i];
        }
        scores[f] = (m < 2 || bad) ? (double)NAN : sqrt(q);
    }
}

__global__ void niqe_nan_kernel(double* __restrict__ scores, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) scores[i] = (double)NAN;
}

struct Dims {                        // the crop to whole blocks and the block counts
    int Hc, Wc, nbx, nb;
    Dims(int H, int W) : Hc((H / BLK) * BLK), Wc((W / BLK) * BLK), nbx(Wc / BLK), nb((Hc / BLK) * nbx) {}
};

struct NiqeWs : Carve {              // the workspace: a member takes the next region, in the members' order
    double *half, *feat, *sharp;
    NiqeWs(void* ws, size_t n, const Dims& d)
        : Carve(ws), half(take<double>(n * (d.Hc / 2) * (d.Wc / 2))), feat(take<double>(n * d.nb * NF)),
          sharp(take<double>(n * d.nb)) {}
};

}  // namespace

struct evr_niqe : evr_nss::Model {};        // d_model: mu [36], cov [36*36]; d_table: [4][9801]

extern "C" int evr_niqe_create(const double* mu, const double* cov, evr_niqe** out) {
    EVR_REQUIRE(mu && cov && out, "evr_niqe_create: null pointer");
    *out = nullptr;
    for (int i = 0; i < NF; ++i) EVR_REQUIRE(std::isfinite(mu[i]), "evr_niqe_create: mu[%d] is not finite", i);
    // symmetric positive definite: a Cholesky factorisation on the host
    std::vector<double> L(cov, cov + NF * NF);
    for (int i = 0; i < NF; ++i)
        for (int j = 0; j < NF; ++j)
            EVR_REQUIRE(std::isfinite(L[i * NF + j]) && L[i * NF + j] == cov[j * NF + i], "evr_niqe_create: cov is not a finite symmetric matrix");
    for (int k = 0; k < NF; ++k) {
        double d = L[k * NF + k];
        for (int p = 0; p < k; ++p) d -= L[k * NF + p] * L[k * NF + p];
        EVR_REQUIRE(d > 0.0, "evr_niqe_create: cov is not positive definite");
        L[k * NF + k] = std::sqrt(d);
        for (int i = k + 1; i < NF; ++i) {
            double s = L[i * NF + k];
            for (int p = 0; p < k; ++p) s -= L[i * NF + p] * L[k * NF + p];
            L[i * NF + k] = s / L[k * NF + k];
        }
    }
    std::vector<double> model(NF + NF * NF);
    for (int i = 0; i < NF; ++i) model[i] = mu[i];
    for (int i = 0; i < NF * NF; ++i) model[NF + i] = cov[i];
    evr_niqe* h = new (std::nothrow) evr_niqe();
    EVR_REQUIRE(h, "evr_niqe_create: out of host memory");
    return finish_create(h, model, 4, out);
}

extern "C" int evr_niqe_destroy(evr_niqe* h) { return destroy(h); }

extern "C" size_t evr_niqe_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H < 1 || W < 1) return 0;
    return NiqeWs(nullptr, n, Dims(H, W)).bytes();
}

static int niqe_run(evr_niqe* h, const float* img, int n, int H, int W, int clip, double* scores, double* feat,
                    double* sharp, void* ws, size_t ws_bytes, evr_stream_t stream_, const char* what) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(h, "%s: null handle", what);
    const int rc = check_run(what, 0, n, H, W, img && (scores || (feat && sharp)));
    if (rc != EVR_OK || n == 0) return rc;
    const Dims d(H, W);
    EVR_REQUIRE(d.nb <= MAX_BLOCKS, "%s: %d blocks per frame > %d", what, d.nb, MAX_BLOCKS);
    EVR_REQUIRE_WORKSPACE(what, ws, ws_bytes, evr_niqe_workspace_bytes(n, H, W));
    if (d.nb == 0) {              // no whole 96 x 96 block: NaN scores, no features
        if (scores) {
            hipLaunchKernelGGL(niqe_nan_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, stream, scores, n);
            EVR_LAUNCH_CHECK();
        }
        return EVR_OK;
    }
    const NiqeWs w(ws, n, d);
    if (!feat) feat = w.feat;
    if (!sharp) sharp = w.sharp;
    const int Hh = d.Hc / 2, Wh = d.Wc / 2;
    const size_t px = (size_t)H * W, hpx = (size_t)Hh * Wh;
    const int run = for_frame_chunks(n, [&](int f0, int nf) -> int {
        double* half = w.half + f0 * hpx;
        double* cfeat = feat + (size_t)f0 * d.nb * NF;
        hipLaunchKernelGGL(niqe_resize_kernel, dim3((unsigned)((hpx + NT - 1) / NT), nf), dim3(NT), 0, stream, img + f0 * px,
                           H, W, d.Hc, d.Wc, clip, half);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL((niqe_block_kernel<BLK, float>), dim3(d.nb, nf), dim3(NT), 0, stream, img + f0 * px,
                           (const double*)nullptr, H, W, d.Hc, d.Wc, clip, d.nbx, h->taps, (const double*)h->d_table, cfeat,
                           sharp + (size_t)f0 * d.nb);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL((niqe_block_kernel<BLK / 2, double>), dim3(d.nb, nf), dim3(NT), 0, stream, (const float*)nullptr,
                           (const double*)half, H, W, Hh, Wh, clip, d.nbx, h->taps, (const double*)h->d_table, cfeat,
                           (double*)nullptr);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
    if (run != EVR_OK) return run;
    if (scores) {
        hipLaunchKernelGGL(niqe_score_kernel, dim3(n), dim3(NT), 0, stream, (const double*)feat, d.nb, (const double*)h->d_model,
                           scores);
        EVR_LAUNCH_CHECK();
    }
    return EVR_OK;
}

extern "C" int evr_niqe_score(evr_niqe* h, const float* img, int n, int H, int W, int clip, double* out_scores,
                              void* workspace, size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE(out_scores || n <= 0, "evr_niqe_score: null pointer");
    return niqe_run(h, img, n, H, W, clip, out_scores, nullptr, nullptr, workspace, workspace_bytes, stream, "evr_niqe_score");
}

extern "C" int evr_niqe_features(evr_niqe* h, const float* img, int n, int H, int W, int clip, double* out_feat,
                                 double* out_sharpness, void* workspace, size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE((out_feat && out_sharpness) || n <= 0, "evr_niqe_features: null pointer");
    return niqe_run(h, img, n, H, W, clip, nullptr, out_feat, out_sharpness, workspace, workspace_bytes, stream,
                    "evr_niqe_features");
}

// =====================================================================================================================
// BRISQUE (Mittal, Moorthy, Bovik 2012): the no-reference score of the reference's `-qm brisque` (-> pyiqa), following the
// published MATLAB release (brisquescore.m, brisque_feature.m, estimateggdparam.m, estimateaggdparam.m) and libsvm's
// svm-scale -r / svm-predict.  Conventions (tests/brisque_ref.py states them in the same words):
//   input     u = rint(255 * clip(v)) in fp32 (half to even), fp64 from here on; no crop: the whole frame is used
//   MSCN      at each of two scales: mu = filter2(w, I, 'same'), sigma = sqrt(|filter2(w, I.*I) - mu^2|),
//             M = (I - mu)/(sigma + 1); w: 7x7 Gaussian, sigma 7/6, sum 1; ZERO padding; the 49 taps accumulated row by row
//   resize    MATLAB imresize(I, 0.5), bicubic, antialiased, symmetric borders: ceil(H/2) x ceil(W/2)
//   features  18 per scale, 36 in all, scale 1 first.  GGD fit of all of M: rho = mean(M^2)/mean(|M|)^2, alpha = the grid
//             point 0.2 + 0.001 k minimising |rho - G(1/a)G(3/a)/G(2/a)^2| -> [alpha, mean(M^2)].  For each circshift
//             (0,1) (1,0) (1,1) (-1,1) of the whole frame (wrapping at its edges), the AGGD fit of P = M . circshift(M, s)
//             (NIQE's estimateaggdparam) -> [alpha, (sr - sl) G(2/a)/G(1/a) sqrt(G(1/a)/G(3/a)), sl^2, sr^2].  Every grid
//             search takes the first point on ties; a NaN ratio takes k = 0 (numpy's argmin); an empty AGGD side is NaN.
//   scaling   svm-scale: x' = lower + (upper - lower)(x - min)/(max - min); x == min -> lower, x == max -> upper; a feature
//             whose range has min == max is dropped (0 in the sparse vector)
//   score     RBF SVR: sum_i coef_i exp(-gamma |x' - sv_i|^2) - rho, |.|^2 a sum of squared differences in feature order.
//             A frame with any NaN feature scores NaN (a flat frame is one).  Nothing goes through the release's %f / %g
//             text round trips: fp64 throughout.
// Launches per batch, whatever n: resize, statistics kernel at scale 1, statistics kernel at scale 2, finisher.  The
// statistics kernels run one work-group per (32 x 32 tile, frame) and write the tile's 26 partial sums; the finisher runs
// one work-group per frame and adds them in tile order.  No atomics: results are bitwise independent of the batch.

namespace {

constexpr int BT = 32;                 // statistics tile: BT x BT pixels per work-group
constexpr int BNS = 26;                // partial sums per tile: sum M^2, sum |M|, then per shift the six below

__device__ __forceinline__ float load_px(const float* p, int64_t i, int clip) { return quant(p[i], clip); }
__device__ __forceinline__ double load_px(const double* p, int64_t i, int) { return p[i]; }
__device__ __forceinline__ int wrap(int i, int n) { i %= n; return i < 0 ? i + n : i; }

// One work-group per (tile, frame) at one scale.  The tile's input and a 4-pixel zero-padded halo are staged in LDS; M is
// computed on chip for the tile plus the row above, the row below and the column to the left (the pairs' neighbours).
// Where one of those lies outside the frame it is the wrapped row or column at the other edge, whose neighbourhood is
// read from memory.  -> part[f][t][26]: sum M^2, sum |M|, then for the shifts (0,1) (1,0) (1,1) (-1,1):
// sum P^2 | P<0, n<0, sum P^2 | P>0, n>0, sum |P|, sum P^2.
// T = float reads the fp32 frame (quantised on load, exact in fp32); T = double reads the fp64 half-size image.
template <typename T>
__global__ __launch_bounds__(NT) void brisque_stats_kernel(const T* __restrict__ src, int Hs, int Ws, int clip, int ntx,
                                                           Taps taps, double* __restrict__ part) {
    constexpr int TR = BT + 8, TC = BT + 7;     // input rows y0-4 .. y0+BT+3, columns x0-4 .. x0+BT+2
    constexpr int MR = BT + 2, MC = BT + 1;     // M rows y0-1 .. y0+BT, columns x0-1 .. x0+BT-1
    __shared__ T tile[TR][TC + 1];
    __shared__ double m[MR][MC];
    __shared__ double red[NT / 64][BNS];
    const int t = blockIdx.x, f = blockIdx.y, nt = gridDim.x, tid = threadIdx.x;
    const int y0 = (t / ntx) * BT, x0 = (t % ntx) * BT;
    const T* img = src + (int64_t)f * Hs * Ws;

    for (int i = tid; i < TR * TC; i += NT) {
        const int r = i / TC, c = i % TC;
        const int yy = y0 + r - 4, xx = x0 + c - 4;
        tile[r][c] = (yy >= 0 && yy < Hs && xx >= 0 && xx < Ws) ? load_px(img, (int64_t)yy * Ws + xx, clip) : (T)0;
    }
    __syncthreads();

    for (int i = tid; i < MR * MC; i += NT) {
        const int r = i / MC, c = i % MC;
        const int gy = y0 + r - 1, gx = x0 + c - 1;
        double v = 0.0;
        if (gy >= 0 && gy < Hs && gx >= 0 && gx < Ws) {
            // tile[r + dy][c + dx] holds the input at (gy + dy - 3, gx + dx - 3), zero outside the frame
            v = mscn_at(taps, (double)tile[r + 3][c + 3], [&](int dy, int dx) { return (double)tile[r + dy][c + dx]; }).m;
        } else if (gy >= -1 && gy <= Hs && gx >= -1 && gx < Ws) {
            // a neighbour across the frame's edge: the pixel at the other side, its zero-padded neighbourhood from memory
            const int wy = wrap(gy, Hs), wx = wrap(gx, Ws);
            auto get = [&](int dy, int dx) {
                const int yy = wy + dy - 3, xx = wx + dx - 3;
                return (yy >= 0 && yy < Hs && xx >= 0 && xx < Ws) ? (double)load_px(img, (int64_t)yy * Ws + xx, clip) : 0.0;
            };
            v = mscn_at(taps, get(3, 3), get).m;
        }
        m[r][c] = v;
    }
    __syncthreads();

    double a[BNS];
#pragma unroll
    for (int k = 0; k < BNS; ++k) a[k] = 0.0;
    for (int i = tid; i < BT * BT; i += NT) {
        const int r = i / BT + 1, c = i % BT + 1;              // (r, c) in m: the pixel (y0 + r - 1, x0 + c - 1)
        if (y0 + r - 1 >= Hs || x0 + c - 1 >= Ws) continue;
        const double x = m[r][c];
        a[0] += x * x;
        a[1] += fabs(x);
        double v[4];
        v[0] = x * m[r][c - 1];                                 // circshift by (0, 1): M(y, x - 1)
        v[1] = x * m[r - 1][c];                                 // (1, 0): M(y - 1, x)
        v[2] = x * m[r - 1][c - 1];                             // (1, 1): M(y - 1, x - 1)
        v[3] = x * m[r + 1][c - 1];                             // (-1, 1): M(y + 1, x - 1)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            aggd_add(v[k], a + 2 + 6 * k);
            a[2 + 6 * k + 5] += v[k] * v[k];
        }
    }
    block_totals(a, red, part + ((int64_t)f * nt + t) * BNS);
}

struct SvrParams { int nsv; double gamma, rho, lower, upper; };

// One work-group per frame: the tile sums in tile order, the 2 x (1 GGD + 4 AGGD) fits (one wave per fit), the 36
// features, svm-scale and the SVR.  model: fmin [36], fmax [36], coef [nsv], sv [nsv][36].
__global__ __launch_bounds__(NT) void brisque_finish_kernel(const double* __restrict__ part1, int nt1, int N1,
                                                            const double* __restrict__ part2, int nt2, int N2,
                                                            const double* __restrict__ table, const double* __restrict__ model,
                                                            SvrParams svr, double* __restrict__ feat, double* __restrict__ scores) {
    __shared__ double st[2][BNS];
    __shared__ double fe[NF], xs[NF];
    __shared__ double red[NT / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2 * BNS) {
        const int s = tid / BNS, k = tid % BNS, nt = s ? nt2 : nt1;
        const double* p = (s ? part2 : part1) + (int64_t)f * nt * BNS + k;
        double sum = 0.0;
        for (int t = 0; t < nt; ++t) sum += p[(int64_t)t * BNS];
        st[s][k] = sum;
    }
    __syncthreads();

    const double* R = table;
    const double* ALPHA = table + NGRID;
    const double* F1 = table + 2 * NGRID;
    const double* F2 = table + 3 * NGRID;
    const double* RG = table + 4 * NGRID;
    for (int v = wave; v < 10; v += NT / 64) {                 // one wave per fit
        const int sc = v / 5, j = v % 5;
        const double* S = st[sc];
        const double N = (double)(sc ? N2 : N1);
        double rn, ls = 0.0, rs = 0.0, msq = 0.0;
        if (j == 0) {
            msq = S[0] / N;
            const double ma = S[1] / N;
            rn = msq / (ma * ma);
        } else {
            const double* s = S + 2 + 6 * (j - 1);
            const Aggd fit = aggd_ratio(s, s[5], N);
            ls = fit.ls; rs = fit.rs; rn = fit.rn;
        }
        const int bk = alpha_argmin(rn, [&](int k) { return j == 0 ? fabs(rn - RG[k]) : (R[k] - rn) * (R[k] - rn); });
        if (lane == 0) {
            double* o = fe + 18 * sc;
            if (j == 0) {
                o[0] = ALPHA[bk];
                o[1] = msq;
            } else {
                o += 2 + 4 * (j - 1);
                o[0] = ALPHA[bk];
                o[1] = ((rs - ls) * F2[bk]) * F1[bk];
                o[2] = ls * ls;
                o[3] = rs * rs;
            }
        }
    }
    __syncthreads();
    if (feat && tid < NF) feat[(int64_t)f * NF + tid] = fe[tid];
    if (!scores) return;

    if (tid < NF) {                                             // svm-scale
        const double x = fe[tid], lo = model[tid], hi = model[NF + tid];
        double y;
        if (lo == hi) y = 0.0;
        else if (x == lo) y = svr.lower;
        else if (x == hi) y = svr.upper;
        else y = svr.lower + ((svr.upper - svr.lower) * (x - lo)) / (hi - lo);
        xs[tid] = y;
    }
    __syncthreads();
    const double* coef = model + 2 * NF;
    const double* sv = coef + svr.nsv;
    double acc = 0.0;
    for (int i = tid; i < svr.nsv; i += NT) {
        double d = 0.0;
        for (int k = 0; k < NF; ++k) {
            const double e = xs[k] - sv[(int64_t)i * NF + k];
            d = d + e * e;
        }
        acc = acc + coef[i] * exp(-svr.gamma * d);
    }
    acc = block_total(acc, red);
    if (tid == 0) {
        bool nan = false;
        for (int k = 0; k < NF; ++k) nan = nan || isnan(fe[k]);
        scores[f] = nan ? (double)NAN : acc - svr.rho;
    }
}

struct BDims {                       // the half-size image and the tile counts of both scales
    int Hh, Wh, ntx1, nt1, ntx2, nt2;
    BDims(int H, int W)
        : Hh((H + 1) / 2), Wh((W + 1) / 2), ntx1((W + BT - 1) / BT), nt1(((H + BT - 1) / BT) * ntx1), ntx2((Wh + BT - 1) / BT),
          nt2(((Hh + BT - 1) / BT) * ntx2) {}
};

struct BrisqueWs : Carve {           // the workspace: a member takes the next region, in the members' order
    double *half, *part1, *part2;
    BrisqueWs(void* ws, size_t n, const BDims& d)
        : Carve(ws), half(take<double>(n * d.Hh * d.Wh)), part1(take<double>(n * d.nt1 * BNS)),
          part2(take<double>(n * d.nt2 * BNS)) {}
};

}  // namespace

struct evr_brisque : evr_nss::Model {   // d_model: fmin [36], fmax [36], coef [nsv], sv [nsv*36]; d_table: [5][9801]
    SvrParams svr;
};

extern "C" int evr_brisque_create(const double* sv, const double* coef, int nsv, double gamma, double rho, const double* fmin,
                                  const double* fmax, double lower, double upper, evr_brisque** out) {
    EVR_REQUIRE(out && fmin && fmax, "evr_brisque_create: null pointer");
    *out = nullptr;
    EVR_REQUIRE(nsv >= 0, "evr_brisque_create: nsv = %d < 0", nsv);
    EVR_REQUIRE(nsv == 0 || (sv && coef), "evr_brisque_create: null support vectors");
    EVR_REQUIRE(std::isfinite(gamma) && std::isfinite(rho) && std::isfinite(lower) && std::isfinite(upper),
                "evr_brisque_create: gamma, rho, lower and upper must be finite");
    EVR_REQUIRE(lower < upper, "evr_brisque_create: lower %g >= upper %g", lower, upper);
    for (int k = 0; k < NF; ++k) {
        EVR_REQUIRE(std::isfinite(fmin[k]) && std::isfinite(fmax[k]), "evr_brisque_create: range of feature %d is not finite", k + 1);
        EVR_REQUIRE(fmin[k] <= fmax[k], "evr_brisque_create: feature %d has min %g > max %g", k + 1, fmin[k], fmax[k]);
    }
    for (int i = 0; i < nsv; ++i) {
        EVR_REQUIRE(std::isfinite(coef[i]), "evr_brisque_create: coef[%d] is not finite", i);
        for (int k = 0; k < NF; ++k)
            EVR_REQUIRE(std::isfinite(sv[(size_t)i * NF + k]), "evr_brisque_create: sv[%d][%d] is not finite", i, k);
    }
    std::vector<double> model(2 * NF + (size_t)nsv * (NF + 1));
    for (int k = 0; k < NF; ++k) { model[k] = fmin[k]; model[NF + k] = fmax[k]; }
    for (int i = 0; i < nsv; ++i) model[2 * NF + i] = coef[i];
    for (size_t i = 0; i < (size_t)nsv * NF; ++i) model[2 * NF + nsv + i] = sv[i];
    evr_brisque* h = new (std::nothrow) evr_brisque();
    EVR_REQUIRE(h, "evr_brisque_create: out of host memory");
    h->svr = SvrParams{nsv, gamma, rho, lower, upper};
    return finish_create(h, model, 5, out);
}

extern "C" int evr_brisque_destroy(evr_brisque* h) { return destroy(h); }

extern "C" size_t evr_brisque_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H < 1 || W < 1) return 0;
    return BrisqueWs(nullptr, n, BDims(H, W)).bytes();
}

static int brisque_run(evr_brisque* h, const float* img, int n, int H, int W, int clip, double* scores, double* feat, void* ws,
                       size_t ws_bytes, evr_stream_t stream_, const char* what) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(h, "%s: null handle", what);
    EVR_REQUIRE((int64_t)H * W <= (int64_t)1 << 30, "%s: %d x %d frame is too large", what, H, W);
    const int rc = check_run(what, 0, n, H, W, img != nullptr);
    if (rc != EVR_OK || n == 0) return rc;
    EVR_REQUIRE_WORKSPACE(what, ws, ws_bytes, evr_brisque_workspace_bytes(n, H, W));
    const BDims d(H, W);
    const BrisqueWs w(ws, n, d);
    const size_t px = (size_t)H * W, hpx = (size_t)d.Hh * d.Wh;
    const int run = for_frame_chunks(n, [&](int f0, int nf) -> int {
        double* half = w.half + f0 * hpx;
        hipLaunchKernelGGL(niqe_resize_kernel, dim3((unsigned)((hpx + NT - 1) / NT), nf), dim3(NT), 0, stream, img + f0 * px,
                           H, W, H, W, clip, half);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(brisque_stats_kernel<float>, dim3(d.nt1, nf), dim3(NT), 0, stream, img + f0 * px, H, W, clip, d.ntx1,
                           h->taps, w.part1 + (size_t)f0 * d.nt1 * BNS);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(brisque_stats_kernel<double>, dim3(d.nt2, nf), dim3(NT), 0, stream, (const double*)half, d.Hh, d.Wh,
                           clip, d.ntx2, h->taps, w.part2 + (size_t)f0 * d.nt2 * BNS);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
    if (run != EVR_OK) return run;
    hipLaunchKernelGGL(brisque_finish_kernel, dim3(n), dim3(NT), 0, stream, (const double*)w.part1, d.nt1, H * W,
                       (const double*)w.part2, d.nt2, d.Hh * d.Wh, (const double*)h->d_table, (const double*)h->d_model, h->svr,
                       feat, scores);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" int evr_brisque_score(evr_brisque* h, const float* img, int n, int H, int W, int clip, double* out_scores,
                                 void* workspace, size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE(h, "evr_brisque_score: null handle");
    EVR_REQUIRE(h->svr.nsv > 0, "evr_brisque_score: a features-only handle (no support vectors) gives no score");
    EVR_REQUIRE(out_scores || n <= 0, "evr_brisque_score: null pointer");
    return brisque_run(h, img, n, H, W, clip, out_scores, nullptr, workspace, workspace_bytes, stream, "evr_brisque_score");
}

extern "C" int evr_brisque_features(evr_brisque* h, const float* img, int n, int H, int W, int clip, double* out_feat,
                                    void* workspace, size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE(out_feat || n <= 0, "evr_brisque_features: null pointer");
    return brisque_run(h, img, n, H, W, clip, nullptr, out_feat, workspace, workspace_bytes, stream, "evr_brisque_features");
}

// =====================================================================================================================
// PIQE (N. Venkatanath, D. Praneeth, M. Chandrasekhar Bh, S. S. Channappayya, S. S. Medasani, "Blind image quality
// evaluation using perception based features", NCC 2015): the no-reference score of the reference's `-qm piqe` (-> pyiqa),
// as MATLAB's `piqe` and pyiqa's `piqe` compute it.  Opinion-unaware and training-free: no model file, no weights, no
// handle.  Conventions (tests/piqe_ref.py states them in the same words):
//   input     u = rint(255 * clip(v)) in fp32 (half to even), fp64 from here on
//   padding   bottom and right up to multiples of 16 by edge replication (MATLAB's padarray(..., 'replicate', 'post')),
//             THEN the filter
//   MSCN      mu = G*u, sigma = sqrt(|G*(u.u) - mu^2|), m = (u - mu)/(sigma + 1); G: NIQE's 7x7 Gaussian, sigma 7/6, sum 1,
//             a correlation with a replicate border over the padded image, the 49 taps accumulated row by row
//   block     per 16 x 16 block of m: var = the unbiased variance of its 256 values (N - 1); active iff var > 0.1
//   whsa      (noticeable artefacts) the four edges of an active block -- first row, last row, first column, last column --
//             have 16 values and 11 sliding segments of length 6 each; set iff any of the 44 segments has an unbiased
//             standard deviation < 0.1
//   wnc       (noise) centre = the two central columns (0-based 7 and 8, 32 values), surround = the other 14 columns (224
//             values); r = std(centre)/std(surround), unbiased, a NaN ratio (0/0) becomes 0; sg = sqrt(var),
//             beta = |sg - r| / max(sg, r); set iff sg > 2 beta
//   block     contribution: 1 - var if whsa (with or without wnc), var if only wnc, 0 otherwise
//   score     100 (sum of contributions + 1) / (1 + number of active blocks); a frame with no active block (a constant
//             frame) scores exactly 100: the formula's own value, not a special case
//   NaN       comparisons with NaN are false
// The centre columns and the 'post' padding are this project's reading of the ports, stated here as conventions.
// (Replicating the padded image's border is replicating the frame's: an index is clamped to the frame, once.)
// Launches per batch, whatever n: the block kernel (one work-group per 32 x 32 tile = 2 x 2 blocks of one frame, one wave
// per block; the MSCN map lives in LDS only: the frame is read once) and the finisher (one work-group per frame adds the
// block records in a fixed order).  No atomics: results are bitwise independent of the batch.
// Tile: 38 x 39 fp32 + 32 x 33 fp64 = 14.4 KB of LDS -> eight 4-wave work-groups per CU (the 32-wave cap, not LDS, bounds the
// occupancy), and a 346 x 260 frame is 99 work-groups; a 4 x 4-block tile (52 KB) would leave three per CU and 30 per frame.

namespace {

constexpr int PB = 16;                 // block
constexpr int PTB = 2;                 // blocks per tile side: one wave per block
constexpr int PT = PB * PTB;           // tile: PT x PT pixels per work-group
constexpr unsigned char PIQE_ACTIVE = 1, PIQE_WHSA = 2, PIQE_WNC = 4;
static_assert(PTB * PTB == NT / 64, "one wave per block");

__device__ __forceinline__ double wave_sum_all(double v) { return __shfl(evr_wave_sum(v), 0, 64); }

// One work-group per (tile, frame).  var / contribution / flags: [n, nby, nbx], blocks in raster order.
__global__ __launch_bounds__(NT) void piqe_block_kernel(const float* __restrict__ img, int H, int W, int clip, int nby, int nbx,
                                                        int ntx, Taps taps, double* __restrict__ var_out,
                                                        double* __restrict__ contribution, unsigned char* __restrict__ flags) {
    constexpr int TS = PT + 6;
    __shared__ float tile[TS][TS + 1];
    __shared__ double m[PT][PT + 1];
    const int t = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int y0 = (t / ntx) * PT, x0 = (t % ntx) * PT;
    const float* src = img + (int64_t)f * H * W;

    for (int i = tid; i < TS * TS; i += NT) {
        const int r = i / TS, c = i % TS;
        tile[r][c] = quant(src[(int64_t)clampi(y0 + r - 3, H) * W + clampi(x0 + c - 3, W)], clip);
    }
    __syncthreads();
    // four pixels of one row per thread: a row of the neighbourhoods is read, widened and squared once for the four;
    // each pixel's taps still accumulate row by row, as mscn_at does
    static_assert(PT * PT == 4 * NT, "four pixels per thread");
    {
        const int r = tid / (PT / 4), c = (tid % (PT / 4)) * 4;
        double mu[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0}, centre[4];
#pragma unroll
        for (int dy = 0; dy < 7; ++dy) {
            double v[10], q[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                v[k] = (double)tile[r + dy][c + k];
                q[k] = v[k] * v[k];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (dy == 3) centre[p] = v[p + 3];
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) {
                    const double g = taps.g[dy * 7 + dx];
                    mu[p] = mu[p] + g * v[p + dx];
                    s2[p] = s2[p] + g * q[p + dx];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) m[r][c + p] = mscn_close(centre[p], mu[p], s2[p]).m;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int oy = (wave / PTB) * PB, ox = (wave % PTB) * PB;
    const int by = (y0 + oy) / PB, bx = (x0 + ox) / PB;
    if (by >= nby || bx >= nbx) return;                        // a ragged tile: no such block (no barrier follows)

    // lane l holds row l / 4, columns 4 (l % 4) .. + 3; columns 7 and 8 are the last of quarter 1 and the first of quarter 2
    const int q = lane & 3;
    const double* row = &m[oy + (lane >> 2)][ox + 4 * q];
    const double x0v = row[0], x1v = row[1], x2v = row[2], x3v = row[3];
    const bool c0 = q == 2, c3 = q == 1;                       // x0v / x3v lies in the centre
    const double sum_c = wave_sum_all((c0 ? x0v : 0.0) + (c3 ? x3v : 0.0));
    const double sum_s = wave_sum_all((((c0 ? 0.0 : x0v) + x1v) + x2v) + (c3 ? 0.0 : x3v));
    const double sum_a = wave_sum_all(((x0v + x1v) + x2v) + x3v);
    const double mean_a = sum_a / 256.0, mean_c = sum_c / 32.0, mean_s = sum_s / 224.0;
    const double a0 = x0v - mean_a, a1 = x1v - mean_a, a2 = x2v - mean_a, a3 = x3v - mean_a;
    const double var = wave_sum_all(((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3) / 255.0;
    const double e0 = x0v - (c0 ? mean_c : mean_s), e1 = x1v - mean_s, e2 = x2v - mean_s, e3 = x3v - (c3 ? mean_c : mean_s);
    const double var_c = wave_sum_all((c0 ? e0 * e0 : 0.0) + (c3 ? e3 * e3 : 0.0)) / 31.0;
    const double var_s = wave_sum_all((((c0 ? 0.0 : e0 * e0) + e1 * e1) + e2 * e2) + (c3 ? 0.0 : e3 * e3)) / 223.0;

    // the 44 edge segments: lane = 11 edge + start
    bool low = false;
    if (lane < 44) {
        const int e = lane / 11, s = lane % 11;
        const int rr = oy + (e == 1 ? PB - 1 : (e >= 2 ? s : 0)), cc = ox + (e == 3 ? PB - 1 : (e < 2 ? s : 0));
        const int dr = e >= 2 ? 1 : 0, dc = 1 - dr;
        double v[6], sum = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            v[k] = m[rr + k * dr][cc + k * dc];
            sum = sum + v[k];
        }
        const double mean = sum / 6.0;
        double ssd = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) ssd = ssd + (v[k] - mean) * (v[k] - mean);
        low = sqrt(ssd / 5.0) < 0.1;
    }
    const bool any_low = __any(low ? 1 : 0) != 0;

    if (lane == 0) {
        unsigned char fl = 0;
        double contrib = 0.0;
        if (var > 0.1) {
            double r = sqrt(var_c) / sqrt(var_s);
            if (isnan(r)) r = 0.0;
            const double sg = sqrt(var);
            const double beta = fabs(sg - r) / (sg > r ? sg : r);
            const bool whsa = any_low, wnc = sg > 2.0 * beta;
            fl = PIQE_ACTIVE | (whsa ? PIQE_WHSA : 0) | (wnc ? PIQE_WNC : 0);
            contrib = whsa ? 1.0 - var : (wnc ? var : 0.0);
        }
        const int64_t o = ((int64_t)f * nby + by) * nbx + bx;
        var_out[o] = var;
        contribution[o] = contrib;
        flags[o] = fl;
    }
}

// One work-group per frame: the block records in a fixed order (thread t takes blocks t, t + 256, ...; then the waves).
__global__ __launch_bounds__(NT) void piqe_finish_kernel(const double* __restrict__ contribution,
                                                         const unsigned char* __restrict__ flags, int nb,
                                                         double* __restrict__ scores) {
    __shared__ double red[NT / 64];
    __shared__ int cnt[NT / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    int c = 0;
    for (int b = tid; b < nb; b += NT) {
        s += contribution[(int64_t)f * nb + b];
        c += wave_votes(flags[(int64_t)f * nb + b] & PIQE_ACTIVE);
    }
    const double sum = block_total(s, red);
    const int active = block_count(c, cnt);
    if (tid == 0) scores[f] = 100.0 * ((sum + 1.0) / (1.0 + (double)active));
}

struct PDims {                       // the block and tile counts
    int nby, nbx, nb, ntx, nt;
    PDims(int H, int W)
        : nby((H + PB - 1) / PB), nbx((W + PB - 1) / PB), nb(nby * nbx), ntx((nbx + PTB - 1) / PTB),
          nt(((nby + PTB - 1) / PTB) * ntx) {}
};

struct PiqeWs : Carve {              // the workspace: a member takes the next region, in the members' order
    double *var, *contrib;
    unsigned char* flags;
    PiqeWs(void* ws, size_t n, const PDims& d)
        : Carve(ws), var(take<double>(n * d.nb)), contrib(take<double>(n * d.nb)), flags(take<unsigned char>(n * d.nb)) {}
};

const Taps& piqe_taps() {
    static const Taps t = gaussian_taps();
    return t;
}

}  // namespace

extern "C" size_t evr_piqe_workspace_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || W < 1) return 0;
    return PiqeWs(nullptr, n, PDims(H, W)).bytes();
}

static int piqe_run(const float* img, int n, int H, int W, int clip, double* scores, double* out_var, unsigned char* out_flags,
                    void* ws, size_t ws_bytes, evr_stream_t stream_, const char* what) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE((int64_t)H * W <= (int64_t)1 << 30, "%s: %d x %d frame is too large", what, H, W);
    const int rc = check_run(what, 1, n, H, W, img && (scores || (out_var && out_flags)));
    if (rc != EVR_OK) return rc;
    EVR_REQUIRE_WORKSPACE(what, ws, ws_bytes, evr_piqe_workspace_bytes(n, H, W));
    const PDims d(H, W);
    const PiqeWs w(ws, n, d);
    double* var = out_var ? out_var : w.var;
    unsigned char* flags = out_flags ? out_flags : w.flags;
    const int run = for_frame_chunks(n, [&](int f0, int nf) -> int {
        const size_t o = (size_t)f0 * d.nb;
        hipLaunchKernelGGL(piqe_block_kernel, dim3(d.nt, nf), dim3(NT), 0, stream, img + (size_t)f0 * H * W, H, W, clip, d.nby,
                           d.nbx, d.ntx, piqe_taps(), var + o, w.contrib + o, flags + o);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
    if (run != EVR_OK) return run;
    if (scores) {
        hipLaunchKernelGGL(piqe_finish_kernel, dim3(n), dim3(NT), 0, stream, (const double*)w.contrib,
                           (const unsigned char*)flags, d.nb, scores);
        EVR_LAUNCH_CHECK();
    }
    return EVR_OK;
}

extern "C" int evr_piqe_score(const float* img, int n, int H, int W, int clip, double* out_scores, void* workspace,
                              size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE(out_scores, "evr_piqe_score: null pointer");
    return piqe_run(img, n, H, W, clip, out_scores, nullptr, nullptr, workspace, workspace_bytes, stream, "evr_piqe_score");
}

extern "C" int evr_piqe_blocks(const float* img, int n, int H, int W, int clip, double* out_var, unsigned char* out_flags,
                               void* workspace, size_t workspace_bytes, evr_stream_t stream) {
    EVR_REQUIRE(out_var && out_flags, "evr_piqe_blocks: null pointer");
    return piqe_run(img, n, H, W, clip, nullptr, out_var, out_flags, workspace, workspace_bytes, stream, "evr_piqe_blocks");
}
