// Per-frame VIFp (pixel-domain Visual Information Fidelity, full-reference) on gfx950, in fp64.
//
// Sheikh & Bovik, "Image Information and Visual Quality", IEEE TIP 2006, in its pixel-domain multi-scale form: vifp_mscale.m of
// the LIVE release, sewar.vifp.  For one frame pair `img` (the reconstruction, "distorted") and `ref`, both float32 [H, W]:
//   0. input     with clip, both are clamped to [0,1] in fp32; then x = 255.0 * (double)ref, y = 255.0 * (double)img.  Nothing is
//                quantised to bytes; everything from here on is fp64 and a pyramid level is never rounded back to fp32.
//   1. windows   scale s = 1..4 has N = 2^(5-s) + 1 = 17, 9, 5, 3 taps, w_k = exp(-(k - (N-1)/2)^2 / (2 (N/5)^2)) normalised to
//                sum 1 (evr_vifp_taps returns the very numbers); F(a) is the window w (x) w over the VALID region only, as two
//                separable passes, axis 0 first and then axis 1, the taps added in index order (a = w0*v0; a += wk*vk), no
//                contraction into fused multiply-adds.
//   2. pyramid   for s > 1: x = F(x)[::2, ::2], y = F(y)[::2, ::2] with this scale's own window, the even indices kept: a side
//                becomes ceil((side - N + 1) / 2).
//   3. moments   mu1 = F(x), mu2 = F(y), s1 = F(x*x) - mu1*mu1, s2 = F(y*y) - mu2*mu2, s12 = F(x*y) - mu1*mu2;
//                s1 = max(s1, 0), s2 = max(s2, 0); g = s12 / (s1 + EPS); sv = s2 - g*s12; then, in this order:
//                s1 < EPS: g = 0, sv = s2, s1 = 0;  s2 < EPS: g = 0, sv = 0;  g < 0: sv = s2, g = 0;  sv <= EPS: sv = EPS
//                (EPS = 1e-10, as the MATLAB release and sewar; piq.vif_p uses 1e-8).
//   4. score     num_s = sum log10(1 + g*g*s1 / (sv + 2)), den_s = sum log10(1 + s1 / 2) (sigma_nsq = 2);
//                vifp = (((num_1 + num_2) + num_3) + num_4) / (((den_1 + den_2) + den_3) + den_4), no epsilon: a reference
//                that is flat everywhere gives 0 / 0 = NaN.
// Needs min(H, W) >= 41: the sides go 41 -> 17 -> 7 -> 3 and the last scale holds one 3 x 3 window.  tests/vifp_ref.py is the
// numpy restatement the kernels are held to.
//
// One launch per scale.  A work-group owns a TH x TW tile of window ANCHORS (a window starts at its output pixel: only the valid
// region exists, nothing is centred) and stages the (TH + N - 1) x (TW + N - 1) pixels under them of both planes in LDS as fp64
// (255 * (double)clamped float at scale 1, the fp64 level below).  From that one staged tile it
//   * writes the pixels of the NEXT level whose anchor (2i, 2j) lies in the tile: the valid filter with the next scale's shorter
//     window -- pass 1 into the first two intermediate planes, pass 2 to global memory;
//   * runs both separable passes of the five moments on chip and reduces its num and den terms to one fp64 pair.
// So each level is read once and the next one written once.  The next level's anchors reach further (side - N' + 1 > side - N
// + 1): the grid covers them and the moment sums are masked to their own domain.  A finishing launch (one work-group per
// frame) adds a frame's pairs in tile order and forms the ratio.  The moment passes, the tile and frame sums, the workspace
// plan and the frame chunks are the family's scaffold (metric_tiles.h): a frame's nine numbers are bitwise independent of n
// and of its place in the batch.
//
// Tile: 16 x 32 anchors at every scale, 256 threads, two anchors per thread.  LDS at scale 1 (the largest): 2 staged planes of
// 32 x 48 doubles (rows padded to 49: 25,088 B) + 5 intermediate planes of 16 x 48 (31,360 B) + 64 B = 56,512 B, so two
// work-groups are resident in a CU's 160 KiB (the 64 KiB a work-group may hold caps the tile; a 16 x 64 tile would need 94 KB).
// Scale 2 holds 42,048 B (three resident), scales 3 and 4 35,584 and 32,544 B.  Rows of 49 / 41 / 37 / 35 doubles: lanes of a
// wave walk consecutive doubles of a row in both passes (ds_read_b64, 32 lanes a group: conflict-free but where a group wraps
// to the next row in pass 1, two-way).  Algorithmic bytes per frame: 2*4*H*W read at scale 1, 2*8*h*w written then read for
// each of the three lower levels (0.33 of a frame's pixels together).
#include "metric_tiles.h"
#include <cmath>

namespace {

using namespace evr_tiles;

constexpr int SCALES = 4;
constexpr int MIN_SIDE = 41;         // 41 -> 17 -> 7 -> 3: the fourth scale still holds one 3 x 3 window
constexpr int MAX_TAPS = 17;
constexpr int TH = 16, TW = 32;      // anchors per tile (both even: a tile owns whole next-level pixels)
constexpr double EPS = 1e-10, SIGMA_NSQ = 2.0;

constexpr int taps_of(int s) { return (1 << (5 - s)) + 1; }      // s = 1..4

struct Taps { double w[MAX_TAPS]; double wn[MAX_TAPS / 2 + 1]; };   // this scale's window, the next scale's

void make_taps(int s, double* w) {
    const int N = taps_of(s);
    const double sd = (double)N / 5.0, mid = (double)(N - 1) / 2.0;
    double sum = 0.0;
    for (int k = 0; k < N; ++k) {
        const double d = (double)k - mid;
        w[k] = std::exp(-(d * d) / (2.0 * sd * sd));
        sum += w[k];
    }
    for (int k = 0; k < N; ++k) w[k] /= sum;
}

__device__ __forceinline__ double stage(float v, int clip) {
    if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
    return 255.0 * (double)v;
}
__device__ __forceinline__ double stage(double v, int) { return v; }

// X = reference, Y = image of one level: [n, h, w] of T.  partials: [n, tiles_total, 2] = {num, den}, this scale's tiles from
// tile_off on in row-major order.  PX / PY: the next level [n, h2, w2] in fp64, or null at the last scale (NN is unused then).
template <typename T, int N, int NN>
__global__ __launch_bounds__(NT) void vifp_scale_kernel(const T* __restrict__ Xl, const T* __restrict__ Yl, int h, int w, int clip,
                                                        Taps g, double* __restrict__ partials, int tiles_total, int tile_off,
                                                        double* __restrict__ PX, double* __restrict__ PY, int h2, int w2, int f0) {
    constexpr int IH = TH + N - 1, IW = TW + N - 1;
    __shared__ double sx[IH][IW + 1], sy[IH][IW + 1];
    __shared__ double v[5][TH][IW + 1];      // after the pass along axis 0: x, y, xx, yy, xy (first the next level's x, y)
    __shared__ double red[2][NT / 64];
    const int f = blockIdx.z + f0, ty = blockIdx.y, tx = blockIdx.x, tid = threadIdx.x;
    const T* X = Xl + (int64_t)f * h * w;
    const T* Y = Yl + (int64_t)f * h * w;
    const int y0 = ty * TH, x0 = tx * TW;

    for (int i = tid; i < IH * IW; i += NT) {
        const int r = i / IW, c = i % IW;
        const int yy = y0 + r, xx = x0 + c;
        double a = 0.0, b = 0.0;             // beyond the level: never inside a valid window
        if (yy < h && xx < w) { a = stage(X[(int64_t)yy * w + xx], clip); b = stage(Y[(int64_t)yy * w + xx], clip); }
        sx[r][c] = a; sy[r][c] = b;
    }
    __syncthreads();

    if (PX) {   // the next level's pixels (i, j) with the anchor (2i, 2j) in this tile: F'(x)[2i, 2j], axis 0 then axis 1
        for (int i = tid; i < (TH / 2) * IW; i += NT) {
            const int r = i / IW, c = i % IW;
            double a = g.wn[0] * sx[2 * r][c], b = g.wn[0] * sy[2 * r][c];
#pragma unroll
            for (int k = 1; k < NN; ++k) { a += g.wn[k] * sx[2 * r + k][c]; b += g.wn[k] * sy[2 * r + k][c]; }
            v[0][r][c] = a; v[1][r][c] = b;
        }
        __syncthreads();
        for (int i = tid; i < (TH / 2) * (TW / 2); i += NT) {
            const int r = i / (TW / 2), c = i % (TW / 2);
            const int oy = (y0 >> 1) + r, ox = (x0 >> 1) + c;
            if (oy >= h2 || ox >= w2) continue;          // the window would leave the level
            double a = g.wn[0] * v[0][r][2 * c], b = g.wn[0] * v[1][r][2 * c];
#pragma unroll
            for (int j = 1; j < NN; ++j) { a += g.wn[j] * v[0][r][2 * c + j]; b += g.wn[j] * v[1][r][2 * c + j]; }
            const int64_t o = ((int64_t)f * h2 + oy) * w2 + ox;
            PX[o] = a; PY[o] = b;
        }
        __syncthreads();
    }

    // pass 1: along axis 0, for every staged column (rows r .. r + N - 1 belong to anchor row r)
    moments_pass1<N, TH, TW>(sx, sy, g.w, v);
    __syncthreads();

    // pass 2: along axis 1, and the num / den terms over this scale's own valid region
    double num = 0.0, den = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i % TW;
        if (y0 + r > h - N || x0 + c > w - N) continue;
        double u[5];
        moments_pass2<N, TH, TW>(v, g.w, r, c, u);
        const double mu1 = u[0], mu2 = u[1];
        double s1 = u[2] - mu1 * mu1, s2 = u[3] - mu2 * mu2;
        const double s12 = u[4] - mu1 * mu2;
        if (s1 < 0.0) s1 = 0.0;
        if (s2 < 0.0) s2 = 0.0;
        double gain = s12 / (s1 + EPS);
        double sv = s2 - gain * s12;
        if (s1 < EPS) { gain = 0.0; sv = s2; s1 = 0.0; }
        if (s2 < EPS) { gain = 0.0; sv = 0.0; }
        if (gain < 0.0) { sv = s2; gain = 0.0; }
        if (sv <= EPS) sv = EPS;
        num += log10(1.0 + ((gain * gain) * s1) / (sv + SIGMA_NSQ));
        den += log10(1.0 + s1 / SIGMA_NSQ);
    }
    tile_partials(red, partials, [&] { return (int64_t)f * tiles_total + tile_off; }, num, den);
}

// One block per frame: the pairs of every scale in tile order, then the row {score, num_1..4, den_1..4}.
__global__ __launch_bounds__(NT) void vifp_finish_kernel(const double* __restrict__ partials, LevelTiles<SCALES> p,
                                                         double* __restrict__ out, int f0) {
    __shared__ double red[NT / 64];
    __shared__ double tot[SCALES][2];
    const int f = blockIdx.x + f0, tid = threadIdx.x;
    for (int l = 0; l < SCALES; ++l) {
        for (int q = 0; q < 2; ++q) {
            const double a = frame_total<2>(partials + ((int64_t)f * p.tiles_total + p.tile_off[l]) * 2 + q, p.tiles[l], red);
            if (tid == 0) tot[l][q] = a;
            __syncthreads();
        }
    }
    if (tid != 0) return;
    double* o = out + (int64_t)f * 9;
    const double num = ((tot[0][0] + tot[1][0]) + tot[2][0]) + tot[3][0];
    const double den = ((tot[0][1] + tot[1][1]) + tot[2][1]) + tot[3][1];
    o[0] = num / den;                                            // a flat reference: 0 / 0, NaN
#pragma unroll
    for (int l = 0; l < SCALES; ++l) { o[1 + l] = tot[l][0]; o[5 + l] = tot[l][1]; }
}

using VifPlan = Plan<SCALES>;

VifPlan make_plan(int n, int H, int W) {
    VifPlan p{};
    for (int l = 0, h = H, w = W; l < SCALES; ++l) {
        // anchors: the next level's valid domain where there is one (it contains this scale's own)
        const int N = l + 1 < SCALES ? taps_of(l + 2) : taps_of(l + 1);
        p.add_level(n, h, w, (h - N + 1 + TH - 1) / TH, (w - N + 1 + TW - 1) / TW);
        h = (h - N + 2) / 2; w = (w - N + 2) / 2;               // the next level: ceil((side - N + 1) / 2)
    }
    p.close(n, 2);
    return p;
}

template <typename T, int N, int NN>
void launch_scale(const T* x, const T* y, const VifPlan& p, int l, int n, int nf, int f0, int clip, void* ws, hipStream_t stream) {
    Taps g{};
    make_taps(l + 1, g.w);
    if (l + 1 < SCALES) make_taps(l + 2, g.wn);
    const VifPlan::Next nx = p.next(ws, l, SCALES, n);
    hipLaunchKernelGGL((vifp_scale_kernel<T, N, NN>), dim3(p.tx[l], p.ty[l], nf), dim3(NT), 0, stream, x, y, p.h[l], p.w[l], clip, g,
                       p.partials(ws), p.t.tiles_total, p.t.tile_off[l], nx.x, nx.y, nx.h, nx.w, f0);
}

}  // namespace

extern "C" int evr_vifp_taps(int scale, double* taps) {
    EVR_REQUIRE(scale >= 1 && scale <= SCALES, "evr_vifp_taps: scale must be 1..%d, got %d", SCALES, scale);
    EVR_REQUIRE(taps, "evr_vifp_taps: null pointer");
    make_taps(scale, taps);
    return EVR_OK;
}

extern "C" size_t evr_vifp_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H < MIN_SIDE || W < MIN_SIDE) return 0;
    return make_plan(n, H, W).bytes;
}

extern "C" int evr_vifp(const float* img, const float* ref, int n, int H, int W, int clip, double* out, void* workspace,
                        size_t workspace_bytes, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(n >= 0 && H >= 1 && W >= 1, "evr_vifp: bad shape");
    EVR_REQUIRE(H >= MIN_SIDE && W >= MIN_SIDE,
                "evr_vifp: needs frames of at least %d x %d pixels (four scales, the last one 3 x 3 window), got %d x %d", MIN_SIDE,
                MIN_SIDE, H, W);
    if (n == 0) return EVR_OK;
    EVR_REQUIRE(img && ref && out, "evr_vifp: null pointer");
    const VifPlan p = make_plan(n, H, W);
    EVR_REQUIRE(workspace && workspace_bytes >= p.bytes, "evr_vifp: workspace %zu B < required %zu B", workspace_bytes, p.bytes);
    EVR_REQUIRE(p.ty[0] <= 65535, "evr_vifp: frames of more than %d rows are not supported, got %d", 65535 * TH, H);
    auto level = [&](int l, int which) { return (const double*)p.plane(workspace, l, which, n); };
    return for_frame_chunks(n, [&](int f0, int nf) -> int {
        launch_scale<float, 17, 9>(ref, img, p, 0, n, nf, f0, clip, workspace, stream);
        EVR_LAUNCH_CHECK();
        launch_scale<double, 9, 5>(level(1, 0), level(1, 1), p, 1, n, nf, f0, 0, workspace, stream);
        EVR_LAUNCH_CHECK();
        launch_scale<double, 5, 3>(level(2, 0), level(2, 1), p, 2, n, nf, f0, 0, workspace, stream);
        EVR_LAUNCH_CHECK();
        launch_scale<double, 3, 1>(level(3, 0), level(3, 1), p, 3, n, nf, f0, 0, workspace, stream);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(vifp_finish_kernel, dim3(nf), dim3(NT), 0, stream, p.partials(workspace), p.t, out, f0);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
}
