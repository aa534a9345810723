// Per-frame PSNR and MS-SSIM (full-reference) on gfx950, in fp64.
//
// Reference call sites: utils/eval_metrics.py:195-203 (any metric name other than mse / ssim is a pyiqa metric),
// :253-255 (clip to [0,1]), :119-147 (queued in groups of four; the tracker books the scores, eval_metrics.py here).
//   psnr    : 10 log10(1 / (mse + 1e-8)); mse with the arithmetic of metrics.hip (fp32 difference, fp32 square, fp64 sum
//             over the same 16 x 64 tiles in the same order).
//   ms_ssim : Wang, Simoncelli & Bovik 2003 as pytorch-msssim / pyiqa compute it on [0,1] frames (data_range 1): five
//             scales, 11-tap Gaussian (sigma 1.5) over the VALID region only (maps of (h-10) x (w-10)), axis 0 then
//             axis 1, taps added in index order; per pixel cs = (2 vxy + C2) / (vx + vy + C2),
//             s = (2 ux uy + C1) / (ux^2 + uy^2 + C1) * cs; CS_l, S_l = plain means; next scale = 2x2 mean, stride 2, an
//             odd side zero-padded by one on BOTH ends first (avg_pool2d(x, 2, padding=(h % 2, w % 2)): the leading pad
//             counts in the mean, the trailing one is never reached);
//             score = prod_{l<5} max(CS_l, 0)^w_l * max(S_5, 0)^w_5.  Needs min(H, W) >= 161.
// Every moment, map, mean and pyramid level is fp64 (a level is never rounded back to fp32); tests/frmetrics_ref.py is the
// numpy restatement the kernels are held to.
//
// One launch per scale: a tile of the level plus its 5-pixel halo is staged in LDS (fp32 at scale 1, fp64 below), both
// separable passes run on chip, the tile writes fp64 partial sums of its cs and s maps (and of the squared error at scale 1)
// and -- from the same staged tile -- the pooled pixels of the next level whose lower-right source pixel it owns.  Each level
// is read once and the next one written once.  A finishing launch adds a frame's partials in a fixed order and applies the
// clamp, the powers and the PSNR formula, so a frame's numbers do not depend on n or on its place in the batch.  The moment
// passes, the tile and frame sums, the workspace plan and the frame chunks are the family's scaffold (metric_tiles.h).
// Algorithmic bytes per frame: 2*4*H*W read at scale 1, 2*8*h_l*w_l written then read for each of the four pooled levels.
#include "metric_tiles.h"
#include <cmath>

namespace {

using namespace evr_tiles;

constexpr int R = 5;                 // Gaussian radius (11 taps)
constexpr int LEVELS = 5;
constexpr int MIN_SIDE = 161;        // 161 -> 81 -> 41 -> 21 -> 11: the fifth scale still holds one 11 x 11 window

struct Gauss { double w[2 * R + 1]; };

struct Finish {
    int levels;                      // 5 with ms_ssim, 1 for psnr alone
    LevelTiles<LEVELS> t;
    double map_px[LEVELS];           // (h_l - 10) * (w_l - 10)
    double inv_px;                   // 1 / (H * W)
    double wgt[LEVELS];
};

// X = reference, Y = image of one level: [n, h, w] of T.  partials: [n, tiles_total, 3] = {sum cs, sum s, sum sq err}, this
// level's tiles starting at tile_off.  PX / PY: the next level [n, h2, w2] in fp64, or null (last scale, psnr alone).
template <typename T, int TH, int TW>
__global__ __launch_bounds__(256) void fr_scale_kernel(const T* __restrict__ Xl, const T* __restrict__ Yl, int h, int w, int clip,
                                                        unsigned which, Gauss g, double* __restrict__ partials, int tiles_total,
                                                        int tile_off, double* __restrict__ PX, double* __restrict__ PY, int h2, int w2,
                                                        int f0) {
    constexpr int IH = TH + 2 * R, IW = TW + 2 * R;
    __shared__ T sx[IH][IW + 1], sy[IH][IW + 1];
    __shared__ double v[5][TH][IW + 1];      // after the pass along axis 0: x, y, xx, yy, xy
    __shared__ double red[3][4];
    const int f = blockIdx.z + f0, ty = blockIdx.y, tx = blockIdx.x, tid = threadIdx.x;
    const T* X = Xl + (int64_t)f * h * w;
    const T* Y = Yl + (int64_t)f * h * w;
    const int y0 = ty * TH, x0 = tx * TW;

    for (int i = tid; i < IH * IW; i += 256) {
        const int r = i / IW, c = i % IW;
        const int yy = y0 + r - R, xx = x0 + c - R;
        T a = 0, b = 0;                      // beyond the level: the zero padding of the pooling (never enters a valid window)
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            a = X[(int64_t)yy * w + xx]; b = Y[(int64_t)yy * w + xx];
            if (clip) { a = a < (T)0 ? (T)0 : (a > (T)1 ? (T)1 : a); b = b < (T)0 ? (T)0 : (b > (T)1 ? (T)1 : b); }
        }
        sx[r][c] = a; sy[r][c] = b;
    }
    __syncthreads();

    double se = 0.0, scs = 0.0, ss = 0.0;
    if constexpr (sizeof(T) == 4) {
        if (which & 1u) {   // squared error over the tile interior: the loop of metrics_tile_kernel
            for (int i = tid; i < TH * TW; i += 256) {
                const int r = i / TW, c = i % TW;
                if (y0 + r < h && x0 + c < w) {
                    const float d = sx[r + R][c + R] - sy[r + R][c + R];
                    const float d2 = d * d;
                    se += (double)d2;
                }
            }
        }
    }
    if (which & 2u) {
        if (PX) {           // the pooled pixels whose lower-right source pixel lies in this tile
            const int ph = h & 1, pw = w & 1;
            for (int i = tid; i < (TH / 2) * (TW / 2); i += 256) {
                const int r = (1 - ph) + 2 * (i / (TW / 2)), c = (1 - pw) + 2 * (i % (TW / 2));
                const int gy = y0 + r, gx = x0 + c;
                if (gy >= h || gx >= w) continue;
                const int oy = (gy + ph - 1) >> 1, ox = (gx + pw - 1) >> 1;
                if (oy >= h2 || ox >= w2) continue;
                const int64_t o = ((int64_t)f * h2 + oy) * w2 + ox;
                PX[o] = 0.25 * (((to_f64(sx[r + R - 1][c + R - 1]) + to_f64(sx[r + R - 1][c + R])) + to_f64(sx[r + R][c + R - 1])) +
                                to_f64(sx[r + R][c + R]));
                PY[o] = 0.25 * (((to_f64(sy[r + R - 1][c + R - 1]) + to_f64(sy[r + R - 1][c + R])) + to_f64(sy[r + R][c + R - 1])) +
                                to_f64(sy[r + R][c + R]));
            }
        }
        // pass 1: along axis 0, for every column of the haloed tile (rows r .. r + 10 of the staged tile centre on row r)
        moments_pass1<2 * R + 1, TH, TW>(sx, sy, g.w, v);
        __syncthreads();
        // pass 2: along axis 1, and the cs / s maps over the valid region
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        for (int i = tid; i < TH * TW; i += 256) {
            const int r = i / TW, c = i % TW;
            const int gy = y0 + r, gx = x0 + c;
            if (gy < R || gy >= h - R || gx < R || gx >= w - R) continue;
            double u[5];
            moments_pass2<2 * R + 1, TH, TW>(v, g.w, r, c, u);
            const double ux = u[0], uy = u[1];
            const double vx = u[2] - ux * ux, vy = u[3] - uy * uy, vxy = u[4] - ux * uy;
            const double cs = (2.0 * vxy + C2) / (vx + vy + C2);
            const double s = (2.0 * ux * uy + C1) / (ux * ux + uy * uy + C1) * cs;
            scs += cs; ss += s;
        }
    }
    tile_partials(red, partials, [&] { return (int64_t)f * tiles_total + tile_off; }, scs, ss, se);
}

// One block per frame: the partials of every level in tile order, then the scores.
__global__ __launch_bounds__(256) void fr_finish_kernel(const double* __restrict__ partials, Finish p, unsigned which,
                                                         double* __restrict__ out_scores, double* __restrict__ out_scales, int f0) {
    __shared__ double red[4];
    __shared__ double tot[LEVELS][3];
    const int f = blockIdx.x + f0, tid = threadIdx.x;
    for (int l = 0; l < p.levels; ++l) {
        for (int q = 0; q < 3; ++q) {
            const double a = frame_total<3>(partials + ((int64_t)f * p.t.tiles_total + p.t.tile_off[l]) * 3 + q, p.t.tiles[l], red);
            if (tid == 0) tot[l][q] = a;
            __syncthreads();
        }
    }
    if (tid != 0) return;
    double psnr = 0.0, score = 0.0, cs[LEVELS] = {0, 0, 0, 0, 0}, s[LEVELS] = {0, 0, 0, 0, 0};
    if (which & 1u) {
        const double mse = tot[0][2] * p.inv_px;
        psnr = 10.0 * log10(1.0 / (mse + 1e-8));
    }
    if (which & 2u) {
        score = 1.0;
#pragma unroll
        for (int l = 0; l < LEVELS; ++l) {
            cs[l] = tot[l][0] / p.map_px[l];
            s[l] = tot[l][1] / p.map_px[l];
            const double t = l < LEVELS - 1 ? cs[l] : s[l];
            score *= pow(t > 0.0 ? t : 0.0, p.wgt[l]);
        }
    }
    out_scores[(int64_t)f * 2 + 0] = psnr;
    out_scores[(int64_t)f * 2 + 1] = score;
    if (out_scales) {
#pragma unroll
        for (int l = 0; l < LEVELS; ++l) {
            out_scales[(int64_t)f * 10 + l] = cs[l];
            out_scales[(int64_t)f * 10 + 5 + l] = s[l];
        }
    }
}

constexpr int TH0 = 16, TW0 = 64;    // scale 1 (fp32 staging): the tile of metrics.hip, 62 KiB of LDS -> two blocks per CU
constexpr int THP = 16, TWP = 32;    // pooled scales (fp64 staging): 44 KiB -> three blocks per CU

using FrPlan = Plan<LEVELS>;

FrPlan make_plan(int n, int H, int W) {
    FrPlan p{};
    const int levels = (H < W ? H : W) >= MIN_SIDE ? LEVELS : 1;
    for (int l = 0, h = H, w = W; l < levels; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        const int th = l ? THP : TH0, tw = l ? TWP : TW0;
        p.add_level(n, h, w, (h + th - 1) / th, (w + tw - 1) / tw);
    }
    p.close(n, 3);
    return p;
}

}  // namespace

extern "C" size_t evr_fr_metrics_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H < 1 || W < 1) return 0;
    return make_plan(n, H, W).bytes;
}

extern "C" int evr_fr_metrics(const float* img, const float* ref, int n, int H, int W, unsigned which, int clip,
                              double* out_scores, double* out_scales, void* workspace, size_t workspace_bytes, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(n >= 0 && H >= 1 && W >= 1, "evr_fr_metrics: bad shape");
    EVR_REQUIRE(which >= 1u && which <= 3u, "evr_fr_metrics: which must be 1 (psnr), 2 (ms_ssim) or 3 (both)");
    EVR_REQUIRE(!(which & 2u) || (H >= MIN_SIDE && W >= MIN_SIDE),
                "evr_fr_metrics: ms_ssim needs frames of at least %d x %d (five scales of an 11 x 11 window), got %d x %d", MIN_SIDE,
                MIN_SIDE, H, W);
    if (n == 0) return EVR_OK;
    EVR_REQUIRE(img && ref && out_scores, "evr_fr_metrics: null pointer");
    const FrPlan p = make_plan(n, H, W);
    EVR_REQUIRE_WORKSPACE("evr_fr_metrics", workspace, workspace_bytes, p.bytes);
    Gauss g;
    {
        double sum = 0.0;
        for (int i = -R; i <= R; ++i) { g.w[i + R] = std::exp(-0.5 * (double)i * (double)i / 2.25); sum += g.w[i + R]; }
        for (int i = 0; i < 2 * R + 1; ++i) g.w[i] /= sum;
    }
    double* partials = p.partials(workspace);
    const int levels = (which & 2u) ? LEVELS : 1;
    Finish fin{};
    fin.levels = levels;
    fin.t = p.t;
    fin.inv_px = 1.0 / ((double)H * W);
    const double wgt[LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int l = 0; l < levels; ++l) {
        fin.map_px[l] = (double)(p.h[l] - 2 * R) * (double)(p.w[l] - 2 * R);
        fin.wgt[l] = wgt[l];
    }
    return for_frame_chunks(n, [&](int f0, int nf) -> int {
        for (int l = 0; l < levels; ++l) {
            const FrPlan::Next nx = p.next(workspace, l, levels, n);
            if (l == 0) {
                hipLaunchKernelGGL((fr_scale_kernel<float, TH0, TW0>), dim3(p.tx[0], p.ty[0], nf), dim3(NT), 0, stream, ref, img, H, W,
                                   clip, which, g, partials, p.t.tiles_total, p.t.tile_off[0], nx.x, nx.y, nx.h, nx.w, f0);
            } else {
                hipLaunchKernelGGL((fr_scale_kernel<double, THP, TWP>), dim3(p.tx[l], p.ty[l], nf), dim3(NT), 0, stream,
                                   (const double*)p.plane(workspace, l, 0, n), (const double*)p.plane(workspace, l, 1, n), p.h[l],
                                   p.w[l], 0, which, g, partials, p.t.tiles_total, p.t.tile_off[l], nx.x, nx.y, nx.h, nx.w, f0);
            }
            EVR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(fr_finish_kernel, dim3(nf), dim3(NT), 0, stream, partials, fin, which, out_scores, out_scales, f0);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
}
