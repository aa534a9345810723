// Per-frame GMSD (full-reference) on gfx950, in fp64, with its GMS map.
//
// Xue, Zhang, Mou & Bovik, "Gradient Magnitude Similarity Deviation", IEEE TIP 2014; pyiqa's `gmsd`.  Reference call sites:
// utils/eval_metrics.py:195-203 (any metric name other than mse / ssim is a pyiqa metric), :253-255 (clip to [0,1]), :119-147
// (queued in groups of four; the tracker books the scores, eval_metrics.py here).  For one frame pair `img`, `ref`, both
// float32 [H, W]:
//   1. luminance  u = rint(255 * clip(v, 0, 1)) in float32, round half to even, then exact in fp64 (what the NIQE, BRISQUE and
//                 PIQE kernels do; pyiqa's to_y_channel(x, 255) on a grey frame replicated to three channels is recalled to
//                 round the same way: a convention until tests/test_gmsd_pins.py has run).  With clip = 0 the clamp is left
//                 out and the rounding stays.
//   2. pooling    2x2 mean at stride 2 with no padding: h2 = H // 2, w2 = W // 2, a trailing odd row or column is dropped (it
//                 does not exist in the pooled plane).  p = 0.25 * (((a00 + a01) + a10) + a11): exact, the inputs being
//                 integers.
//   3. gradients  Prewitt on the pooled plane with zero padding of one pixel (F.conv2d(..., padding=1) in pyiqa, conv2 'same'
//                 in MATLAB), indices [row offset, column offset], the three-term sums added left to right:
//                 gx = ((p[-1,-1] + p[0,-1] + p[+1,-1]) - (p[-1,+1] + p[0,+1] + p[+1,+1])) / 3,
//                 gy the same with the roles of row and column exchanged (the sign does not reach the score);
//                 g = sqrt((gx*gx + gy*gy) + 1e-12).
//   4. GMS map    q = (2 * g_img * g_ref + 170) / ((g_img^2 + g_ref^2) + 170), so q in (0, 1].
//   5. score      the standard deviation of q over the N = h2 * w2 pooled pixels with N - 1 in the denominator (torch.std's
//                 default, MATLAB's std2), formed from the moments of d = 1 - q:
//                 var = (sum d^2 - (sum d)^2 / N) / (N - 1), clamped at 0 before the square root (1 - q is exact for
//                 q >= 0.5 and keeps the sums small for similar frames: identical frames score exactly 0).
//                 Needs H >= 2 and W >= 2; N == 1 gives NaN, as torch.std does.
// Everything from step 1's output onward is fp64; tests/gmsd_ref.py is the numpy restatement the kernels are held to.  The
// score is symmetric in its two arguments to the last bit: (2a) * b is an exact scaling and the two additions commute.
//
// Two launches.  The tile kernel stages the source pixels of a TH x TW tile of the pooled plane plus a one-pixel pooled halo
// of both frames in LDS, clipped and quantised; pools them on chip (a pooled pixel beyond the pooled plane is the zero padding
// of step 3 -- the dropped odd row or column is never read); forms both gradient magnitudes and q, writes the map if asked and
// reduces sum d and sum d^2 to one fp64 pair per tile.  The finisher adds a frame's pairs in tile order and writes the score
// and 1 - sum d / N.  No atomics: a frame's numbers and its map do not depend on n, on its place in the batch or on earlier
// calls (the tile and frame sums and the frame chunks are the family's scaffold, metric_tiles.h).  Algorithmic bytes per frame: 2*4*H*W read (8*h2*w2 written with the map).
#include "metric_tiles.h"
#include <cmath>

namespace {

using namespace evr_tiles;

constexpr int TH = 16, TW = 32;              // pooled pixels per tile: 512, two per thread
constexpr int PH = TH + 2, PW = TW + 2;      // ... with the one-pixel halo
constexpr int SH = 2 * PH, SW = 2 * PW;      // the source pixels under them (36 x 68)

__device__ __forceinline__ float quant(float v, int clip) {
    if (clip) v = fminf(fmaxf(v, 0.f), 1.f);
    return rintf(255.f * v);
}

__device__ __forceinline__ double grad_mag(const double (*p)[PW + 1], int r, int c) {
    // p[r][c] is the centre; rows r - 1 .. r + 1 and columns c - 1 .. c + 1 are staged
    const double gx = (((p[r - 1][c - 1] + p[r][c - 1]) + p[r + 1][c - 1]) - ((p[r - 1][c + 1] + p[r][c + 1]) + p[r + 1][c + 1])) / 3.0;
    const double gy = (((p[r - 1][c - 1] + p[r - 1][c]) + p[r - 1][c + 1]) - ((p[r + 1][c - 1] + p[r + 1][c]) + p[r + 1][c + 1])) / 3.0;
    return sqrt((gx * gx + gy * gy) + 1e-12);
}

// A = image, B = reference: [n, H, W] float32.  partials: [n, tiles, 2] = {sum d, sum d^2} of each tile, tiles in row-major
// order.  map: [n, h2, w2] or null.
__global__ __launch_bounds__(NT) void gmsd_tile_kernel(const float* __restrict__ A, const float* __restrict__ B, int H, int W, int h2,
                                                       int w2, int clip, double* __restrict__ partials, double* __restrict__ map,
                                                       int f0) {
    __shared__ __align__(8) float sa[SH][SW], sb[SH][SW];       // quantised source pixels (even row length: float2 reads below)
    __shared__ double pa[PH][PW + 1], pb[PH][PW + 1];           // pooled planes with their halo
    __shared__ double red[2][NT / 64];
    const int f = blockIdx.z + f0, ty = blockIdx.y, tx = blockIdx.x, tid = threadIdx.x;
    const float* a = A + (int64_t)f * H * W;
    const float* b = B + (int64_t)f * H * W;
    const int py0 = ty * TH - 1, px0 = tx * TW - 1;             // pooled coordinates of the staged planes' corner
    const int hs = 2 * h2, ws = 2 * w2;                         // the source region that is pooled at all

    for (int i = tid; i < SH * SW; i += NT) {
        const int r = i / SW, c = i % SW;
        const int y = 2 * py0 + r, x = 2 * px0 + c;
        float u = 0.f, v = 0.f;
        if (y >= 0 && y < hs && x >= 0 && x < ws) {
            u = quant(a[(int64_t)y * W + x], clip);
            v = quant(b[(int64_t)y * W + x], clip);
        }
        sa[r][c] = u; sb[r][c] = v;
    }
    __syncthreads();

    for (int i = tid; i < PH * PW; i += NT) {
        const int r = i / PW, c = i % PW;
        const int py = py0 + r, px = px0 + c;
        double u = 0.0, v = 0.0;                                // beyond the pooled plane: the zero padding of the gradients
        if (py >= 0 && py < h2 && px >= 0 && px < w2) {
            const float2 a0 = *reinterpret_cast<const float2*>(&sa[2 * r][2 * c]);
            const float2 a1 = *reinterpret_cast<const float2*>(&sa[2 * r + 1][2 * c]);
            const float2 b0 = *reinterpret_cast<const float2*>(&sb[2 * r][2 * c]);
            const float2 b1 = *reinterpret_cast<const float2*>(&sb[2 * r + 1][2 * c]);
            u = 0.25 * ((((double)a0.x + (double)a0.y) + (double)a1.x) + (double)a1.y);
            v = 0.25 * ((((double)b0.x + (double)b0.y) + (double)b1.x) + (double)b1.y);
        }
        pa[r][c] = u; pb[r][c] = v;
    }
    __syncthreads();

    double sd = 0.0, sd2 = 0.0;
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i % TW;
        const int py = ty * TH + r, px = tx * TW + c;
        if (py >= h2 || px >= w2) continue;
        const double ga = grad_mag(pa, r + 1, c + 1), gb = grad_mag(pb, r + 1, c + 1);
        const double q = ((2.0 * ga) * gb + 170.0) / ((ga * ga + gb * gb) + 170.0);
        if (map) map[((int64_t)f * h2 + py) * w2 + px] = q;
        const double d = 1.0 - q;
        sd += d; sd2 += d * d;
    }
    tile_partials(red, partials, [&] { return (int64_t)f * gridDim.x * gridDim.y; }, sd, sd2);
}

// One block per frame: its tiles' pairs in tile order, then the score and the mean GMS.
__global__ __launch_bounds__(NT) void gmsd_finish_kernel(const double* __restrict__ partials, int tiles, double N,
                                                         double* __restrict__ out, int f0) {
    __shared__ double red[NT / 64];
    __shared__ double tot[2];
    const int f = blockIdx.x + f0, tid = threadIdx.x;
    for (int q = 0; q < 2; ++q) {
        const double s = frame_total<2>(partials + (int64_t)f * tiles * 2 + q, tiles, red);
        if (tid == 0) tot[q] = s;
        __syncthreads();
    }
    if (tid != 0) return;
    const double sd = tot[0], sd2 = tot[1];
    double var = (sd2 - sd * sd / N) / (N - 1.0);               // N == 1: 0 / 0, NaN as torch.std gives
    if (var < 0.0) var = 0.0;                                   // (a NaN passes through)
    out[(int64_t)f * 2 + 0] = sqrt(var);
    out[(int64_t)f * 2 + 1] = 1.0 - sd / N;
}

inline int tiles_of(int H, int W) { return ((H / 2 + TH - 1) / TH) * ((W / 2 + TW - 1) / TW); }

}  // namespace

extern "C" size_t evr_gmsd_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H < 2 || W < 2) return 0;
    return (size_t)n * tiles_of(H, W) * 2 * sizeof(double) + 256;
}

extern "C" int evr_gmsd(const float* img, const float* ref, int n, int H, int W, int clip, double* out, double* out_map,
                        void* workspace, size_t workspace_bytes, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(n >= 0 && H >= 1 && W >= 1, "evr_gmsd: bad shape");
    EVR_REQUIRE(H >= 2 && W >= 2, "evr_gmsd: needs frames of at least 2 x 2 pixels (one pixel of the 2x2-pooled plane), got %d x %d", H,
                W);
    if (n == 0) return EVR_OK;
    EVR_REQUIRE(img && ref && out, "evr_gmsd: null pointer");
    const size_t need = evr_gmsd_workspace_bytes(n, H, W);
    EVR_REQUIRE_WORKSPACE("evr_gmsd", workspace, workspace_bytes, need);
    const int h2 = H / 2, w2 = W / 2;
    const int gy = (h2 + TH - 1) / TH, gx = (w2 + TW - 1) / TW;
    EVR_REQUIRE(gy <= 65535, "evr_gmsd: frames of more than %d rows are not supported, got %d", 65535 * 2 * TH, H);
    double* partials = (double*)workspace;
    return for_frame_chunks(n, [&](int f0, int nf) -> int {
        hipLaunchKernelGGL(gmsd_tile_kernel, dim3(gx, gy, nf), dim3(NT), 0, stream, img, ref, H, W, h2, w2, clip, partials, out_map, f0);
        EVR_LAUNCH_CHECK();
        hipLaunchKernelGGL(gmsd_finish_kernel, dim3(nf), dim3(NT), 0, stream, partials, gx * gy, (double)h2 * (double)w2, out, f0);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    });
}
