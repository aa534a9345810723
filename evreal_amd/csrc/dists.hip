// DISTS on gfx950 -- the 'dists' metric of the reference (utils/eval_metrics.py:100-156: pyiqa.create_metric('dists') on [n,3,H,W]
// batches built by cv2torch(img, num_ch=3), eval_utils.py:46-54).
//
// PARITY UNPINNED: pyiqa is neither in the reference tree nor installed, and the weights are downloaded at run time (unobtainable
// offline).  The arithmetic below follows the published algorithm (Ding, Ma, Wang, Simoncelli, "Image Quality Assessment: Unifying
// Structure and Texture Similarity", 2020; dingkeyan93/DISTS as wrapped by pyiqa), recalled from the published code, not read from it:
//   x = the gray frame g in [0,1] on three channels; h = (x - mean_c)/std_c, mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225);
//   five VGG-16 stages conv1_1-1_2, conv2_1-2_2, conv3_1-3_3, conv4_1-4_3, conv5_1-5_3 (3x3, padding 1, ReLU); stages 2-5 begin
//   with an L2 pool instead of the max pool: sqrt(conv2d(f^2, k, stride 2, padding 1, depthwise) + 1e-12), k = (1 2 1)x(1 2 1)/16,
//   zero padding, output side (s + 1)/2 (ceil; LPIPS-VGG's max pool floors);
//   six feature sets: x itself (3 channels, before the normalisation), relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256,
//   512, 512 channels; 1475 in all); per set and channel, over the spatial positions, the means mx, my, the variances
//   vx = mean((fx - mx)^2), vy, the covariance cxy = mean(fx fy) - mx my, S1 = (2 mx my + c1)/(mx^2 + my^2 + c1),
//   S2 = (2 cxy + c2)/(vx + vy + c2), c1 = c2 = 1e-6; with w = sum(alpha) + sum(beta) the score is
//   1 - (sum_c (alpha_c/w) S1_c + sum_c (beta_c/w) S2_c).
// Conventions that stay unpinned until tests/test_dists_pins.py has run where pyiqa exists: the state-dict names stage1.{0,2},
// stage2.{5,7}, stage3.{10,12,14}, stage4.{17,19,21}, stage5.{24,26,28} (.weight, .bias), alpha and beta ([1,1475,1,1], positive), the
// optional buffers mean and std (used when present), the pools' stageK.N.filter buffers (ignored), and everything above.
// Scores agree with the restatement tests/dists_ref.py on any weights, and with pyiqa only once its weights are supplied.
//
// Layers: the thirteen convolutions are LPIPS-VGG's, kernels (vgg_backbone.h) and host side (vgg_trunk.h: the handle holds a VggTrunk,
// here with ceil-mode level sizes) -- conv1_1 is the direct kernel on the gray frame with DISTS's normalisation folded in (lpips_host.h
// fold_scaling_layer), the other twelve run on conv.hip in the process's arithmetic (activations PACKED / H2 in the split modes, PLAIN
// in fp32).  This file's own: the state-dict names, mean / std, alpha / beta, the head buffers and
//   dists_stat_pool_kernel, one launch per stage: the five sums (fx, fy, fx^2, fy^2, fx fy) of every channel and, for stages 1-4,
//     the L2 pool of both frames into the other ping-pong buffer;
//   dists_gray_kernel: the five sums of the gray frames themselves (feature set 0: its three channels are equal, so one S1 and one
//     S2 weighted by alpha_0 + alpha_1 + alpha_2 and beta_0 + beta_1 + beta_2);
//   dists_channel_kernel + dists_finish_kernel: partial sums -> mx, my, vx = sum(fx^2)/N - mx^2, cxy, S1, S2 in fp64, times
//     alpha_c/w and beta_c/w (normalised on the host in fp64), 64 channels per block; then one block per pair adds them up.
// All sums are fp64 from the first addition on (a feature is fp32, so its square and the product of two are exact in fp64: a 1x1
// map's variance and covariance cancel exactly) and are added in an order that depends on the stage's shape only: no atomics, and
// the block count per pair does not depend on the number of pairs.
//
// Memory plan (vgg_trunk.h): as lpips_vgg.hip -- features are not kept: two ping-pong activation buffers sized for relu1_2, 2*P*H*W*64*4 B each
// for P pairs per pass, P chosen so that both fit ACT_BUDGET_BYTES (at least 1; `max_pairs` at create overrides it); a call with
// more pairs runs in passes.
//
// Measured on an MI355X, default h3 arithmetic.  tests/test_gpu_dists.py against the fp64 restatement at 16x16, 37x53, 64x80: totals
// and the twelve stage distances at most 0.010 of max(2e-4 |want| + 1e-7, 8 |fp32 - fp64|) in h3 and fp32, 0.025 of ten times that in
// mx / mx6.  tools/dists_bench.py (profiles/dists_bench.json), 16 pairs per call beside LPIPSVGG: 6.24 / 20.9 / 47.8 ms at 346x260 /
// 640x480 / 970x624, 1.11 / 1.06 / 1.11 times LPIPS-VGG, 286 / 287 / 247 algorithmic TFLOP/s.  profiles/dists_kernel_stats.md
// (346x260): the five statistics / pool launches 1086 us per call, the gray launch 23 us, the two finishing launches 62 us -- 19 %
// of the byte floor (225 us at the 8 TB/s HBM peak) where LPIPS-VGG's tap kernels reach 33 %.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "conv.h"
#include "packed.h"
#include "vgg_trunk.h"

using namespace evr;

namespace {

// the backbone's kernels have only ever run down to the 1x1 maps of a 16x16 frame (the published metric accepts smaller frames)
constexpr int MIN_SIDE = 16;
constexpr int NSETS = 6;                                 // feature sets: the input, then the five stages
constexpr int NCH = 3 + 64 + 128 + 256 + 512 + 512;       // 1475
constexpr int STAT_BLOCKS_MAX = 256;                      // work-groups per pair and 256-channel chunk of the statistics kernel
constexpr int GRAY_BLOCKS_MAX = 32;

// ---- one stage: the five sums per channel + the L2 pool of both frames' features ----------------------------------------------
// feat: [2n, h, w, C] (first n = img, last n = ref) in format `fmt`; pooled: [2n, (h+1)/2, (w+1)/2, C] in the same format (POOL).
// Work item = one pooled pixel (oy, ox) of the grid ceil(h/2) x ceil(w/2).  Its pool window is the 3x3 block centred on (2oy, 2ox),
// zeros outside the map; the 2x2 block (2oy .. 2oy+1, 2ox .. 2ox+1) inside it is what the item COUNTS into the sums, so every input
// pixel is counted exactly once and read by up to four items (2.25 reads per pixel on average).  The re-reads are neighbours of
// the same wave or the next one and are served by the caches -- no LDS staging: the byte floor of the kernel is one read of the
// stage and one write of the pooled tensor (profiles/dists_kernel_stats.md has the measured fraction).  Without POOL (relu5_3) only
// the 2x2 block is read.
// A lane owns one 4-channel run (ld4_any / st4_any) and walks items: with R = C/4 runs per pixel a wave takes 64/R items at once
// for C < 256; from C = 256 on a wave takes one item and 256 channels, blockIdx.z picks the 256-channel chunk.  The 20 sums of a
// lane are private fp64 registers until the block's end; there the lanes of one run add up in a fixed order (wave-internal
// exchange, then the four waves through LDS) and the block writes partials[pair][block][C][5].
// Pool arithmetic: squares and the weighted sum in fp32, products and additions rounded separately (no contraction; the weights
// 1/16, 2/16, 4/16 are exact), then sqrtf(s + 1e-12f).
struct StatArgs {
    const float* feat; float* pooled;
    int n, h, w, C, fmt;
    double* partials;      // [n][gridDim.x][C][5]
    unsigned* sat;
};

template <bool POOL>
__global__ __launch_bounds__(256) void dists_stat_pool_kernel(const StatArgs a) {
    __shared__ double red[4][64][5];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = a.C >> 2;
    const int L = R < 64 ? R : 64;            // lanes per item (16, 32, 64)
    const int PW = 64 / L;                    // items per wave
    const int sub = lane / L, run0 = lane % L;
    const int ch = blockIdx.z * 256 + run0 * 4;
    const int ho = (a.h + 1) >> 1, wo = (a.w + 1) >> 1;
    const int nwin = ho * wo;
    const float* f0 = a.feat + (int64_t)b * a.h * a.w * a.C;
    const float* f1 = a.feat + (int64_t)(b + a.n) * a.h * a.w * a.C;
    double acc[5][4];
#pragma unroll
    for (int v = 0; v < 5; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[v][q] = 0.0;
    for (int w0 = (blockIdx.x * 4 + wave) * PW; w0 < nwin; w0 += gridDim.x * 4 * PW) {
        const int win = w0 + sub;
        const bool wok = win < nwin;
        const int oy = wok ? win / wo : 0, ox = wok ? win % wo : 0;
        float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = POOL ? 0 : 1; r < 3; ++r)
#pragma unroll
            for (int c = POOL ? 0 : 1; c < 3; ++c) {
                const int y = 2 * oy + r - 1, x = 2 * ox + c - 1;
                if (!(wok && (unsigned)y < (unsigned)a.h && (unsigned)x < (unsigned)a.w)) continue;
                const int64_t poff = ((int64_t)y * a.w + x) * a.C;
                const float4 u4 = ld4_any(f0 + poff, ch, a.fmt), v4 = ld4_any(f1 + poff, ch, a.fmt);
                const float u[4] = {u4.x, u4.y, u4.z, u4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
                if (r >= 1 && c >= 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double du = (double)u[q], dv = (double)v[q];
                        acc[0][q] += du; acc[1][q] += dv;
                        acc[2][q] = fma(du, du, acc[2][q]); acc[3][q] = fma(dv, dv, acc[3][q]); acc[4][q] = fma(du, dv, acc[4][q]);
                    }
                }
                if (POOL) {
                    const float kw = (r == 1 ? 2.f : 1.f) * (c == 1 ? 2.f : 1.f) * 0.0625f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma clang fp contract(off)
                        const float uu = u[q] * u[q], vv = v[q] * v[q];
                        px[q] = px[q] + kw * uu; py[q] = py[q] + kw * vv;
                    }
                }
            }
        if (POOL && wok) {
            const int64_t ooff = ((int64_t)oy * wo + ox) * a.C;
            float* o0 = a.pooled + (int64_t)b * nwin * a.C + ooff;
            float* o1 = a.pooled + (int64_t)(b + a.n) * nwin * a.C + ooff;
            const float4 p0 = make_float4(sqrtf(px[0] + 1e-12f), sqrtf(px[1] + 1e-12f), sqrtf(px[2] + 1e-12f), sqrtf(px[3] + 1e-12f));
            const float4 p1 = make_float4(sqrtf(py[0] + 1e-12f), sqrtf(py[1] + 1e-12f), sqrtf(py[2] + 1e-12f), sqrtf(py[3] + 1e-12f));
#if defined(__HIP_DEVICE_COMPILE__)
            if (a.fmt) {      // (an L2 pool never exceeds its window's largest value: the counter can only trip where the stage's did)
                const float mx = fmaxf(fmaxf(fmaxf(p0.x, p0.y), fmaxf(p0.z, p0.w)), fmaxf(fmaxf(p1.x, p1.y), fmaxf(p1.z, p1.w)));
                if (a.fmt == 2) sat_note<2>(a.sat, mx); else sat_note<1>(a.sat, mx);
            }
#endif
            st4_any(o0, ch, p0, a.fmt); st4_any(o1, ch, p1, a.fmt);
        }
    }
    // the lanes of one run: first the items of a wave (lane ^ L, lane ^ 2L, ...), then the four waves in order
    double res[5][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            double s = acc[v][q];
            for (int o = L; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
            red[wave][lane][v] = s;
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 5; ++v) res[v][q] = ((red[0][lane][v] + red[1][lane][v]) + red[2][lane][v]) + red[3][lane][v];
        __syncthreads();
    }
    if (threadIdx.x < L) {
        double* p = a.partials + (((int64_t)b * gridDim.x + blockIdx.x) * a.C + ch) * 5;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int v = 0; v < 5; ++v) p[q * 5 + v] = res[v][q];
    }
}

// ---- feature set 0: the five sums of the gray frames (after the clip, when asked) --------------------------------------------
// partials: [n][gridDim.x][5].  A thread walks pixels a grid's width apart with fp64 sums; fixed-order tree at the end.
__global__ __launch_bounds__(256) void dists_gray_kernel(const float* __restrict__ img, const float* __restrict__ ref, int hw, int clip,
                                                         double* __restrict__ partials) {
    __shared__ double red[4][5];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* p0 = img + (int64_t)b * hw;
    const float* p1 = ref + (int64_t)b * hw;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        float u = p0[i], v = p1[i];
        if (clip) { u = fminf(fmaxf(u, 0.f), 1.f); v = fminf(fmaxf(v, 0.f), 1.f); }
        const double du = (double)u, dv = (double)v;
        s[0] += du; s[1] += dv; s[2] = fma(du, du, s[2]); s[3] = fma(dv, dv, s[3]); s[4] = fma(du, dv, s[4]);
    }
#pragma unroll
    for (int v = 0; v < 5; ++v) {
        for (int o = 32; o > 0; o >>= 1) s[v] += __shfl_xor(s[v], o, 64);
        if (lane == 0) red[wave][v] = s[v];
    }
    __syncthreads();
    if (threadIdx.x < 5) partials[((int64_t)b * gridDim.x + blockIdx.x) * 5 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- the similarities of the 1472 trunk channels, then the finish (one block per pair) ------------------------------------------
// dists_channel_kernel: a block takes 64 consecutive channels of one pair (23 chunks: 1, 2, 4, 8, 8 for the five stages -- a chunk
// never straddles a stage).  Wave k of the block adds the partial sums of the stage's blocks k, k + 4, ... in order, the four waves'
// sums are added in order, and wave 0 forms mx, my, vx = sum(fx^2)/N - mx^2, vy, cxy, S1 and S2 in fp64, multiplies by alpha_c/w
// and beta_c/w and adds its 64 channels in a fixed tree: terms[pair][chunk] = {sum a (1 - S1), sum b (1 - S2), sum a S1, sum b S2}.
// (One block per pair walking all 1472 channels' partial sums took 127 us per pass at 346x260: 1270 dependent loads per thread.)
// dists_finish_kernel, one block per pair: the chunks of a stage in order, the gray frames' sums (feature set 0) in order;
// out_stages[b][k] = {sum (alpha_c/w)(1 - S1_c), sum (beta_c/w)(1 - S2_c)}; out[b] = 1 - (D1 + D2) with D1 = sum (alpha_c/w) S1_c.
constexpr int NCHUNK = (NCH - 3) / 64;      // 23
struct ChannelArgs {
    const double* partials[5]; int blocks[5]; int hw[5];
    const double* aw; const double* bw;      // [1475] alpha_c / w, beta_c / w
    double* terms;                           // [n][NCHUNK][4]
};

__device__ __forceinline__ void dists_similarity(const double (&s)[5], double N, double& s1, double& s2) {
#pragma clang fp contract(off)      // (identical frames: mx mx + my my must round like 2 (mx my))
    constexpr double C1 = 1e-6, C2 = 1e-6;
    const double mx = s[0] / N, my = s[1] / N;
    const double vx = s[2] / N - mx * mx, vy = s[3] / N - my * my, cxy = s[4] / N - mx * my;
    s1 = (2.0 * (mx * my) + C1) / (mx * mx + my * my + C1);
    s2 = (2.0 * cxy + C2) / (vx + vy + C2);
}

__global__ __launch_bounds__(256) void dists_channel_kernel(const ChannelArgs f) {
#pragma clang fp contract(off)
    __shared__ double red[4][64][5];
    const int chunk = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = chunk < 1 ? 0 : chunk < 3 ? 1 : chunk < 7 ? 2 : chunk < 15 ? 3 : 4;      // the chunk's stage
    const int first = l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 3 : l == 3 ? 7 : 15;             // the stage's first chunk
    const int C = 64 << (l < 3 ? l : 3);
    const int nb = l == 0 ? f.blocks[0] : l == 1 ? f.blocks[1] : l == 2 ? f.blocks[2] : l == 3 ? f.blocks[3] : f.blocks[4];
    const int hw = l == 0 ? f.hw[0] : l == 1 ? f.hw[1] : l == 2 ? f.hw[2] : l == 3 ? f.hw[3] : f.hw[4];
    const double* part = l == 0 ? f.partials[0] : l == 1 ? f.partials[1] : l == 2 ? f.partials[2] : l == 3 ? f.partials[3] : f.partials[4];
    const int c = (chunk - first) * 64 + lane;
    const double* p = part + ((int64_t)b * nb * C + c) * 5;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = wave; j < nb; j += 4)
#pragma unroll
        for (int v = 0; v < 5; ++v) s[v] += p[(int64_t)j * C * 5 + v];
#pragma unroll
    for (int v = 0; v < 5; ++v) red[wave][lane][v] = s[v];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int v = 0; v < 5; ++v) s[v] = ((red[0][lane][v] + red[1][lane][v]) + red[2][lane][v]) + red[3][lane][v];
    double s1, s2;
    dists_similarity(s, (double)hw, s1, s2);
    const double aw = f.aw[3 + chunk * 64 + lane], bw = f.bw[3 + chunk * 64 + lane];
    double d[4] = {aw * (1.0 - s1), bw * (1.0 - s2), aw * s1, bw * s2};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        for (int o = 32; o > 0; o >>= 1) d[v] += __shfl_xor(d[v], o, 64);
        if (lane == 0) f.terms[((int64_t)b * NCHUNK + chunk) * 4 + v] = d[v];
    }
}

struct FinishArgs {
    const double* terms;                     // [n][NCHUNK][4]
    const double* gray; int gray_blocks; int hw0;
    const double* aw; const double* bw;
};

__global__ __launch_bounds__(64) void dists_finish_kernel(const FinishArgs f, double* __restrict__ out, double* __restrict__ out_stages) {
#pragma clang fp contract(off)
    __shared__ double tm[NCHUNK][4];
    __shared__ double gr[GRAY_BLOCKS_MAX][5];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < NCHUNK) {
#pragma unroll
        for (int v = 0; v < 4; ++v) tm[t][v] = f.terms[((int64_t)b * NCHUNK + t) * 4 + v];
    }
    if (t >= 32 && t - 32 < f.gray_blocks) {
#pragma unroll
        for (int v = 0; v < 5; ++v) gr[t - 32][v] = f.gray[((int64_t)b * f.gray_blocks + t - 32) * 5 + v];
    }
    __syncthreads();
    if (t != 0) return;
    double tot1 = 0.0, tot2 = 0.0;      // D1, D2
    {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < f.gray_blocks; ++j)
#pragma unroll
            for (int v = 0; v < 5; ++v) s[v] += gr[j][v];
        double s1, s2;
        dists_similarity(s, (double)f.hw0, s1, s2);
        const double aw = (f.aw[0] + f.aw[1]) + f.aw[2], bw = (f.bw[0] + f.bw[1]) + f.bw[2];
        if (out_stages) { out_stages[(int64_t)b * NSETS * 2] = aw * (1.0 - s1); out_stages[(int64_t)b * NSETS * 2 + 1] = bw * (1.0 - s2); }
        tot1 = aw * s1; tot2 = bw * s2;
    }
    int chunk = 0;
    for (int k = 1; k < NSETS; ++k) {
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = chunk + (k < 4 ? 1 << (k - 1) : 8); chunk < e; ++chunk)
#pragma unroll
            for (int v = 0; v < 4; ++v) d[v] += tm[chunk][v];
        if (out_stages) { out_stages[((int64_t)b * NSETS + k) * 2] = d[0]; out_stages[((int64_t)b * NSETS + k) * 2 + 1] = d[1]; }
        tot1 += d[2]; tot2 += d[3];
    }
    out[b] = 1.0 - (tot1 + tot2);
}

// work-groups per pair (and 256-channel chunk) of the statistics kernel: eight rounds per wave, at most STAT_BLOCKS_MAX -- from the
// stage's shape alone, so that a pair's partial sums do not depend on the pairs beside it (a pass of the largest frames holds one
// pair: its first stages then run on 256 blocks)
int stat_blocks(int nwin, int C) {
    const int pw = C >= 256 ? 1 : 256 / C;      // items per wave and round
    int want = (nwin + 4 * pw * 8 - 1) / (4 * pw * 8);
    if (want > STAT_BLOCKS_MAX) want = STAT_BLOCKS_MAX;
    return want < 1 ? 1 : want;
}
int gray_blocks(int hw) {
    int want = (hw + 256 * 16 - 1) / (256 * 16);      // sixteen pixels per thread
    if (want > GRAY_BLOCKS_MAX) want = GRAY_BLOCKS_MAX;
    return want < 1 ? 1 : want;
}

}  // namespace

struct evr_dists {
    VggTrunk trunk;
    double* d_ab = nullptr;          // alpha / w [1475] | beta / w [1475]
    int blocks[5], gblocks = 0;      // work-groups per pair of the statistics launches
    // of trunk.allocs:
    double* partials[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // [cap][blocks][C][5]
    double* gray = nullptr;          // [cap][gblocks][5]
    double* terms = nullptr;         // [cap][NCHUNK][4]
    void release() {
        trunk.release();
        gray = nullptr; terms = nullptr;
        for (auto& p : partials) p = nullptr;
    }
    // (vgg_forward) the trunk's buffers with ceil-mode pools, then the head's
    int buffers(int cap, int H, int W, hipStream_t stream) {
        int rc;
        if ((rc = trunk.buffers(cap, H, W, true, stream))) return rc;
        for (int l = 0; l < 5; ++l) {
            blocks[l] = stat_blocks(((trunk.h[l] + 1) / 2) * ((trunk.w[l] + 1) / 2), VGG_TAP_C[l]);
            if ((rc = trunk.allocs.alloc(&partials[l], (size_t)cap * blocks[l] * VGG_TAP_C[l] * 5))) return rc;
        }
        gblocks = gray_blocks(H * W);
        if ((rc = trunk.allocs.alloc(&gray, (size_t)cap * gblocks * 5))) return rc;
        return trunk.allocs.alloc(&terms, (size_t)cap * NCHUNK * 4);
    }
    ~evr_dists() { if (d_ab) (void)hipFree(d_ab); }
};

extern "C" int evr_dists_create(const evr_tensor* tensors, int n_tensors, int max_pairs, evr_dists** out) {
    EVR_REQUIRE(tensors && out && max_pairs >= 0, "evr_dists_create: bad argument");
    const StateDict sd("DISTS", tensors, n_tensors);
    evr_dists* m = new evr_dists();
    int rc = EVR_OK;
    const evr_tensor *al, *be;
    // torchvision vgg16.features indices inside the published stages (conv1_1 first)
    const char* const names[VGG_NCONV + 1] = {"stage1.0", "stage1.2", "stage2.5", "stage2.7", "stage3.10", "stage3.12", "stage3.14",
                                              "stage4.17", "stage4.19", "stage4.21", "stage5.24", "stage5.26", "stage5.28"};
    do {
        // x_c = (g - mean_c)/std_c = g/std_c - mean_c/std_c; the buffers of the state dict where it carries them
        double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225}, fa[3], fb[3];
        if (sd.sd.count("mean") && sd.sd.count("std")) {
            const evr_tensor *tm, *ts;
            if ((rc = sd.get("mean", 3, &tm))) break;
            if ((rc = sd.get("std", 3, &ts))) break;
            for (int c = 0; c < 3; ++c) { mean[c] = (double)tm->data_host[c]; stdv[c] = (double)ts->data_host[c]; }
        }
        if (!(stdv[0] > 0.0 && stdv[1] > 0.0 && stdv[2] > 0.0)) { set_error("DISTS tensor 'std' must be positive"); rc = EVR_ERR_INVALID; break; }
        for (int c = 0; c < 3; ++c) { fa[c] = 1.0 / stdv[c]; fb[c] = -mean[c] / stdv[c]; }
        if ((rc = m->trunk.create(sd, names, fa, fb, max_pairs))) break;
        if ((rc = sd.get("alpha", NCH, &al))) break;
        if ((rc = sd.get("beta", NCH, &be))) break;
        double wsum = 0.0;
        for (int c = 0; c < NCH; ++c) wsum += (double)al->data_host[c];
        for (int c = 0; c < NCH; ++c) wsum += (double)be->data_host[c];
        if (!(wsum > 0.0) || !std::isfinite(wsum)) { set_error("DISTS: sum(alpha) + sum(beta) must be positive and finite"); rc = EVR_ERR_INVALID; break; }
        std::vector<double> ab((size_t)2 * NCH);
        for (int c = 0; c < NCH; ++c) { ab[c] = (double)al->data_host[c] / wsum; ab[NCH + c] = (double)be->data_host[c] / wsum; }
        if (hipMalloc((void**)&m->d_ab, ab.size() * sizeof(double)) != hipSuccess) { rc = hip_fail(hipGetLastError(), "hipMalloc(alpha, beta)", __FILE__, __LINE__); break; }
        if (hipMemcpy(m->d_ab, ab.data(), ab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { rc = hip_fail(hipGetLastError(), "hipMemcpy(alpha, beta)", __FILE__, __LINE__); break; }
    } while (0);
    if (rc) { delete m; return rc; }
    *out = m;
    return EVR_OK;
}

extern "C" int evr_dists_destroy(evr_dists* m) { delete m; return EVR_OK; }

// one pass: np pairs starting at img / ref, scores to out[0..np) (and out_stages[0..12 np))
static int dists_pass(evr_dists* m, const float* img, const float* ref, int np, int clip, double* out, double* out_stages, hipStream_t stream) {
    VggTrunk& t = m->trunk;
    int rc, src = 0;
    VggTrunk::Plan* P = nullptr;
    if ((rc = t.begin_pass(np, stream, &P))) return rc;
    hipLaunchKernelGGL(dists_gray_kernel, dim3(m->gblocks, np), dim3(256), 0, stream, img, ref, t.H * t.W, clip, m->gray);
    EVR_LAUNCH_CHECK();
    if ((rc = t.conv1_1(img, ref, np, clip, stream))) return rc;
    ChannelArgs ca{};
    for (int l = 0; l < 5; ++l) {
        if ((rc = t.level_convs(P, l, stream, &src))) return rc;
        StatArgs st{};
        st.feat = t.act[src]; st.pooled = l < 4 ? t.act[src ^ 1] : nullptr;
        st.n = np; st.h = t.h[l]; st.w = t.w[l]; st.C = VGG_TAP_C[l]; st.fmt = t.fmt();
        st.partials = m->partials[l]; st.sat = t.d_sat;
        const dim3 grid(m->blocks[l], np, st.C >= 256 ? st.C / 256 : 1);
        if (l < 4) hipLaunchKernelGGL(dists_stat_pool_kernel<true>, grid, dim3(256), 0, stream, st);
        else hipLaunchKernelGGL(dists_stat_pool_kernel<false>, grid, dim3(256), 0, stream, st);
        EVR_LAUNCH_CHECK();
        ca.partials[l] = st.partials; ca.blocks[l] = m->blocks[l]; ca.hw[l] = st.h * st.w;
    }
    ca.aw = m->d_ab; ca.bw = m->d_ab + NCH; ca.terms = m->terms;
    hipLaunchKernelGGL(dists_channel_kernel, dim3(NCHUNK, np), dim3(256), 0, stream, ca);
    EVR_LAUNCH_CHECK();
    FinishArgs fa{};
    fa.terms = m->terms; fa.gray = m->gray; fa.gray_blocks = m->gblocks; fa.hw0 = t.H * t.W;
    fa.aw = ca.aw; fa.bw = ca.bw;
    hipLaunchKernelGGL(dists_finish_kernel, dim3(np), dim3(64), 0, stream, fa, out, out_stages);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" int evr_dists_forward(evr_dists* m, const float* img, const float* ref, int n, int H, int W, int clip, double* out,
                                 double* out_stages, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(m && img && ref && out && n >= 1 && H >= 1 && W >= 1, "evr_dists_forward: bad argument");
    EVR_REQUIRE(H >= MIN_SIDE && W >= MIN_SIDE, "evr_dists: image %dx%d too small (this backbone runs on frames of at least %d pixels a side)", W, H, MIN_SIDE);
    EVR_REQUIRE((int64_t)2 * H * W * 64 * 4 < ACT_BUFFER_MAX_BYTES, "evr_dists: image %dx%d too large: one pair's 64-channel features must stay below 2 GiB (H*W < 2^22)", W, H);
    return vgg_forward(m, n, H, W, stream, [&](int o, int np) {
        return dists_pass(m, img + (int64_t)o * H * W, ref + (int64_t)o * H * W, np, clip, out + o,
                          out_stages ? out_stages + (int64_t)NSETS * 2 * o : nullptr, stream);
    });
}

// (the statistics and the pools are not counted)
extern "C" double evr_dists_flops(const evr_dists* m) { return m ? m->trunk.flops() : 0.0; }

extern "C" int evr_dists_saturation(evr_dists* m, int64_t* count, evr_stream_t stream_) {
    EVR_REQUIRE(m && count, "evr_dists_saturation: null argument");
    return m->trunk.saturation(count, (hipStream_t)stream_);
}
