// LPIPS (AlexNet, v0.1) on gfx950 -- the 'lpips' metric of the reference (utils/eval_metrics.py:100-156:
// pyiqa.create_metric('lpips') on [n,3,H,W] batches built by cv2torch(img, num_ch=3), eval_utils.py:46-54).
//
// PARITY UNPINNED: pyiqa is neither in the reference tree nor installed, and its AlexNet + linear-head weights are
// downloaded at run time (unobtainable offline).  The arithmetic below follows the published algorithm (Zhang et
// al. 2018; richzhang/PerceptualSimilarity v0.1 as wrapped by pyiqa): x <- 2x-1; (x-shift)/scale per channel;
// AlexNet features after relu1..relu5; unit-normalise every pixel's feature vector (eps 1e-10); squared
// difference; non-negative 1x1 "lin" weights; spatial mean; sum over the five layers.  Scores therefore agree with
// the oracle restatement (oracle/lpips.py) on any weights, and with pyiqa only once its weights are supplied.
//
// Layers: conv1 (3->64, k11 s4 p2) is a direct VALU kernel on the gray input (the three input channels are affine
// in the same gray value); conv2..conv5 run on the convolution kernels of conv.hip (split arithmetic: conv2 on the implicit
// GEMM, conv3..conv5 on the band kernel; pool1/feat1.. are then PACKED tensors, conv.h); 3x3/2 max pools and the
// per-layer score are NHWC streaming kernels (one wave per pixel for the channel norms).
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <atomic>
#include "conv.h"
#include "lpips_host.h"
#include "packed.h"

using namespace evr;

namespace {

// ---- conv1: gray [n2,H,W] -> NHWC [n2,h1,w1,64], relu ------------------------------------------------------------
// The three input channels are the same gray value g pushed through per-channel affine maps
// x_c = ((2g-1) - shift_c)/scale_c = alpha_c*g + beta_c (and 0 where the conv pads), so
//   sum_c sum_t w[co][c][t] x_c[t] = sum_t inside[t] * (wg[t][co]*g[t] + wb[t][co]),
// with wg = sum_c w*alpha_c, wb = sum_c w*beta_c folded on the host: a ONE-channel 11x11 conv (121 taps instead of
// 363) plus, for output tiles whose receptive field leaves the image, the wb term under the inside mask; interior
// tiles take sum_t wb[t] from the bias.  Weights are wave-uniform (scalar loads); the gray tile and mask sit in LDS.
struct Conv1Args {
    const float* img; const float* ref;   // [n,H,W] each; batch index >= n reads ref
    int n, H, W, h1, w1, clip;
    const float* wg;                       // [121][64]
    const float* wb;                       // [121][64]
    const float* bias;                     // [64]
    const float* bias_in;                  // [64] bias + sum_t wb[t]  (interior tiles)
    float* out;
    const unsigned* wfrag;                 // matrix-core form: wg in MFMA-fragment order (conv1_pack_wfrag), bf16 hi / lo
    const float* wbsum;                    // [12][12][64] prefix sums of wb over (ky, kx): the padding term of a border pixel
};

__global__ __launch_bounds__(256) void lpips_conv1_kernel(const Conv1Args a) {
    constexpr int TS = 16, K = 11, S = 4, P = 2, IS = (TS - 1) * S + K;   // 71
    extern __shared__ float smem[];
    float* tile = smem;                 // [IS][IS] gray (0 outside the image)
    float* mask = smem + IS * IS;       // [IS][IS] 1 inside / 0 outside
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, tid = threadIdx.x;
    const float* src = (b < a.n ? a.img + (int64_t)b * a.H * a.W : a.ref + (int64_t)(b - a.n) * a.H * a.W);
    const int y_lo = ty0 * S - P, x_lo = tx0 * S - P;
    const bool interior = y_lo >= 0 && x_lo >= 0 && y_lo + IS <= a.H && x_lo + IS <= a.W;   // block-uniform
    for (int i = tid; i < IS * IS; i += 256) {
        const int rr = i / IS, cc = i % IS;
        const int y = y_lo + rr, x = x_lo + cc;
        float g = 0.f, in = 0.f;
        if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
            g = src[(int64_t)y * a.W + x];
            if (a.clip) g = fminf(fmaxf(g, 0.f), 1.f);
            in = 1.f;
        }
        tile[i] = g; mask[i] = in;
    }
    __syncthreads();
    const int ly = tid / TS, lx = tid % TS, oy = ty0 + ly, ox = tx0 + lx;
    float acc[64];
    if (interior) {
#pragma unroll
        for (int co = 0; co < 64; ++co) acc[co] = a.bias_in[co];
        for (int ky = 0; ky < K; ++ky)
            for (int kx = 0; kx < K; ++kx) {
                const float v = tile[(ly * S + ky) * IS + lx * S + kx];
                const float* w = a.wg + (ky * K + kx) * 64;                 // wave-uniform -> scalar loads
#pragma unroll
                for (int co = 0; co < 64; ++co) acc[co] = fmaf(v, w[co], acc[co]);
            }
    } else {
#pragma unroll
        for (int co = 0; co < 64; ++co) acc[co] = a.bias[co];
        for (int ky = 0; ky < K; ++ky)
            for (int kx = 0; kx < K; ++kx) {
                const int ti = (ly * S + ky) * IS + lx * S + kx;
                const float v = tile[ti], mk = mask[ti];
                const float* w = a.wg + (ky * K + kx) * 64;
                const float* wbp = a.wb + (ky * K + kx) * 64;
#pragma unroll
                for (int co = 0; co < 64; ++co) acc[co] = fmaf(mk, wbp[co], fmaf(v, w[co], acc[co]));
            }
    }
    if (oy < a.h1 && ox < a.w1) {
        float* o = a.out + (((int64_t)b * a.h1 + oy) * a.w1 + ox) * 64;
#pragma unroll
        for (int co = 0; co < 64; co += 4)
            *(float4*)(o + co) = make_float4(fmaxf(acc[co], 0.f), fmaxf(acc[co + 1], 0.f), fmaxf(acc[co + 2], 0.f), fmaxf(acc[co + 3], 0.f));
    }
}

// conv1 on the matrix cores (split mode): GEMM M = pixels, N = 64, K = 121 taps padded to 128, three bf16 products
// (x = hi + lo, w = hi + lo) like the networks' head conv.  The gray tile sits in LDS; lane (pixel r, half h) gathers the 8
// taps k = 16s + 8h + j of slab s at compile-time offsets from its pixel's window origin; the weight fragments (32 KB, packed
// on the host) are copied to LDS once per block.  The padding term sum_t inside[t] * wb[t] is a rectangle sum over the
// window's in-image taps: 4 look-ups in the prefix table for border pixels, the folded bias for the others.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void lpips_conv1_mfma_kernel(const Conv1Args a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int TS = 16, K = 11, S = 4, P = 2, IS = (TS - 1) * S + K;   // 71
    extern __shared__ float smem[];
    float* tile = smem;                                   // [IS][IS] gray (0 outside the image)
    const float4* wf = (const float4*)(smem + IS * IS + 3);   // [8 slabs][2 blocks][hi, lo][64 lanes] x 16 B (16-B aligned: 5041 + 3)
    const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS, tid = threadIdx.x;
    const float* src = (b < a.n ? a.img + (int64_t)b * a.H * a.W : a.ref + (int64_t)(b - a.n) * a.H * a.W);
    const int y_lo = ty0 * S - P, x_lo = tx0 * S - P;
    for (int i = tid; i < IS * IS; i += 256) {
        const int rr = i / IS, cc = i % IS;
        const int y = y_lo + rr, x = x_lo + cc;
        float g = 0.f;
        if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
            g = src[(int64_t)y * a.W + x];
            if (a.clip) g = fminf(fmaxf(g, 0.f), 1.f);
        }
        tile[i] = g;
    }
    {
        float4* dst = (float4*)(smem + IS * IS + 3);
        const float4* wsrc = (const float4*)a.wfrag;
        for (int i = tid; i < 8 * 2 * 2 * 64; i += 256) dst[i] = wsrc[i];
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nb][i] = 0.f;
    int base[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int ly = 2 * (2 * wv + mt) + (r >> 4), lx = r & 15;
        base[mt] = ly * S * IS + lx * S;
    }
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
        u32x4_t ah[2], al[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                constexpr int NT = K * K;
                const int k0 = 16 * s8 + j, k1 = k0 + 8;                              // this lane's tap for h = 0 / 1
                const int o0 = k0 < NT ? (k0 / K) * IS + k0 % K : 0, o1 = k1 < NT ? (k1 / K) * IS + k1 % K : 0;   // (padding taps: zero weights)
                e[j] = tile[base[mt] + (h ? o1 : o0)];
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                ah[mt][d] = cvt_pk_bf16(e[2 * d], e[2 * d + 1]);
                al[mt][d] = cvt_pk_bf16(e[2 * d] - __uint_as_float(ah[mt][d] << 16), e[2 * d + 1] - __uint_as_float(ah[mt][d] & 0xffff0000u));
            }
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const bf16x8 b_hi = __builtin_bit_cast(bf16x8, wf[((s8 * 2 + nb) * 2 + 0) * 64 + lane]);
            const bf16x8 b_lo = __builtin_bit_cast(bf16x8, wf[((s8 * 2 + nb) * 2 + 1) * 64 + lane]);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[mt]), a_lo = __builtin_bit_cast(bf16x8, al[mt]);
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b_hi, a_lo, acc[mt][nb], 0, 0, 0);
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b_lo, a_hi, acc[mt][nb], 0, 0, 0);
                acc[mt][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b_hi, a_hi, acc[mt][nb], 0, 0, 0);
            }
        }
    }
    // epilogue: lane = pixel r, registers = channels nb*32 + (i & 3) + 8 * (i >> 2) + 4h
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int ly = 2 * (2 * wv + mt) + (r >> 4), lx = r & 15, oy = ty0 + ly, ox = tx0 + lx;
        if (oy >= a.h1 || ox >= a.w1) continue;
        // in-image taps of this pixel's window: ky in [ky0, ky1], kx in [kx0, kx1]
        const int ky0 = max(0, P - oy * S), ky1 = min(K - 1, a.H - 1 - oy * S + P);
        const int kx0 = max(0, P - ox * S), kx1 = min(K - 1, a.W - 1 - ox * S + P);
        const bool inside = ky0 == 0 && kx0 == 0 && ky1 == K - 1 && kx1 == K - 1;
        float* o = a.out + (((int64_t)b * a.h1 + oy) * a.w1 + ox) * 64;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c4 = nb * 32 + 8 * q + 4 * h;
                float4 add;
                if (inside) add = *(const float4*)(a.bias_in + c4);
                else {
                    const float4 bb = *(const float4*)(a.bias + c4);
                    const float4 p11 = *(const float4*)(a.wbsum + ((ky1 + 1) * 12 + kx1 + 1) * 64 + c4), p01 = *(const float4*)(a.wbsum + (ky0 * 12 + kx1 + 1) * 64 + c4);
                    const float4 p10 = *(const float4*)(a.wbsum + ((ky1 + 1) * 12 + kx0) * 64 + c4), p00 = *(const float4*)(a.wbsum + (ky0 * 12 + kx0) * 64 + c4);
                    add = make_float4(bb.x + ((p11.x - p01.x) - (p10.x - p00.x)), bb.y + ((p11.y - p01.y) - (p10.y - p00.y)),
                                      bb.z + ((p11.z - p01.z) - (p10.z - p00.z)), bb.w + ((p11.w - p01.w) - (p10.w - p00.w)));
                }
                *(float4*)(o + c4) = make_float4(fmaxf(acc[mt][nb][4 * q] + add.x, 0.f), fmaxf(acc[mt][nb][4 * q + 1] + add.y, 0.f),
                                                 fmaxf(acc[mt][nb][4 * q + 2] + add.z, 0.f), fmaxf(acc[mt][nb][4 * q + 3] + add.w, 0.f));
            }
    }
#endif
}

// ---- max pool 3x3 stride 2 (no padding), NHWC --------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ in, float* __restrict__ out, int n, int h, int w,
                                                          int c, int ho, int wo, int in_packed, int out_packed) {
    const int c4n = c / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * ho * wo * c4n) return;
    const int c4 = (int)(i % c4n); int64_t p = i / c4n;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho);
    const int b = (int)(p / ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const float4 v = ld4_any(in + (((int64_t)b * h + 2 * oy + ky) * w + 2 * ox + kx) * c, c4 * 4, in_packed);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    st4_any(out + (((int64_t)b * ho + oy) * wo + ox) * c, c4 * 4, m, out_packed);
}

// ---- per-layer score ------------------------------------------------------------------------------------------------
// feat: NHWC [2n, h, w, C] (first n = img, last n = ref); out partial[n][blocks] of sum over pixels.
// A lane owns 4-channel runs (one 16-B access on PLAIN rows, 8 B + 4 B on PACKED ones): R = C / 4 runs per pixel.  With
// R = 16 (relu1, C = 64) a wave takes four pixels at once (16-lane reductions); otherwise one pixel per wave and up to two
// runs per lane (C <= 512).
struct ScoreArgs { const float* feat[5]; const float* lin[5]; int hw[5], C[5], packed[5]; };
// (one launch for the five layers -- grid.z = layer -- so their small grids share the chip instead of queueing one by one)
__global__ __launch_bounds__(256) void lpips_score_kernel(const ScoreArgs sa, int n, double* __restrict__ partials_all, int blocks_per_img, int layer0) {
    __shared__ double red[4];
    const int layer = layer0 + blockIdx.z;
    const float* __restrict__ feat = sa.feat[layer]; const float* __restrict__ lin = sa.lin[layer];
    const int hw = sa.hw[layer], C = sa.C[layer], packed = sa.packed[layer];
    double* __restrict__ partials = partials_all + (size_t)layer * n * blocks_per_img;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* f0 = feat + (int64_t)b * hw * C;
    const float* f1 = feat + (int64_t)(b + n) * hw * C;
    const int R = C >> 2;
    const int P = (R <= 16) ? 4 : 1;                    // pixels per wave
    const int sub = (P == 4) ? (lane >> 4) : 0;         // the lane's pixel inside the wave
    const int run0 = (P == 4) ? (lane & 15) : lane;
    double acc = 0.0;
    for (int p0 = (blockIdx.x * 4 + wave) * P; p0 < hw; p0 += blocks_per_img * 4 * P) {
        const int p = p0 + sub;
        const bool pok = p < hw;
        float4 a[2], c[2];
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int run = run0 + 64 * k;
            a[k] = make_float4(0.f, 0.f, 0.f, 0.f); c[k] = a[k];
            if (pok && run < R && (k == 0 || P == 1)) {
                a[k] = ld4_any(f0 + (int64_t)p * C, run * 4, packed);
                c[k] = ld4_any(f1 + (int64_t)p * C, run * 4, packed);
            }
            s0 += (a[k].x * a[k].x + a[k].y * a[k].y) + (a[k].z * a[k].z + a[k].w * a[k].w);
            s1 += (c[k].x * c[k].x + c[k].y * c[k].y) + (c[k].z * c[k].z + c[k].w * c[k].w);
        }
        const int top = (P == 4) ? 8 : 32;               // reduce over the lanes of one pixel
        for (int o = top; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
        const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int run = run0 + 64 * k;
            if (pok && run < R && (k == 0 || P == 1)) {
                const float4 w = *(const float4*)(lin + run * 4);
                const float e0 = a[k].x / n0 - c[k].x / n1, e1 = a[k].y / n0 - c[k].y / n1;
                const float e2 = a[k].z / n0 - c[k].z / n1, e3 = a[k].w / n0 - c[k].w / n1;
                d = fmaf(w.x, e0 * e0, d); d = fmaf(w.y, e1 * e1, d); d = fmaf(w.z, e2 * e2, d); d = fmaf(w.w, e3 * e3, d);
            }
        }
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);      // all pixels of the wave together
        acc += (double)d;
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(int64_t)b * blocks_per_img + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per image: lanes stride over a layer's partial sums, fixed-order tree (deterministic), layers added in order
// (round 5: one THREAD per image walked 5 x blocks_per_img dependent loads -- 19 us of a one-sequence frame's evaluation chain)
__global__ __launch_bounds__(64) void lpips_final_kernel(const double* __restrict__ partials, double* __restrict__ out, int blocks_per_img, int nlayers,
                                   int n, const int* __restrict__ hw) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= n) return;
    double total = 0.0;
    for (int l = 0; l < nlayers; ++l) {
        double s = 0.0;
        for (int k = lane; k < blocks_per_img; k += 64) s += partials[((int64_t)l * n + b) * blocks_per_img + k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        total += s / (double)hw[l];
    }
    if (lane == 0) out[b] = total;
}

// work-groups per image and layer of the score kernel: 32 at 64 images (2048 per launch); a small batch takes more of them -- at one
// image 32 work-groups walked relu1's 5440 pixels in eleven dependent rounds (16 us per layer)
constexpr int SCORE_BLOCKS_MAX = 256;
static int score_blocks(int n) { int b = 2048 / (n > 0 ? n : 1); return b < 32 ? 32 : (b > SCORE_BLOCKS_MAX ? SCORE_BLOCKS_MAX : b); }

}  // namespace

struct evr_lpips {
    // conv1 (direct) + 4 igemm layers
    std::vector<float> wg, wb, b1, b1in, wfrag1, wbsum;
    float* d_wg = nullptr; float* d_wb = nullptr; float* d_b1 = nullptr; float* d_b1in = nullptr;
    float* d_wfrag1 = nullptr; float* d_wbsum = nullptr;     // matrix-core form of conv1 (split mode)
    float* d_lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    BackboneConv L[4];
    // shape-dependent.  Buffers are sized for `cap` image pairs at H x W and only ever grow; what depends on the pair count n of a call
    // (the four ConvArgs with their tile choice) lives in the plan cache (lpips_host.h).
    int n = 0, H = 0, W = 0, cap = 0;
    int h[5], w[5];              // feature map sizes of relu1..relu5
    DeviceAllocs allocs;
    float* feat[5] = {}; float* pool1 = nullptr; float* pool2 = nullptr;
    PlanCache<4> plans;
    SplitWorkspace kws;
    double* partials = nullptr; int* d_hw = nullptr;
    void release() {
        allocs.release();
        n = 0; cap = 0; plans.clear(); kws = SplitWorkspace();
    }
    ~evr_lpips() {
        release();
        if (d_wg) (void)hipFree(d_wg); if (d_wb) (void)hipFree(d_wb); if (d_b1) (void)hipFree(d_b1); if (d_b1in) (void)hipFree(d_b1in);
        if (d_wfrag1) (void)hipFree(d_wfrag1); if (d_wbsum) (void)hipFree(d_wbsum);
        for (auto& p : d_lin) if (p) (void)hipFree(p);
        for (auto& l : L) free_backbone_conv(l);
    }
};

extern "C" int evr_lpips_create(const evr_tensor* tensors, int n_tensors, evr_lpips** out) {
    EVR_REQUIRE(tensors && out, "evr_lpips_create: null argument");
    const StateDict sd("LPIPS", tensors, n_tensors);
    evr_lpips* m = new evr_lpips();
    int rc = EVR_OK;
    const evr_tensor *w, *b;
    // torchvision alexnet.features indices 0,3,6,8,10 inside pyiqa's slices
    const char* names[5] = {"net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10"};
    const int cin[5] = {3, 64, 192, 384, 256}, cout[5] = {64, 192, 384, 256, 256}, ks[5] = {11, 5, 3, 3, 3};
    do {
        if ((rc = sd.get(std::string(names[0]) + ".weight", 64 * 3 * 121, &w))) break;
        if ((rc = sd.get(std::string(names[0]) + ".bias", 64, &b))) break;
        fold_scaling_layer(w->data_host, b->data_host, 64, 121, m->wg, m->wb, m->b1, m->b1in);
        if ((rc = upload(m->wg, &m->d_wg))) break;
        if ((rc = upload(m->wb, &m->d_wb))) break;
        if ((rc = upload(m->b1, &m->d_b1))) break;
        if ((rc = upload(m->b1in, &m->d_b1in))) break;
        if (use_split_mode()) {
            // weight fragments of lpips_conv1_mfma_kernel: [slab s][block nb][hi, lo][lane] x 4 dwords, lane (r, h) holding the
            // 8 taps k = 16s + 8h + j of output channel nb*32 + r as bf16 pairs (taps >= 121: zero)
            m->wfrag1.assign((size_t)8 * 2 * 2 * 64 * 4, 0.f);
            unsigned* wf = (unsigned*)m->wfrag1.data();
            for (int s8 = 0; s8 < 8; ++s8) for (int nb = 0; nb < 2; ++nb) for (int lane = 0; lane < 64; ++lane) {
                const int r = lane & 31, hh = lane >> 5;
                unsigned short hi[8], lo[8];
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s8 + 8 * hh + j;
                    const float wv = k < 121 ? m->wg[(size_t)k * 64 + nb * 32 + r] : 0.f;
                    hi[j] = bf16_rne(wv); lo[j] = bf16_rne(wv - bf16_to_f32(hi[j]));
                }
                for (int d = 0; d < 4; ++d) {
                    wf[((((size_t)s8 * 2 + nb) * 2 + 0) * 64 + lane) * 4 + d] = (unsigned)hi[2 * d] | ((unsigned)hi[2 * d + 1] << 16);
                    wf[((((size_t)s8 * 2 + nb) * 2 + 1) * 64 + lane) * 4 + d] = (unsigned)lo[2 * d] | ((unsigned)lo[2 * d + 1] << 16);
                }
            }
            // prefix sums of wb over the window: P[i][j][co] = sum_{ky < i, kx < j} wb[ky][kx][co] (fp64, rounded once)
            m->wbsum.assign((size_t)12 * 12 * 64, 0.f);
            for (int co = 0; co < 64; ++co) {
                double Pd[12][12] = {};
                for (int i = 1; i < 12; ++i) for (int j = 1; j < 12; ++j)
                    Pd[i][j] = Pd[i - 1][j] + Pd[i][j - 1] - Pd[i - 1][j - 1] + (double)m->wb[(size_t)((i - 1) * 11 + (j - 1)) * 64 + co];
                for (int i = 0; i < 12; ++i) for (int j = 0; j < 12; ++j) m->wbsum[(size_t)(i * 12 + j) * 64 + co] = (float)Pd[i][j];
            }
            if ((rc = upload(m->wfrag1, &m->d_wfrag1))) break;
            if ((rc = upload(m->wbsum, &m->d_wbsum))) break;
        }
        // conv2..conv5 run on the same implicit-GEMM family as the networks, in their mode
        for (int l = 1; l < 5 && !rc; ++l) rc = prepare_backbone_conv(sd, names[l], cin[l], cout[l], ks[l], backbone_mode(), &m->L[l - 1]);
        if (rc) break;
        for (int l = 0; l < 5 && !rc; ++l) {
            if ((rc = sd.get("lin" + std::to_string(l) + ".model.1.weight", cout[l], &w))) break;
            std::vector<float> lw(w->data_host, w->data_host + cout[l]);
            rc = upload(lw, &m->d_lin[l]);
        }
    } while (0);
    if (rc) { delete m; return rc; }
    *out = m;
    return EVR_OK;
}

extern "C" int evr_lpips_destroy(evr_lpips* m) { delete m; return EVR_OK; }

// (re)allocate the feature buffers for `cap` image pairs of H x W: the only place that synchronises
static int lpips_buffers(evr_lpips* m, int cap, int H, int W, hipStream_t stream) {
    EVR_HIP(hipStreamSynchronize(stream));
    m->release();
    m->cap = cap; m->H = H; m->W = W;
    const int n2 = 2 * cap;
    m->h[0] = (H + 4 - 11) / 4 + 1; m->w[0] = (W + 4 - 11) / 4 + 1;
    const int hp1 = (m->h[0] - 3) / 2 + 1, wp1 = (m->w[0] - 3) / 2 + 1;
    m->h[1] = hp1; m->w[1] = wp1;
    const int hp2 = (hp1 - 3) / 2 + 1, wp2 = (wp1 - 3) / 2 + 1;
    for (int l = 2; l < 5; ++l) { m->h[l] = hp2; m->w[l] = wp2; }
    if (!(hp2 >= 1 && wp2 >= 1)) { m->cap = 0; m->H = m->W = 0; }
    EVR_REQUIRE(hp2 >= 1 && wp2 >= 1, "evr_lpips: image %dx%d too small for AlexNet", W, H);
    const int C[5] = {64, 192, 384, 256, 256};
    int rc;
    for (int l = 0; l < 5; ++l) if ((rc = m->allocs.alloc(&m->feat[l], (size_t)n2 * m->h[l] * m->w[l] * C[l]))) return rc;
    if ((rc = m->allocs.alloc(&m->pool1, (size_t)n2 * hp1 * wp1 * 64))) return rc;
    if ((rc = m->allocs.alloc(&m->pool2, (size_t)n2 * hp2 * wp2 * 192))) return rc;
    if ((rc = m->allocs.alloc(&m->partials, (size_t)5 * cap * SCORE_BLOCKS_MAX))) return rc;
    if ((rc = m->allocs.alloc(&m->d_hw, 8))) return rc;
    if ((rc = m->allocs.alloc(&m->plans.d_args, (size_t)m->plans.NPLANS * 4))) return rc;
    int hw[5]; for (int l = 0; l < 5; ++l) hw[l] = m->h[l] * m->w[l];
    EVR_HIP(hipMemcpy(m->d_hw, hw, sizeof(hw), hipMemcpyHostToDevice));
    return EVR_OK;
}

// the plan of n image pairs inside the current buffers (PlanCache::get fills a slot with this)
static void lpips_fill_plan(evr_lpips* m, PlanCache<4>::Plan& pl, int n) {
    const float* ins[4] = {m->pool1, m->pool2, m->feat[2], m->feat[3]};
    for (int i = 0; i < 4; ++i) {
        ConvArgs& a = pl.args[i];
        fill_backbone_conv(a, m->L[i], ins[i], m->feat[i + 1], 2 * n, m->h[i + 1], m->w[i + 1]);      // (pool1 / pool2 / feat1..feat4)
        {   // conv2 (5x5) on the band kernel with 8 KB of LDS padding (two blocks per CU instead of three); EVR_LPIPS_BAND5=<KB> sets the
            // padding, EVR_LPIPS_BAND5=-1 keeps the implicit GEMM (the default until the evaluation stream moved behind the residual
            // blocks: beside the ConvLSTM layers its LDS footprint cost more than the kernel gained; now +0.7 .. 1.0 %, profiles/r03_env_ab.txt)
            const int kb = lib_knobs().lpips_band5_kb;
            a.no_band5 = kb < 0 ? 1 : 0; a.band_lds_pad = kb < 0 ? 0 : kb * 1024;
        }
        pick_conv_tile(a, 32, &pl.wm[i], &pl.nb[i]);
    }
    attach_split_workspace(m->kws, m->allocs, pl.args, 4, 1);      // (conv3..conv5 are the ones that may split)
}

extern "C" int evr_lpips_forward(evr_lpips* m, const float* img, const float* ref, int n, int H, int W, int clip, double* out,
                                 evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(m && img && ref && out && n >= 1 && H >= 1 && W >= 1, "evr_lpips_forward: bad argument");
    int rc;
    if (m->H != H || m->W != W || n > m->cap) if ((rc = lpips_buffers(m, n, H, W, stream))) { m->release(); m->H = m->W = 0; return rc; }      // (a half-built set of buffers must not look like capacity)
    PlanCache<4>::Plan* plan = nullptr;
    if ((rc = m->plans.get(n, stream, [m](PlanCache<4>::Plan& pl, int np) { lpips_fill_plan(m, pl, np); }, &plan))) return rc;
    m->n = n;
    const PlanCache<4>::Plan& P = *plan;
    ConvArgs* const d_args = m->plans.device_args(plan);
    const int n2 = 2 * n;
    Conv1Args c1{};
    c1.img = img; c1.ref = ref; c1.n = n; c1.H = H; c1.W = W; c1.h1 = m->h[0]; c1.w1 = m->w[0]; c1.clip = clip;
    c1.wg = m->d_wg; c1.wb = m->d_wb; c1.bias = m->d_b1; c1.bias_in = m->d_b1in; c1.out = m->feat[0];
    c1.wfrag = (const unsigned*)m->d_wfrag1; c1.wbsum = m->d_wbsum;
    static std::atomic<unsigned> attr_done[64];      // the LDS-size attribute is per device
    int dev = 0;
    EVR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_done[dev].load(std::memory_order_relaxed)) {
        EVR_HIP(hipFuncSetAttribute((const void*)lpips_conv1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        EVR_HIP(hipFuncSetAttribute((const void*)lpips_conv1_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (dev >= 0 && dev < 64) attr_done[dev].store(1, std::memory_order_relaxed);
    }
    const bool conv1_valu = lib_knobs().lpips_conv1_valu;      // EVR_LPIPS_CONV1_VALU, A/B switch: the direct VALU kernel in split mode too
    if (m->d_wfrag1 && !conv1_valu) {
        const size_t lds = (size_t)(71 * 71 + 3) * sizeof(float) + (size_t)8 * 2 * 2 * 64 * 16;
        hipLaunchKernelGGL(lpips_conv1_mfma_kernel, dim3((m->w[0] + 15) / 16, (m->h[0] + 15) / 16, n2), dim3(256), lds, stream, c1);
    } else {
        const size_t lds1 = (size_t)(2 * 71 * 71) * sizeof(float);
        hipLaunchKernelGGL(lpips_conv1_kernel, dim3((m->w[0] + 15) / 16, (m->h[0] + 15) / 16, n2), dim3(256), lds1, stream, c1);
    }
    EVR_LAUNCH_CHECK();
    const int pk = packed_fmt(m->L[0].x3);
    auto pool = [&](const float* in, float* o, int h, int w, int c, int ho, int wo, int in_pk) -> int {
        const int64_t total = (int64_t)n2 * ho * wo * (c / 4);
        hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, o, n2, h, w, c, ho, wo, in_pk, pk);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    };
    // The layer scores read both images' features again: scored right behind the layer that wrote them (EVR_LPIPS_SCORE_SPLIT, default
    // 1) they come from the Infinity Cache -- 446 MB per 64-frame step that one launch at the end fetched from HBM (conv1's 180 MB of
    // features are long evicted by then).  Same partial sums, same final reduction: bit-identical scores.
    const int score_split = lib_knobs().lpips_score_split;
    const int C[5] = {64, 192, 384, 256, 256};
    ScoreArgs sa;
    const int sblocks = score_blocks(n);
    for (int l = 0; l < 5; ++l) { sa.feat[l] = m->feat[l]; sa.lin[l] = m->d_lin[l]; sa.hw[l] = m->h[l] * m->w[l]; sa.C[l] = C[l]; sa.packed[l] = l > 0 ? pk : 0; }
    auto score = [&](int l0, int nl) -> int {
        hipLaunchKernelGGL(lpips_score_kernel, dim3(sblocks, n, nl), dim3(256), 0, stream, sa, n, m->partials, sblocks, l0);
        EVR_LAUNCH_CHECK();
        return EVR_OK;
    };
    if (score_split && (rc = score(0, 1))) return rc;
    if ((rc = pool(m->feat[0], m->pool1, m->h[0], m->w[0], 64, m->h[1], m->w[1], 0))) return rc;
    if ((rc = launch_conv_igemm(P.args[0], d_args + 0, 32, P.wm[0], P.nb[0], stream))) return rc;
    if (score_split && (rc = score(1, 1))) return rc;
    if ((rc = pool(m->feat[1], m->pool2, m->h[1], m->w[1], 192, m->h[2], m->w[2], pk))) return rc;
    // (relu3 .. relu5 are 69 MB together at 64 frames -- they outlive their convolutions in the Infinity Cache -- so ONE launch scores
    // the three of them behind conv5 (grid.z = layer): two launches fewer on the evaluation stream; EVR_LPIPS_SCORE_SPLIT=2: one each)
    for (int i = 1; i < 4; ++i) {
        if ((rc = launch_conv_igemm(P.args[i], d_args + i, 32, P.wm[i], P.nb[i], stream))) return rc;
        if (score_split == 2 && (rc = score(i + 1, 1))) return rc;
    }
    if (score_split == 1 && (rc = score(2, 3))) return rc;
    if (!score_split && (rc = score(0, 5))) return rc;
    hipLaunchKernelGGL(lpips_final_kernel, dim3(n), dim3(64), 0, stream, m->partials, out, sblocks, 5, n, m->d_hw);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" double evr_lpips_flops(const evr_lpips* m) {
    if (!m || m->n == 0) return 0.0;
    const int cin[5] = {3, 64, 192, 384, 256}, cout[5] = {64, 192, 384, 256, 256}, ks[5] = {11, 5, 3, 3, 3};
    double f = 0.0;
    for (int l = 0; l < 5; ++l) f += 2.0 * (2.0 * m->n) * m->h[l] * m->w[l] * cin[l] * cout[l] * ks[l] * ks[l];
    return f;
}
