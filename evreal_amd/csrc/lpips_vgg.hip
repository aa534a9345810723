// LPIPS (VGG-16, v0.1) on gfx950 -- the 'lpips-vgg' metric of the reference (utils/eval_metrics.py:100-156:
// pyiqa.create_metric('lpips-vgg') on [n,3,H,W] batches built by cv2torch(img, num_ch=3), eval_utils.py:46-54).
//
// PARITY UNPINNED: pyiqa and torchvision are neither in the reference tree nor installed, and the VGG + linear-head weights are
// downloaded at run time (unobtainable offline).  The arithmetic below follows the published algorithm (Zhang et al. 2018;
// richzhang/PerceptualSimilarity v0.1 with net='vgg', as wrapped by pyiqa): x <- 2g-1; (x-shift)/scale per channel (the constants
// of lpips_host.h); torchvision vgg16.features with taps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; MaxPool2d(2, 2) in floor
// mode as the first operation of slices 2-5; unit-normalise every pixel's feature vector, f/(|f| + 1e-10); squared difference;
// non-negative 1x1 "lin" weights; spatial mean; sum over the five layers.  Conventions that stay unpinned until
// tests/test_lpips_vgg_pins.py has run where pyiqa exists -- recalled from the published code, not read from it: the state-dict
// names net.slice1.{0,2}, net.slice2.{5,7}, net.slice3.{10,12,14}, net.slice4.{17,19,21}, net.slice5.{24,26,28} (.weight, .bias)
// and lin{0..4}.model.1.weight (64, 128, 256, 512, 512 elements), and the pool positions (torchvision indices 4, 9, 16, 23).
// Scores agree with the restatement tests/lpips_vgg_ref.py on any weights, and with pyiqa only once its weights are supplied.
//
// Layers: the thirteen convolutions are the VGG-16 trunk this metric shares with dists.hip, kernels (vgg_backbone.h) and host side
// (vgg_trunk.h: the handle holds a VggTrunk) -- conv1_1 (3->64) is a direct VALU kernel on the gray input (the three input channels are
// affine in the same gray value); the other twelve 3x3 convolutions run on the convolution kernels of conv.hip (split arithmetic: every
// activation tensor is PACKED / H2; fp32 mode: PLAIN, Winograd where eligible).  This file's own: the state-dict names, the scaling
// constants, and the head -- one streaming kernel per tap layer scores it and writes the 2x2 max pool (floor mode) of both images'
// features -- the 64-channel full-resolution tensor is read once.
//
// Memory plan (vgg_trunk.h): relu1_2 is 2*H*W*64*4 B per pair (46 MB at 346x260), so features are NOT kept: two ping-pong activation
// buffers sized for the largest layer, 2*P*H*W*64*4 B each for P pairs per pass, P chosen so that both fit ACT_BUDGET_BYTES (at least 1;
// `max_pairs` at create overrides it); a call with more pairs runs in passes, both frames of a pair always in the same pass.
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "conv.h"
#include "packed.h"
#include "vgg_trunk.h"

using namespace evr;

namespace {

constexpr int MIN_SIDE = 16;                               // four floor-mode 2x2 pools must leave one pixel
constexpr const int* TAP_C = VGG_TAP_C;      // (the tables of the trunk and conv1_1: vgg_backbone.h)

// ---- one tap layer: LPIPS partial sums + the 2x2 max pool of both images' features -------------------------------------
// feat: [2n, h, w, C] (first n = img, last n = ref) in format `fmt`; pooled: [2n, h/2, w/2, C] in the same format, or null
// (relu5_3).  Work item = one 2x2 window of the grid ceil(h/2) x ceil(w/2): its pixels inside the image are scored (the odd last
// row / column too, which the floor-mode pool drops), and a window that lies wholly inside writes its pooled pixel.  A lane owns
// 4-channel runs (16 B on PLAIN rows): with R = C/4 runs per pixel a wave takes 64/R windows at once for R <= 64 (reductions
// over R lanes), one window and two runs per lane at C = 512.  Per-lane fp64 partial sums, reduced in a fixed order.
// NOT DONE: in the split modes a 4-channel run is an 8-B + 8-B (H2) or 8-B + 4-B + 4-B (PACKED) access through ld4_any / st4_any,
// not 16 B per lane; a whole-group form (16 channels per lane, four 16-B pieces each way as conv1_1 stores them) is the next step.
struct TapArgs {
    const float* feat; float* pooled; const float* lin;
    int n, h, w, C, fmt;
    double* partials;      // [n][blocks]
};

__global__ __launch_bounds__(256) void vgg_pool_score_kernel(const TapArgs a) {
    __shared__ double red[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = a.C >> 2;
    const int L = R < 64 ? R : 64;            // lanes per pixel (16, 32, 64)
    const int PW = 64 / L;                    // windows per wave
    const int sub = lane / L, run0 = lane % L;
    const int hw2 = (a.h + 1) >> 1, ww2 = (a.w + 1) >> 1, ho = a.h >> 1, wo = a.w >> 1;
    const int nwin = hw2 * ww2;
    const float* f0 = a.feat + (int64_t)b * a.h * a.w * a.C;
    const float* f1 = a.feat + (int64_t)(b + a.n) * a.h * a.w * a.C;
    float4 lw[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) lw[k] = (run0 + 64 * k < R) ? *(const float4*)(a.lin + (run0 + 64 * k) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    double acc = 0.0;
    for (int w0 = (blockIdx.x * 4 + wave) * PW; w0 < nwin; w0 += gridDim.x * 4 * PW) {
        const int win = w0 + sub;
        const bool wok = win < nwin;
        const int wy = wok ? win / ww2 : 0, wx = wok ? win % ww2 : 0;
        // the window's four pixels are loaded first and their eight squared norms reduced together: one dependent chain of
        // lane exchanges per window instead of one per pixel
        float4 va[4][2], vc[4][2];
        float s0[4], s1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = 2 * wy + (q >> 1), x = 2 * wx + (q & 1);
            const bool pok = wok && y < a.h && x < a.w;
            const int64_t poff = ((int64_t)y * a.w + x) * a.C;
            s0[q] = 0.f; s1[q] = 0.f;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int run = run0 + 64 * k;
                va[q][k] = make_float4(0.f, 0.f, 0.f, 0.f); vc[q][k] = va[q][k];
                if (pok && run < R) {
                    va[q][k] = ld4_any(f0 + poff, run * 4, a.fmt);
                    vc[q][k] = ld4_any(f1 + poff, run * 4, a.fmt);
                }
                s0[q] += (va[q][k].x * va[q][k].x + va[q][k].y * va[q][k].y) + (va[q][k].z * va[q][k].z + va[q][k].w * va[q][k].w);
                s1[q] += (vc[q][k].x * vc[q][k].x + vc[q][k].y * vc[q][k].y) + (vc[q][k].z * vc[q][k].z + vc[q][k].w * vc[q][k].w);
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) {      // over the lanes of one pixel
#pragma unroll
            for (int q = 0; q < 4; ++q) { s0[q] += __shfl_xor(s0[q], o, 64); s1[q] += __shfl_xor(s1[q], o, 64); }
        }
        float4 ma[2], mc[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) { ma[k] = make_float4(0.f, 0.f, 0.f, 0.f); mc[k] = ma[k]; }      // (relu outputs: 0 is the identity of max)
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // (a reciprocal per pixel and image instead of a division per channel: one more rounding of 2^-24, the same for both
            // images -- identical frames still score exactly 0)
            const float r0 = 1.0f / (sqrtf(s0[q]) + 1e-10f), r1 = 1.0f / (sqrtf(s1[q]) + 1e-10f);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float4 u = va[q][k], v = vc[q][k];
                ma[k].x = fmaxf(ma[k].x, u.x); ma[k].y = fmaxf(ma[k].y, u.y); ma[k].z = fmaxf(ma[k].z, u.z); ma[k].w = fmaxf(ma[k].w, u.w);
                mc[k].x = fmaxf(mc[k].x, v.x); mc[k].y = fmaxf(mc[k].y, v.y); mc[k].z = fmaxf(mc[k].z, v.z); mc[k].w = fmaxf(mc[k].w, v.w);
                float e0, e1, e2, e3;
                {   // both products rounded: contracted into a fused multiply-add, u r0 - v r1 is not 0 for u = v
#pragma clang fp contract(off)
                    e0 = u.x * r0 - v.x * r1; e1 = u.y * r0 - v.y * r1; e2 = u.z * r0 - v.z * r1; e3 = u.w * r0 - v.w * r1;
                }
                d = fmaf(lw[k].x, e0 * e0, d); d = fmaf(lw[k].y, e1 * e1, d); d = fmaf(lw[k].z, e2 * e2, d); d = fmaf(lw[k].w, e3 * e3, d);
            }
        }
        acc += (double)d;
        if (a.pooled && wok && wy < ho && wx < wo) {
            const int64_t ooff = ((int64_t)wy * wo + wx) * a.C;
            float* o0 = a.pooled + (int64_t)b * ho * wo * a.C + ooff;
            float* o1 = a.pooled + (int64_t)(b + a.n) * ho * wo * a.C + ooff;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int run = run0 + 64 * k;
                if (run < R) { st4_any(o0, run * 4, ma[k], a.fmt); st4_any(o1, run * 4, mc[k], a.fmt); }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.partials[(int64_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per pair: lanes stride over a layer's partial sums, fixed-order tree, layers added in order
struct FinalArgs { const double* partials[5]; int hw[5]; int blocks[5]; };
__global__ __launch_bounds__(64) void vgg_final_kernel(const FinalArgs f, int n, double* __restrict__ out, double* __restrict__ out_layers) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= n) return;
    double total = 0.0;
    for (int l = 0; l < 5; ++l) {
        double s = 0.0;
        for (int k = lane; k < f.blocks[l]; k += 64) s += f.partials[l][(int64_t)b * f.blocks[l] + k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const double dl = s / (double)f.hw[l];
        if (lane == 0 && out_layers) out_layers[(int64_t)b * 5 + l] = dl;
        total += dl;
    }
    if (lane == 0) out[b] = total;
}

// work-groups per pair of the tap kernel: every wave of a block wants at least a few windows; at most SCORE_BLOCKS_MAX
constexpr int SCORE_BLOCKS_MAX = 256;
int score_blocks(int n, int nwin, int C) {
    const int pw = C >= 256 ? 1 : 256 / C;                  // windows per wave and round
    int want = (nwin + 4 * pw * 4 - 1) / (4 * pw * 4);      // four rounds per wave
    const int cap = 4096 / (n > 0 ? n : 1);                 // ~16 blocks per CU over the whole launch
    if (want > cap) want = cap;
    if (want > SCORE_BLOCKS_MAX) want = SCORE_BLOCKS_MAX;
    return want < 1 ? 1 : want;
}

}  // namespace

struct evr_lpips_vgg {
    VggTrunk trunk;
    float* d_lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double* partials = nullptr;      // [5][cap][SCORE_BLOCKS_MAX], of trunk.allocs
    void release() { trunk.release(); partials = nullptr; }
    // (vgg_forward) the trunk's buffers with floor-mode pools, then the head's
    int buffers(int cap, int H, int W, hipStream_t stream) {
        int rc;
        if ((rc = trunk.buffers(cap, H, W, false, stream))) return rc;
        return trunk.allocs.alloc(&partials, (size_t)5 * cap * SCORE_BLOCKS_MAX);
    }
    ~evr_lpips_vgg() { for (auto& p : d_lin) if (p) (void)hipFree(p); }
};

extern "C" int evr_lpips_vgg_create(const evr_tensor* tensors, int n_tensors, int max_pairs, evr_lpips_vgg** out) {
    EVR_REQUIRE(tensors && out && max_pairs >= 0, "evr_lpips_vgg_create: bad argument");
    const StateDict sd("LPIPS-VGG", tensors, n_tensors);
    // torchvision vgg16.features indices inside pyiqa's slices (conv1_1 first)
    const char* const names[VGG_NCONV + 1] = {"net.slice1.0", "net.slice1.2", "net.slice2.5", "net.slice2.7", "net.slice3.10", "net.slice3.12", "net.slice3.14",
                                              "net.slice4.17", "net.slice4.19", "net.slice4.21", "net.slice5.24", "net.slice5.26", "net.slice5.28"};
    double a[3], b[3];
    lpips_scaling(a, b);
    evr_lpips_vgg* m = new evr_lpips_vgg();
    int rc = m->trunk.create(sd, names, a, b, max_pairs);
    for (int l = 0; l < 5 && !rc; ++l) {
        const evr_tensor* w;
        if ((rc = sd.get("lin" + std::to_string(l) + ".model.1.weight", TAP_C[l], &w))) break;
        rc = upload(std::vector<float>(w->data_host, w->data_host + TAP_C[l]), &m->d_lin[l]);
    }
    if (rc) { delete m; return rc; }
    *out = m;
    return EVR_OK;
}

extern "C" int evr_lpips_vgg_destroy(evr_lpips_vgg* m) { delete m; return EVR_OK; }

// one pass: np pairs starting at img / ref, scores to out[0..np) (and out_layers[0..5 np))
static int vgg_pass(evr_lpips_vgg* m, const float* img, const float* ref, int np, int clip, double* out, double* out_layers, hipStream_t stream) {
    VggTrunk& t = m->trunk;
    int rc, src = 0;
    VggTrunk::Plan* P = nullptr;
    if ((rc = t.begin_pass(np, stream, &P))) return rc;
    if ((rc = t.conv1_1(img, ref, np, clip, stream))) return rc;
    FinalArgs fa{};
    for (int l = 0; l < 5; ++l) {
        if ((rc = t.level_convs(P, l, stream, &src))) return rc;
        TapArgs tp{};
        tp.feat = t.act[src]; tp.pooled = l < 4 ? t.act[src ^ 1] : nullptr; tp.lin = m->d_lin[l];
        tp.n = np; tp.h = t.h[l]; tp.w = t.w[l]; tp.C = TAP_C[l]; tp.fmt = t.fmt();
        tp.partials = m->partials + (size_t)l * t.cap * SCORE_BLOCKS_MAX;
        const int nwin = ((tp.h + 1) / 2) * ((tp.w + 1) / 2), blocks = score_blocks(np, nwin, tp.C);
        hipLaunchKernelGGL(vgg_pool_score_kernel, dim3(blocks, np), dim3(256), 0, stream, tp);
        EVR_LAUNCH_CHECK();
        fa.partials[l] = tp.partials; fa.hw[l] = tp.h * tp.w; fa.blocks[l] = blocks;
    }
    hipLaunchKernelGGL(vgg_final_kernel, dim3(np), dim3(64), 0, stream, fa, np, out, out_layers);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" int evr_lpips_vgg_forward(evr_lpips_vgg* m, const float* img, const float* ref, int n, int H, int W, int clip, double* out,
                                     double* out_layers, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(m && img && ref && out && n >= 1 && H >= 1 && W >= 1, "evr_lpips_vgg_forward: bad argument");
    EVR_REQUIRE(H >= MIN_SIDE && W >= MIN_SIDE, "evr_lpips_vgg: image %dx%d too small for VGG-16 (four 2x2 pools need %d pixels a side)", W, H, MIN_SIDE);
    EVR_REQUIRE((int64_t)2 * H * W * 64 * 4 < ACT_BUFFER_MAX_BYTES, "evr_lpips_vgg: image %dx%d too large: one pair's 64-channel features must stay below 2 GiB (H*W < 2^22)", W, H);
    return vgg_forward(m, n, H, W, stream, [&](int o, int np) {
        return vgg_pass(m, img + (int64_t)o * H * W, ref + (int64_t)o * H * W, np, clip, out + o, out_layers ? out_layers + (int64_t)5 * o : nullptr, stream);
    });
}

extern "C" double evr_lpips_vgg_flops(const evr_lpips_vgg* m) { return m ? m->trunk.flops() : 0.0; }

extern "C" int evr_lpips_vgg_saturation(evr_lpips_vgg* m, int64_t* count, evr_stream_t stream_) {
    EVR_REQUIRE(m && count, "evr_lpips_vgg_saturation: null argument");
    return m->trunk.saturation(count, (hipStream_t)stream_);
}
