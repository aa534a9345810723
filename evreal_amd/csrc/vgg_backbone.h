// The kernel side of what the metrics on the VGG-16 trunk share (lpips_vgg.hip: LPIPS-VGG, dists.hip: DISTS): the table of the twelve
// convolutions that run on the kernels of conv.hip, and conv1_1 -- the direct kernel on the gray frame with its launcher.  The host side
// (weights, buffers, plans, the passes of a call) is vgg_trunk.h; the fold of a metric's input scaling into conv1_1's weights is
// lpips_host.h fold_scaling_layer.
#pragma once
#include "conv.h"
#include "packed.h"

namespace evr {

constexpr int VGG_NCONV = 12;                              // convolutions on conv.hip (conv1_2 .. conv5_3)
constexpr int VGG_CIN[VGG_NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int VGG_COUT[VGG_NCONV] = {64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int VGG_LEVEL[VGG_NCONV] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};      // resolution level: one pool in front of every new level
constexpr int VGG_TAP_C[5] = {64, 128, 256, 512, 512};      // channels of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
// Two ping-pong activation buffers: conv1_1 writes buffer 0, and every convolution and every pool writes the buffer it does not read.
// -> the buffer convolution i (0 = conv1_2) reads: one flip per convolution before it, plus one per pool in front of its level
inline int vgg_conv_src(int i) { return (1 + i + VGG_LEVEL[i]) & 1 ? 0 : 1; }

// ---- conv1_1: gray [n2,H,W] -> [n2,H,W,64], 3x3 pad 1, relu ---------------------------------------------------------
// x_c = alpha_c*g + beta_c inside the image (LPIPS: ((2g-1) - shift_c)/scale_c; DISTS: (g - mean_c)/std_c) and 0 where the convolution pads, so
//   sum_c sum_t w[co][c][t] x_c[t] = sum_t inside[t] * (wg[t][co]*g[t] + wb[t][co])
// with wg = sum_c w*alpha_c, wb = sum_c w*beta_c folded on the host in fp64: a ONE-channel 3x3 convolution plus, for pixels on
// the image border, the wb term under the inside mask; interior pixels take sum_t wb[t] from the bias.
// A thread owns 16 consecutive channels (one 64-B group of the output row: four 16-B stores in every format) of two pixels in
// a row; the 2 x 9 x 64 folded weights sit in LDS (a lane reads the 16-B slots of its group: four distinct addresses per wave).
struct Conv11Args {
    const float* img; const float* ref;   // [n,H,W] each; batch index >= n reads ref
    int n, H, W, clip;
    const float* wg;                       // [9][64]
    const float* wb;                       // [9][64]
    const float* bias;                     // [64]
    const float* bias_in;                  // [64] bias + sum_t wb[t]  (interior pixels)
    float* out;
    unsigned* sat;
};

constexpr int C11_PX = 2;      // pixels per thread (four: 172 registers, two waves per SIMD)
template <int FMT>
__global__ __launch_bounds__(256) void vgg_conv1_1_kernel(const Conv11Args a) {
    constexpr int PX = C11_PX;
    __shared__ __attribute__((aligned(16))) float s_w[2 * 9 * 64];      // wg | wb
    for (int i = threadIdx.x; i < 2 * 9 * 64; i += 256) s_w[i] = i < 576 ? a.wg[i] : a.wb[i - 576];
    __syncthreads();
    const int wq = (a.W + PX - 1) / PX;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)2 * a.n * a.H * wq * 4) return;
    const int g = (int)(i & 3); int64_t p = i >> 2;
    const int x0 = (int)(p % wq) * PX; p /= wq;
    const int y = (int)(p % a.H);
    const int b = (int)(p / a.H);
    const float* src = (b < a.n ? a.img + (int64_t)b * a.H * a.W : a.ref + (int64_t)(b - a.n) * a.H * a.W);
    // the 3 x (PX + 2) gray window of the thread's pixels (0 outside the image); inside mask = rowm x colm
    float gv[3][PX + 2], rowm[3], colm[PX + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) rowm[r] = (unsigned)(y + r - 1) < (unsigned)a.H ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < PX + 2; ++c) colm[c] = (unsigned)(x0 + c - 1) < (unsigned)a.W ? 1.f : 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < PX + 2; ++c) {
            const int yy = y + r - 1, xx = x0 + c - 1;
            float v = 0.f;
            if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) {
                v = src[(int64_t)yy * a.W + xx];
                if (a.clip) v = fminf(fmaxf(v, 0.f), 1.f);
            }
            gv[r][c] = v;
        }
    const bool interior = y >= 1 && y + 1 < a.H && x0 >= 1 && x0 + PX < a.W;      // every tap of the thread's pixels is inside
    float acc[PX][16];
    {
        const float4* bp = (const float4*)((interior ? a.bias_in : a.bias) + 16 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bv = bp[q];
#pragma unroll
            for (int px = 0; px < PX; ++px) { acc[px][4 * q] = bv.x; acc[px][4 * q + 1] = bv.y; acc[px][4 * q + 2] = bv.z; acc[px][4 * q + 3] = bv.w; }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t % 3;
        float w[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 wv = *(const float4*)(s_w + t * 64 + 16 * g + 4 * q);
            w[4 * q] = wv.x; w[4 * q + 1] = wv.y; w[4 * q + 2] = wv.z; w[4 * q + 3] = wv.w;
        }
#pragma unroll
        for (int px = 0; px < PX; ++px)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[px][k] = fmaf(gv[ky][px + kx], w[k], acc[px][k]);
        if (!interior) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 wv = *(const float4*)(s_w + 576 + t * 64 + 16 * g + 4 * q);
                w[4 * q] = wv.x; w[4 * q + 1] = wv.y; w[4 * q + 2] = wv.z; w[4 * q + 3] = wv.w;
            }
#pragma unroll
            for (int px = 0; px < PX; ++px) {
                const float mk = rowm[ky] * colm[px + kx];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[px][k] = fmaf(mk, w[k], acc[px][k]);
            }
        }
    }
#pragma unroll
    for (int px = 0; px < PX; ++px) {
        if (x0 + px >= a.W) continue;
        float* o = a.out + (((int64_t)b * a.H + y) * a.W + x0 + px) * 64;
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = fmaxf(acc[px][k], 0.f);
        if constexpr (FMT == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *(float4*)(o + 16 * g + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
            sat_check16<FMT>(a.sat, v);
            store16_fmt<FMT>(o, 0u, 16 * g, v);
#endif
        }
    }
}

template <int FMT>
inline int launch_conv1_1(const Conv11Args& c, hipStream_t stream) {
    const int64_t total = (int64_t)2 * c.n * c.H * ((c.W + C11_PX - 1) / C11_PX) * 4;
    hipLaunchKernelGGL(vgg_conv1_1_kernel<FMT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, c);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}
// the instantiation of an activation format (conv.h packed_fmt: 0 PLAIN, 1 PACKED, 2 H2)
inline int launch_conv1_1_fmt(int fmt, const Conv11Args& c, hipStream_t stream) {
    return fmt == 2 ? launch_conv1_1<2>(c, stream) : fmt == 1 ? launch_conv1_1<1>(c, stream) : launch_conv1_1<0>(c, stream);
}

}  // namespace evr
