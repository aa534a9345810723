// Colour reconstruction helpers (ColorNet, model/model.py:46-105 of the reference; merge in utils/color_utils.py:53-88).
//
//   evr_bayer_split   event tensor [n,B,H,W] -> the four half-resolution Bayer sub-lattices R,G,B,W
//                     (model.py:54-57: R = [0::2,0::2], G = [0::2,1::2], B = [1::2,1::2], W = [1::2,0::2]) stacked as
//                     [4n,B,H/2,W/2] (sequence-major: R,G,B,W of sequence 0, then sequence 1, ...), so the recurrent
//                     network advances all four colour streams of all sequences in one batched step.
//   evr_color_merge   the five reconstructions -> one BGR uint8 frame: per-channel clip(img*255) -> uint8 (truncation,
//                     model.py:101), bilinear x2 of the four colour planes, the 1-pixel Bayer origin shifts with edge
//                     replication, G/W averaging, BGR -> CIE Lab, L replaced by the full-resolution gray reconstruction,
//                     Lab -> BGR (color_utils.py:20-88).
// PARITY: the split and the uint8 planes are pinned against the reference (tests/golden/colornet_seq.npz).  The merge
// follows OpenCV's documented formulas in floating point; OpenCV's own 8-bit fixed-point resize / Lab tables are not
// available offline (cv2 is absent), so merged pixels may differ from the reference by a few LSB -- UNPINNED.
//
//   evr_color_percentile_normalize   post_process_normalization (eval.py:380-395) of a merged uint8 BGR frame, as the reference
//                     applies it in colour mode: img = float32(u8) / 255 (exp of that for 'exprobust'), lo / hi = np.percentile over
//                     all 3*H*W values together, (img - lo) / (hi - lo), and the image writer's round(clip(., 0, 1) * 255).  Every
//                     step is a function of the byte level alone given the frame's 256-bin histogram, so no float image exists:
//                     color_hist_kernel counts the levels (integers: exact, order-independent), color_norm_apply_kernel finds the
//                     four order statistics in the cumulative counts, forms lo and hi with the float32 rule of pct.h from the
//                     caller's table level -> float32 value (the host's numpy computes it, exp included: no device expf), builds
//                     the 256-entry byte table and remaps the frame through it.  Bit-exact against numpy (tests/color_norm_ref.py).
//                     DEGENERATE FRAMES, hi == lo: the reference divides by zero -- levels above lo become +inf -> 255, levels
//                     below lo -inf -> 0, and the levels equal to lo are NaN.  NaN is DEFINED as byte 0 here (what numpy's cast
//                     to uint8 gives on x86); a constant frame therefore comes out all 0.
#include "common.h"
#include "pct.h"

namespace {

__global__ __launch_bounds__(256) void bayer_split_kernel(const float* __restrict__ vox, float* __restrict__ out, int n, int B,
                                                           int H, int W) {
    const int h2 = H / 2, w2 = W / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)n * 4 * B * h2 * w2;
    if (i >= total) return;
    const int x = (int)(i % w2); int64_t p = i / w2;
    const int y = (int)(p % h2); p /= h2;
    const int b = (int)(p % B); p /= B;
    const int ch = (int)(p % 4);
    const int s = (int)(p / 4);
    // R (0,0)  G (0,1)  B (1,1)  W (1,0)   as (row offset, column offset)
    const int oy = (ch >= 2) ? 1 : 0, ox = (ch == 1 || ch == 2) ? 1 : 0;
    out[i] = vox[(((int64_t)s * B + b) * H + 2 * y + oy) * W + 2 * x + ox];
}

__device__ __forceinline__ float q8(float v) {   // np.clip(img * 255, 0, 255).astype(np.uint8): truncation
    v = v * 255.f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return floorf(v);
}

// value of colour plane `ch` after cv2.resize(x2, INTER_LINEAR) and shift_image(dx, dy), at full-res pixel (y, x)
__device__ float plane_at(const float* __restrict__ pl, int h2, int w2, int y, int x, int dx, int dy) {
    const int H = 2 * h2, W = 2 * w2;
    // shift_image: np.roll by (dy, dx) then replicate the row/column just inside the wrapped border
    int sy = y - dy, sx = x - dx;
    if (dy > 0 && y < dy) sy = 0;          // X[:dy] = X[dy] (which holds source row 0 after the roll)
    if (dx > 0 && x < dx) sx = 0;
    sy = min(max(sy, 0), H - 1); sx = min(max(sx, 0), W - 1);
    // bilinear x2 (half-pixel centres, edge clamp) of the uint8 plane, result rounded to uint8
    float fy = (sy + 0.5f) * 0.5f - 0.5f, fx = (sx + 0.5f) * 0.5f - 0.5f;
    int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    float ly = fy - y0, lx = fx - x0;
    if (y0 < 0) { y0 = 0; ly = 0.f; }
    if (x0 < 0) { x0 = 0; lx = 0.f; }
    if (y0 >= h2 - 1) { y0 = h2 - 1; ly = 0.f; }
    if (x0 >= w2 - 1) { x0 = w2 - 1; lx = 0.f; }
    const int y1 = min(y0 + 1, h2 - 1), x1 = min(x0 + 1, w2 - 1);
    const float a = q8(pl[y0 * w2 + x0]), b = q8(pl[y0 * w2 + x1]), c = q8(pl[y1 * w2 + x0]), d = q8(pl[y1 * w2 + x1]);
    const float v = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
    return floorf(v + 0.5f);
}

__device__ __forceinline__ float srgb_to_lin(float c) { return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float lin_to_srgb(float c) { return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.f / 2.4f) - 0.055f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.f / 116.f; }
__device__ __forceinline__ float lab_finv(float t) { const float t3 = t * t * t; return t3 > 0.008856f ? t3 : (t - 16.f / 116.f) / 7.787f; }

// planes: [n][4][h2][w2] float (R,G,B,W streams, network output), gray: [n][H][W] float; out: [n][H][W][3] uint8 BGR
__global__ __launch_bounds__(256) void color_merge_kernel(const float* __restrict__ planes, const float* __restrict__ gray,
                                                           unsigned char* __restrict__ out, int n, int h2, int w2) {
    const int H = 2 * h2, W = 2 * w2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * H * W) return;
    const int x = (int)(i % W); int64_t p = i / W;
    const int y = (int)(p % H);
    const int s = (int)(p / H);
    const float* pl = planes + (int64_t)s * 4 * h2 * w2;
    const float R = plane_at(pl, h2, w2, y, x, 0, 0);
    const float G = plane_at(pl + (int64_t)h2 * w2, h2, w2, y, x, 1, 0);
    const float Bc = plane_at(pl + 2 * (int64_t)h2 * w2, h2, w2, y, x, 1, 1);
    const float Wc = plane_at(pl + 3 * (int64_t)h2 * w2, h2, w2, y, x, 0, 1);
    const float Gm = rintf(0.5f * G + 0.5f * Wc);           // cv2.addWeighted(..., dtype=CV_8U): round half to even
    // BGR (uint8) -> Lab (8-bit convention: L*255/100, a+128, b+128), D65, sRGB gamma
    const float r = srgb_to_lin(R / 255.f), g = srgb_to_lin(Gm / 255.f), b = srgb_to_lin(Bc / 255.f);
    float X = (0.412453f * r + 0.357580f * g + 0.180423f * b) / 0.950456f;
    float Z = (0.019334f * r + 0.119193f * g + 0.950227f * b) / 1.088754f;
    float Y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
    const float fxv = lab_f(X), fyv = lab_f(Y), fzv = lab_f(Z);
    float a8 = rintf(500.f * (fxv - fyv) + 128.f), b8 = rintf(200.f * (fyv - fzv) + 128.f);
    a8 = fminf(fmaxf(a8, 0.f), 255.f); b8 = fminf(fmaxf(b8, 0.f), 255.f);
    const float L8 = q8(gray[i]);                            // lab[:, :, 0] = grayscale_highres
    // Lab -> BGR
    const float L = L8 * 100.f / 255.f, aa = a8 - 128.f, bb = b8 - 128.f;
    const float fy2 = (L + 16.f) / 116.f, fx2 = fy2 + aa / 500.f, fz2 = fy2 - bb / 200.f;
    X = lab_finv(fx2) * 0.950456f; Y = lab_finv(fy2); Z = lab_finv(fz2) * 1.088754f;
    const float ro = 3.240479f * X - 1.537150f * Y - 0.498535f * Z;
    const float go = -0.969256f * X + 1.875991f * Y + 0.041556f * Z;
    const float bo = 0.055648f * X - 0.204043f * Y + 1.057311f * Z;
    auto to8 = [](float lin) { float v = rintf(lin_to_srgb(fminf(fmaxf(lin, 0.f), 1.f)) * 255.f); return (unsigned char)fminf(fmaxf(v, 0.f), 255.f); };
    out[i * 3 + 0] = to8(bo); out[i * 3 + 1] = to8(go); out[i * 3 + 2] = to8(ro);
}

// ---------------------------------------------------------------- percentile normalisation of uint8 BGR frames
// A clipped frame is often dominated by one or two levels (0 or 255) and a constant frame puts every byte in one bin, so the
// sub-histograms are split BY LANE: hist[level][lane] (64 KB of LDS per work-group).  A lane only ever touches its own column,
// column = LDS bank, so one ds_add instruction of a wave never meets a same-address or a same-bank conflict whatever the
// frame holds; the four waves of a work-group share the columns through the atomics.
constexpr int CH_THREADS = 256;
constexpr int CH_UNROLL = 4;                    // 16-B loads in flight per lane
constexpr int CH_VEC_PER_GROUP = 4096;          // 64 KB of the frame per work-group and grid-stride trip: amortises zeroing + merging

__device__ __forceinline__ void ch_add_word(unsigned* hist, unsigned w, int lane) {
    atomicAdd(&hist[(w & 255u) * 64 + lane], 1u);
    atomicAdd(&hist[((w >> 8) & 255u) * 64 + lane], 1u);
    atomicAdd(&hist[((w >> 16) & 255u) * 64 + lane], 1u);
    atomicAdd(&hist[(w >> 24) * 64 + lane], 1u);
}

// the bytes of frame f that 16-B accesses aligned on `p` do not cover: [0, head) and [head + 16 * nvec, nbytes)
__device__ __forceinline__ void ch_split(const void* p, int nbytes, int& head, int& nvec) {
    head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
    if (head > nbytes) head = nbytes;
    nvec = (nbytes - head) >> 4;
}

// in: [n][nbytes] uint8 (frame f starts at in + f * nbytes: any alignment); counts: [n][256], zeroed by the caller
__global__ __launch_bounds__(CH_THREADS) void color_hist_kernel(const unsigned char* __restrict__ in, int nbytes,
                                                                 unsigned* __restrict__ counts) {
    __shared__ unsigned hist[256 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned char* p = in + (int64_t)blockIdx.y * nbytes;
    for (int i = tid; i < 256 * 64 / 4; i += CH_THREADS) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    int head, nvec;
    ch_split(p, nbytes, head, nvec);
    const uint4* v = (const uint4*)(p + head);
    for (int i0 = blockIdx.x * (CH_THREADS * CH_UNROLL); i0 < nvec; i0 += gridDim.x * (CH_THREADS * CH_UNROLL)) {
        uint4 x[CH_UNROLL];
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {
            const int i = i0 + u * CH_THREADS + tid;
            x[u] = (i < nvec) ? v[i] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {
            if (i0 + u * CH_THREADS + tid < nvec) {
                ch_add_word(hist, x[u].x, lane); ch_add_word(hist, x[u].y, lane);
                ch_add_word(hist, x[u].z, lane); ch_add_word(hist, x[u].w, lane);
            }
        }
    }
    if (blockIdx.x == 0) {          // the unaligned head (wave 0) and the tail (wave 1): at most 15 bytes each
        const int tail0 = head + 16 * nvec;
        if (tid < head) atomicAdd(&hist[(unsigned)p[tid] * 64 + lane], 1u);
        else if (tid >= 64 && tail0 + (tid - 64) < nbytes) atomicAdd(&hist[(unsigned)p[tail0 + (tid - 64)] * 64 + lane], 1u);
    }
    __syncthreads();
    // thread t sums level t over the 64 columns, starting at its own column so that a wave reads 64 different banks per step
    unsigned s = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) s += hist[tid * 64 + ((j + tid) & 63)];
    if (s) atomicAdd(&counts[(int64_t)blockIdx.y * 256 + tid], s);
}

// Every work-group rebuilds its frame's cumulative counts, lo, hi and the byte table (a few hundred operations), then remaps its
// slice.  16-B accesses are aligned on the OUTPUT frame; the input is read through memcpy, so `in` and `out` may differ in alignment.
// values: [256] float32, level -> image value (non-decreasing); range: [n][2] = {lo, hi}
__global__ __launch_bounds__(CH_THREADS) void color_norm_apply_kernel(const unsigned char* in, unsigned char* out, int nbytes,
                                                                       const float* __restrict__ values, float q_lo, float q_hi,
                                                                       const unsigned* __restrict__ counts, float* __restrict__ range) {
    __shared__ unsigned wsum[CH_THREADS / 64];
    __shared__ int level[4];                    // lo.prev, lo.next, hi.prev, hi.next
    __shared__ unsigned char table[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t off = (int64_t)blockIdx.y * nbytes;
    const unsigned c = counts[(int64_t)blockIdx.y * 256 + tid];
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[tid >> 6] = incl;
    if (tid < 4) level[tid] = 0;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < (tid >> 6); ++w) base += wsum[w];
    const unsigned excl = base + incl - c;      // bytes of the frame below level tid
    int rank[4]; float gamma[2];
    pct_rank(nbytes, q_lo, rank[0], rank[1], gamma[0]);
    pct_rank(nbytes, q_hi, rank[2], rank[3], gamma[1]);
#pragma unroll
    for (int s = 0; s < 4; ++s)                 // the counts sum to nbytes: exactly one level holds each rank
        if (c > 0 && (unsigned)rank[s] >= excl && (unsigned)rank[s] < excl + c) level[s] = tid;
    __syncthreads();
    const float lo = pct_lerp(values[level[0]], values[level[1]], gamma[0]);
    const float hi = pct_lerp(values[level[2]], values[level[3]], gamma[1]);
    if (blockIdx.x == 0 && tid == 0) { range[(int64_t)blockIdx.y * 2] = lo; range[(int64_t)blockIdx.y * 2 + 1] = hi; }
    float x = (values[tid] - lo) / (hi - lo);
    x = (x == x) ? x : 0.f;                     // NaN (hi == lo at this level) -> byte 0
    x = fminf(fmaxf(x, 0.f), 1.f);
    table[tid] = (unsigned char)rintf(x * 255.f);
    __syncthreads();
    const unsigned char* src = in + off;
    unsigned char* dst = out + off;
    int head, nvec;
    ch_split(dst, nbytes, head, nvec);
    // (`in` may be `out`, so the compiler keeps every load behind the stores before it: the loads of a trip are issued together by hand)
    for (int i0 = blockIdx.x * (CH_THREADS * CH_UNROLL); i0 < nvec; i0 += gridDim.x * (CH_THREADS * CH_UNROLL)) {
        uint4 x4[CH_UNROLL];
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {
            const int i = i0 + u * CH_THREADS + tid;
            if (i < nvec) __builtin_memcpy(&x4[u], src + head + 16 * (int64_t)i, 16);
            else x4[u] = make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < CH_UNROLL; ++u) {
            const int i = i0 + u * CH_THREADS + tid;
            unsigned w[4] = {x4[u].x, x4[u].y, x4[u].z, x4[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (unsigned)table[w[k] & 255u] | ((unsigned)table[(w[k] >> 8) & 255u] << 8) |
                       ((unsigned)table[(w[k] >> 16) & 255u] << 16) | ((unsigned)table[w[k] >> 24] << 24);
            if (i < nvec) *(uint4*)(dst + head + 16 * (int64_t)i) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (blockIdx.x == 0) {
        const int tail0 = head + 16 * nvec;
        if (tid < head) dst[tid] = table[src[tid]];
        else if (tid >= 64 && tail0 + (tid - 64) < nbytes) dst[tail0 + (tid - 64)] = table[src[tail0 + (tid - 64)]];
    }
}

}  // namespace

extern "C" int evr_bayer_split(const float* vox, int n, int B, int H, int W, float* out, evr_stream_t stream) {
    EVR_REQUIRE(vox && out && n >= 1 && B >= 1, "evr_bayer_split: bad argument");
    EVR_REQUIRE(H % 2 == 0 && W % 2 == 0, "evr_bayer_split: sensor %dx%d must have even sides", W, H);
    const int64_t total = (int64_t)n * 4 * B * (H / 2) * (W / 2);
    hipLaunchKernelGGL(bayer_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vox, out, n, B, H, W);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" int evr_color_merge(const float* planes, const float* gray, int n, int H, int W, unsigned char* bgr_out,
                               evr_stream_t stream) {
    EVR_REQUIRE(planes && gray && bgr_out && n >= 1, "evr_color_merge: bad argument");
    EVR_REQUIRE(H % 2 == 0 && W % 2 == 0 && H >= 4 && W >= 4, "evr_color_merge: sensor %dx%d must have even sides", W, H);
    const int64_t total = (int64_t)n * H * W;
    hipLaunchKernelGGL(color_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes, gray,
                       bgr_out, n, H / 2, W / 2);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}

extern "C" size_t evr_color_percentile_normalize_workspace_bytes(int n) {
    return n > 0 ? (size_t)n * (256 * sizeof(unsigned) + 2 * sizeof(float)) : 0;      // counts [n][256], then {lo, hi} [n][2]
}

extern "C" int evr_color_percentile_normalize(const uint8_t* bgr_in, uint8_t* bgr_out, int n, int H, int W, const float* values256,
                                              float q_lo, float q_hi, void* workspace, size_t workspace_bytes, evr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    EVR_REQUIRE(n >= 0 && H >= 1 && W >= 1, "evr_color_percentile_normalize: bad shape");
    EVR_REQUIRE(q_lo >= 0.f && q_hi <= 100.f && q_lo <= q_hi, "evr_color_percentile_normalize: percentiles must be in [0,100]");
    // the ranks (n-1)*q are formed in float32 as numpy forms them: exact integers only below 2^24
    EVR_REQUIRE(3 * (int64_t)H * W < (1LL << 24), "evr_color_percentile_normalize: frame %dx%dx3 has 2^24 bytes or more", W, H);
    if (n == 0) return EVR_OK;
    EVR_REQUIRE(bgr_in != nullptr && bgr_out != nullptr && values256 != nullptr, "evr_color_percentile_normalize: null argument");
    const size_t need = evr_color_percentile_normalize_workspace_bytes(n);
    EVR_REQUIRE_WORKSPACE("evr_color_percentile_normalize", workspace, workspace_bytes, need);
    EVR_REQUIRE((((uintptr_t)workspace) & 3) == 0, "evr_color_percentile_normalize: workspace must be 4-byte aligned");
    const int nbytes = 3 * H * W;
    unsigned* counts = (unsigned*)workspace;
    float* range = (float*)(counts + (size_t)n * 256);
    EVR_HIP(hipMemsetAsync(counts, 0, (size_t)n * 256 * sizeof(unsigned), stream));
    const int nvec = nbytes / 16;
    int gh = (nvec + CH_VEC_PER_GROUP - 1) / CH_VEC_PER_GROUP;
    gh = gh < 1 ? 1 : (gh > 64 ? 64 : gh);
    hipLaunchKernelGGL(color_hist_kernel, dim3(gh, n), dim3(CH_THREADS), 0, stream, bgr_in, nbytes, counts);
    EVR_LAUNCH_CHECK();
    int ga = (nvec + CH_THREADS * CH_UNROLL * 2 - 1) / (CH_THREADS * CH_UNROLL * 2);        // two trips of CH_UNROLL 16-B pieces per lane
    ga = ga < 1 ? 1 : ga;
    hipLaunchKernelGGL(color_norm_apply_kernel, dim3(ga, n), dim3(CH_THREADS), 0, stream, bgr_in, bgr_out, nbytes, values256, q_lo,
                       q_hi, (const unsigned*)counts, range);
    EVR_LAUNCH_CHECK();
    return EVR_OK;
}
