// Probe (not part of the product): does the chip hold a higher clock on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16 for
// the h3 mix (lo.hi + hi.lo + hi.hi into one fp32 accumulator set)?  Four loops, {32x32x16, 16x16x32} x {operands held in registers,
// every operand re-read from LDS with ds_read_b128}, all with the wave tile of conv3x3_wide_kernel: 64 pixels x 128 columns = 128
// accumulator registers, per 32-channel step 24 operand fragments of 1 KiB (8 pixel-side, 16 weight-side) and 48 / 96 MFMAs
// (1536 matrix cycles either way).  Operands are x = uniform [-1, 1), hi = f16(x), lo = f16(x - hi) as the H2 format stores them
// (zeros or small integers raise the clock and hide the effect).  One and two waves per SIMD; all variants interleaved over ROUNDS
// rounds in one process on one device.  Per variant: wall time (events around REPS back-to-back launches), algorithmic TFLOP/s
// (2 * 64 * 128 * 32 per wave and step), shader cycles per step and the in-kernel clock (s_memtime / s_memrealtime at 100 MHz,
// median over blocks), median and min over the rounds.
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_shape_probe.hip -o tools/_bin/mfma_shape_probe && tools/_bin/mfma_shape_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

constexpr int NFRAG = 24;                  // fragments per step: 0-7 pixel side, 8-23 weight side; even = hi, odd = lo of the same values
constexpr int FRAG_H = 64 * 8;             // f16 elements per fragment (64 lanes x 16 B)
constexpr int NBUF = 2;                    // the LDS loops alternate between two operand sets, so no read can be hoisted

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// SHAPE 0: 32x32x16 -- pixel fragment (pb, kh) = 4*pb + 2*kh (+1 lo), weight fragment (cb, kh) = 8 + 4*cb + 2*kh (+1 lo), 2 x 4 blocks
// SHAPE 1: 16x16x32 -- pixel fragment pb = 2*pb (+1 lo), weight fragment cb = 8 + 2*cb (+1 lo), 4 x 8 blocks
template <int SHAPE, int LDS>
__global__ __launch_bounds__(256, 2) void probe(float* out, unsigned long long* stamps, int iters, unsigned seed) {
    __shared__ v8h lds[NBUF * NFRAG * 64];
    const int lane = threadIdx.x & 63;
    unsigned s = seed ^ (threadIdx.x * 2654435761u) ^ (blockIdx.x * 40503u);
    for (int i = threadIdx.x; i < NBUF * (NFRAG / 2) * 64; i += 256) {
        v8h hi, lo;
        for (int j = 0; j < 8; ++j) {
            s = s * 1664525u + 1013904223u;
            const float x = (int)(s >> 8) * (1.0f / 8388608.0f) - 1.0f;
            hi[j] = (_Float16)x; lo[j] = (_Float16)(x - (float)hi[j]);
        }
        const int pair = i >> 6, l = i & 63;
        lds[(2 * pair) * 64 + l] = hi; lds[(2 * pair + 1) * 64 + l] = lo;
    }
    __syncthreads();
    v8h r[NFRAG];
    if (!LDS) for (int f = 0; f < NFRAG; ++f) r[f] = lds[f * 64 + lane];
    v16f a32[2][4] = {}; v4f a16[4][8] = {};
    v8h x[8], w[4];
    const unsigned long long c0 = __builtin_readcyclecounter(), t0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
        const v8h* src = lds + (it & (NBUF - 1)) * NFRAG * 64 + lane;
        const v8h* nxt = lds + ((it + 1) & (NBUF - 1)) * NFRAG * 64 + lane;
        auto frag = [&](const v8h* p, int f) { return LDS ? p[f * 64] : r[f]; };
        // weight fragments of the next column block are requested before the MFMAs of the current one (the LDS loops wait for them
        // behind a block of MFMAs, as the kernel's loop does); the pixel fragments of the next step during the last block
        if (SHAPE == 0) {
            if (it == 0 || !LDS) { for (int f = 0; f < 8; ++f) x[f] = frag(src, f); for (int f = 0; f < 4; ++f) w[f] = frag(src, 8 + f); }
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                v8h wn[4], xn[8];
#pragma unroll
                for (int f = 0; f < 4; ++f) wn[f] = frag(cb < 3 ? src : nxt, 8 + 4 * ((cb + 1) & 3) + f);
                if (cb == 3)
#pragma unroll
                    for (int f = 0; f < 8; ++f) xn[f] = frag(nxt, f);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        a32[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[2 * kh + 1], x[4 * pb + 2 * kh], a32[pb][cb], 0, 0, 0);
                        a32[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[2 * kh], x[4 * pb + 2 * kh + 1], a32[pb][cb], 0, 0, 0);
                        a32[pb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[2 * kh], x[4 * pb + 2 * kh], a32[pb][cb], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = 0; f < 4; ++f) w[f] = wn[f];
                if (cb == 3)
#pragma unroll
                    for (int f = 0; f < 8; ++f) x[f] = xn[f];
            }
        } else {
            if (it == 0 || !LDS) { for (int f = 0; f < 8; ++f) x[f] = frag(src, f); for (int f = 0; f < 2; ++f) w[f] = frag(src, 8 + f); }
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                v8h wn[2], xn[8];
#pragma unroll
                for (int f = 0; f < 2; ++f) wn[f] = frag(cb < 7 ? src : nxt, 8 + 2 * ((cb + 1) & 7) + f);
                if (cb == 7)
#pragma unroll
                    for (int f = 0; f < 8; ++f) xn[f] = frag(nxt, f);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int pb = 0; pb < 4; ++pb) {
                    a16[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[1], x[2 * pb], a16[pb][cb], 0, 0, 0);
                    a16[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[0], x[2 * pb + 1], a16[pb][cb], 0, 0, 0);
                    a16[pb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[0], x[2 * pb], a16[pb][cb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int f = 0; f < 2; ++f) w[f] = wn[f];
                if (cb == 7)
#pragma unroll
                    for (int f = 0; f < 8; ++f) x[f] = xn[f];
            }
        }
    }
    const unsigned long long c1 = __builtin_readcyclecounter(), t1 = __builtin_amdgcn_s_memrealtime();
    float sum = 0.f;
    for (int p = 0; p < 2; ++p) for (int c = 0; c < 4; ++c) for (int j = 0; j < 16; ++j) sum += a32[p][c][j];
    for (int p = 0; p < 4; ++p) for (int c = 0; c < 8; ++c) for (int j = 0; j < 4; ++j) sum += a16[p][c][j];
    out[blockIdx.x * 256 + threadIdx.x] = sum;
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = c1 - c0; stamps[2 * blockIdx.x + 1] = t1 - t0; }
}

struct Sample { double ms, tflops, cyc, ghz; };
typedef void (*kern_t)(float*, unsigned long long*, int, unsigned);

static Sample measure(kern_t k, int waves_per_simd, float* out, unsigned long long* stamps, hipEvent_t e0, hipEvent_t e1) {
    const int blocks = 256 * waves_per_simd, iters = 4000 / waves_per_simd, REPS = 20;      // ~3 ms per launch, ~60 ms per sample
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, stamps, iters, 1u + i);
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < REPS; ++i) hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, stamps, iters, 7u + i);
    CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st(2 * blocks);
    CHECK(hipMemcpy(st.data(), stamps, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> cyc(blocks), ghz(blocks);
    for (int b = 0; b < blocks; ++b) { cyc[b] = (double)st[2 * b] / iters; ghz[b] = (double)st[2 * b] / ((double)st[2 * b + 1] * 10.0); }
    std::sort(cyc.begin(), cyc.end()); std::sort(ghz.begin(), ghz.end());
    const double flops = (double)REPS * blocks * 4 * iters * (2.0 * 64 * 128 * 32);
    return {ms / REPS, flops / (ms * 1e-3) / 1e12, cyc[blocks / 2], ghz[blocks / 2]};
}

int main() {
    constexpr int ROUNDS = 7, NV = 4;
    const char* names[NV] = {"32x32x16 regs", "16x16x32 regs", "32x32x16 lds ", "16x16x32 lds "};
    const kern_t kerns[NV] = {probe<0, 0>, probe<1, 0>, probe<0, 1>, probe<1, 1>};
    float* out; unsigned long long* stamps;
    CHECK(hipMalloc(&out, 512 * 256 * 4)); CHECK(hipMalloc(&stamps, 512 * 2 * 8));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<Sample> res[2][NV];
    for (int r = 0; r < ROUNDS + 1; ++r)              // round 0 warms the chip up and is dropped
        for (int w = 1; w <= 2; ++w)
            for (int v = 0; v < NV; ++v) {
                const Sample s = measure(kerns[v], w, out, stamps, e0, e1);
                if (r) res[w - 1][v].push_back(s);
            }
    printf("h3 mix, wave tile 64 px x 128 columns, 256 CUs, %d interleaved rounds; per launch: median [min .. max]\n", ROUNDS);
    for (int w = 1; w <= 2; ++w)
        for (int v = 0; v < NV; ++v) {
            auto col = [&](double Sample::*m) { std::vector<double> x; for (auto& s : res[w - 1][v]) x.push_back(s.*m); std::sort(x.begin(), x.end()); return x; };
            const auto ms = col(&Sample::ms), tf = col(&Sample::tflops), cy = col(&Sample::cyc), gh = col(&Sample::ghz);
            const int n = (int)ms.size(), h = n / 2;
            printf("%s  %d wave/SIMD  ms %.4f [%.4f .. %.4f]  alg TFLOP/s %.1f [%.1f .. %.1f]  cycles/step %.1f [%.1f .. %.1f]  clock GHz %.3f [%.3f .. %.3f]\n",
                   names[v], w, ms[h], ms[0], ms[n - 1], tf[h], tf[0], tf[n - 1], cy[h], cy[0], cy[n - 1], gh[h], gh[0], gh[n - 1]);
        }
    return 0;
}
