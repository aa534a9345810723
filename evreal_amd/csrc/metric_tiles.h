// The scaffold under the closed-form metrics (metrics.hip, frmetrics.hip, gmsd.hip, vifp.hip).
//
// Device side: 256-thread blocks of four waves.  A tile kernel owns one tile of one frame (blockIdx.x / y the tile, blockIdx.z
// + f0 the frame), keeps Q running fp64 sums per thread and ends in tile_partials: wave sums, one LDS hand-off, the four wave
// totals added left to right, Q doubles at the tile's slot.  A finish kernel (one block per frame) calls frame_total once per
// sum: a thread walks the frame's slots in steps of 256, then the wave sum and the same four-term add (block_total; block_totals
// is the array form that the no-reference kernels of nriqa.hip end in, see nss.h).  No atomics, and the
// number of tiles depends on the shape alone: a frame's numbers are bitwise independent of n, of its place in the batch and of
// earlier calls.  Windowed second moments (frmetrics.hip, vifp.hip): N taps over the VALID region as two separable passes on a
// staged tile of (TH + N - 1) x (TW + N - 1) pixels, rows padded by one; taps added in index order (a = w0 * v0; a += wk * vk),
// products formed as w[k] * (x * x), no contraction into fused multiply-adds (build.py).  metrics.hip keeps loops of its own:
// scipy's symmetric order with fp32 rounding between the passes.
//
// Host side: Plan<L> lays out a call's workspace -- for each level l >= 1 two fp64 planes [n, h, w] (reference, then image) in
// a block aligned to 256 B, then the partials [n, tiles_total, Q].  The caller states every level's size and tile grid: how a
// level follows from the one above is the metric's own rule.  for_frame_chunks walks a batch in chunks of at most MAX_GRID_Z
// frames, the most one grid axis holds.  A metric's taps, per-pixel formula and staging stay in its own file.
#pragma once
#include "common.h"

namespace evr_tiles {

constexpr int NT = 256;              // threads per block: four waves
constexpr int MAX_GRID_Z = 65535;

template <typename T> __device__ __forceinline__ double to_f64(T v) { return (double)v; }

// Every thread brings Q running sums; the block's totals go to the slot of tile (blockIdx.y, blockIdx.x), row-major, counted
// from first(), the slot of the frame's (and level's) first tile: a callable, worked out by the Q storing threads alone.
template <typename First, typename... D>
__device__ __forceinline__ void tile_partials(double (&red)[sizeof...(D)][NT / 64], double* partials, First first, D... sum) {
    constexpr int Q = sizeof...(D);
    const double s[Q] = {evr_wave_sum(sum)...};          // (straight-line: one sum after the other, as written out by hand)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q][wave] = s[q];
    }
    __syncthreads();
    if (tid < Q) {
        const int64_t t = first() + (int64_t)(int)blockIdx.y * gridDim.x + (int)blockIdx.x;
        partials[t * Q + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    }
}

// The array form (nriqa.hip): Q running sums per thread in a[], the block's totals at dst[0 .. Q), in LDS or at a slot in
// memory, written by threads 0 .. Q - 1.
template <int Q>
__device__ __forceinline__ void block_totals(const double (&a)[Q], double (&red)[NT / 64][Q], double* dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const double s = evr_wave_sum(a[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (tid < Q) dst[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// The block's total of one running sum per thread, in every thread of the block.  A second call with the same `red` needs a
// __syncthreads() in between.
__device__ __forceinline__ double block_total(double a, double (&red)[NT / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    a = evr_wave_sum(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// The sum of src[0], src[Q], ... (`tiles` entries), one column of a frame's tile partials, walked in steps of 256.
template <int Q>
__device__ __forceinline__ double frame_total(const double* src, int tiles, double (&red)[NT / 64]) {
    double a = 0.0;
    for (int t = threadIdx.x; t < tiles; t += NT) a += src[(int64_t)t * Q];
    return block_total(a, red);
}

// Pass 1, along axis 0: rows r .. r + N - 1 of the staged planes belong to output row r.
template <int N, int TH, int TW, typename T, int NW>
__device__ __forceinline__ void moments_pass1(const T (&sx)[TH + N - 1][TW + N], const T (&sy)[TH + N - 1][TW + N],
                                              const double (&w)[NW], double (&v)[5][TH][TW + N]) {
    constexpr int IW = TW + N - 1;
    for (int i = threadIdx.x; i < TH * IW; i += NT) {
        const int r = i / IW, c = i % IW;
        double a[5];
        {
            const double x = to_f64(sx[r][c]), y = to_f64(sy[r][c]);
            a[0] = w[0] * x; a[1] = w[0] * y; a[2] = w[0] * (x * x); a[3] = w[0] * (y * y); a[4] = w[0] * (x * y);
        }
#pragma unroll
        for (int k = 1; k < N; ++k) {
            const double x = to_f64(sx[r + k][c]), y = to_f64(sy[r + k][c]);
            a[0] += w[k] * x; a[1] += w[k] * y; a[2] += w[k] * (x * x); a[3] += w[k] * (y * y); a[4] += w[k] * (x * y);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k][r][c] = a[k];
    }
}

// Pass 2, along axis 1, for the output pixel (r, c) of the tile: columns c .. c + N - 1 of v.
template <int N, int TH, int TW, int NW>
__device__ __forceinline__ void moments_pass2(const double (&v)[5][TH][TW + N], const double (&w)[NW], int r, int c, double (&u)[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double a = w[0] * v[k][r][c];
#pragma unroll
        for (int j = 1; j < N; ++j) a += w[j] * v[k][r][c + j];
        u[k] = a;
    }
}

// What a kernel needs of a plan: level l's tiles are tile_off[l] .. tile_off[l] + tiles[l] of a frame's tiles_total.
template <int L>
struct LevelTiles { int tile_off[L], tiles[L], tiles_total; };

template <int L>
struct Plan {
    int levels, h[L], w[L], tx[L], ty[L];
    LevelTiles<L> t;
    size_t level_off[L];             // bytes from the workspace start to level l's reference plane (l >= 1)
    size_t partial_off, bytes;

    // the next level: planes of h x w, a grid of ty x tx tiles
    void add_level(int n, int h_, int w_, int ty_, int tx_) {
        const int l = levels++;
        h[l] = h_; w[l] = w_; ty[l] = ty_; tx[l] = tx_;
        t.tile_off[l] = t.tiles_total; t.tiles[l] = tx_ * ty_;
        t.tiles_total += tx_ * ty_;
        if (l) {
            level_off[l] = partial_off;
            partial_off += evr::align_up((size_t)2 * n * h_ * w_ * sizeof(double), 256);
        }
    }
    void close(int n, int Q) { bytes = partial_off + (size_t)n * t.tiles_total * Q * sizeof(double) + 256; }

    double* partials(void* ws) const { return (double*)((char*)ws + partial_off); }
    // level l >= 1 of the reference (which = 0) or of the image (1)
    double* plane(void* ws, int l, int which, int n) const {
        return (double*)((char*)ws + level_off[l]) + (which ? (size_t)n * h[l] * w[l] : 0);
    }
    // what level l's launch writes: level l + 1, or nulls and zeros where a run of `run_levels` levels ends at l
    struct Next { double *x, *y; int h, w; };
    Next next(void* ws, int l, int run_levels, int n) const {
        if (l + 1 >= run_levels) return Next{nullptr, nullptr, 0, 0};
        return Next{plane(ws, l + 1, 0, n), plane(ws, l + 1, 1, n), h[l + 1], w[l + 1]};
    }
};

// launch(f0, nf) -> status for every chunk of at most MAX_GRID_Z frames; stops at the first failure
template <typename F>
int for_frame_chunks(int n, F&& launch) {
    for (int f0 = 0; f0 < n; f0 += MAX_GRID_Z) {
        const int rc = launch(f0, n - f0 < MAX_GRID_Z ? n - f0 : MAX_GRID_Z);
        if (rc != EVR_OK) return rc;
    }
    return EVR_OK;
}

}  // namespace evr_tiles
