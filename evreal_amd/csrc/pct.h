// numpy's percentile rule (method 'linear') in float32, shared by the percentile normalisations of prepost.hip (float frames)
// and color.hip (uint8 BGR frames).  Both files are built with -ffp-contract=off: every operation below is one IEEE rounding.
#pragma once
#include "common.h"

// numpy: q = q/100 in the array dtype; virtual index (n-1)*q; method 'linear' (_get_indexes/_get_gamma)
__device__ __forceinline__ void pct_rank(int n, float q100, int& prev, int& next, float& gamma) {
    const float q = q100 / 100.0f;
    const float vi = (float)(n - 1) * q;
    prev = (int)floorf(vi); next = prev + 1;
    if (vi >= (float)(n - 1)) { prev = next = n - 1; gamma = vi - (-1.0f); }
    else if (vi < 0.f) { prev = next = 0; gamma = vi - 0.0f; }
    else gamma = vi - (float)prev;
}

// numpy _lerp of the two order statistics a = sorted[prev], b = sorted[next]
__device__ __forceinline__ float pct_lerp(float a, float b, float gamma) {
    const float diff = b - a;
    float r = a + diff * gamma;
    if (gamma >= 0.5f) r = b - diff * (1.0f - gamma);
    return r;
}
