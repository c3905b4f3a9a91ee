// resample.hpp -- the bilinear filter of include/jpeg_amd.h ("resized decode"), stated once for the kernels that apply it:
// k_resize_bilinear (kernels_resize.hip, bytes out) and k_resize_tensor (kernels_tensor.hip, normalised elements out).  Both
// walk the output in the same tiles with the same roles, so the tile is here too.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.
#pragma once
#pragma clang fp contract(off)

#include "fused_common.hpp"

namespace jpeg_amd {

constexpr int kTileW = 64, kTileH = 32;    // output pixels per tile
constexpr int kRun = 4;                    // output pixels per work-item and row
constexpr int kLanesX = kTileW / kRun;     // work-items across a tile
constexpr int kRowStep = kThreads / kLanesX;
static_assert(kTileW + kTileH <= kThreads && kTileH % kRowStep == 0 && kThreads % kLanesX == 0, "roles");

// One axis of the contract: output index j of an axis of n source samples, k = (float)n / (float)n_out.
__device__ __forceinline__ void axis_tap(int j, float k, int n, int &i0, int &i1, float &f)
{
    float s = ((float)j + 0.5f) * k - 0.5f;
    s = fmaxf(s, 0.0f);
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    f = s - (float)i0;
}

// One channel: the horizontal pass on both rows, the vertical pass, the clamping byte conversion.
__device__ __forceinline__ uint32_t resample(float a, float b, float c, float d, float fx, float fy)
{
    const float top = a + fx * (b - a);
    const float bot = c + fx * (d - c);
    const float v = top + fy * (bot - top);
    return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f);
}

}  // namespace jpeg_amd
