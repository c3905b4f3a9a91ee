// region.hpp -- the sample window of a pixel region (jpeg_amd_region_window, k_region_decode): which samples of a plane
// Planar.interleaved(cosite:) reads for the pixels of a rectangle (decode.swift:4182-4276).  Shared by the host (capi.hip)
// and the kernel (kernels_region.hip), so both draw the halo the same way.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpeg_amd.h"
#include "dct.hpp"

namespace jpeg_amd {

// One axis of one plane.  Pixel t reads sample i = (a + b t) / c (truncating, like quotientAndRemainder) and its neighbour
// min(i + 1, last) with last = 8 units - 1, the PADDED plane's edge; a direct plane (single-plane image, or factor == scale
// on both axes: the crop copy of decode.swift:4185-4215) reads sample t alone.  64-bit: b t can pass 2^31 on wide images.
struct RegionAxis {
    int32_t a, b, c, last, direct;
};

__host__ __device__ inline RegionAxis region_axis(const jpeg_amd_layout &L, int p, bool cosited, bool vertical)
{
    const int32_t f = vertical ? L.factor_y[p] : L.factor_x[p];
    const int32_t s = vertical ? L.scale_y : L.scale_x;
    const int32_t u = vertical ? L.units_y[p] : L.units_x[p];
    RegionAxis m;
    m.direct = L.nplanes == 1 || (L.factor_x[p] == L.scale_x && L.factor_y[p] == L.scale_y);
    m.last = 8 * u - 1;
    if (cosited) { m.a = 0; m.b = f; m.c = s; }          // decode.swift:4223-4234
    else { m.a = f - s; m.b = 2 * f; m.c = 2 * s; }
    return m;
}

__host__ __device__ inline int32_t axis_index(const RegionAxis &m, int32_t t)
{
    return m.direct ? t : (int32_t)(((int64_t)m.a + (int64_t)m.b * t) / m.c);
}

__host__ __device__ inline int32_t axis_neighbour(const RegionAxis &m, int32_t t)
{
    if (m.direct) return t;
    const int32_t i = axis_index(m, t);
    return i + 1 < m.last ? i + 1 : m.last;
}

// Samples [lo, hi] that pixels t0 .. t1 (inclusive) read: both maps are non-decreasing in t (truncation is monotone).
__host__ __device__ inline void axis_span(const RegionAxis &m, int32_t t0, int32_t t1, int32_t &lo, int32_t &hi)
{
    lo = axis_index(m, t0);
    hi = axis_neighbour(m, t1);
}

// ---- the per-pixel arithmetic of k_region_decode, the reference's literal expressions (no rounding shortcut) ----------
// One upsampled sample (decode.swift:4250-4264): u00 .. u11 the four neighbours, t = the clamped fractions.
__device__ __forceinline__ uint32_t bilinear_literal(float u00, float u01, float u10, float u11, float tx, float ty)
{
    const float v0 = u00 * (1.0f - tx) + u01 * tx;
    const float v1 = u10 * (1.0f - tx) + u11 * tx;
    return (uint32_t)round_half_away(v0 * (1.0f - ty) + v1 * ty);   // Float.rounded(), exactly
}

// YCbCr.rgb (jpeg.swift:441-453) + the truncating UInt8 conversion (:343-354): x = (y + m_cb (cb - 128)) + m_cr (cr - 128);
// the two `0.0 * c` products only add a signed zero, which cannot change any sum here.
__device__ __forceinline__ uint32_t clamp_byte(float v) { return (uint32_t)__builtin_amdgcn_fmed3f(v, 0.0f, 255.0f); }
__device__ __forceinline__ void ycc_to_rgb_literal(uint32_t y, uint32_t cb, uint32_t cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const float fy = (float)y, pb = (float)cb - 128.0f, pr = (float)cr - 128.0f;
    r = clamp_byte(fy + 1.40200f * pr);
    g = clamp_byte((fy + -0.34414f * pb) + -0.71414f * pr);
    b = clamp_byte(fy + 1.77200f * pb);
}

}  // namespace jpeg_amd
