// interleave.hpp -- Planar.interleaved(cosite:) (decode.swift:4182-4276) and the built-in colour formats (jpeg.swift:343-354,
// 441-478), written down literally and ONCE: the per-axis index map, its neighbour clamp and fraction, the two-step
// bilinear sum, YCbCr.rgb, RGB.ycc and the clamping byte conversion.  Host (capi.hip, the launchers) and device (the
// staged and the region kernels) use the same text; the tuned kernels (kernels_quad / _fused / _encode / _generic)
// specialise these formulas in forms proven equal to them.
//
// Compile with -ffp-contract=off (see dct.hpp); the pragma is the second line of defence.
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpeg_amd.h"
#include "dct.hpp"

namespace jpeg_amd {

// A direct plane is copied, cropped to the image, sample t for pixel t: a single-plane image, or factor == scale on both
// axes (decode.swift:4185-4215).
__host__ __device__ inline bool plane_is_direct(const jpeg_amd_layout &L, int p)
{
    return L.nplanes == 1 || (L.factor_x[p] == L.scale_x && L.factor_y[p] == L.scale_y);
}

// One axis of one plane.  Pixel t reads sample i = (a + b t) / c (truncating, like quotientAndRemainder and C's /,
// decode.swift:4240-4241) and its neighbour min(i + 1, last) with last = 8 units - 1, the PADDED plane's edge
// (:4245-4246), weighted by the fraction clamp(Float(a + b t - i c) / Float(c)) (:4250-4251), where (a, b, c) =
// (0, f, s) cosited and (f - s, 2 f, 2 s) centred, f the plane's factor and s the image's scale on the axis
// (:4223-4234); a direct plane reads sample t alone.
struct InterleaveAxis {
    int32_t a, b, c, last, direct;
};

__host__ __device__ inline InterleaveAxis interleave_axis(const jpeg_amd_layout &L, int p, bool cosited, bool vertical)
{
    const int32_t f = vertical ? L.factor_y[p] : L.factor_x[p];
    const int32_t s = vertical ? L.scale_y : L.scale_x;
    const int32_t u = vertical ? L.units_y[p] : L.units_x[p];
    InterleaveAxis m;
    m.direct = plane_is_direct(L, p);
    m.last = 8 * u - 1;
    if (cosited) { m.a = 0; m.b = f; m.c = s; }          // decode.swift:4223-4234
    else { m.a = f - s; m.b = 2 * f; m.c = 2 * s; }
    return m;
}

// What pixel t reads along the axis: sample i, neighbour j, and the neighbour's weight.
struct AxisTap {
    int32_t i, j;
    float t;
};

// The map of a plane that is NOT direct.  I is the integer a + b t is formed in: int64_t is exact for every layout
// (b t can pass 2^31 on wide images); int32_t is the same number while b t < 2^31 -- with JPEG's factors (b <= 8) for
// every t < 2^28 -- and spares a kernel that maps every pixel two 64-bit divisions per plane.  The remainder keeps the
// numerator's sign (pixel 0 of a centred axis: a < 0), hence the clamp; the fraction is a true division.
template <typename I = int64_t>
__host__ __device__ inline AxisTap interpolated_tap(const InterleaveAxis &m, int32_t t)
{
    const I n = (I)m.a + (I)m.b * t;
    const int32_t i = (int32_t)(n / m.c), f = (int32_t)(n - (I)i * m.c);
    return {i, i + 1 < m.last ? i + 1 : m.last, fmaxf(0.0f, fminf((float)f / (float)m.c, 1.0f))};
}

__host__ __device__ inline AxisTap axis_tap(const InterleaveAxis &m, int32_t t)
{
    return m.direct ? AxisTap{t, t, 0.0f} : interpolated_tap(m, t);
}

__host__ __device__ inline int32_t axis_index(const InterleaveAxis &m, int32_t t) { return axis_tap(m, t).i; }
__host__ __device__ inline int32_t axis_neighbour(const InterleaveAxis &m, int32_t t) { return axis_tap(m, t).j; }
__host__ __device__ inline float axis_fraction(const InterleaveAxis &m, int32_t t) { return axis_tap(m, t).t; }

// Samples [lo, hi] that pixels t0 .. t1 (inclusive) read: both maps are non-decreasing in t (truncation is monotone).
__host__ __device__ inline void axis_span(const InterleaveAxis &m, int32_t t0, int32_t t1, int32_t &lo, int32_t &hi)
{
    lo = axis_index(m, t0);
    hi = axis_neighbour(m, t1);
}

// ---- device only: the per-pixel arithmetic ----------------------------------------------------------------------------
// One upsampled sample (decode.swift:4250-4264): u00 .. u11 the four neighbours, tx / ty the clamped fractions.
__device__ __forceinline__ uint32_t bilinear_sample(float u00, float u01, float u10, float u11, float tx, float ty)
{
    const float v0 = u00 * (1.0f - tx) + u01 * tx;                   // :4260-4261
    const float v1 = u10 * (1.0f - tx) + u11 * tx;
    return (uint32_t)round_half_away(v0 * (1.0f - ty) + v1 * ty);   // :4264  Float.rounded(), exactly
}

// colour math  jpeg.swift:441-453 (YCbCr.rgb), :463-478 (RGB.ycc), :343-354 (the clamping, truncating UInt8 conversion)
__device__ __forceinline__ uint32_t clamp_u8(float v)
{
    return (uint32_t)__builtin_amdgcn_fmed3f(v, 0.0f, 255.0f);
}

// x = (Float(y) + m_cb * (Float(cb) - 128)) + m_cr * (Float(cr) - 128); the two `0.0 * c`
// products only add a signed zero, which cannot change any sum here.
__device__ __forceinline__ void ycc_to_rgb(float y, float cb, float cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const float pb = cb - 128.0f;
    const float pr = cr - 128.0f;
    r = clamp_u8(y + 1.40200f * pr);
    g = clamp_u8((y + -0.34414f * pb) + -0.71414f * pr);
    b = clamp_u8(y + 1.77200f * pb);
}

// x = ((m0 + m_r * r) + m_g * g) + m_b * b; for Y m0 = 0 and `0 + x` is exact.
__device__ __forceinline__ uint32_t rgb_to_ycc_component(int p, float r, float g, float b)
{
    if (p == 0) return clamp_u8((0.2990f * r + 0.5870f * g) + 0.1140f * b);
    if (p == 1) return clamp_u8(((128.0f + -0.1687f * r) + -0.3313f * g) + 0.5000f * b);
    return clamp_u8(((128.0f + 0.5000f * r) + -0.4187f * g) + -0.0813f * b);
}

}  // namespace jpeg_amd
