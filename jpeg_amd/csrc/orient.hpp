// orient.hpp -- the eight EXIF orientations, stated once (include/jpeg_amd.h, "oriented resample"): plain C++ with no HIP
// in it, for the host route (capi_view.hip, capi_files.hip, entropy.cpp), the kernels' records (resample.hpp, antialias.hpp)
// and tests/cpp/orient_sanitize.cpp, which g++ compiles.  Every function is constexpr, so hipcc takes it on either side.
//
// An orientation o in 1 .. 8 is three bits (T, fx, fy):
//     o          1      2      3      4      5      6      7      8
//     T fx fy    0 0 0  0 1 0  0 1 1  0 0 1  1 0 0  1 0 1  1 1 1  1 1 0
// For a stored image S of w x h the oriented image D is w' x h' = (T ? h : w) x (T ? w : h), and D[y'][x'] = S[ys][xs] with
//     without T:  xs = fx ? w - 1 - x' : x',  ys = fy ? h - 1 - y' : y'
//     with T:     xs = fx ? w - 1 - y' : y',  ys = fy ? h - 1 - x' : x'
// (in numpy: S[::-1] if fy, then [:, ::-1] if fx, then .transpose(1, 0, 2) if T; PIL.ImageOps.exif_transpose gives the same
// for all eight).  As a byte address, channel c of D[y'][x'] is at base + x' step_x + y' step_y + c, the steps signed.
#pragma once

#include <cstdint>

namespace jpeg_amd {

struct Orientation { bool T, fx, fy; };

constexpr bool orientation_valid(int o) { return o >= 1 && o <= 8; }

// o in 1 .. 8.
constexpr Orientation orientation_bits(int o)
{
    return Orientation{o >= 5, o == 2 || o == 3 || o == 7 || o == 8, o == 3 || o == 4 || o == 6 || o == 7};
}

// The oriented image as a source of bytes: its extent, its first byte from the launch's source, and the bytes from a pixel to
// its right-hand and its lower neighbour.
struct OrientedSource {
    uint64_t base;
    int32_t  w, h;             // w', h'
    int64_t  step_x, step_y;
};

// The stored image of w x h pixels (rows of 3 w bytes) at `offset`, in orientation o (1 .. 8).
constexpr OrientedSource oriented_source(int o, uint64_t offset, int32_t w, int32_t h)
{
    const Orientation b = orientation_bits(o);
    const int64_t px = b.fx ? -3 : 3, row = (b.fy ? -3 : 3) * (int64_t)w;
    return OrientedSource{offset + 3u * ((uint64_t)(b.fy ? h - 1 : 0) * (uint64_t)w + (uint64_t)(b.fx ? w - 1 : 0)),
                          b.T ? h : w, b.T ? w : h, b.T ? row : px, b.T ? px : row};
}

// A rectangle of the oriented image (inside w' x h') as the rectangle of the stored image of w x h that holds its pixels.
struct OrientRect { int32_t x, y, width, height; };
constexpr OrientRect oriented_rect_to_stored(int o, int32_t w, int32_t h, OrientRect r)
{
    const Orientation b = orientation_bits(o);
    const OrientRect a = b.T ? OrientRect{r.y, r.x, r.height, r.width} : r;
    return OrientRect{b.fx ? w - a.x - a.width : a.x, b.fy ? h - a.y - a.height : a.y, a.width, a.height};
}

}  // namespace jpeg_amd
