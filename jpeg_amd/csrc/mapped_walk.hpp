// mapped_walk.hpp -- the walk of the mapped kernels of kernels_resample.hip (include/jpeg_amd.h, "warped resample", "projective
// resample", "bicubic warp"): a MAP takes the centre of every output pixel to a point of the source, and TAPS around that point
// make the pixel.  A rotation is not separable, so there are no per-column and per-row tables: every work-item computes the
// coordinates of each of its pixels, in the contract's order of operations.
//
// mapped_walk runs on resample_walk's grid -- (tiles of 64 x 32 output pixels) x (images), 256 work-items, each with runs of
// kRun = 4 pixels of one row, 16 rows per trip, 2 trips -- and hands every run to the same sinks.  Per run the map's products
// with xc are kept across the rows, per row its products with yc across the run: single operations of the contract, in its
// order, computed once.  The maps are AffineMap ("warped resample") and ProjectiveMap ("projective resample"); the taps are
// TwoTaps (the filter of "resized decode") and CubicTaps ("bicubic warp").  AffineMap with CubicTaps has no kernel: the host
// sends the six numbers of an affine map as a homography.
//
// Reads stay inside the image's w x h x 3 bytes: every tap index is clamped into the image in front of its load, or the load
// goes through a resource over exactly those bytes (CubicTaps).  Under JPEG_AMD_EDGE_REPLICATE the clamped tap IS the tap;
// under JPEG_AMD_EDGE_FILL the value of a tap whose index was outside is replaced by the fill behind the load, and a pixel that
// the taps call outside loads nothing at all, so a tile that misses the source reads no byte of it.  The edge mode is the same
// in every record of a launch: one uniform branch per workgroup.  Pixels of a run past out_w and rows past out_h compute
// nothing and reach no sink.  No LDS: nothing is shared between work-items, and the bicubic launch measured within 1.5 x of
// the two-tap one, so the tile's footprint is not staged.
//
// The kernels are to stay the instructions they are (tools/isa_digest.py --kernels): each map keeps its statements in its own
// order, which the schedule follows.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.
#pragma once
#pragma clang fp contract(off)

#include "antialias.hpp"
#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

// ---- the maps: the source coordinate of an output pixel, through "- 0.5f" and the clamp into lo .. xhi, lo .. yhi ----

struct AffineMap {
    typedef WarpRecord Record;
    struct Row { float bx, by; };   // m01 * yc, m11 * yc
    float ax[kRun], ay[kRun];       // m00 * xc, m10 * xc

    __device__ __forceinline__ void run(const Record &r, int k, float xc)
    {
        ax[k] = r.m[0] * xc;
        ay[k] = r.m[3] * xc;
    }
    static __device__ __forceinline__ Row row(const Record &r, float yc) { return {r.m[1] * yc, r.m[4] * yc}; }
    __device__ __forceinline__ void pixel(const Record &r, const Row &b, int k, float lo, float xhi, float yhi, float &sx, float &sy) const
    {
        sx = (ax[k] + b.bx) + r.m[2];
        sx = sx - 0.5f;
        sx = fminf(fmaxf(sx, lo), xhi);
        sy = (ay[k] + b.by) + r.m[5];
        sy = sy - 0.5f;
        sy = fminf(fmaxf(sy, lo), yhi);
    }
};

// Two numerators and a denominator, each an affine form of the pixel centre, and ONE division per pixel.  The division is the
// correctly rounded one, written 1.0f / nw: the compiler's div_scale / rcp / fma / div_fmas / div_fixup sequence, about eleven
// instructions of which the reciprocal is quarter rate.  No fast reciprocal stands in for it -- the host's conditioning check
// keeps nw positive and normal, so the sequence's scaling paths are never taken, and they cost nothing but their instructions.
struct ProjectiveMap {
    typedef ProjectRecord Record;
    struct Row { float bx, by, bw; };     // m01 * yc, m11 * yc, m21 * yc
    float ax[kRun], ay[kRun], aw[kRun];   // m00 * xc, m10 * xc, m20 * xc

    __device__ __forceinline__ void run(const Record &r, int k, float xc)
    {
        ax[k] = r.m[0] * xc;
        ay[k] = r.m[3] * xc;
        aw[k] = r.m[6] * xc;
    }
    static __device__ __forceinline__ Row row(const Record &r, float yc) { return {r.m[1] * yc, r.m[4] * yc, r.m[7] * yc}; }
    __device__ __forceinline__ void pixel(const Record &r, const Row &b, int k, float lo, float xhi, float yhi, float &sx, float &sy) const
    {
        const float nx = (ax[k] + b.bx) + r.m[2];
        const float ny = (ay[k] + b.by) + r.m[5];
        const float nw = (aw[k] + b.bw) + r.m[8];
        const float rw = 1.0f / nw;
        sx = nx * rw;
        sx = sx - 0.5f;
        sx = fminf(fmaxf(sx, lo), xhi);
        sy = ny * rw;
        sy = sy - 0.5f;
        sy = fminf(fmaxf(sy, lo), yhi);
    }
};

// ---- the taps: the rows of mapped_walk in one edge mode, with what follows the clamp for one pixel ----
//
// rows(): x is the first stored column of the run, npix > 0 its pixels inside the output.  The row loop and the pixel's text
// stand in each policy's rows(), not in a function that both call: handed to a helper (a function per pixel, or a lambda per
// row), every kernel compiled to other instructions, and the two row loops ask the unroller for different things.

// The two-tap filter of "resized decode" (resample(), resample.hpp) at a coordinate clamped into -1 .. w, -1 .. h.  Under
// JPEG_AMD_EDGE_FILL a pixel none of whose taps lies inside loads nothing and is the fill.
struct TwoTaps {
    template <typename Map, bool Replicate, typename Sink>
    static __device__ __forceinline__ void rows(const ResampleArgs &a, const typename Map::Record &r, bool flip, int py0, int ly, int x, int npix,
                                                uint32_t fill, Sink sink)
    {
        const float fw = (float)r.w, fh = (float)r.h;
        Map map;
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const int xs = flip ? a.out_w - 1 - (x + k) : x + k;   // (k >= npix: not used)
            map.run(r, k, (float)xs + 0.5f);
        }
        const float fill_f[3] = {(float)(fill & 0xffu), (float)((fill >> 8) & 0xffu), (float)((fill >> 16) & 0xffu)};
        const uint8_t *src = a.src + r.offset;
        const size_t row_bytes = (size_t)3 * (uint32_t)r.w;
#pragma unroll
        for (int u = ly; u < kTileH; u += kRowStep) {
            const int y = py0 + u;
            if (y >= a.out_h) break;
            const typename Map::Row b = Map::row(r, (float)y + 0.5f);
            uint32_t o[kRun][3];
#pragma unroll
            for (int k = 0; k < kRun; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = 0u;
                if (k >= npix) continue;
                float sx, sy;
                map.pixel(r, b, k, -1.0f, fw, fh, sx, sy);
                const float fx0 = floorf(sx), fy0 = floorf(sy);
                const int x0 = (int)fx0, y0 = (int)fy0;   // -1 .. w, -1 .. h
                const float fx = sx - fx0, fy = sy - fy0;
                // the taps' indices inside the image, and whether they were
                const int cx0 = min(max(x0, 0), r.w - 1), cx1 = min(x0 + 1, r.w - 1);
                const int cy0 = min(max(y0, 0), r.h - 1), cy1 = min(y0 + 1, r.h - 1);
                const bool in_x0 = cx0 == x0, in_x1 = cx1 == x0 + 1, in_y0 = cy0 == y0, in_y1 = cy1 == y0 + 1;
                if constexpr (!Replicate) {
                    if (!((in_x0 || in_x1) && (in_y0 || in_y1))) {   // no tap inside: a = b = c = d = fill gives the fill exactly
#pragma unroll
                        for (int c = 0; c < 3; ++c) o[k][c] = (fill >> (8 * c)) & 0xffu;
                        continue;
                    }
                }
                const uint8_t *r0 = src + (size_t)(uint32_t)cy0 * row_bytes, *r1 = src + (size_t)(uint32_t)cy1 * row_bytes;
                const size_t o0 = (size_t)3 * (uint32_t)cx0, o1 = (size_t)3 * (uint32_t)cx1;
                const uint8_t *pa = r0 + o0, *pb = r0 + o1, *pc = r1 + o0, *pd = r1 + o1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ta = (float)pa[c], tb = (float)pb[c], tc = (float)pc[c], td = (float)pd[c];
                    if constexpr (!Replicate) {
                        ta = in_y0 && in_x0 ? ta : fill_f[c];
                        tb = in_y0 && in_x1 ? tb : fill_f[c];
                        tc = in_y1 && in_x0 ? tc : fill_f[c];
                        td = in_y1 && in_x1 ? td : fill_f[c];
                    }
                    o[k][c] = resample(ta, tb, tc, td, fx, fy);
                }
            }
            sink(o, y, x, npix);
        }
    }
};

typedef uint32_t cubic_u32x3_t __attribute__((ext_vector_type(3)));

// Byte b (0 .. 11) of the three dwords of a row segment as binary32: v_cvt_f32_ubyte0 .. 3.
__device__ __forceinline__ float cubic_byte(const uint32_t (&d)[3], int b) { return (float)((d[b >> 2] >> (8 * (b & 3))) & 0xffu); }

// 4 x 4 fixed taps of the Keys cubic with a = -0.5 -- BicubicFilter::weight (antialias.hpp), the polynomial of "bicubic
// resample" -- not widened by the scale and not renormalised, at a coordinate clamped into -2 .. w + 1, -2 .. h + 1.  Per
// pixel: the eight weights, and four ROWS of taps -- row j's 4 taps x 3 channels are 12 bytes in three dwords, twelve
// conversions, nine products and nine sums per channel triple, and one product and sum into the pixel's three accumulators,
// ascending: the contract's order.
//
// THE FETCH.  Sixteen taps through byte loads are 48 loads per pixel, on the path that bounds the bilinear kernel already
// (DESIGN.md 8q).  The four taps of a row whose columns x0 - 1 .. x0 + 2 all lie inside the image are 12 CONTIGUOUS bytes: one
// buffer_load_dwordx3 through a resource over the image's w x h x 3 bytes (make_srd's words; such loads may start at any byte
// address, profiles/r05_probe_buffer.txt) -- four loads per pixel.  A pixel goes this way when
//   - the image is below 4 GiB (a resource's offsets and its num_records are 32 bits),
//   - none of its four columns and four rows is clamped or outside, and
//   - its last segment ends at least 4 bytes in front of the image's end: the range check is per dword and a dword that
//     straddles the end arrives as 0; with this margin no dword of a segment, wherever the hardware cuts it,
//     reaches the last byte, at the price of the per-tap way for a few pixels of the last row.
// Every other pixel takes the per-tap way: 16 taps whose indices are clamped into the image in front of their three byte
// loads, packed into the same three dwords per row, under JPEG_AMD_EDGE_FILL the bytes of the fill where the index was outside
// ((float) of a fill byte is the contract's (float)fill[c]).  The split is per pixel; the arithmetic behind it exists once.
// Under JPEG_AMD_EDGE_FILL a pixel whose coordinate the clamp has bound on either axis loads nothing and is the fill ("bicubic
// warp", far outside under FILL).  The two trips of the row loop are not unrolled: the per-tap way is long, and it is there
// twice (the edge modes) as it is.
struct CubicTaps {
    template <typename Map, bool Replicate, typename Sink>
    static __device__ __forceinline__ void rows(const ResampleArgs &a, const typename Map::Record &r, bool flip, int py0, int ly, int x, int npix,
                                                uint32_t fill, Sink sink)
    {
        const float fw1 = (float)r.w + 1.0f, fh1 = (float)r.h + 1.0f;   // (exact: w, h <= 2^24)
        Map map;
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const int xs = flip ? a.out_w - 1 - (x + k) : x + k;   // (k >= npix: not used)
            map.run(r, k, (float)xs + 0.5f);
        }
        const uint8_t *src = a.src + r.offset;
        const size_t row_bytes = (size_t)3 * (uint32_t)r.w;
        const uint64_t image_bytes = (uint64_t)row_bytes * (uint32_t)r.h;
        const bool small = image_bytes < 0x100000000ull;   // uniform: the wide way exists for this image
        const uint32_t bytes32 = small ? (uint32_t)image_bytes : 0u;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(src), 0, (int)bytes32, 0x00020000);
#pragma unroll 1
        for (int u = ly; u < kTileH; u += kRowStep) {
            const int y = py0 + u;
            if (y >= a.out_h) break;
            const typename Map::Row b = Map::row(r, (float)y + 0.5f);
            uint32_t o[kRun][3];
#pragma unroll
            for (int k = 0; k < kRun; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = 0u;
                if (k >= npix) continue;
                float sx, sy;
                map.pixel(r, b, k, -2.0f, fw1, fh1, sx, sy);
                const float fx0 = floorf(sx), fy0 = floorf(sy);
                const int x0 = (int)fx0, y0 = (int)fy0;   // -2 .. w + 1, -2 .. h + 1
                const float fx = sx - fx0, fy = sy - fy0;
                const int xa = x0 - 1, ya = y0 - 1;       // the first column and row of the taps
                if constexpr (!Replicate) {
                    // At a bound of the clamp the fraction is 0 and the weights are exactly 0, 1, 0, 0: the one tap that counts is
                    // column -2 or w + 1 (row -2 or h + 1), outside, and every row sum is the fill -- "far outside under FILL".
                    if (sx <= -2.0f || sx >= fw1 || sy <= -2.0f || sy >= fh1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) o[k][c] = (fill >> (8 * c)) & 0xffu;
                        continue;
                    }
                }
                const float wx[4] = {BicubicFilter::weight(fx + 1.0f), BicubicFilter::weight(fx), BicubicFilter::weight(1.0f - fx),
                                     BicubicFilter::weight(2.0f - fx)};
                const float wy[4] = {BicubicFilter::weight(fy + 1.0f), BicubicFilter::weight(fy), BicubicFilter::weight(1.0f - fy),
                                     BicubicFilter::weight(2.0f - fy)};
                uint32_t d[4][3];   // row j's taps: byte 3 i + c is channel c of column xa + i
                // (inside: xa >= 0, xa + 3 <= w - 1, likewise the rows; first < 2^32 - 16 follows from small and the rows below it)
                const uint32_t first = ((uint32_t)ya * (uint32_t)r.w + (uint32_t)xa) * 3u;
                const bool inside = xa >= 0 && xa + 3 <= r.w - 1 && ya >= 0 && ya + 3 <= r.h - 1;
                if (small && inside && (uint64_t)first + 3u * (uint64_t)row_bytes + 16u <= image_bytes) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const cubic_u32x3_t v = __builtin_amdgcn_raw_buffer_load_b96(rsrc, first + (uint32_t)j * (uint32_t)row_bytes, 0, 0);
                        d[j][0] = v.x; d[j][1] = v.y; d[j][2] = v.z;
                    }
                } else {
                    size_t ox[4];
                    bool in_x[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int cx = min(max(xa + i, 0), r.w - 1);
                        in_x[i] = cx == xa + i;
                        ox[i] = (size_t)3 * (uint32_t)cx;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cy = min(max(ya + j, 0), r.h - 1);
                        const bool in_y = cy == ya + j;
                        const uint8_t *row = src + (size_t)(uint32_t)cy * row_bytes;
                        d[j][0] = d[j][1] = d[j][2] = 0u;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const uint8_t *p = row + ox[i];
                            uint32_t t = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
                            if constexpr (!Replicate) t = in_y && in_x[i] ? t : fill;
#pragma unroll
                            for (int c = 0; c < 3; ++c) d[j][(3 * i + c) >> 2] |= ((t >> (8 * c)) & 0xffu) << (8 * ((3 * i + c) & 3));
                        }
                    }
                }
                float v[3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float rj = wx[0] * cubic_byte(d[j], c);
                        rj = rj + wx[1] * cubic_byte(d[j], 3 + c);
                        rj = rj + wx[2] * cubic_byte(d[j], 6 + c);
                        rj = rj + wx[3] * cubic_byte(d[j], 9 + c);
                        const float p = wy[j] * rj;
                        v[c] = j == 0 ? p : v[c] + p;
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = (uint32_t)(int)(fminf(fmaxf(v[c], 0.0f), 255.0f) + 0.5f);
            }
            sink(o, y, x, npix);
        }
    }
};

// ---- the walk ----

// The tile blockIdx.x of image blockIdx.y: sink(o, y, x, npix) for every run of the tile, as resample_walk's.  flips: the
// image's Record::flip counts (the tensor kernels); fill: the launch's, channel c in bits 8 c ...
template <typename Map, typename Taps, typename Sink>
__device__ __forceinline__ void mapped_walk(const ResampleArgs &a, const typename Map::Record *records, bool flips, uint32_t fill, Sink sink)
{
    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const typename Map::Record r = records[blockIdx.y];
    const bool flip = flips && r.flip;
    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
    if (r.edge == JPEG_AMD_EDGE_REPLICATE)
        Taps::template rows<Map, true>(a, r, flip, py0, ly, x, npix, fill, sink);
    else
        Taps::template rows<Map, false>(a, r, flip, py0, ly, x, npix, fill, sink);
}

}  // namespace jpeg_amd
