// project_cubic.hpp -- the walk of the bicubic project kernels of kernels_resample.hip (include/jpeg_amd.h, "bicubic warp"): the
// coordinates of "projective resample" up to the clamp (project_rows' text, project.hpp), then 4 x 4 fixed taps of the Keys
// cubic with a = -0.5 -- BicubicFilter::weight (antialias.hpp), the polynomial of "bicubic resample" -- not widened by the
// scale and not renormalised.
//
// project_cubic_walk runs on project_walk's grid -- (tiles of 64 x 32 output pixels) x (images), 256 work-items, each with runs
// of kRun = 4 pixels of one row, 16 rows per trip, 2 trips -- and hands every run to the same sinks.  Per run and per row the
// products of the matrix are kept as there.  Per pixel: the six adds, the division, the clamp, the eight weights, and four
// ROWS of taps -- row j's 4 taps x 3 channels are 12 bytes in three dwords, twelve conversions, nine products and nine sums
// per channel triple, and one product and sum into the pixel's three accumulators, ascending: the contract's order.
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
//
// Reads stay inside the image's w x h x 3 bytes on both ways.  Under JPEG_AMD_EDGE_FILL a pixel whose coordinate the clamp
// has bound on either axis loads nothing and is the fill ("bicubic warp", far outside under FILL).  The edge mode is the same
// in every record of a launch: one uniform branch per workgroup.  Pixels of a run past out_w and rows past out_h compute
// nothing and reach no sink.  No LDS: the launch measured within 1.5 x of the bilinear warp's, so the tile's
// footprint is not staged.  The two trips of the row loop are not unrolled: the per-tap way is long, and it is there twice
// (the edge modes) as it is.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.
#pragma once
#pragma clang fp contract(off)

#include "antialias.hpp"
#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

typedef uint32_t cubic_u32x3_t __attribute__((ext_vector_type(3)));

// Byte b (0 .. 11) of the three dwords of a row segment as binary32: v_cvt_f32_ubyte0 .. 3.
__device__ __forceinline__ float cubic_byte(const uint32_t (&d)[3], int b) { return (float)((d[b >> 2] >> (8 * (b & 3))) & 0xffu); }

// The rows of project_cubic_walk in one edge mode.  x: the first stored column of the run, npix > 0 its pixels inside the output.
template <bool Replicate, typename Sink>
__device__ __forceinline__ void project_cubic_rows(const ResampleArgs &a, const ProjectRecord &r, bool flip, int py0, int ly, int x, int npix,
                                                   uint32_t fill, Sink sink)
{
    const float fw1 = (float)r.w + 1.0f, fh1 = (float)r.h + 1.0f;   // (exact: w, h <= 2^24)
    float ax[kRun], ay[kRun], aw[kRun];   // m00 * xc, m10 * xc, m20 * xc
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        const int xs = flip ? a.out_w - 1 - (x + k) : x + k;   // (k >= npix: not used)
        const float xc = (float)xs + 0.5f;
        ax[k] = r.m[0] * xc;
        ay[k] = r.m[3] * xc;
        aw[k] = r.m[6] * xc;
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
        const float yc = (float)y + 0.5f;
        const float bx = r.m[1] * yc, by = r.m[4] * yc, bw = r.m[7] * yc;
        uint32_t o[kRun][3];
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[k][c] = 0u;
            if (k >= npix) continue;
            const float nx = (ax[k] + bx) + r.m[2];
            const float ny = (ay[k] + by) + r.m[5];
            const float nw = (aw[k] + bw) + r.m[8];
            const float rw = 1.0f / nw;   // correctly rounded: nw is positive and normal (the host's conditioning check)
            float sx = nx * rw;
            sx = sx - 0.5f;
            sx = fminf(fmaxf(sx, -2.0f), fw1);
            float sy = ny * rw;
            sy = sy - 0.5f;
            sy = fminf(fmaxf(sy, -2.0f), fh1);
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

// The tile blockIdx.x of image blockIdx.y: sink(o, y, x, npix) for every run of the tile, as project_walk's.
template <typename Sink>
__device__ __forceinline__ void project_cubic_walk(const ResampleArgs &a, const ProjectRecord *records, bool flips, uint32_t fill, Sink sink)
{
    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const ProjectRecord r = records[blockIdx.y];
    const bool flip = flips && r.flip;
    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
    if (r.edge == JPEG_AMD_EDGE_REPLICATE)
        project_cubic_rows<true>(a, r, flip, py0, ly, x, npix, fill, sink);
    else
        project_cubic_rows<false>(a, r, flip, py0, ly, x, npix, fill, sink);
}

}  // namespace jpeg_amd
