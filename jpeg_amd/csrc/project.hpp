// project.hpp -- the walk of the project kernels of kernels_resample.hip (include/jpeg_amd.h, "projective resample"): a 3 x 3
// homography takes the centre of every output pixel to a point of the source -- two numerators and a denominator, each an
// affine form of the pixel centre, and ONE division per pixel -- and from the clamped coordinate on everything is warp.hpp's:
// the two-tap filter of "resized decode" (resample(), resample.hpp), the fill or the replicated edge.
//
// project_walk runs on warp_walk's grid -- (tiles of 64 x 32 output pixels) x (images), 256 work-items, each with runs of
// kRun = 4 pixels of one row, 16 rows per trip, 2 trips -- and hands every run to the same sinks.  Per run the products
// m00 * xc, m10 * xc and m20 * xc are kept across the rows, per row m01 * yc, m11 * yc and m21 * yc across the run: single
// operations of the contract, in its order, computed once.  Per pixel: the six adds, the division, the two products, the
// clamp and the taps.  The division is the correctly rounded one, written 1.0f / nw: the compiler's div_scale / rcp / fma /
// div_fmas / div_fixup sequence, about eleven instructions of which the reciprocal is quarter rate.  No fast reciprocal
// stands in for it -- the host's conditioning check keeps nw positive and normal, so the sequence's scaling paths are never
// taken, and they cost nothing but their instructions.
//
// The tap part repeats warp_rows' text (as colour_sink repeats tensor_sink's): shared, the warp kernels would have to compile
// to the instructions they have, which nothing promises.  A change to the taps is made in both places.
//
// Reads stay inside the image's w x h x 3 bytes: every tap index is clamped into the image in front of its load.  Under
// JPEG_AMD_EDGE_REPLICATE the clamped tap IS the tap; under JPEG_AMD_EDGE_FILL the value of a tap whose index was outside is
// replaced by the fill behind the load, and a pixel none of whose taps lies inside loads nothing at all.  The edge mode is the
// same in every record of a launch: one uniform branch per workgroup.  Pixels of a run past out_w and rows past out_h compute
// nothing and reach no sink.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.
#pragma once
#pragma clang fp contract(off)

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

// The rows of project_walk in one edge mode.  x: the first stored column of the run, npix > 0 its pixels inside the output.
template <bool Replicate, typename Sink>
__device__ __forceinline__ void project_rows(const ResampleArgs &a, const ProjectRecord &r, bool flip, int py0, int ly, int x, int npix,
                                             uint32_t fill, Sink sink)
{
    const float fw = (float)r.w, fh = (float)r.h;
    float ax[kRun], ay[kRun], aw[kRun];   // m00 * xc, m10 * xc, m20 * xc
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        const int xs = flip ? a.out_w - 1 - (x + k) : x + k;   // (k >= npix: not used)
        const float xc = (float)xs + 0.5f;
        ax[k] = r.m[0] * xc;
        ay[k] = r.m[3] * xc;
        aw[k] = r.m[6] * xc;
    }
    const float fill_f[3] = {(float)(fill & 0xffu), (float)((fill >> 8) & 0xffu), (float)((fill >> 16) & 0xffu)};
    const uint8_t *src = a.src + r.offset;
    const size_t row_bytes = (size_t)3 * (uint32_t)r.w;
#pragma unroll
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
            sx = fminf(fmaxf(sx, -1.0f), fw);
            float sy = ny * rw;
            sy = sy - 0.5f;
            sy = fminf(fmaxf(sy, -1.0f), fh);
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

// The tile blockIdx.x of image blockIdx.y: sink(o, y, x, npix) for every run of the tile, as warp_walk's.  flips: the image's
// ProjectRecord::flip counts (the tensor kernels); fill: the launch's, channel c in bits 8 c ...
template <typename Sink>
__device__ __forceinline__ void project_walk(const ResampleArgs &a, const ProjectRecord *records, bool flips, uint32_t fill, Sink sink)
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
        project_rows<true>(a, r, flip, py0, ly, x, npix, fill, sink);
    else
        project_rows<false>(a, r, flip, py0, ly, x, npix, fill, sink);
}

}  // namespace jpeg_amd
