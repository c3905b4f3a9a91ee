// resample.hpp -- the bilinear filter of include/jpeg_amd.h ("resized decode") and the walk that applies it, for the bilinear
// kernels of kernels_resample.hip: the filter, the tile, the head of the kernels' arguments with the host code that fills it,
// and resample_walk, which computes every run of output bytes of a workgroup's tile and hands it to a sink.
// k_resize_oriented_bytes and k_resize_tensor are resample_walk with a sink; k_resize_bilinear keeps a text of its own of the
// same walk (kernels_resample.hip says why), so a change here is made there too.  store_run, the byte store of a run, is here
// for every byte kernel; the tile and the head are antialias.hpp's as well.
//
// resample_walk: a static grid of (tiles of the output) x (images); the output size is the same for every image, so there is
// no prefix and no search.  A tile is 64 x 32 output pixels.  Its workgroup
//   1. writes the tile's per-column (x0, x1, fx) and per-row (y0, y1, fy) into LDS, one work-item per column or row -- they
//      are not computed again per pixel.  The column table is written for the SOURCE column of the stored pixel: the work-item
//      of stored column x computes the taps of xs = flip ? out_w - 1 - x : x, so a flipped image costs nothing per pixel and
//      the partial last tile column needs no case of its own;
//   2. gives every work-item runs of 4 output pixels of one row (16 work-items across, 16 rows per trip, 2 trips): the four
//      taps of each channel come straight from the source (byte loads; neighbouring lanes share the lines), and the 12
//      result bytes go to the sink.
// Reads stay inside the image (x0, x1 <= w - 1, y0, y1 <= h - 1, both >= 0: the contract clamps them).  The columns and rows
// of an edge tile that lie past the output get the taps of index 0 and never reach the sink.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.
#pragma once
#pragma clang fp contract(off)

#include <type_traits>

#include "fused_common.hpp"
#include "kernels.hpp"

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

// nbytes <= 12 bytes, little-endian in (w0, w1, w2), to o: bytes up to the first 4-byte boundary, dwords from there, bytes
// behind the last whole dword.
__device__ __forceinline__ void store_run(uint8_t *o, uint32_t w0, uint32_t w1, uint32_t w2, int nbytes)
{
    const int head = min((int)((4u - (uint32_t)(uintptr_t)o) & 3u), nbytes);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < head) o[k] = (uint8_t)(w0 >> (8 * k));
    const int sh = 8 * head;
    const uint32_t d0 = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
    const uint32_t d1 = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
    const uint32_t d2 = w2 >> sh;
    uint8_t *p = o + head;
    const int rem = nbytes - head;
    if (rem >= 4) *reinterpret_cast<uint32_t *>(p) = d0;
    if (rem >= 8) *reinterpret_cast<uint32_t *>(p + 4) = d1;
    if (rem >= 12) *reinterpret_cast<uint32_t *>(p + 8) = d2;
    const int nd = rem & ~3;
    const uint32_t t = nd == 0 ? d0 : nd == 4 ? d1 : d2;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (nd + k < rem) p[nd + k] = (uint8_t)(t >> (8 * k));
}

// What the arguments of both kernels begin with.
struct ResampleArgs {
    const uint8_t *src;
    const ResizeRecord *records;
    int out_w, out_h;
    FastDiv tiles_x;     // tiles across the output; the reciprocal comes from the host
};

// The head and the grid of a launch over n_images > 0 images, or what the launchers refuse.
inline hipError_t resample_launch(int n_images, const uint8_t *d_src, const ResizeRecord *d_records, int out_w, int out_h,
                                  ResampleArgs &a, dim3 &grid)
{
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide || n_images < 0 || n_images > 65535)
        return hipErrorInvalidValue;
    const uint64_t tiles = resize_tiles(out_w, out_h);
    if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
    a.src = d_src;
    a.records = d_records;
    a.out_w = out_w;
    a.out_h = out_h;
    a.tiles_x.d = (uint32_t)((out_w + kTileW - 1) / kTileW);
    a.tiles_x.m = 0xffffffffu / a.tiles_x.d;
    grid = dim3((uint32_t)tiles, (uint32_t)n_images);
    return hipSuccess;
}

// The rows of resample_walk for a placed record: its loop with a select per pixel in front of the loads.  A run that
// straddles a window edge has pixels of both kinds; a padded row is all fill.
template <typename Sink>
__device__ __forceinline__ void placed_rows(const ResampleArgs &a, const PlacedResizeRecord &r, const int *cx0, const int *cx1,
                                            const float *cfx, const int *ry0, const int *ry1, const float *rfy, int px0, int py0,
                                            int ly, int lx, int x, int npix, uint32_t fill, Sink sink)
{
    int64_t x0[kRun], x1[kRun];
    float fx[kRun];
    bool xpad[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        const int i0 = cx0[kRun * lx + k];
        xpad[k] = i0 < 0;
        x0[k] = r.step_x * (uint32_t)max(i0, 0);
        x1[k] = r.step_x * (uint32_t)cx1[kRun * lx + k];
        fx[k] = cfx[kRun * lx + k];
    }
    const uint8_t *src = a.src + r.offset;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.out_h) break;
        const int j0 = ry0[u];
        const bool ypad = j0 < 0;
        const uint8_t *r0 = src + (int64_t)(uint32_t)max(j0, 0) * r.step_y, *r1 = src + (int64_t)(uint32_t)ry1[u] * r.step_y;
        const float fy = rfy[u];
        uint32_t o[kRun][3];
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            if (ypad || xpad[k]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = (fill >> (8 * c)) & 0xffu;
            } else {
                const uint8_t *pa = r0 + x0[k], *pb = r0 + x1[k], *pc = r1 + x0[k], *pd = r1 + x1[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) o[k][c] = resample((float)pa[c], (float)pb[c], (float)pc[c], (float)pd[c], fx[k], fy);
            }
        }
        sink(o, y, x, npix);
    }
}

// The tile blockIdx.x of image blockIdx.y: sink(o, y, x, npix) for every run of the tile, o[k][c] the byte of channel c of the
// pixel stored at (x + k, y), k < npix <= kRun.  flips: the image's ResizeRecord::flip counts (it is not read otherwise).
// Oriented: the records are OrientedResizeRecords ("oriented resample": a.records points at them) -- w and h are the ORIENTED
// image's, offset its first byte, and the byte of channel c of its pixel (x', y') lies at offset + x' step_x + y' step_y + c,
// the steps signed; everything else of the walk, the filter included, is the text below, which compiles as it did without.
// Placed: the records are PlacedResizeRecords ("placed resample", oriented as well): canvas column xs = flip ? out_w - 1 - x : x
// takes the taps of xs - x0 where that lies in [0, ww), and is padded (cx0 = -1) otherwise; rows likewise (ry0 = -1).  A padded
// pixel reads nothing -- so a tile without a window pixel reads no source byte -- and its three values are `fill`'s bytes
// (channel c in bits 8 c ...).  Without Placed the text compiles as it did.
template <bool Oriented = false, bool Placed = false, typename Sink>
__device__ __forceinline__ void resample_walk(const ResampleArgs &a, bool flips, Sink sink, uint32_t fill = 0u)
{
    static_assert(Oriented || !Placed, "a placed record is an oriented one");
    using Record = typename std::conditional<Placed, PlacedResizeRecord,
                                             typename std::conditional<Oriented, OrientedResizeRecord, ResizeRecord>::type>::type;
    __shared__ int cx0[kTileW], cx1[kTileW], ry0[kTileH], ry1[kTileH];
    __shared__ float cfx[kTileW], rfy[kTileH];

    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const Record r = reinterpret_cast<const Record *>(a.records)[blockIdx.y];
    const bool flip = flips && r.flip;
    if (t < kTileW) {
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if constexpr (Placed) {
            const int xs = (flip ? a.out_w - 1 - (px0 + t) : px0 + t) - r.x0;   // (past the output: its taps reach no sink)
            if (xs >= 0 && xs < r.ww) axis_tap(xs, r.kx, r.w, i0, i1, f);
            else i0 = -1;
        } else {
            if (px0 + t < a.out_w) axis_tap(flip ? a.out_w - 1 - (px0 + t) : px0 + t, r.kx, r.w, i0, i1, f);
        }
        cx0[t] = i0; cx1[t] = i1; cfx[t] = f;
    } else if (t < kTileW + kTileH) {
        const int u = t - kTileW;
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if constexpr (Placed) {
            const int ys = py0 + u - r.y0;
            if (ys >= 0 && ys < r.wh) axis_tap(ys, r.ky, r.h, i0, i1, f);
            else i0 = -1;
        } else {
            if (py0 + u < a.out_h) axis_tap(py0 + u, r.ky, r.h, i0, i1, f);
        }
        ry0[u] = i0; ry1[u] = i1; rfy[u] = f;
    }
    __syncthreads();

    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
    if constexpr (Placed) {
        placed_rows(a, r, cx0, cx1, cfx, ry0, ry1, rfy, px0, py0, ly, lx, x, npix, fill, sink);
        return;
    }
    using Step = typename std::conditional<Oriented, int64_t, size_t>::type;   // (the additions wrap to the same address)
    Step x0[kRun], x1[kRun], pixel_bytes = 3, row_bytes = (Step)3 * (uint32_t)r.w;
    if constexpr (Oriented) {
        pixel_bytes = r.step_x;
        row_bytes = r.step_y;
    }
    float fx[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        x0[k] = pixel_bytes * (uint32_t)cx0[kRun * lx + k];
        x1[k] = pixel_bytes * (uint32_t)cx1[kRun * lx + k];
        fx[k] = cfx[kRun * lx + k];
    }
    const uint8_t *src = a.src + r.offset;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.out_h) break;
        const uint8_t *r0 = src + (Step)(uint32_t)ry0[u] * row_bytes, *r1 = src + (Step)(uint32_t)ry1[u] * row_bytes;
        const float fy = rfy[u];
        uint32_t o[kRun][3];
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const uint8_t *pa = r0 + x0[k], *pb = r0 + x1[k], *pc = r1 + x0[k], *pd = r1 + x1[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[k][c] = resample((float)pa[c], (float)pb[c], (float)pc[c], (float)pd[c], fx[k], fy);
        }
        sink(o, y, x, npix);
    }
}

}  // namespace jpeg_amd
