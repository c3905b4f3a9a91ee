// kernels_resize.hip -- bilinear resample of pixel images to one target size (jpeg_amd_resize_batch, and behind
// jpeg_amd_decode_view_batch in jpeg_amd_decode_resized_batch).  include/jpeg_amd.h ("resized decode") holds the contract:
// half-pixel centres, the horizontal pass first, every operation one binary32 operation, the scale factors divided on the
// host.  axis_tap and resample (resample.hpp, shared with k_resize_tensor) are that text, statement by statement.
//
// k_resize_bilinear: a static grid of (tiles of the output) x (images); the output size is the same for every image, so
// there is no prefix and no search.  A tile is 64 x 32 output pixels.  Its workgroup
//   1. writes the tile's per-column (x0, x1, fx) and per-row (y0, y1, fy) into LDS, one work-item per column or row --
//      they are not computed again per pixel;
//   2. gives every work-item runs of 4 output pixels of one row (16 work-items across, 16 rows per trip, 2 trips): the four
//      taps of each channel come straight from the source (byte loads; neighbouring lanes share the lines), the 12 result
//      bytes are packed into three dwords and leave as dword stores from the first 4-byte boundary of the run on, with
//      byte stores in front of and behind them (store_run).  Where 3 out_w, dst_stride and d_dst are multiples of 4 --
//      224 x 224 into a dense tensor -- every full run is three dword stores.
// Reads stay inside the image (x0, x1 <= w - 1, y0, y1 <= h - 1, both >= 0: the contract clamps them); writes stay inside
// out_h rows of 3 out_w bytes.  The columns and rows of an edge tile that lie past the output get the taps of index 0 and
// are never stored.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

namespace {

struct ResizeArgs {
    const uint8_t *src;
    const ResizeRecord *records;
    int out_w, out_h;
    FastDiv tiles_x;     // tiles across the output; the reciprocal comes from the host
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

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

__global__ __launch_bounds__(kThreads) void k_resize_bilinear(ResizeArgs a)
{
    __shared__ int cx0[kTileW], cx1[kTileW], ry0[kTileH], ry1[kTileH];
    __shared__ float cfx[kTileW], rfy[kTileH];

    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const ResizeRecord r = a.records[blockIdx.y];
    if (t < kTileW) {
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if (px0 + t < a.out_w) axis_tap(px0 + t, r.kx, r.w, i0, i1, f);
        cx0[t] = i0; cx1[t] = i1; cfx[t] = f;
    } else if (t < kTileW + kTileH) {
        const int u = t - kTileW;
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if (py0 + u < a.out_h) axis_tap(py0 + u, r.ky, r.h, i0, i1, f);
        ry0[u] = i0; ry1[u] = i1; rfy[u] = f;
    }
    __syncthreads();

    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
    size_t x0[kRun], x1[kRun];
    float fx[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        x0[k] = (size_t)3 * (uint32_t)cx0[kRun * lx + k];
        x1[k] = (size_t)3 * (uint32_t)cx1[kRun * lx + k];
        fx[k] = cfx[kRun * lx + k];
    }
    const size_t row_bytes = (size_t)3 * (uint32_t)r.w;
    const uint8_t *src = a.src + r.offset;
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.out_h) break;
        const uint8_t *r0 = src + (size_t)(uint32_t)ry0[u] * row_bytes, *r1 = src + (size_t)(uint32_t)ry1[u] * row_bytes;
        const float fy = rfy[u];
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const uint8_t *pa = r0 + x0[k], *pb = r0 + x1[k], *pc = r1 + x0[k], *pd = r1 + x1[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t o = resample((float)pa[c], (float)pb[c], (float)pc[c], (float)pd[c], fx[k], fy);
                w[(3 * k + c) >> 2] |= o << (8 * ((3 * k + c) & 3));
            }
        }
        store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
    }
}

}  // namespace

uint64_t resize_tiles(int out_w, int out_h)
{
    return (uint64_t)((out_w + kTileW - 1) / kTileW) * (uint64_t)((out_h + kTileH - 1) / kTileH);
}

hipError_t launch_resize_bilinear(hipStream_t stream, int n_images, const uint8_t *d_src, const ResizeRecord *d_records,
                                  int out_w, int out_h, uint8_t *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide || n_images < 0 || n_images > 65535)
        return hipErrorInvalidValue;
    const uint64_t tiles = resize_tiles(out_w, out_h);
    if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
    ResizeArgs a{};
    a.src = d_src;
    a.records = d_records;
    a.out_w = out_w;
    a.out_h = out_h;
    a.tiles_x.d = (uint32_t)((out_w + kTileW - 1) / kTileW);
    a.tiles_x.m = 0xffffffffu / a.tiles_x.d;
    a.dst = d_dst;
    a.dst_stride = dst_stride;
    hipLaunchKernelGGL(k_resize_bilinear, dim3((uint32_t)tiles, (uint32_t)n_images), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace jpeg_amd
