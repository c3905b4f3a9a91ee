// kernels_resize.hip -- bilinear resample of pixel images to one target size, bytes out (jpeg_amd_resize_batch, and behind
// the view decode in the resized calls).  include/jpeg_amd.h ("resized decode") holds the contract: half-pixel centres, the
// horizontal pass first, every operation one binary32 operation, the scale factors divided on the host.  The filter, the tile
// and the head of the arguments are resample.hpp's, shared with k_resize_tensor.
//
// k_resize_bilinear: the walk that resample.hpp describes (resample_walk, never flipped: ResizeRecord::flip is not read),
// written out here with the packing inside the tap loop.  Through resample_walk, which hands over a finished run, the compiler
// packs the 12 bytes with four instructions per dword where this text gets three, and the kernel measured 1.3 % slower on the
// MI355X (profiles/resample_refactor.txt); so this kernel keeps its own text, and a change to the walk is made in both places.
// The 12 result bytes of a run are packed into three dwords and leave as dword stores from the first 4-byte boundary of the
// run on, with byte stores in front of and behind them (store_run).  Where 3 out_w, dst_stride and d_dst are multiples of 4 --
// 224 x 224 into a dense tensor -- every full run is three dword stores.  Writes stay inside out_h rows of 3 out_w bytes.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

namespace {

struct ResizeArgs : ResampleArgs {
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

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
    ResizeArgs a{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, d_records, out_w, out_h, a, grid)) return e;
    a.dst = d_dst;
    a.dst_stride = dst_stride;
    hipLaunchKernelGGL(k_resize_bilinear, grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace jpeg_amd
