// kernels_pixels.hip -- tensors to the encoders' bytes (jpeg_amd_tensor_pixels_batch, and in front of the encoders in the
// tensor encode and compress calls).  include/jpeg_amd.h ("tensor sources") holds the contract: per element one conversion to
// binary32, one product, one sum, the clamp and the rounding byte conversion of the resample kernels; a uint8 element is its
// byte.  The loads and the conversion are tensor_source.hpp's.
//
// k_tensor_pixels<T, CHW>: the grid of the resample kernels -- (tiles of 64 x 32 pixels) x (images), a work-item takes runs of
// kRun = 4 pixels of one row, 16 work-items across, 16 rows per trip, 2 trips -- with nothing to share between work-items, so no
// LDS.  A run is read as HWC one run of 12 consecutive elements, CHW three runs of 4: element loads up to the first address
// that is a multiple of 4 elements, 4-element vector loads from there (16 bytes at binary32, 8 at the 16-bit types, 4 at
// uint8), element loads behind the last whole vector (load_elems).  The 12 bytes are packed into three dwords and leave
// through store_run, as in k_resize_bilinear.  Any element-aligned base and any stride are correct; where w is a multiple of
// 4 and d_src and src_stride are multiples of 4 elements every full run arrives in vector loads only.
// Element offsets are 64-bit (an image is up to 3 * 65 535^2 elements).  Reads stay inside 3 w h elements of each image (only
// the elements of the run's npix pixels are read; the others stay zero and their bytes are not stored) and writes inside h
// rows of 3 w bytes.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"
#include "tensor_source.hpp"

namespace jpeg_amd {

namespace {

template <typename T>
struct PixelsArgs {
    const T *src;
    size_t src_stride;   // elements between source images
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
    int w, h;
    FastDiv tiles_x;     // tiles across the image; the reciprocal comes from the host
    float scale[3], offset[3];
};

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_tensor_pixels(PixelsArgs<T> a)
{
    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.w - x);
    if (npix <= 0) return;
    const T *src = a.src + (size_t)blockIdx.y * a.src_stride;
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.w * (uint32_t)a.h;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.h) break;
        const size_t at = (size_t)(uint32_t)y * (uint32_t)a.w + (uint32_t)x;
        T e[CHW ? 3 : 1][CHW ? kRun : 3 * kRun] = {};   // CHW: three runs of kRun, HWC: one run of 3 kRun
        if constexpr (CHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) load_elems<T, kRun>(src + c * plane + at, e[c], npix);
        } else {
            load_elems<T, 3 * kRun>(src + 3 * at, e[0], 3 * npix);
        }
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t o = to_byte<T>(e[CHW ? c : 0][CHW ? k : 3 * k + c], a.scale[c], a.offset[c]);
                w[(3 * k + c) >> 2] |= o << (8 * ((3 * k + c) & 3));
            }
        }
        store_run(dst + 3 * at, w[0], w[1], w[2], 3 * npix);
    }
}

template <typename T, bool CHW>
hipError_t launch(hipStream_t stream, int n_images, const void *d_src, size_t src_stride, int w, int h,
                  const jpeg_amd_tensor_source &source, uint8_t *d_dst, size_t dst_stride)
{
    PixelsArgs<T> a{};
    a.src = static_cast<const T *>(d_src);
    a.src_stride = src_stride;
    a.dst = d_dst;
    a.dst_stride = dst_stride;
    a.w = w;
    a.h = h;
    a.tiles_x.d = (uint32_t)((w + kTileW - 1) / kTileW);
    a.tiles_x.m = 0xffffffffu / a.tiles_x.d;
    for (int c = 0; c < 3; ++c) {
        a.scale[c] = source.scale[c];
        a.offset[c] = source.offset[c];
    }
    const dim3 grid((uint32_t)resize_tiles(w, h), (uint32_t)n_images);
    hipLaunchKernelGGL((k_tensor_pixels<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tensor_pixels(hipStream_t stream, int n_images, const void *d_src, size_t src_stride, int w, int h,
                                const jpeg_amd_tensor_source &source, uint8_t *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    if (w < 1 || h < 1 || w > kTensorSourceMaxSide || h > kTensorSourceMaxSide || n_images < 0 || n_images > 65535)
        return hipErrorInvalidValue;
    const bool chw = source.layout == JPEG_AMD_TENSOR_CHW;
    if (!chw && source.layout != JPEG_AMD_TENSOR_HWC) return hipErrorInvalidValue;
    switch (source.dtype) {
    case JPEG_AMD_F32:
        return chw ? launch<float, true>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride)
                   : launch<float, false>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride);
    case JPEG_AMD_F16:
        return chw ? launch<_Float16, true>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride)
                   : launch<_Float16, false>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride);
    case JPEG_AMD_BF16:
        return chw ? launch<bf16_t, true>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride)
                   : launch<bf16_t, false>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride);
    case JPEG_AMD_U8:
        return chw ? launch<uint8_t, true>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride)
                   : launch<uint8_t, false>(stream, n_images, d_src, src_stride, w, h, source, d_dst, dst_stride);
    default:
        return hipErrorInvalidValue;
    }
}

}  // namespace jpeg_amd
