// kernels_oriented.hip -- the bilinear, the antialiased and the bicubic resample of pixel images read in one of the eight EXIF
// orientations (the *_oriented_* calls of include/jpeg_amd.h; "oriented resample" there holds the contract, orient.hpp the orientations):
// the contract of the filter applied to the oriented image, which is the stored one read through a base and two signed steps
// (OrientedResizeRecord, OrientedAntialiasRecord: made on the host).  No arithmetic of its own: the walks are resample.hpp's
// and antialias.hpp's with Oriented set, the sinks those of the four kernels beside which these stand.
//
// k_resize_oriented_bytes: resample_walk<true>, never flipped, with the byte sink of k_antialias_bytes (store_run).
// k_resize_oriented_tensor<T, CHW>: resample_walk<true>, flipped where the record says so (after the orientation: the flip
//   mirrors the OUTPUT columns), with tensor_sink.
// k_antialias_oriented_bytes, k_antialias_oriented_tensor<T, CHW>: antialias_walk over OrientedAntialiasRecords, likewise.
// k_bicubic_oriented_bytes, k_bicubic_oriented_tensor<T, CHW>: the same two with the bicubic weights (BicubicFilter).
//
// Reads: an oriented pixel (x', y') with 0 <= x' < w', 0 <= y' < h' is a stored pixel, so the walks' own clamps keep every
// read inside the stored image.  With a transposing orientation (5 .. 8) neighbouring lanes read bytes a stored row apart
// instead of 3 bytes apart: more cache lines per load, the same lines per tile.  LDS as the walks' (antialias: 38 016 bytes).
// Writes stay inside the image's slot as in the kernels beside which these stand.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "antialias.hpp"
#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"
#include "tensor_sink.hpp"

namespace jpeg_amd {

namespace {

struct OrientedBytesArgs : ResampleArgs {
    const OrientedAntialiasRecord *aa_records;   // the antialias kernel's; the bilinear one reads ResampleArgs::records
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

template <typename T>
struct OrientedTensorArgs : TensorArgs<T> {
    const OrientedAntialiasRecord *aa_records;
};

__device__ __forceinline__ void byte_sink(uint8_t *dst, int out_w, const uint32_t (&o)[kRun][3], int y, int x, int npix)
{
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kRun; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= o[k][c] << (8 * ((3 * k + c) & 3));
    store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
}

__global__ __launch_bounds__(kThreads) void k_resize_oriented_bytes(OrientedBytesArgs a)
{
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    resample_walk<true>(a, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

__global__ __launch_bounds__(kThreads) void k_antialias_oriented_bytes(OrientedBytesArgs a)
{
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    antialias_walk<TriangleFilter>(a, a.aa_records, false,
                                   [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

__global__ __launch_bounds__(kThreads) void k_bicubic_oriented_bytes(OrientedBytesArgs a)
{
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    antialias_walk<BicubicFilter>(a, a.aa_records, false,
                                  [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_resize_oriented_tensor(OrientedTensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    resample_walk<true>(a, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_antialias_oriented_tensor(OrientedTensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    antialias_walk<TriangleFilter>(a, a.aa_records, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_bicubic_oriented_tensor(OrientedTensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    antialias_walk<BicubicFilter>(a, a.aa_records, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

template <typename T, bool CHW>
hipError_t launch(hipStream_t stream, const ResampleArgs &head, dim3 grid, const OrientedAntialiasRecord *aa_records, bool bicubic,
                  const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    OrientedTensorArgs<T> a{};
    static_cast<ResampleArgs &>(a) = head;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = spec.mean[c];
        a.scale[c] = spec.scale[c];
    }
    a.dst = static_cast<T *>(d_dst);
    a.dst_stride = dst_stride;
    a.aa_records = aa_records;
    if (aa_records && bicubic)
        hipLaunchKernelGGL((k_bicubic_oriented_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    else if (aa_records)
        hipLaunchKernelGGL((k_antialias_oriented_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((k_resize_oriented_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// Any filter: aa_records of the antialiasing one or (bicubic) the bicubic one, or nullptr and the bilinear records in `head`.
hipError_t launch_oriented(hipStream_t stream, const ResampleArgs &head, dim3 grid, const OrientedAntialiasRecord *aa_records,
                           bool bicubic, const jpeg_amd_tensor_spec *spec, void *d_dst, size_t dst_stride)
{
    if (!spec) {
        OrientedBytesArgs a{};
        static_cast<ResampleArgs &>(a) = head;
        a.aa_records = aa_records;
        a.dst = static_cast<uint8_t *>(d_dst);
        a.dst_stride = dst_stride;
        if (aa_records && bicubic)
            hipLaunchKernelGGL(k_bicubic_oriented_bytes, grid, dim3(kThreads), 0, stream, a);
        else if (aa_records)
            hipLaunchKernelGGL(k_antialias_oriented_bytes, grid, dim3(kThreads), 0, stream, a);
        else
            hipLaunchKernelGGL(k_resize_oriented_bytes, grid, dim3(kThreads), 0, stream, a);
        return hipGetLastError();
    }
    const bool chw = spec->layout == JPEG_AMD_TENSOR_CHW;
    if (!chw && spec->layout != JPEG_AMD_TENSOR_HWC) return hipErrorInvalidValue;
    switch (spec->dtype) {
    case JPEG_AMD_F32:
        return chw ? launch<float, true>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride)
                   : launch<float, false>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride);
    case JPEG_AMD_F16:
        return chw ? launch<_Float16, true>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride)
                   : launch<_Float16, false>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride);
    case JPEG_AMD_BF16:
        return chw ? launch<bf16_t, true>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride)
                   : launch<bf16_t, false>(stream, head, grid, aa_records, bicubic, *spec, d_dst, dst_stride);
    default:
        return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_resize_oriented(hipStream_t stream, int n_images, const uint8_t *d_src, const OrientedResizeRecord *d_records,
                                  int out_w, int out_h, const jpeg_amd_tensor_spec *spec, void *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    if (!d_records) return hipErrorInvalidValue;
    ResampleArgs head{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, d_records, out_w, out_h, head, grid)) return e;
    return launch_oriented(stream, head, grid, nullptr, false, spec, d_dst, dst_stride);
}

namespace {

hipError_t launch_tables_oriented(hipStream_t stream, bool bicubic, int n_images, const uint8_t *d_src,
                                  const OrientedAntialiasRecord *d_records, int out_w, int out_h, const jpeg_amd_tensor_spec *spec,
                                  void *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    if (!d_records) return hipErrorInvalidValue;
    ResampleArgs head{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, nullptr, out_w, out_h, head, grid)) return e;
    return launch_oriented(stream, head, grid, d_records, bicubic, spec, d_dst, dst_stride);
}

}  // namespace

hipError_t launch_antialias_oriented(hipStream_t stream, int n_images, const uint8_t *d_src,
                                     const OrientedAntialiasRecord *d_records, int out_w, int out_h,
                                     const jpeg_amd_tensor_spec *spec, void *d_dst, size_t dst_stride)
{
    return launch_tables_oriented(stream, false, n_images, d_src, d_records, out_w, out_h, spec, d_dst, dst_stride);
}

hipError_t launch_bicubic_oriented(hipStream_t stream, int n_images, const uint8_t *d_src,
                                   const OrientedAntialiasRecord *d_records, int out_w, int out_h,
                                   const jpeg_amd_tensor_spec *spec, void *d_dst, size_t dst_stride)
{
    return launch_tables_oriented(stream, true, n_images, d_src, d_records, out_w, out_h, spec, d_dst, dst_stride);
}

}  // namespace jpeg_amd
