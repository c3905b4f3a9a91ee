// kernels_antialias.hip -- the antialiased resample of pixel images to one target size (the *_filter_* calls of
// include/jpeg_amd.h with JPEG_AMD_FILTER_ANTIALIAS; "antialiased resample" there holds the contract): the triangle filter
// widened by the scale factor, normalised weights, the horizontal pass first, every operation one binary32 operation, and
// k, s = max(k, 1) and r = 1 / s of both axes made on the host.  antialias.hpp holds the filter and the walk.
//
// k_antialias_bytes: antialias_walk, never flipped, with the sink that packs the 12 bytes of a run into three dwords and
// stores them as k_resize_bilinear does (store_run): dword stores from the first 4-byte boundary of the run on.  Writes stay
// inside out_h rows of 3 out_w bytes.
// k_antialias_tensor<T, CHW>: antialias_walk, flipped where the image's record says so, with k_resize_tensor's sink
// (tensor_sink.hpp).  Writes stay inside 3 out_w out_h elements of the image.
// k_bicubic_bytes, k_bicubic_tensor<T, CHW>: the same two bodies with the weights of JPEG_AMD_FILTER_BICUBIC ("bicubic
// resample" in the header: the Keys cubic, a = -0.5, widened by the scale factor; BicubicFilter in antialias.hpp).  The same
// records, tables, LDS and stores; the host keeps kx and ky at or below kBicubicMaxScale.
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

struct AntialiasBytesArgs : ResampleArgs {
    const AntialiasRecord *aa_records;
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

template <typename T>
struct AntialiasTensorArgs : TensorArgs<T> {
    const AntialiasRecord *aa_records;
};

// (Each kernel states its few lines itself: behind a shared body or sink function the compiler allots k_antialias_bytes'
// registers differently from the way it did before there were two filters.)
__global__ __launch_bounds__(kThreads) void k_antialias_bytes(AntialiasBytesArgs a)
{
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    antialias_walk<TriangleFilter>(a, a.aa_records, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kRun; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= o[k][c] << (8 * ((3 * k + c) & 3));
        store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
    });
}

__global__ __launch_bounds__(kThreads) void k_bicubic_bytes(AntialiasBytesArgs a)
{
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    antialias_walk<BicubicFilter>(a, a.aa_records, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kRun; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= o[k][c] << (8 * ((3 * k + c) & 3));
        store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
    });
}

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_antialias_tensor(AntialiasTensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    antialias_walk<TriangleFilter>(a, a.aa_records, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_bicubic_tensor(AntialiasTensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    antialias_walk<BicubicFilter>(a, a.aa_records, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

template <typename T, bool CHW>
hipError_t launch(hipStream_t stream, bool bicubic, const ResampleArgs &head, dim3 grid, const AntialiasRecord *d_records,
                  const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    AntialiasTensorArgs<T> a{};
    static_cast<ResampleArgs &>(a) = head;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = spec.mean[c];
        a.scale[c] = spec.scale[c];
    }
    a.dst = static_cast<T *>(d_dst);
    a.dst_stride = dst_stride;
    a.aa_records = d_records;
    if (bicubic)
        hipLaunchKernelGGL((k_bicubic_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((k_antialias_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_bytes(hipStream_t stream, bool bicubic, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                        int out_w, int out_h, uint8_t *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    AntialiasBytesArgs a{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, nullptr, out_w, out_h, a, grid)) return e;
    a.aa_records = d_records;
    a.dst = d_dst;
    a.dst_stride = dst_stride;
    if (bicubic)
        hipLaunchKernelGGL(k_bicubic_bytes, grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(k_antialias_bytes, grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_tensor(hipStream_t stream, bool bicubic, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                         int out_w, int out_h, const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    ResampleArgs head{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, nullptr, out_w, out_h, head, grid)) return e;
    const bool chw = spec.layout == JPEG_AMD_TENSOR_CHW;
    if (!chw && spec.layout != JPEG_AMD_TENSOR_HWC) return hipErrorInvalidValue;
    switch (spec.dtype) {
    case JPEG_AMD_F32:
        return chw ? launch<float, true>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride)
                   : launch<float, false>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride);
    case JPEG_AMD_F16:
        return chw ? launch<_Float16, true>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride)
                   : launch<_Float16, false>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride);
    case JPEG_AMD_BF16:
        return chw ? launch<bf16_t, true>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride)
                   : launch<bf16_t, false>(stream, bicubic, head, grid, d_records, spec, d_dst, dst_stride);
    default:
        return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_antialias_bytes(hipStream_t stream, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                                  int out_w, int out_h, uint8_t *d_dst, size_t dst_stride)
{
    return launch_bytes(stream, false, n_images, d_src, d_records, out_w, out_h, d_dst, dst_stride);
}

hipError_t launch_antialias_tensor(hipStream_t stream, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                                   int out_w, int out_h, const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    return launch_tensor(stream, false, n_images, d_src, d_records, out_w, out_h, spec, d_dst, dst_stride);
}

hipError_t launch_bicubic_bytes(hipStream_t stream, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                                int out_w, int out_h, uint8_t *d_dst, size_t dst_stride)
{
    return launch_bytes(stream, true, n_images, d_src, d_records, out_w, out_h, d_dst, dst_stride);
}

hipError_t launch_bicubic_tensor(hipStream_t stream, int n_images, const uint8_t *d_src, const AntialiasRecord *d_records,
                                 int out_w, int out_h, const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    return launch_tensor(stream, true, n_images, d_src, d_records, out_w, out_h, spec, d_dst, dst_stride);
}

}  // namespace jpeg_amd
