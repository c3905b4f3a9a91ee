// kernels_tensor.hip -- the bilinear resample with the loader's output stage in the same launch (jpeg_amd_resize_tensor_batch,
// and behind the view decode in the tensor calls).  include/jpeg_amd.h ("tensor output") holds the contract: the byte u that
// the resample defines ("resized decode"; the filter and the walk over the output are resample.hpp's, the filter shared
// with k_resize_bilinear), then
//     t = (float)u - mean[c];  v = t * scale[c]          two binary32 operations, nothing contracted, no division
// and v stored as binary32, or rounded to nearest even to binary16 or bfloat16.
//
// k_resize_tensor<T, CHW>: resample_walk, flipped where the image's record says so, with the sink that turns the 12 bytes of
// a run into elements (the conversions and the stores are tensor_sink.hpp's, shared with k_antialias_tensor; the sink's own
// dozen lines stand here and, as a function, there: handed the function, the compiler builds other code for these kernels, as
// it does for k_resize_bilinear through resample_walk, and the bilinear kernels are to stay the code they were), which stay in registers and leave through store_elems: HWC one run of 12 consecutive elements, CHW
// three runs of 4.  Element stores up to the first address that is a multiple of 4 elements, 4-element vector stores from
// there (16 bytes at binary32, 8 bytes at the 16-bit types; two of them merged into one 16-byte store where the address
// allows), element stores behind the last whole vector.  Any element-aligned base and any stride are correct; where out_w is a
// multiple of 4 and d_dst and dst_stride are multiples of 4 elements -- 224 x 224 into a dense tensor -- every run leaves in
// vector stores only.
// Conversions: binary16 is the compiler's float -> _Float16 conversion of the finished binary32 product (v_cvt_f16_f32, round
// to nearest even in the default mode; see to_element).  bfloat16 is INTEGER ARITHMETIC ON THE BITS, bits + 0x7fff + ((bits >> 16) & 1), the upper half kept -- not the
// packed hardware convert: it is the contract's own formula, it needs no inline assembly, and every value here is finite.
// Reads stay inside the image and writes inside 3 out_w out_h elements of the image, as in kernels_resize.hip.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"
#include "tensor_sink.hpp"

namespace jpeg_amd {

namespace {

template <typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_resize_tensor(TensorArgs<T> a)
{
    T *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
    const size_t plane = (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h;
    resample_walk(a, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        T e[CHW ? 3 : 1][CHW ? kRun : 3 * kRun];   // CHW: three runs of kRun, HWC: one run of 3 kRun
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = (float)o[k][c] - a.mean[c];
                e[CHW ? c : 0][CHW ? k : 3 * k + c] = to_element<T>(d * a.scale[c]);
            }
        }
        const size_t at = (size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x;
        if constexpr (CHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) store_elems<T, kRun>(dst + c * plane + at, e[c], npix);
        } else {
            store_elems<T, 3 * kRun>(dst + 3 * at, e[0], 3 * npix);
        }
    });
}

template <typename T, bool CHW>
hipError_t launch(hipStream_t stream, const ResampleArgs &head, dim3 grid, const jpeg_amd_tensor_spec &spec, void *d_dst,
                  size_t dst_stride)
{
    TensorArgs<T> a{};
    static_cast<ResampleArgs &>(a) = head;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = spec.mean[c];
        a.scale[c] = spec.scale[c];
    }
    a.dst = static_cast<T *>(d_dst);
    a.dst_stride = dst_stride;
    hipLaunchKernelGGL((k_resize_tensor<T, CHW>), grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resize_tensor(hipStream_t stream, int n_images, const uint8_t *d_src, const ResizeRecord *d_records,
                                int out_w, int out_h, const jpeg_amd_tensor_spec &spec, void *d_dst, size_t dst_stride)
{
    if (n_images == 0) return hipSuccess;
    ResampleArgs head{};
    dim3 grid;
    if (const hipError_t e = resample_launch(n_images, d_src, d_records, out_w, out_h, head, grid)) return e;
    const bool chw = spec.layout == JPEG_AMD_TENSOR_CHW;
    if (!chw && spec.layout != JPEG_AMD_TENSOR_HWC) return hipErrorInvalidValue;
    switch (spec.dtype) {
    case JPEG_AMD_F32:
        return chw ? launch<float, true>(stream, head, grid, spec, d_dst, dst_stride)
                   : launch<float, false>(stream, head, grid, spec, d_dst, dst_stride);
    case JPEG_AMD_F16:
        return chw ? launch<_Float16, true>(stream, head, grid, spec, d_dst, dst_stride)
                   : launch<_Float16, false>(stream, head, grid, spec, d_dst, dst_stride);
    case JPEG_AMD_BF16:
        return chw ? launch<bf16_t, true>(stream, head, grid, spec, d_dst, dst_stride)
                   : launch<bf16_t, false>(stream, head, grid, spec, d_dst, dst_stride);
    default:
        return hipErrorInvalidValue;
    }
}

}  // namespace jpeg_amd
