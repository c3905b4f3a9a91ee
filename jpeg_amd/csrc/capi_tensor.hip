// capi_tensor.hip -- the C ABI, tensor sources of the encoders (include/jpeg_amd.h, "tensor sources"): the front launch alone
// and in front of jpeg_amd_encode_batch.  Its place in the batch file pipeline, jpeg_amd_compress_tensor_batch_device, is in
// capi_file.hip.  No arithmetic on samples happens here; all of it is in kernels_pixels.hip.
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace jpeg_amd {
namespace capi {

int check_tensor_source(int n_images, const void *d_src, size_t src_stride, int32_t w, int32_t h,
                        const jpeg_amd_tensor_source *src, size_t *elem_bytes)
{
    size_t image_elems = 0;
    JA_TRY(jpeg_amd_tensor_source_extent(src, w, h, elem_bytes, &image_elems));
    if (n_images > 0 && !d_src) return JPEG_AMD_EINVAL;
    if ((uintptr_t)d_src % *elem_bytes != 0) return JPEG_AMD_EINVAL;
    if (n_images > 1 && src_stride < image_elems) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

}  // namespace capi
}  // namespace jpeg_amd

namespace {

constexpr size_t kTensorChunkBytes = (size_t)1 << 30;   // of bytes between the front launch and the encoder, per chunk

bool is_pixels(const jpeg_amd_tensor_source *src) { return src->dtype == JPEG_AMD_U8 && src->layout == JPEG_AMD_TENSOR_HWC; }

}  // namespace

int jpeg_amd_tensor_source_extent(const jpeg_amd_tensor_source *src, int32_t w, int32_t h, size_t *elem_bytes, size_t *image_elems)
{
    if (!src) return JPEG_AMD_EINVAL;
    if (src->dtype != JPEG_AMD_F32 && src->dtype != JPEG_AMD_F16 && src->dtype != JPEG_AMD_BF16 && src->dtype != JPEG_AMD_U8)
        return JPEG_AMD_EINVAL;
    if (src->layout != JPEG_AMD_TENSOR_HWC && src->layout != JPEG_AMD_TENSOR_CHW) return JPEG_AMD_EINVAL;
    if (src->dtype != JPEG_AMD_U8)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(src->scale[c]) || !std::isfinite(src->offset[c])) return JPEG_AMD_EINVAL;
    if (w < 1 || h < 1 || w > kTensorSourceMaxSide || h > kTensorSourceMaxSide) return JPEG_AMD_EINVAL;
    if (elem_bytes) *elem_bytes = src->dtype == JPEG_AMD_F32 ? 4 : src->dtype == JPEG_AMD_U8 ? 1 : 2;
    if (image_elems) *image_elems = (size_t)3 * w * h;
    return JPEG_AMD_OK;
}

int jpeg_amd_tensor_pixels_batch(jpeg_amd_ctx *ctx, int n_images, const void *d_src, size_t src_stride, int32_t w, int32_t h,
                                 const jpeg_amd_tensor_source *src, uint8_t *d_pixels, size_t pixel_stride)
{
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    size_t elem_bytes = 0;
    JA_TRY(check_tensor_source(n_images, d_src, src_stride, w, h, src, &elem_bytes));
    const size_t npx = (size_t)3 * w * h;
    if (pixel_stride == 0) pixel_stride = npx;
    if (n_images > 0 && !d_pixels) return JPEG_AMD_EINVAL;
    if (n_images > 1 && pixel_stride < npx) return JPEG_AMD_EINVAL;
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;
    JA_HIP(ctx, launch_tensor_pixels(ctx->stream, n_images, d_src, src_stride, w, h, *src, d_pixels, pixel_stride));
    return JPEG_AMD_OK;
}

int jpeg_amd_encode_tensor_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const void *d_src, size_t src_stride,
                                 const jpeg_amd_tensor_source *src, jpeg_amd_color color, const uint16_t *d_quanta,
                                 size_t quanta_stride, int ntables, int16_t *const d_coef[], const size_t coef_stride[])
{
    // what jpeg_amd_encode_batch judges, in its order, then the source; the first chunk is enqueued behind all of it
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_batch8(L, n_images, color));
    if (n_images > 0) {
        if (!d_coef || !coef_stride || !d_quanta || !d_src) return JPEG_AMD_EINVAL;
        PlaneSetMut cs;
        JA_TRY(plane_set(L, d_coef, coef_stride, false, &cs));
    }
    size_t elem_bytes = 0;
    JA_TRY(check_tensor_source(n_images, d_src, src_stride, L->width, L->height, src, &elem_bytes));
    if (n_images == 0) return JPEG_AMD_OK;
    if (is_pixels(src))   // the existing call: no launch, no buffer
        return jpeg_amd_encode_batch(ctx, L, n_images, static_cast<const uint8_t *>(d_src), src_stride, color, d_quanta, quanta_stride,
                                     ntables, d_coef, coef_stride);
    const size_t npx = (size_t)3 * L->width * L->height;
    const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_images, kTensorChunkBytes / npx));
    JA_TRY(ensure_buffer(ctx, ctx->tensor_px, npx * (size_t)per));
    uint8_t *d_px = static_cast<uint8_t *>(ctx->tensor_px.ptr);
    for (int i0 = 0; i0 < n_images; i0 += per) {
        const int m = std::min(per, n_images - i0);
        JA_HIP(ctx, launch_tensor_pixels(ctx->stream, m, static_cast<const uint8_t *>(d_src) + (size_t)i0 * src_stride * elem_bytes,
                                         src_stride, L->width, L->height, *src, d_px, npx));
        int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        for (int p = 0; p < L->nplanes; ++p) coef[p] = d_coef[p] ? d_coef[p] + (size_t)i0 * coef_stride[p] : nullptr;
        JA_TRY(jpeg_amd_encode_batch(ctx, L, m, d_px, npx, color, d_quanta + (size_t)i0 * quanta_stride, quanta_stride, ntables, coef,
                                     coef_stride));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_encode_tensor(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const void *d_src, const jpeg_amd_tensor_source *src,
                           jpeg_amd_color color, const uint16_t *h_quanta, int ntables, int16_t *const d_coef[])
{
    // what can be refused is refused before a table is staged
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_batch8(L, 1, color));
    if (!d_coef || !d_src || !h_quanta) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, kOneImage, false, &cs));
    size_t elem_bytes = 0;
    JA_TRY(check_tensor_source(1, d_src, 0, L->width, L->height, src, &elem_bytes));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_encode_tensor_batch(ctx, L, 1, d_src, 0, src, color, d_q, 0, ntables, d_coef, kOneImage);
}
