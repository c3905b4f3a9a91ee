// capi_host.hip -- the C ABI, host-buffer unit: upload, the device call, download, for callers without device memory.
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace {

size_t rect_samples(const jpeg_amd_layout *L) { return (size_t)L->width * L->height * L->nplanes; }

}  // namespace

int jpeg_amd_host_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                const int16_t *const h_coef[], const uint16_t *h_quanta,
                                int ntables, uint16_t *const h_planes[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    JA_TRY(bag.alloc_planes(L, d_planes));
    JA_TRY(jpeg_amd_spectral_idct(ctx, L, d_coef, h_quanta, ntables, d_planes));
    JA_TRY(bag.download_planes(L, h_planes, d_planes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                     const uint16_t *const h_planes[], int cosited,
                                     uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!h_planes || !h_rect) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_planes, d_planes));
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.alloc(rect_samples(L) * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_planar_interleaved(ctx, L, d_planes, cosited, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, rect_samples(L) * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *h_rect, size_t npixels,
                                     int nplanes, jpeg_amd_color color, uint8_t *h_pixels)
try {
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_rect, npixels * nplanes * 2, (void **)&d_rect));
    JA_TRY(bag.alloc(npixels * 3, (void **)&d_px));
    JA_TRY(jpeg_amd_rectangular_unpack(ctx, d_rect, npixels, nplanes, color, d_px));
    JA_TRY(bag.download(h_pixels, d_px, npixels * 3));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                         const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                         int cosited, jpeg_amd_color color, uint8_t *h_pixels)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_pixels) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    uint8_t *d_px = nullptr;
    const size_t nbytes = (size_t)L->width * L->height * 3;
    JA_TRY(bag.alloc(nbytes, (void **)&d_px));
    JA_TRY(jpeg_amd_decode(ctx, L, d_coef, h_quanta, ntables, cosited, color, d_px));
    JA_TRY(bag.download(h_pixels, d_px, nbytes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                       const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                                       int cosited, uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_rect) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.alloc(rect_samples(L) * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_spectral_rectangular(ctx, L, d_coef, h_quanta, ntables, cosited, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, rect_samples(L) * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint16_t *h_rect,
                                       const uint16_t *h_quanta, int ntables, int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_rect || !h_coef) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.upload(h_rect, rect_samples(L) * 2, (void **)&d_rect));
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_rectangular_spectral(ctx, L, d_rect, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *h_pixels, size_t npixels,
                                   int nplanes, jpeg_amd_color color, uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_pixels, npixels * 3, (void **)&d_px));
    JA_TRY(bag.alloc(npixels * nplanes * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_rectangular_pack(ctx, d_px, npixels, nplanes, color, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, npixels * nplanes * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                         const uint16_t *h_rect, uint16_t *const h_planes[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!h_rect || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.upload(h_rect, rect_samples(L) * 2, (void **)&d_rect));
    uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_planes));
    JA_TRY(jpeg_amd_rectangular_decomposed(ctx, L, d_rect, d_planes));
    JA_TRY(bag.download_planes(L, h_planes, d_planes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                              const uint16_t *const h_planes[], const uint16_t *h_quanta,
                              int ntables, int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_planes, d_planes));
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_planar_fdct(ctx, L, d_planes, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint8_t *h_pixels,
                         jpeg_amd_color color, const uint16_t *h_quanta, int ntables,
                         int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_pixels) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_pixels, (size_t)L->width * L->height * 3, (void **)&d_px));
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_encode(ctx, L, d_px, color, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL
