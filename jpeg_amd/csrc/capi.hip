// capi.hip -- the C ABI declared in include/jpeg_amd.h, first unit: the helpers every unit shares (capi_internal.hpp),
// the context with its memory and timing calls, and the whole-image decode and encode stages.  The view and resample calls
// are in capi_view.hip, the host-buffer conveniences in capi_host.hip, the file calls in capi_file.hip (files of mixed
// sizes to one tensor: capi_files.hip), the coefficient-domain calls in capi_spectral.hip and the tensor sources of the
// encoders in capi_tensor.hip.
// No arithmetic on samples happens here; all of it is in kernels_*.hip.
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace jpeg_amd {
namespace capi {

int bind(jpeg_amd_ctx *ctx)
{
    if (!ctx) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipSetDevice(ctx->device));
    return JPEG_AMD_OK;
}

// The preconditions the reference traps on (decode.swift:1710-1712, 2227, 2599) plus the
// bounds this ABI needs.
int check_layout(const jpeg_amd_layout *L, int ntables)
{
    if (!L) return JPEG_AMD_EINVAL;
    if (L->width <= 0 || L->height <= 0) return JPEG_AMD_EINVAL;
    if (L->precision < 1 || L->precision > 16) return JPEG_AMD_EINVAL;
    if (L->nplanes < 1 || L->nplanes > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (L->scale_x < 1 || L->scale_y < 1) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p) {
        if (L->factor_x[p] < 1 || L->factor_y[p] < 1) return JPEG_AMD_EINVAL;
        if (L->factor_x[p] > L->scale_x || L->factor_y[p] > L->scale_y) return JPEG_AMD_EINVAL;
        if (L->units_x[p] < 0 || L->units_y[p] < 0) return JPEG_AMD_EINVAL;
        if ((long long)L->units_x[p] * L->units_y[p] > (1LL << 30)) return JPEG_AMD_EINVAL;
        if (ntables >= 0 && (L->qi[p] < 0 || L->qi[p] >= ntables)) return JPEG_AMD_EINVAL;
    }
    return JPEG_AMD_OK;
}

// Planar.interleaved reads plane samples up to the image size (crop copy) or up to the
// padded plane (bilinear): the planes must cover the image (decode.swift:4190-4215).
int check_planes_cover_image(const jpeg_amd_layout *L)
{
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_is_direct(*L, p)) {
            if (8 * L->units_x[p] < L->width || 8 * L->units_y[p] < L->height) return JPEG_AMD_EINVAL;
        } else {
            // bilinear: the sample index of the last pixel (decode.swift:4223-4246; its neighbour i + 1 is clamped to the
            // plane, i itself is not) must lie inside the plane.  The cosited form is the larger of the two.
            if (L->units_x[p] < 1 || L->units_y[p] < 1) return JPEG_AMD_EINVAL;
            const long long ix = axis_index(interleave_axis(*L, p, true, false), L->width - 1);
            const long long iy = axis_index(interleave_axis(*L, p, true, true), L->height - 1);
            if (ix >= 8LL * L->units_x[p] || iy >= 8LL * L->units_y[p]) return JPEG_AMD_EINVAL;
        }
    }
    return JPEG_AMD_OK;
}

size_t plane_samples(const jpeg_amd_layout *L, int p)
{
    return (size_t)64 * L->units_x[p] * L->units_y[p];
}

// One of the context's buffers with room for `bytes`, grown with an eighth to spare.  The one place that frees such a
// buffer between calls: the previous call's kernels may still use it, so the stream is synchronised first.
int ensure_buffer(jpeg_amd_ctx *ctx, DeviceBuffer &buf, size_t bytes)
{
    if (bytes <= buf.bytes) return JPEG_AMD_OK;
    if (buf.ptr) {
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        JA_HIP(ctx, hipFree(buf.ptr));
        buf = DeviceBuffer{};
    }
    const size_t want = bytes + bytes / 8 + 4096;
    JA_HIP(ctx, hipMalloc(&buf.ptr, want));
    buf.bytes = want;
    return JPEG_AMD_OK;
}

// Copy host tables [ntables][64] into the next ring slot; returns the device pointer.
int stage_quanta(jpeg_amd_ctx *ctx, const uint16_t *h_quanta, int ntables, const uint16_t **d_out)
{
    if (!h_quanta || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    uint16_t *slot = ctx->d_qstage + (size_t)ctx->qslot * kQSlotElems;
    ctx->qslot = (ctx->qslot + 1) % kQSlots;
    JA_HIP(ctx, hipMemcpyAsync(slot, h_quanta, (size_t)ntables * 64 * sizeof(uint16_t),
                               hipMemcpyHostToDevice, ctx->stream));
    *d_out = slot;
    return JPEG_AMD_OK;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bytes of scratch_planes's planes: they take [0, this) of the scratch.
size_t scratch_planes_bytes(const jpeg_amd_layout *L, int n_images, size_t sample_bytes)
{
    size_t total = 0;
    for (int p = 0; p < L->nplanes; ++p) total += align256(plane_samples(L, p) * (size_t)n_images * sample_bytes);
    return total;
}

// The planes of the staged paths in the context's scratch: n_images images of every plane, `sample_bytes` per sample.
int scratch_planes(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, size_t sample_bytes, PlaneSetMut *ps)
{
    size_t offset[JPEG_AMD_MAX_PLANES], total = 0;
    for (int p = 0; p < L->nplanes; ++p) {
        offset[p] = total;
        total += align256(plane_samples(L, p) * (size_t)n_images * sample_bytes);
    }
    JA_TRY(ensure_buffer(ctx, ctx->scratch, total));
    *ps = PlaneSetMut{};
    for (int p = 0; p < L->nplanes; ++p) {
        ps->ptr[p] = static_cast<uint8_t *>(ctx->scratch.ptr) + offset[p];
        ps->stride[p] = plane_samples(L, p);
    }
    return JPEG_AMD_OK;
}

// What the batch entry points of the built-in 8-bit colour formats require, in the order that decides the status of a
// call that is wrong twice (EINVAL against ENOSUP).
int check_batch8(const jpeg_amd_layout *L, int n_images, jpeg_amd_color color)
{
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (L->nplanes != 1 && L->nplanes != 3) return JPEG_AMD_EINVAL;   // built-in colour formats
    if (L->precision != 8) return JPEG_AMD_ENOSUP;                   // JPEG.Common is 8-bit
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// A decoded frame's layout: its first `nplanes` components, table c for component c.
jpeg_amd_layout layout_of_info(const jpeg_amd_frame_info &fi, int nplanes)
{
    jpeg_amd_layout L{};
    L.width = fi.width; L.height = fi.height; L.precision = fi.precision; L.nplanes = nplanes;
    L.scale_x = fi.scale_x; L.scale_y = fi.scale_y;          // the scale of ALL components (decode.swift:2181-2190)
    for (int c = 0; c < nplanes; ++c) {
        L.factor_x[c] = fi.factor_x[c]; L.factor_y[c] = fi.factor_y[c];
        L.units_x[c] = fi.units_x[c];   L.units_y[c] = fi.units_y[c];
        L.qi[c] = c;
    }
    return L;
}

// The layout of a frame to be encoded: scale and units from its factors (both written back into the frame), each
// component's table found by its key.  Precision and component count are the caller's to check.
int layout_of_frame(jpeg_amd_frame_info *frame, const int32_t *quanta_key, const int32_t *h_quanta_keys, int ntables,
                    jpeg_amd_layout *L)
{
    if (frame->width < 1 || frame->height < 1 || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    const int nc = frame->ncomponents;
    *L = jpeg_amd_layout{};
    L->width = frame->width; L->height = frame->height; L->precision = frame->precision; L->nplanes = nc;
    L->scale_x = L->scale_y = 1;
    for (int c = 0; c < nc; ++c) {
        if (frame->factor_x[c] < 1 || frame->factor_y[c] < 1) return JPEG_AMD_EINVAL;
        L->factor_x[c] = frame->factor_x[c]; L->factor_y[c] = frame->factor_y[c];
        L->scale_x = std::max(L->scale_x, L->factor_x[c]); L->scale_y = std::max(L->scale_y, L->factor_y[c]);
        L->qi[c] = -1;
        for (int t = 0; t < ntables; ++t) if (h_quanta_keys[t] == quanta_key[c]) L->qi[c] = t;
        if (L->qi[c] < 0) return JPEG_AMD_EINVAL;   // missing quantization table (decode.swift:2527)
    }
    JA_TRY(jpeg_amd_layout_units(L));
    frame->scale_x = L->scale_x; frame->scale_y = L->scale_y;
    for (int c = 0; c < nc; ++c) { frame->units_x[c] = L->units_x[c]; frame->units_y[c] = L->units_y[c]; }
    return JPEG_AMD_OK;
}

}  // namespace capi
}  // namespace jpeg_amd

namespace {

int units_of(int size, int stride) { return size / stride + (size % stride != 0 ? 1 : 0); }

// The staged decode (any factors): IDCT every plane into scratch planes of bytes or halfwords, then upsample + interleave
// (+ colour) into `kind` pixels.
int staged_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const PlaneSet &coef, QuantaRef q, bool cosited,
                  bool planes_u8, PixelKind kind, void *d_out, size_t out_stride_bytes)
{
    PlaneSetMut scratch;
    JA_TRY(scratch_planes(ctx, L, n_images, planes_u8 ? sizeof(uint8_t) : sizeof(uint16_t), &scratch));
    PlaneSet ps{};
    for (int p = 0; p < L->nplanes; ++p) {
        JA_HIP(ctx, launch_idct_plane(ctx->stream, n_images, static_cast<const int16_t *>(coef.ptr[p]), coef.stride[p], q, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, scratch.ptr[p], scratch.stride[p], planes_u8));
        ps.ptr[p] = scratch.ptr[p];
        ps.stride[p] = scratch.stride[p];
    }
    JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, n_images, *L, ps, planes_u8, cosited, kind, d_out, out_stride_bytes));
    return JPEG_AMD_OK;
}

// The staged encode (any factors): decomposed() into uint16 scratch planes, then fdct(quanta:) plane by plane.
int staged_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const void *d_in, size_t in_stride_bytes,
                  PixelKind kind, QuantaRef q, const PlaneSetMut &coef)
{
    PlaneSetMut ps;
    JA_TRY(scratch_planes(ctx, L, n_images, sizeof(uint16_t), &ps));
    JA_HIP(ctx, launch_decompose(ctx->stream, n_images, *L, d_in, in_stride_bytes, kind, ps));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        JA_HIP(ctx, launch_fdct_plane(ctx->stream, n_images, static_cast<const uint16_t *>(ps.ptr[p]), ps.stride[p], q, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, static_cast<int16_t *>(coef.ptr[p]),
                                      coef.stride[p]));
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_version(void) { return JPEG_AMD_VERSION; }

const char *jpeg_amd_strerror(int status)
{
    switch (status) {
        case JPEG_AMD_OK: return "ok";
        case JPEG_AMD_EINVAL: return "invalid argument (violated precondition)";
        case JPEG_AMD_ENOMEM: return "out of memory";
        case JPEG_AMD_EHIP: return "HIP runtime error";
        case JPEG_AMD_ENODEV: return "no such device";
        case JPEG_AMD_ENOSUP: return "not supported";
        default: return "unknown status";
    }
}

int jpeg_amd_device_count(int *count)
{
    if (!count) return JPEG_AMD_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return JPEG_AMD_ENODEV; }
    *count = n;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_create(int device, void *stream, int flags, jpeg_amd_ctx **out)
{
    if (!out) return JPEG_AMD_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return JPEG_AMD_ENODEV;
    jpeg_amd_ctx *ctx = new (std::nothrow) jpeg_amd_ctx();
    if (!ctx) return JPEG_AMD_ENOMEM;
    ctx->device = device;
    ctx->flags = flags;
    int status = JPEG_AMD_OK;
    do {
        if (hipSetDevice(device) != hipSuccess) { status = JPEG_AMD_ENODEV; break; }
        if (flags & JPEG_AMD_CTX_OWN_STREAM) {
            if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
            ctx->own_stream = true;
        } else {
            ctx->stream = static_cast<hipStream_t>(stream);  // NULL = the default stream
        }
        if (hipEventCreate(&ctx->ev_begin) != hipSuccess || hipEventCreate(&ctx->ev_end) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_qstage), kQSlots * kQSlotElems * sizeof(uint16_t)) != hipSuccess) { status = JPEG_AMD_ENOMEM; break; }
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_walk), 256) != hipSuccess) { status = JPEG_AMD_ENOMEM; break; }
        if (hipMemset(ctx->d_walk, 0, 256) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
    } while (0);
    if (status != JPEG_AMD_OK) {
        jpeg_amd_ctx_destroy(ctx);
        return status;
    }
    *out = ctx;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_destroy(jpeg_amd_ctx *ctx)
{
    if (!ctx) return JPEG_AMD_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->workers.reset();
    ctx->copiers.reset();
    for (DeviceBuffer *buf : {&ctx->scratch, &ctx->region, &ctx->resize_src, &ctx->resize_rec, &ctx->mixed, &ctx->tensor_px, &ctx->expand,
                              &ctx->file_planes, &ctx->entropy})
        if (buf->ptr) (void)hipFree(buf->ptr);
    for (hipEvent_t ev : ctx->entropy_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->d_qstage) (void)hipFree(ctx->d_qstage);
    if (ctx->d_walk) (void)hipFree(ctx->d_walk);
    if (ctx->d_flag) (void)hipFree(ctx->d_flag);
    for (int i = 0; i < 2; ++i) {
        if (ctx->file_pinned[i]) (void)hipHostFree(ctx->file_pinned[i]);
        if (ctx->file_done[i]) (void)hipEventDestroy(ctx->file_done[i]);
        if (ctx->file_decoded[i]) (void)hipEventDestroy(ctx->file_decoded[i]);
        if (ctx->file_fetched[i]) (void)hipEventDestroy(ctx->file_fetched[i]);
    }
    if (ctx->file_d2h) (void)hipStreamDestroy(ctx->file_d2h);
    if (ctx->file_device) (void)hipFree(ctx->file_device);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_synchronize(jpeg_amd_ctx *ctx)
{
    JA_TRY(bind(ctx));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_last_hip_error(const jpeg_amd_ctx *ctx) { return ctx ? ctx->last_hip : 0; }

int jpeg_amd_layout_units(jpeg_amd_layout *L)
{
    if (!L || L->nplanes < 1 || L->nplanes > JPEG_AMD_MAX_PLANES || L->scale_x < 1 ||
        L->scale_y < 1 || L->width <= 0 || L->height <= 0)
        return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p) {
        if (L->factor_x[p] < 1 || L->factor_y[p] < 1) return JPEG_AMD_EINVAL;
        L->units_x[p] = units_of(L->width * L->factor_x[p], 8 * L->scale_x);
        L->units_y[p] = units_of(L->height * L->factor_y[p], 8 * L->scale_y);
    }
    return JPEG_AMD_OK;
}

// ---- memory + timing --------------------------------------------------------------------

int jpeg_amd_malloc(jpeg_amd_ctx *ctx, size_t bytes, void **d_ptr)
{
    JA_TRY(bind(ctx));
    if (!d_ptr) return JPEG_AMD_EINVAL;
    *d_ptr = nullptr;
    if (bytes == 0) return JPEG_AMD_OK;
    JA_HIP(ctx, hipMalloc(d_ptr, bytes));
    return JPEG_AMD_OK;
}

int jpeg_amd_free(jpeg_amd_ctx *ctx, void *d_ptr)
{
    JA_TRY(bind(ctx));
    if (!d_ptr) return JPEG_AMD_OK;
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    JA_HIP(ctx, hipFree(d_ptr));
    return JPEG_AMD_OK;
}

int jpeg_amd_memcpy_h2d(jpeg_amd_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    JA_TRY(bind(ctx));
    if (bytes == 0) return JPEG_AMD_OK;
    if (!d_dst || !h_src) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_memcpy_d2h(jpeg_amd_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    JA_TRY(bind(ctx));
    if (bytes == 0) return JPEG_AMD_OK;
    if (!h_dst || !d_src) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_timer_begin(jpeg_amd_ctx *ctx)
{
    JA_TRY(bind(ctx));
    JA_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_timer_end(jpeg_amd_ctx *ctx, float *elapsed_ms)
{
    JA_TRY(bind(ctx));
    if (!elapsed_ms) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
    // poll instead of sleeping on the event: a blocked host thread takes tens of microseconds to wake up, which a caller
    // that brackets a short timed region with its own clock would charge to the region
    // -- but only for a bounded time (200 us): a long region (the PCIe-bound file paths, a rank per core) must not burn a host
    // core, so after that the thread sleeps on the event like everybody else
    hipError_t q = hipErrorNotReady;
    const auto give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
    while ((q = hipEventQuery(ctx->ev_end)) == hipErrorNotReady && std::chrono::steady_clock::now() < give_up) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (q == hipErrorNotReady) q = hipEventSynchronize(ctx->ev_end);
    JA_HIP(ctx, q);
    JA_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev_begin, ctx->ev_end));
    return JPEG_AMD_OK;
}

// ---- decode stages ----------------------------------------------------------------------

int jpeg_amd_idct_plane(jpeg_amd_ctx *ctx, const int16_t *d_coef, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision, uint16_t *d_plane)
{
    JA_TRY(bind(ctx));
    if (units_x < 0 || units_y < 0 || precision < 1 || precision > 16) return JPEG_AMD_EINVAL;
    if ((long long)units_x * units_y > (1LL << 30)) return JPEG_AMD_EINVAL;
    if (units_x == 0 || units_y == 0) return JPEG_AMD_OK;
    if (!d_coef || !d_plane) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta_zigzag, 1, &d_q));
    JA_HIP(ctx, launch_idct_plane(ctx->stream, 1, d_coef, 0, QuantaRef{d_q, 0}, 0, units_x,
                                  units_y, precision, d_plane, 0, false));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                           const int16_t *const d_coef[], const uint16_t *h_quanta, int ntables,
                           uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!d_coef || !d_planes) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        if (!d_coef[p] || !d_planes[p]) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, launch_idct_plane(ctx->stream, 1, d_coef[p], 0, QuantaRef{d_q, 0}, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, d_planes[p],
                                      0, false));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                const uint16_t *const d_planes[], int cosited, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    if (!d_planes || !d_rect) return JPEG_AMD_EINVAL;
    PlaneSet ps;
    JA_TRY(plane_set(L, d_planes, nullptr, true, &ps));
    JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, 1, *L, ps, false, cosited != 0,
                                        PixelKind::Rect16, d_rect, 0));
    return JPEG_AMD_OK;
}

int jpeg_amd_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *d_rect, size_t npixels,
                                int nplanes, jpeg_amd_color color, uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    if (npixels == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_pixels) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, launch_unpack(ctx->stream, d_rect, npixels, nplanes, color, d_pixels));
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                          const int16_t *const d_coef[], const size_t coef_stride[],
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int cosited, jpeg_amd_color color, uint8_t *d_pixels,
                          size_t pixel_stride)
{
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs));
    const QuantaRef q = c.quanta();
    const bool rgb = c.rgb();
    if (fused_decode_supported(*L, cosited != 0)) {
        JA_HIP(ctx, launch_fused_decode(ctx->stream, n_images, *L, cs, q, rgb, ctx->d_walk, d_pixels, pixel_stride));
        return JPEG_AMD_OK;
    }
    return staged_decode(ctx, L, n_images, cs, q, cosited != 0, true, rgb ? PixelKind::RGB8 : PixelKind::YCC8, d_pixels, pixel_stride);
}

int jpeg_amd_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                    const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                    uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, d_pixels, 0);
}

int jpeg_amd_spectral_expand_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const uint32_t *d_desc,
                                   size_t desc_stride, const uint32_t *d_entries, size_t entries_stride, const uint8_t *d_skip,
                                   int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_desc || !d_entries || !d_coef || !coef_stride) return JPEG_AMD_EINVAL;
    JA_TRY(check_sparse_blocks(*L));
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, true, &cs));
    JA_HIP(ctx, launch_expand_sparse(ctx->stream, n_images, *L, d_desc, desc_stride, d_entries, entries_stride, d_skip, cs));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_sparsify_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const int16_t *const d_coef[],
                                     const size_t coef_stride[], uint32_t *d_desc, size_t desc_stride, uint32_t *d_entries,
                                     size_t entries_stride, uint32_t capacity, uint32_t *d_count)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef || !coef_stride || !d_desc || !d_entries || !d_count) return JPEG_AMD_EINVAL;
    // (the stricter of the two limits: a frame that check_sparse_blocks refuses is refused here)
    if (!sparsify_count_fits(sparse_budget(*L).blocks)) return JPEG_AMD_EINVAL;   // d_count[i] would not be the entry count
    PlaneSet cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, true, &cs));
    JA_HIP(ctx, launch_sparsify(ctx->stream, n_images, *L, cs, d_desc, desc_stride, d_entries, entries_stride, capacity, d_count));
    return JPEG_AMD_OK;
}

namespace jpeg_amd {
namespace capi {

// What jpeg_amd_spectral_expand_mixed requires of one item; *groups: the workgroups it takes.
int check_expand_item(const jpeg_amd_expand_item &it, uint64_t *groups)
{
    JA_TRY(check_layout(&it.layout, -1));
    if (it.head != 1 && it.head != 4 && it.head != 8) return JPEG_AMD_EINVAL;
    for (int p = 0; p < it.layout.nplanes; ++p) {
        if (!it.d_coef[p] || reinterpret_cast<uintptr_t>(it.d_coef[p]) % 16 != 0) return JPEG_AMD_EINVAL;
        const jpeg_amd_region &w = it.window[p];
        if (w.x < 0 || w.y < 0 || w.width < 0 || w.height < 0) return JPEG_AMD_EINVAL;
        if ((long long)w.x + w.width > it.layout.units_x[p] || (long long)w.y + w.height > it.layout.units_y[p]) return JPEG_AMD_EINVAL;
    }
    JA_TRY(check_sparse_blocks(it.layout));
    *groups = expand_mixed_groups(it);
    return JPEG_AMD_OK;
}

}  // namespace capi
}  // namespace jpeg_amd

int jpeg_amd_spectral_expand_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_expand_item *h_items, const uint32_t *d_records)
try {
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    if (!h_items || !d_records) return JPEG_AMD_EINVAL;
    // staged in one copy: the item records [n], then the prefix of their workgroups [n + 1]
    const size_t n = (size_t)n_images, rec_bytes = expand_mixed_record_bytes();
    std::vector<uint8_t> buf(rec_bytes * n + 4 * (n + 1));
    uint64_t acc = 0;
    for (size_t i = 0; i < n; ++i) {
        uint64_t groups = 0;
        JA_TRY(check_expand_item(h_items[i], &groups));
        expand_mixed_record(buf.data() + rec_bytes * i, h_items[i]);
        const uint32_t before = (uint32_t)acc;
        std::memcpy(buf.data() + rec_bytes * n + 4 * i, &before, 4);
        acc += groups;
        if (acc > 0x7fffffffu) return JPEG_AMD_EINVAL;     // more workgroups than a grid holds
    }
    const uint32_t nwg = (uint32_t)acc;
    std::memcpy(buf.data() + rec_bytes * n + 4 * n, &nwg, 4);
    JA_TRY(bind(ctx));
    JA_TRY(ensure_buffer(ctx, ctx->expand, buf.size()));
    // (from a pageable host buffer, so the copy has taken it when the call returns -- as stage_quanta)
    JA_HIP(ctx, hipMemcpyAsync(ctx->expand.ptr, buf.data(), buf.size(), hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *d = static_cast<const uint8_t *>(ctx->expand.ptr);
    JA_HIP(ctx, launch_expand_mixed(ctx->stream, n_images, d, reinterpret_cast<const uint32_t *>(d + rec_bytes * n), nwg, d_records));
    return JPEG_AMD_OK;
}
JA_NOTHROW_TAIL

int jpeg_amd_spectral_rectangular_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, uint16_t *d_rect, size_t rect_stride)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_planes_cover_image(L));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef || !coef_stride || !d_quanta || !d_rect) return JPEG_AMD_EINVAL;
    PlaneSet cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, true, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    if (generic_fused_supported(*L)) {
        JA_HIP(ctx, launch_generic_fused(ctx->stream, n_images, *L, cs, q, cosited != 0,
                                         ctx->d_walk ? ctx->d_walk + 16 : nullptr, d_rect, rect_stride));   // (dword 16: the 4:2:0 walk owns dword 0)
        return JPEG_AMD_OK;
    }
    return staged_decode(ctx, L, n_images, cs, q, cosited != 0, false, PixelKind::Rect16, d_rect, rect_stride * sizeof(uint16_t));
}

int jpeg_amd_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                                  const uint16_t *h_quanta, int ntables, int cosited, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_spectral_rectangular_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, d_rect, 0);
}

// ---- encode stages ----------------------------------------------------------------------

int jpeg_amd_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *d_pixels, size_t npixels,
                              int nplanes, jpeg_amd_color color, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    if (npixels == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_pixels) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, launch_pack(ctx->stream, d_pixels, npixels, nplanes, color, d_rect));
    return JPEG_AMD_OK;
}

int jpeg_amd_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                    const uint16_t *d_rect, uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!d_rect || !d_planes) return JPEG_AMD_EINVAL;
    PlaneSetMut ps;
    JA_TRY(plane_set(L, d_planes, nullptr, false, &ps));
    JA_HIP(ctx, launch_decompose(ctx->stream, 1, *L, d_rect, 0, PixelKind::Rect16, ps));
    return JPEG_AMD_OK;
}

int jpeg_amd_fdct_plane(jpeg_amd_ctx *ctx, const uint16_t *d_plane, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision, int16_t *d_coef)
{
    JA_TRY(bind(ctx));
    if (units_x < 0 || units_y < 0 || precision < 1 || precision > 16) return JPEG_AMD_EINVAL;
    if ((long long)units_x * units_y > (1LL << 30)) return JPEG_AMD_EINVAL;
    if (units_x == 0 || units_y == 0) return JPEG_AMD_OK;
    if (!d_coef || !d_plane) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta_zigzag, 1, &d_q));
    JA_HIP(ctx, launch_fdct_plane(ctx->stream, 1, d_plane, 0, QuantaRef{d_q, 0}, 0, units_x,
                                  units_y, precision, d_coef, 0));
    return JPEG_AMD_OK;
}

int jpeg_amd_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                         const uint16_t *const d_planes[], const uint16_t *h_quanta, int ntables,
                         int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!d_coef || !d_planes) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        if (!d_coef[p] || !d_planes[p]) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, launch_fdct_plane(ctx->stream, 1, d_planes[p], 0, QuantaRef{d_q, 0}, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, d_coef[p], 0));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_encode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                          const uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_color color,
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_batch8(L, n_images, color));
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef || !coef_stride || !d_quanta || !d_pixels) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, false, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    const bool rgb = color == JPEG_AMD_COLOR_RGB8;
    if (fused_encode_supported(*L)) {
        JA_HIP(ctx, launch_fused_encode(ctx->stream, n_images, *L, d_pixels, pixel_stride, rgb, q, cs));
        return JPEG_AMD_OK;
    }
    return staged_encode(ctx, L, n_images, d_pixels, pixel_stride, rgb ? PixelKind::RGB8 : PixelKind::YCC8, q, cs);
}

int jpeg_amd_rectangular_spectral_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const uint16_t *d_rect,
                                        size_t rect_stride, const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_quanta || !d_coef || !coef_stride) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, false, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    if (generic_encode_supported(*L)) {
        JA_HIP(ctx, launch_generic_encode(ctx->stream, n_images, *L, d_rect, rect_stride, q, cs));
        return JPEG_AMD_OK;
    }
    return staged_encode(ctx, L, n_images, d_rect, rect_stride * sizeof(uint16_t), PixelKind::Rect16, q, cs);
}

int jpeg_amd_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint16_t *d_rect,
                                  const uint16_t *h_quanta, int ntables, int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_rectangular_spectral_batch(ctx, L, 1, d_rect, 0, d_q, 0, ntables, d_coef, kOneImage);
}

int jpeg_amd_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint8_t *d_pixels,
                    jpeg_amd_color color, const uint16_t *h_quanta, int ntables,
                    int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_encode_batch(ctx, L, 1, d_pixels, 0, color, d_q, 0, ntables, d_coef, kOneImage);
}
