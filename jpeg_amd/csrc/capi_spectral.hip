// capi_spectral.hip -- the C ABI, coefficient-domain unit: the lossless transforms and the spectral reduce on planes in
// device memory (their file-to-file forms are in capi_file.hip).
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

// ---- lossless spectral transforms: rotate, flip, crop, requantise (examples/rotate, examples/recompress) ------------------
namespace {

// whether the op mirrors the SOURCE's x / y axis (FLIP_H / FLIP_V act in the output frame, after the transpose)
bool mirrors_source_x(int op) { return (op & JPEG_AMD_XFORM_TRANSPOSE) ? (op & JPEG_AMD_XFORM_FLIP_V) : (op & JPEG_AMD_XFORM_FLIP_H); }
bool mirrors_source_y(int op) { return (op & JPEG_AMD_XFORM_TRANSPOSE) ? (op & JPEG_AMD_XFORM_FLIP_H) : (op & JPEG_AMD_XFORM_FLIP_V); }

// The output layout and, per plane, the region's origin in that plane's blocks.
struct TransformPlan {
    jpeg_amd_layout out;
    int ox[JPEG_AMD_MAX_PLANES], oy[JPEG_AMD_MAX_PLANES];
};

int plan_transform(const jpeg_amd_layout *in, int op, const jpeg_amd_region *region, TransformPlan *tp)
{
    JA_TRY(check_layout(in, -1));
    if (op < 0 || op > 7) return JPEG_AMD_EINVAL;
    const jpeg_amd_region r = region ? *region : jpeg_amd_region{0, 0, in->width, in->height};
    const int mx = 8 * in->scale_x, my = 8 * in->scale_y;
    if (r.x < 0 || r.y < 0 || r.x >= in->width || r.y >= in->height || r.x % mx || r.y % my) return JPEG_AMD_EINVAL;
    if (r.width <= 0 || r.height <= 0) return JPEG_AMD_EINVAL;
    // Spectral.set(width:) / set(height:) from the region's origin, then the example's trim of the edges that the op moves
    // to the top or left (examples/rotate/main.swift: set(width: size.x - size.x % (8 * scale.x)))
    jpeg_amd_layout c = *in;
    c.width = r.width;
    c.height = r.height;
    if (mirrors_source_x(op)) c.width -= c.width % mx;
    if (mirrors_source_y(op)) c.height -= c.height % my;
    if (c.width <= 0 || c.height <= 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout o = c;
    if (op & JPEG_AMD_XFORM_TRANSPOSE) {
        o.width = c.height; o.height = c.width;
        o.scale_x = c.scale_y; o.scale_y = c.scale_x;
        for (int p = 0; p < c.nplanes; ++p) { o.factor_x[p] = c.factor_y[p]; o.factor_y[p] = c.factor_x[p]; }
    }
    JA_TRY(jpeg_amd_layout_units(&o));
    for (int p = 0; p < c.nplanes; ++p) {
        if ((long long)o.units_x[p] * o.units_y[p] > (1LL << 30)) return JPEG_AMD_EINVAL;
        tp->ox[p] = r.x / mx * in->factor_x[p];
        tp->oy[p] = r.y / my * in->factor_y[p];
    }
    tp->out = o;
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_transform_layout(const jpeg_amd_layout *in, int op, const jpeg_amd_region *region, jpeg_amd_layout *out)
{
    if (!in || !out) return JPEG_AMD_EINVAL;
    TransformPlan tp;
    JA_TRY(plan_transform(in, op, region, &tp));
    *out = tp.out;
    return JPEG_AMD_OK;
}

int jpeg_amd_transform_quanta(int op, const uint16_t in[64], uint16_t out[64])
{
    if (!in || !out || op < 0 || op > 7) return JPEG_AMD_EINVAL;
    uint16_t t[64];
    for (int z = 0; z < 64; ++z) t[z] = in[xform_source(op, z)];
    std::memcpy(out, t, sizeof t);
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_transform_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, int op,
                                      const jpeg_amd_region *region, const int16_t *const d_coef_in[], const size_t in_stride[],
                                      const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                      const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[],
                                      int32_t *d_overflow)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, d_quanta_out ? ntables : -1));
    if (d_quanta_out && (ntables < 1 || ntables > JPEG_AMD_MAX_PLANES)) return JPEG_AMD_EINVAL;
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    TransformPlan tp;
    JA_TRY(plan_transform(L, op, region, &tp));
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef_in || !in_stride || !d_coef_out || !out_stride || (d_quanta_out && !d_quanta)) return JPEG_AMD_EINVAL;
    PlaneSet cin;
    PlaneSetMut cout;
    JA_TRY(plane_set(L, d_coef_in, in_stride, false, &cin));
    JA_TRY(plane_set(L, d_coef_out, out_stride, true, &cout));
    JA_HIP(ctx, launch_transform(ctx->stream, n_images, op, *L, tp.out, tp.ox, tp.oy, cin, QuantaRef{d_quanta, quanta_stride},
                                 d_quanta_out, cout, d_overflow));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_transform(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int op, const jpeg_amd_region *region,
                                const int16_t *const d_coef_in[], const uint16_t *h_quanta, int ntables,
                                const uint16_t *h_quanta_out, int16_t *const d_coef_out[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr, *d_qo = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    if (h_quanta_out) JA_TRY(stage_quanta(ctx, h_quanta_out, ntables, &d_qo));
    if (!ctx->d_flag) JA_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_flag), 256));
    JA_HIP(ctx, hipMemsetAsync(ctx->d_flag, 0, sizeof(int32_t), ctx->stream));
    JA_TRY(jpeg_amd_spectral_transform_batch(ctx, L, 1, op, region, d_coef_in, kOneImage, d_q, 0, ntables, d_qo, d_coef_out, kOneImage,
                                             ctx->d_flag));
    int32_t flag = 0;
    JA_HIP(ctx, hipMemcpyAsync(&flag, ctx->d_flag, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return flag ? JPEG_AMD_EINVAL : JPEG_AMD_OK;
}

// ---- spectral reduce: 1/2, 1/4, 1/8 size, coefficients in and out (include/jpeg_amd.h, "spectral reduce") ---------------
// N = 8 / denom for a denom of the reduce contract, else 0.
int jpeg_amd::capi::reduce_n(int denom) { return denom == 2 || denom == 4 || denom == 8 ? 8 / denom : 0; }

namespace {

// A zero divisor among the tables the planes of L use.
bool has_zero_quantum(const jpeg_amd_layout *L, const uint16_t *h_tables)
{
    for (int p = 0; p < L->nplanes; ++p)
        for (int z = 0; z < 64; ++z)
            if (h_tables[64 * L->qi[p] + z] == 0) return true;
    return false;
}

}  // namespace

int jpeg_amd_reduce_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out)
{
    if (!out) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(in, -1));
    const int n = reduce_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout r = *in;
    r.width = (int32_t)(((long long)in->width * n + 7) / 8);
    r.height = (int32_t)(((long long)in->height * n + 7) / 8);
    JA_TRY(jpeg_amd_layout_units(&r));
    *out = r;
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_reduce_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, int denom,
                                   const int16_t *const d_coef_in[], const size_t in_stride[],
                                   const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                   const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    const int n = reduce_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout O;
    JA_TRY(jpeg_amd_reduce_layout(L, denom, &O));
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) == 0) return JPEG_AMD_EINVAL;      // no block whose edge could be replicated
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef_in || !in_stride || !d_coef_out || !out_stride || !d_quanta) return JPEG_AMD_EINVAL;
    PlaneSet cin;
    PlaneSetMut cout;
    JA_TRY(plane_set(L, d_coef_in, in_stride, true, &cin));
    JA_TRY(plane_set(L, d_coef_out, out_stride, true, &cout));
    for (int p = 0; p < L->nplanes; ++p) {
        if (n_images > 1 && out_stride[p] < plane_samples(&O, p)) return JPEG_AMD_EINVAL;      // the images' outputs would overlap
        // the kernel loads and stores 16-byte pieces: every block of every image starts on a 16-byte boundary
        if (reinterpret_cast<uintptr_t>(d_coef_in[p]) % 16 || reinterpret_cast<uintptr_t>(d_coef_out[p]) % 16) return JPEG_AMD_EINVAL;
        if (n_images > 1 && (in_stride[p] % 8 || out_stride[p] % 8)) return JPEG_AMD_EINVAL;
    }
    JA_HIP(ctx, launch_spectral_reduce(ctx->stream, n_images, n, *L, O, cin, QuantaRef{d_quanta, quanta_stride}, d_quanta_out, cout));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_reduce(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int denom, const int16_t *const d_coef_in[],
                             const uint16_t *h_quanta, int ntables, const uint16_t *h_quanta_out, int16_t *const d_coef_out[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (reduce_n(denom) == 0 || !h_quanta || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (has_zero_quantum(L, h_quanta_out ? h_quanta_out : h_quanta)) return JPEG_AMD_EINVAL;
    if (!d_coef_in || !d_coef_out) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) == 0 || !d_coef_in[p] || !d_coef_out[p]) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr, *d_qo = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    if (h_quanta_out) JA_TRY(stage_quanta(ctx, h_quanta_out, ntables, &d_qo));
    JA_TRY(jpeg_amd_spectral_reduce_batch(ctx, L, 1, denom, d_coef_in, kOneImage, d_q, 0, ntables, d_qo, d_coef_out, kOneImage));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}
