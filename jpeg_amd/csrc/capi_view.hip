// capi_view.hip -- the C ABI, view unit: region, scaled and view decode, the resample route and its targets (resized,
// tensor, filter), and the mixed calls.
#pragma clang fp contract(off)

#include "capi_internal.hpp"
#include "orient.hpp"
#include "resample_chunks.hpp"
#include "tile_staging.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace {

// A pixel region of jpeg_amd_decode_region_batch / jpeg_amd_region_window: inside the image, not empty.
int check_region(const jpeg_amd_layout *L, const jpeg_amd_region &r)
{
    if (r.x < 0 || r.y < 0 || r.width <= 0 || r.height <= 0) return JPEG_AMD_EINVAL;
    if ((long long)r.x + r.width > L->width || (long long)r.y + r.height > L->height) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

bool whole_image(const jpeg_amd_layout *L, const jpeg_amd_region &r)
{
    return r.x == 0 && r.y == 0 && r.width == L->width && r.height == L->height;
}

// `buf` into the context's region buffer (grown on demand), one copy from a host buffer (pageable, so the copy has taken
// it when the call returns -- as stage_quanta).
int upload_regions(jpeg_amd_ctx *ctx, const std::vector<uint32_t> &buf)
{
    const size_t bytes = 4 * buf.size();
    JA_TRY(ensure_buffer(ctx, ctx->region, bytes));
    JA_HIP(ctx, hipMemcpyAsync(ctx->region.ptr, buf.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    return JPEG_AMD_OK;
}

// The rectangles of the call's views as the payload of what is staged for it (tile_staging.hpp); room for `groups` groups.
TileStaging stage_rects(const jpeg_amd_view *h_views, size_t n, size_t groups)
{
    TileStaging st(n, sizeof(jpeg_amd_region), groups);
    for (size_t i = 0; i < n; ++i) st.rect(i, h_views[i].region);
    return st;
}

// A launch of `kernel` for images of the call c at n samples per block: everything but what is staged.
TileLaunch tile_launch(TileKernel kernel, const DecodeCall &c, const PlaneSet &cs, int n)
{
    TileLaunch l{};
    l.kernel = kernel;
    l.n = n;
    l.nplanes = c.L->nplanes;
    l.rgb = c.rgb();
    l.layout = c.L;
    l.coef = cs;
    l.q = c.quanta();
    l.d_pixels = c.d_pixels;
    l.pixel_stride = c.pixel_stride;
    return l;
}

// ... and what is staged for it: group g of the words that were uploaded to d_words.
void staged(TileLaunch &l, const void *d_words, const TileGroup &g)
{
    const uint32_t *w = static_cast<const uint32_t *>(d_words);
    l.n_images = g.n_images;
    l.d_payload = d_words;
    l.d_index = w + g.index;
    l.d_tiles = w + g.tiles;
    l.nwg = g.nwg;
}

constexpr size_t kFallbackChunkBytes = (size_t)1 << 30;   // scratch per chunk of a fallback's whole-image decodes or planes

constexpr int kViewDenoms = 4;   // slot k: denom 1 << k
int view_slot(int denom) { return denom == 1 ? 0 : denom == 2 ? 1 : denom == 4 ? 2 : denom == 8 ? 3 : -1; }

// The region and the view call's fallback for the layouts without a tile kernel: the whole scaled images of a run of
// consecutive images of one denominator into scratch behind the staged paths' planes (S's planes are no larger than L's),
// then one crop launch; a run is at most a chunk.  S[k]: the image at denominator 1 << k, for every k among the views.
int crop_fallback(jpeg_amd_ctx *ctx, const DecodeCall &c, const jpeg_amd_view *h_views, const jpeg_amd_layout S[kViewDenoms])
{
    const jpeg_amd_layout *L = c.L;
    const int n_images = c.n_images;
    const size_t n = (size_t)n_images;
    size_t full_max = 0;
    for (size_t i = 0; i < n; ++i) {
        const jpeg_amd_layout &Si = S[view_slot(h_views[i].denom)];
        full_max = std::max(full_max, (size_t)3 * Si.width * Si.height);
    }
    const size_t per_image = full_max + scratch_planes_bytes(L, 1, sizeof(uint8_t));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(n, kFallbackChunkBytes / per_image));
    const size_t planes_bytes = scratch_planes_bytes(L, chunk, sizeof(uint8_t));
    JA_TRY(ensure_buffer(ctx, ctx->scratch, planes_bytes + align256(full_max * chunk)));
    uint8_t *d_full = static_cast<uint8_t *>(ctx->scratch.ptr) + planes_bytes;   // the staged paths' planes stay below it
    JA_TRY(upload_regions(ctx, stage_rects(h_views, n, 0).words));
    const int32_t *d_regions = static_cast<const int32_t *>(ctx->region.ptr);
    for (int i0 = 0; i0 < n_images;) {
        const int denom = h_views[i0].denom;
        const jpeg_amd_layout &Sd = S[view_slot(denom)];
        int m = 0;
        size_t max_bytes = 0;
        for (; i0 + m < n_images && m < chunk && h_views[i0 + m].denom == denom; ++m)
            max_bytes = std::max(max_bytes, (size_t)3 * h_views[i0 + m].region.width * h_views[i0 + m].region.height);
        const size_t full = (size_t)3 * Sd.width * Sd.height;
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall run = c.images(i0, m, coef);
        JA_TRY(jpeg_amd_decode_scaled_batch(ctx, L, m, coef, c.coef_stride, run.d_quanta, c.quanta_stride, c.ntables, c.cosited, c.color,
                                            denom, d_full, full));
        JA_HIP(ctx, launch_region_crop(ctx->stream, m, d_full, full, Sd.width, d_regions + 4 * (size_t)i0, max_bytes, run.d_pixels,
                                       c.pixel_stride));
        i0 += m;
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_decode_region_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_region *h_regions,
                                 uint8_t *d_pixels, size_t pixel_stride)
try {
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs, h_regions != nullptr));
    bool whole = true;
    for (int i = 0; i < n_images; ++i) {
        JA_TRY(check_region(L, h_regions[i]));
        if (n_images > 1 && pixel_stride < (size_t)3 * h_regions[i].width * h_regions[i].height) return JPEG_AMD_EINVAL;
        whole = whole && whole_image(L, h_regions[i]);
    }
    if (whole)
        return jpeg_amd_decode_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                     d_pixels, pixel_stride);

    // views at denominator 1, where the scaled image is the image
    const size_t n = (size_t)n_images;
    std::vector<jpeg_amd_view> views(n);
    for (size_t i = 0; i < n; ++i) views[i] = jpeg_amd_view{1, h_regions[i]};
    if (fused_decode_supported(*L, cosited != 0)) {
        // staged in one copy: the rectangles [n][4], then the one group of all images in order (its index list is not read)
        TileStaging st = stage_rects(views.data(), n, 1);
        std::vector<uint32_t> all(n);
        for (size_t i = 0; i < n; ++i) all[i] = (uint32_t)i;
        TileGroup g;
        JA_TRY(st.group(all, [&](uint32_t i) { return rect_tiles(8, kRegionTileH, h_regions[i]); }, &g));
        JA_TRY(upload_regions(ctx, st.words));
        TileLaunch l = tile_launch(TileKernel::Region, c, cs, 8);
        staged(l, ctx->region.ptr, g);
        JA_HIP(ctx, launch_tile_decode(ctx->stream, l));
        return JPEG_AMD_OK;
    }

    // the crop fallback
    const jpeg_amd_layout S[kViewDenoms] = {*L};
    return crop_fallback(ctx, c, views.data(), S);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_region(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_region *region, uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!region) return JPEG_AMD_EINVAL;
    JA_TRY(check_region(L, *region));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_region_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, region, d_pixels, 0);
}

int jpeg_amd_region_window(const jpeg_amd_layout *L, int cosited, const jpeg_amd_region *region,
                           jpeg_amd_region windows[JPEG_AMD_MAX_PLANES])
{
    if (!region || !windows) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    JA_TRY(check_region(L, *region));
    const jpeg_amd_region &r = *region;
    for (int p = 0; p < JPEG_AMD_MAX_PLANES; ++p) {
        windows[p] = jpeg_amd_region{0, 0, 0, 0};
        if (p >= L->nplanes) continue;
        int32_t x0, x1, y0, y1;
        axis_span(interleave_axis(*L, p, cosited != 0, false), r.x, r.x + r.width - 1, x0, x1);
        axis_span(interleave_axis(*L, p, cosited != 0, true), r.y, r.y + r.height - 1, y0, y1);
        windows[p] = jpeg_amd_region{x0 >> 3, y0 >> 3, (x1 >> 3) - (x0 >> 3) + 1, (y1 >> 3) - (y0 >> 3) + 1};
    }
    return JPEG_AMD_OK;
}

namespace {

// N = 8 / denom for a denom of the contract, else 0.
int scaled_n(int denom) { return denom == 1 || denom == 2 || denom == 4 || denom == 8 ? 8 / denom : 0; }

// The planes, N x N samples per block, must cover the scaled image as check_planes_cover_image asks of the full-size one:
// with units = ceil(size factor / (8 scale)) they always do (include/jpeg_amd.h has the proof); units given by hand may not.
int check_planes_cover_scaled(const jpeg_amd_layout *L, const jpeg_amd_layout *S, int n)
{
    for (int p = 0; p < L->nplanes; ++p) {
        const long long sx = (long long)n * L->units_x[p], sy = (long long)n * L->units_y[p];
        if (plane_is_direct(*L, p)) {
            if (sx < S->width || sy < S->height) return JPEG_AMD_EINVAL;
        } else {
            if (sx < 1 || sy < 1) return JPEG_AMD_EINVAL;
            if (axis_index(interleave_axis(*L, p, true, false), S->width - 1) >= sx) return JPEG_AMD_EINVAL;
            if (axis_index(interleave_axis(*L, p, true, true), S->height - 1) >= sy) return JPEG_AMD_EINVAL;
        }
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_scaled_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out)
{
    if (!out) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(in, -1));
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout s = *in;
    s.width = (int32_t)(((long long)in->width * n + 7) / 8);
    s.height = (int32_t)(((long long)in->height * n + 7) / 8);
    for (int p = 0; p < in->nplanes; ++p) {
        s.units_x[p] = (int32_t)(((long long)in->units_x[p] * n + 7) / 8);
        s.units_y[p] = (int32_t)(((long long)in->units_y[p] * n + 7) / 8);
    }
    *out = s;
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_scaled_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, int denom,
                                 uint8_t *d_pixels, size_t pixel_stride)
{
    if (denom == 1)
        return jpeg_amd_decode_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                     d_pixels, pixel_stride);
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout S;
    JA_TRY(jpeg_amd_scaled_layout(L, denom, &S));
    JA_TRY(check_planes_cover_scaled(L, &S, n));
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs));
    if (n_images > 1 && pixel_stride < (size_t)3 * S.width * S.height) return JPEG_AMD_EINVAL;
    if (fused_decode_supported(*L, cosited != 0)) {
        TileLaunch l = tile_launch(TileKernel::Scaled, c, cs, n);
        l.width = S.width;
        l.height = S.height;
        l.n_images = n_images;
        JA_HIP(ctx, launch_tile_decode(ctx->stream, l));
        return JPEG_AMD_OK;
    }

    // fallback: every plane N x N per block into byte planes in scratch, padded to S's whole blocks by edge replication, then
    // the staged interleave + colour kernel under S, chunk by chunk
    const size_t per_image = std::max<size_t>(1, scratch_planes_bytes(&S, 1, sizeof(uint8_t)));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_images, kFallbackChunkBytes / per_image));
    PlaneSetMut scratch;
    JA_TRY(scratch_planes(ctx, &S, chunk, sizeof(uint8_t), &scratch));
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int m = std::min(chunk, n_images - i0);
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall part = c.images(i0, m, coef);
        PlaneSet ps{};
        for (int p = 0; p < L->nplanes; ++p) {
            JA_HIP(ctx, launch_idct_scaled_plane(ctx->stream, m, coef[p], coef_stride[p], part.quanta(), L->qi[p], L->units_x[p],
                                                 L->units_y[p], n, L->precision, scratch.ptr[p], scratch.stride[p], true));
            ps.ptr[p] = scratch.ptr[p];
            ps.stride[p] = scratch.stride[p];
        }
        JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, m, S, ps, true, cosited != 0, c.rgb() ? PixelKind::RGB8 : PixelKind::YCC8,
                                            part.d_pixels, pixel_stride));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color, int denom,
                           uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (scaled_n(denom) == 0) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_scaled_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, denom, d_pixels, 0);
}

int jpeg_amd_spectral_idct_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                                  const uint16_t *h_quanta, int ntables, int denom, uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (denom == 1) return jpeg_amd_spectral_idct(ctx, L, d_coef, h_quanta, ntables, d_planes);
    const int n = scaled_n(denom);
    if (n == 0 || !d_coef || !d_planes) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) != 0 && (!d_coef[p] || !d_planes[p])) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p)
        JA_HIP(ctx, launch_idct_scaled_plane(ctx->stream, 1, d_coef[p], 0, QuantaRef{d_q, 0}, L->qi[p], L->units_x[p], L->units_y[p], n,
                                             L->precision, d_planes[p], 0, false));
    return JPEG_AMD_OK;
}

namespace {

// The image at `denom` as the scaled contract defines it: *S is jpeg_amd_scaled_layout's, and the planes cover it.
int scaled_image(const jpeg_amd_layout *L, int denom, jpeg_amd_layout *S)
{
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    JA_TRY(jpeg_amd_scaled_layout(L, denom, S));
    return denom == 1 ? JPEG_AMD_OK : check_planes_cover_scaled(L, S, n);
}

// Every argument of jpeg_amd_decode_view_batch but the context, in the order that decides the status of a call that is wrong
// twice.  S[k] / count[k]: the scaled image and the number of views of denominator 1 << k; *whole: every view a whole image.
int check_views(const DecodeCall &c, const jpeg_amd_view *h_views, jpeg_amd_layout S[kViewDenoms], int count[kViewDenoms], bool *whole,
                PlaneSet *cs)
{
    const jpeg_amd_layout *L = c.L;
    const int n_images = c.n_images;
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    JA_TRY(c.planes(cs, h_views != nullptr));
    for (int i = 0; i < n_images; ++i) {
        const int k = view_slot(h_views[i].denom);
        if (k < 0) return JPEG_AMD_EINVAL;
        if (count[k]++ == 0) JA_TRY(scaled_image(L, h_views[i].denom, &S[k]));
        const jpeg_amd_region &r = h_views[i].region;
        JA_TRY(check_region(&S[k], r));
        if (n_images > 1 && c.pixel_stride < (size_t)3 * r.width * r.height) return JPEG_AMD_EINVAL;
        *whole = *whole && whole_image(&S[k], r);
    }
    return JPEG_AMD_OK;
}

// What jpeg_amd_decode_view and jpeg_amd_decode_resized refuse before a table is staged: check_views for their one view.
int check_one_view(const jpeg_amd_layout *L, int ntables, jpeg_amd_color color, const jpeg_amd_view *view)
{
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_planes_cover_image(L));
    JA_TRY(check_batch8(L, 1, color));
    if (!view) return JPEG_AMD_EINVAL;
    jpeg_amd_layout S;
    JA_TRY(scaled_image(L, view->denom, &S));
    return check_region(&S, view->region);
}

}  // namespace

int jpeg_amd_decode_view_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                               const int16_t *const d_coef[], const size_t coef_stride[],
                               const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                               int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                               uint8_t *d_pixels, size_t pixel_stride)
try {
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(c, h_views, S, count, &whole, &cs));
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;

    const int denom0 = h_views[0].denom;
    if (whole && count[view_slot(denom0)] == n_images)
        return jpeg_amd_decode_scaled_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            denom0, d_pixels, pixel_stride);
    if (count[0] == n_images) {   // every view a region of the full-size image
        std::vector<jpeg_amd_region> regions((size_t)n_images);
        for (int i = 0; i < n_images; ++i) regions[(size_t)i] = h_views[i].region;
        return jpeg_amd_decode_region_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            regions.data(), d_pixels, pixel_stride);
    }

    const size_t n = (size_t)n_images;
    if (fused_decode_supported(*L, cosited != 0)) {
        // staged in one copy: the rectangles [n][4], then per denominator of the call its group
        TileStaging st = stage_rects(h_views, n, kViewDenoms);
        std::vector<uint32_t> members;
        TileGroup group[kViewDenoms];
        for (int k = 0; k < kViewDenoms; ++k) {
            if (count[k] == 0) continue;
            members.clear();
            for (size_t i = 0; i < n; ++i)
                if (view_slot(h_views[i].denom) == k) members.push_back((uint32_t)i);
            JA_TRY(st.group(members, [&](uint32_t i) { return rect_tiles(8 >> k, kViewTileH, h_views[i].region); }, &group[k]));
        }
        JA_TRY(upload_regions(ctx, st.words));
        for (int k = 0; k < kViewDenoms; ++k) {
            if (count[k] == 0) continue;
            TileLaunch l = tile_launch(TileKernel::View, c, cs, 8 >> k);
            staged(l, ctx->region.ptr, group[k]);
            JA_HIP(ctx, launch_tile_decode(ctx->stream, l));
        }
        return JPEG_AMD_OK;
    }

    return crop_fallback(ctx, c, h_views, S);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_view(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                         const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                         const jpeg_amd_view *view, uint8_t *d_pixels)
{
    // as the batch call: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_view_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, d_pixels, 0);
}

int jpeg_amd_view_window(const jpeg_amd_layout *L, int cosited, int denom, const jpeg_amd_region *region,
                         jpeg_amd_region windows[JPEG_AMD_MAX_PLANES])
{
    if (!region || !windows) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    jpeg_amd_layout S;
    JA_TRY(scaled_image(L, denom, &S));
    JA_TRY(check_region(&S, *region));
    const jpeg_amd_region &r = *region;
    const int32_t n = scaled_n(denom);
    for (int p = 0; p < JPEG_AMD_MAX_PLANES; ++p) {
        windows[p] = jpeg_amd_region{0, 0, 0, 0};
        if (p >= L->nplanes) continue;
        InterleaveAxis mx = interleave_axis(*L, p, cosited != 0, false), my = interleave_axis(*L, p, cosited != 0, true);
        mx.last = n * L->units_x[p] - 1;   // the scaled plane's padded edge
        my.last = n * L->units_y[p] - 1;
        int32_t x0, x1, y0, y1;
        axis_span(mx, r.x, r.x + r.width - 1, x0, x1);
        axis_span(my, r.y, r.y + r.height - 1, y0, y1);
        windows[p] = jpeg_amd_region{x0 / n, y0 / n, x1 / n - x0 / n + 1, y1 / n - y0 / n + 1};
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_view_of_source(const jpeg_amd_layout *L, int denom, const jpeg_amd_region *source_region, jpeg_amd_region *region)
{
    if (!source_region || !region) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    const long long n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    JA_TRY(check_region(L, *source_region));
    const jpeg_amd_region &s = *source_region;
    const long long w1 = ((long long)L->width * n + 7) / 8, h1 = ((long long)L->height * n + 7) / 8;
    const long long x0 = s.x * n / 8, x1 = std::min(w1, (((long long)s.x + s.width) * n + 7) / 8);
    const long long y0 = s.y * n / 8, y1 = std::min(h1, (((long long)s.y + s.height) * n + 7) / 8);
    *region = jpeg_amd_region{(int32_t)x0, (int32_t)y0, (int32_t)(x1 - x0), (int32_t)(y1 - y0)};
    return JPEG_AMD_OK;
}

int jpeg_amd_view_denom(int32_t src_w, int32_t src_h, int32_t want_w, int32_t want_h)
{
    for (int denom = 8; denom > 1; denom /= 2) {
        const long long n = 8 / denom;
        if (src_w * n / 8 >= want_w && src_h * n / 8 >= want_h) return denom;
    }
    return 1;
}

namespace {

// The records into the context's record buffer, one copy from a host buffer (pageable, so the copy has taken it when the call
// returns -- as stage_quanta).
int upload_records(jpeg_amd_ctx *ctx, const std::vector<uint8_t> &rec)
{
    JA_TRY(ensure_buffer(ctx, ctx->resize_rec, rec.size()));
    JA_HIP(ctx, hipMemcpyAsync(ctx->resize_rec.ptr, rec.data(), rec.size(), hipMemcpyHostToDevice, ctx->stream));
    return JPEG_AMD_OK;
}

// What both resample calls require of the output.
int check_resize_target(int n_images, int32_t out_w, int32_t out_h, const void *d_dst, size_t dst_stride)
{
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    if (resize_tiles(out_w, out_h) > 0x7fffffffu) return JPEG_AMD_EINVAL;   // more workgroups than a grid holds
    if (n_images > 0 && !d_dst) return JPEG_AMD_EINVAL;
    if (n_images > 1 && dst_stride < (size_t)3 * out_w * out_h) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// What the tensor calls require of the output, beyond jpeg_amd_tensor_extent.
int check_tensor_target(int n_images, int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const void *d_dst,
                        size_t dst_stride, size_t *elem_bytes)
{
    size_t image_elems = 0;
    JA_TRY(jpeg_amd_tensor_extent(spec, out_w, out_h, elem_bytes, &image_elems));
    if (n_images > 0 && !d_dst) return JPEG_AMD_EINVAL;
    if ((uintptr_t)d_dst % *elem_bytes != 0) return JPEG_AMD_EINVAL;
    if (n_images > 1 && dst_stride < image_elems) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// A resample call behind its request (resample_request.hpp): what the caller asked for, and what check() derives of it.  The
// records of a call are bytes on the host, record_bytes() per image, of the kind that check() decides ONCE:
//   Stored    no orientations, or every one of them 1: ResizeRecord for the bilinear kernels, AntialiasRecord for the others
//             (the bicubic filter fills the same one);
//   Oriented  ("oriented resample") some orientation is not 1: every record is the oriented one (orientation 1 included: base =
//             offset, steps 3 and 3 w) and ONE launch of the oriented kernels takes them all;
//   Placed    ("placed resample") a placement: check() judges it with the target, window(i) judges and keeps image i's window
//             (behind its orientation), every record is the placed one of its filter, its scale factors the window's, and ONE
//             launch of the placed kernels takes them all.  Also ("colour stage") a colour without a placement: its window is
//             the whole canvas, which "placed resample" makes the oriented and the stored call bit for bit;
//   Warped, Projected  ("warped resample", "projective resample") a map: bilinear, or ("bicubic warp") the bicubic filter with
//             a projective map; no orientations, no placement; window(i) judges image i's matrix, record(i) writes the
//             WarpRecord or the ProjectRecord -- the same one for either filter.
// With a colour, check() judges it with the target (a byte target has no colour stage), and the ColourRecords go up behind the
// call's resample records, 16-byte aligned, in the same copy.
struct ResampleTarget : ResampleRequest {
    int n_call = 0;   // the images of the call, of which launch() takes a part: check() sets it
    ResampleRecords kind = ResampleRecords::Stored;   // check() sets it
    std::vector<jpeg_amd_region> windows;   // of a call with a placement, per image: check() sizes it, window(i) fills it

    explicit ResampleTarget(const ResampleRequest &rq) : ResampleRequest(rq) {}
    bool bicubic() const { return filter == JPEG_AMD_FILTER_BICUBIC; }
    bool antialias() const { return filter == JPEG_AMD_FILTER_ANTIALIAS || bicubic(); }   // the kernels with tables: their records
    float max_scale() const { return bicubic() ? kBicubicMaxScale : kAntialiasMaxScale; }
    int check(int n_images)
    {
        n_call = std::max(n_images, 0);
        bool turned = false;   // (not a verdict: which records the call writes)
        for (int i = 0; h_orient && i < n_images; ++i) turned = turned || h_orient[i] != 1;
        kind = map == ResampleMap::Projective ? ResampleRecords::Projected
               : map == ResampleMap::Affine   ? ResampleRecords::Warped
               : place || colour              ? ResampleRecords::Placed
               : turned                       ? ResampleRecords::Oriented
                                              : ResampleRecords::Stored;
        if (!has_map() && filter != JPEG_AMD_FILTER_BILINEAR && !antialias()) return JPEG_AMD_EINVAL;
        size_t elem_bytes = 1;
        JA_TRY(tensor ? check_tensor_target(n_images, out_w, out_h, spec, d_dst, stride, &elem_bytes)
                      : check_resize_target(n_images, out_w, out_h, d_dst, stride));
        if (colour) JA_TRY(tensor ? check_colour(*colour, n_images) : JPEG_AMD_EINVAL);
        if (has_map()) {
            // the filter of a map is judged here, with the edge mode: nothing is widened under a map, so no antialiasing
            const bool filtered = filter == JPEG_AMD_FILTER_BILINEAR || (bicubic() && map == ResampleMap::Projective);
            if (!filtered || h_orient || place || !warp) return JPEG_AMD_EINVAL;
            if (warp->edge != JPEG_AMD_EDGE_FILL && warp->edge != JPEG_AMD_EDGE_REPLICATE) return JPEG_AMD_EINVAL;
            return n_images > 0 && !h_matrices ? JPEG_AMD_EINVAL : JPEG_AMD_OK;
        }
        if (!place) return JPEG_AMD_OK;
        JA_TRY(check_placement(*place, n_images));
        windows.assign((size_t)std::max(n_images, 0), jpeg_amd_region{0, 0, 0, 0});
        return JPEG_AMD_OK;
    }
    int orientation(int i) const { return h_orient ? h_orient[i] : 1; }
    // Image i's window, w x h as it is STORED: judged behind its orientation (and behind check()), in front of record(i).
    int window(int i, int32_t w, int32_t h)
    {
        if (has_map() && (w > kWarpMaxSourceSide || h > kWarpMaxSourceSide)) return JPEG_AMD_EINVAL;
        switch (kind) {
        case ResampleRecords::Projected: return check_project_matrix(h_matrices + 9 * (size_t)i, out_w, out_h);
        case ResampleRecords::Warped: return check_warp_matrix(h_matrices + 6 * (size_t)i);
        case ResampleRecords::Placed: if (place) break;   // (a colour alone: the whole canvas)
        default: return JPEG_AMD_OK;
        }
        const OrientedSource s = oriented_source(orientation(i), 0, w, h);
        JA_TRY(placed_window(*place, i, s.w, s.h, out_w, out_h, &windows[(size_t)i]));
        if (h_windows_out) h_windows_out[i] = windows[(size_t)i];
        return JPEG_AMD_OK;
    }
    // Image i's orientation: judged with the image's other arguments, behind them, by the callers.  record(i) comes after it.
    int check_orientation(int i) const { return !h_orient || orientation_valid(h_orient[i]) ? JPEG_AMD_OK : JPEG_AMD_EINVAL; }
    size_t record_bytes() const
    {
        switch (kind) {
        case ResampleRecords::Projected: return sizeof(ProjectRecord);
        case ResampleRecords::Warped: return sizeof(WarpRecord);
        case ResampleRecords::Placed: return antialias() ? sizeof(PlacedAntialiasRecord) : sizeof(PlacedResizeRecord);
        case ResampleRecords::Oriented: return antialias() ? sizeof(OrientedAntialiasRecord) : sizeof(OrientedResizeRecord);
        default: return antialias() ? sizeof(AntialiasRecord) : sizeof(ResizeRecord);
        }
    }
    // Image i of the call, w x h as it is STORED at `offset` bytes from the launch's source.  The scale factors of the
    // contract: divided here, in binary32, never on the device; of an oriented call they are the ORIENTED extent's.
    // ENOSUP: the tap limit of the filter the target carries, kx or ky above kAntialiasMaxScale (the bicubic filter, whose
    // record is the antialiasing one's: kBicubicMaxScale).  The record is written either way, and
    // the caller keeps the verdict of the first such image until everything else of the call has been judged.
    int record(std::vector<uint8_t> &rec, int at, int i, uint64_t offset, int32_t w, int32_t h) const
    {
        const uint32_t flip = h_flip && h_flip[i] ? 1u : 0u;
        if (kind == ResampleRecords::Projected) {
            ProjectRecord r{offset, w, h, {}, flip, warp->edge, 0u};
            std::memcpy(r.m, h_matrices + 9 * (size_t)i, sizeof r.m);
            std::memcpy(rec.data() + (size_t)at * sizeof r, &r, sizeof r);
            return JPEG_AMD_OK;
        }
        if (kind == ResampleRecords::Warped) {
            WarpRecord r{offset, w, h, {}, flip, warp->edge};
            std::memcpy(r.m, h_matrices + 6 * (size_t)i, sizeof r.m);
            std::memcpy(rec.data() + (size_t)at * sizeof r, &r, sizeof r);
            return JPEG_AMD_OK;
        }
        const OrientedSource s = oriented_source(orientation(i), offset, w, h);   // (1: the stored image)
        const jpeg_amd_region win = place ? windows[(size_t)i] : jpeg_amd_region{0, 0, out_w, out_h};   // (placed: the window's factors)
        const float kx = (float)s.w / (float)win.width, ky = (float)s.h / (float)win.height;
        if (!antialias()) {
            PlacedResizeRecord r{};
            static_cast<OrientedResizeRecord &>(r) = OrientedResizeRecord{{s.base, s.w, s.h, kx, ky, flip, 0u}, s.step_x, s.step_y};
            r.x0 = win.x; r.y0 = win.y; r.ww = win.width; r.wh = win.height;
            std::memcpy(rec.data() + (size_t)at * record_bytes(), &r, record_bytes());   // (the plain and the oriented record are its head)
            return JPEG_AMD_OK;
        }
        const float sx = std::max(kx, 1.0f), sy = std::max(ky, 1.0f);
        PlacedAntialiasRecord r{};
        static_cast<OrientedAntialiasRecord &>(r) = OrientedAntialiasRecord{{s.base, s.w, s.h, kx, sx, 1.0f / sx, ky, sy, 1.0f / sy, flip, 0u}, s.step_x, s.step_y};
        r.x0 = win.x; r.y0 = win.y; r.ww = win.width; r.wh = win.height;
        std::memcpy(rec.data() + (size_t)at * record_bytes(), &r, record_bytes());
        return kx > max_scale() || ky > max_scale() ? JPEG_AMD_ENOSUP : JPEG_AMD_OK;
    }
    // What a call of n images uploads: their resample records, then ("colour stage") their ColourRecords at colour_at(n) --
    // image i's twelve numbers as the caller wrote them.
    size_t colour_at(int n) const { return ((size_t)n * record_bytes() + 15) & ~(size_t)15; }
    size_t upload_bytes(int n) const { return colour ? colour_at(n) + (size_t)n * sizeof(ColourRecord) : (size_t)n * record_bytes(); }
    void colour_records(std::vector<uint8_t> &rec, int n) const
    {
        if (colour && n > 0) std::memcpy(rec.data() + colour_at(n), colour->h_matrices, (size_t)n * sizeof(ColourRecord));
    }
    // Images [i0, i0 + m) of the call, from their records: record i0 of d_rec onwards, and ColourRecord i0 of the call's.
    hipError_t launch(hipStream_t stream, int m, const uint8_t *d_src, const void *d_rec, int i0) const
    {
        uint8_t *d_out = static_cast<uint8_t *>(d_dst) + (size_t)i0 * stride * element_bytes();
        const uint8_t *rec = static_cast<const uint8_t *>(d_rec) + (size_t)i0 * record_bytes();
        ResampleLaunch l{filter, kind, tensor ? spec : nullptr, m, d_src, rec, out_w, out_h, d_out, stride, {0, 0, 0}};
        for (int c = 0; place && c < 3; ++c) l.fill[c] = place->fill[c];
        for (int c = 0; has_map() && c < 3; ++c) l.fill[c] = warp->fill[c];
        if (colour) {
            l.d_colour = static_cast<const uint8_t *>(d_rec) + colour_at(n_call) + (size_t)i0 * sizeof(ColourRecord);
            l.lo = colour->lo;
            l.hi = colour->hi;
        }
        return launch_resample(stream, l);
    }
};

// The chunks of the resized and tensor decodes: consecutive images, m images at a stride of the chunk's largest view, at most
// kResizeChunkBytes in all (resample_chunks.hpp holds the rule); rec holds image i's record inside its chunk (the target's kind
// of record); need: the bytes the largest chunk takes; status: what the target's record() says of the first image it refuses.
struct ResizePlan {
    std::vector<ResizeChunk> chunks;
    std::vector<uint8_t> rec;
    size_t need = 0;
    int status = JPEG_AMD_OK;
};
ResizePlan plan_resize_chunks(int n_images, const jpeg_amd_view *h_views, const ResampleTarget &t)
{
    ResizePlan plan;
    plan.rec.resize(t.upload_bytes(n_images));
    t.colour_records(plan.rec, n_images);
    plan.chunks = split_resize_chunks(n_images, h_views);
    for (const ResizeChunk &k : plan.chunks) {
        for (int j = 0; j < k.m; ++j) {
            const jpeg_amd_region &r = h_views[k.i0 + j].region;
            const int verdict = t.record(plan.rec, k.i0 + j, k.i0 + j, (uint64_t)j * k.stride, r.width, r.height);
            if (plan.status == JPEG_AMD_OK) plan.status = verdict;
        }
        plan.need = std::max(plan.need, k.stride * (size_t)k.m);
    }
    return plan;
}

// The route of every resized and tensor decode, behind its checks and on a bound context: chunk by chunk,
// decode(c, chunk, d_views) puts the views of chunk c into the context's buffer at the chunk's stride, and the target's launch
// resamples them from there.
template <typename Decode>
int resample_chunks(jpeg_amd_ctx *ctx, const ResizePlan &plan, const ResampleTarget &t, Decode decode)
{
    JA_TRY(ensure_buffer(ctx, ctx->resize_src, plan.need));
    JA_TRY(upload_records(ctx, plan.rec));
    uint8_t *d_views = static_cast<uint8_t *>(ctx->resize_src.ptr);
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const ResizeChunk &k = plan.chunks[c];
        JA_TRY(decode(c, k, d_views));
        JA_HIP(ctx, t.launch(ctx->stream, k.m, d_views, ctx->resize_rec.ptr, k.i0));
    }
    return JPEG_AMD_OK;
}

// jpeg_amd_resize_batch and jpeg_amd_resize_tensor_batch, and their forms with a filter.
int resize_images(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride, const jpeg_amd_extent *h_extents,
                  const ResampleRequest &rq)
{
    ResampleTarget t(rq);
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    JA_TRY(t.check(n_images));
    std::vector<uint8_t> rec(t.upload_bytes(n_images));
    t.colour_records(rec, n_images);
    int taps = JPEG_AMD_OK;   // the tap limit: judged last, by the first image over it
    if (n_images > 0) {
        if (!d_src || !h_extents) return JPEG_AMD_EINVAL;
        for (int i = 0; i < n_images; ++i) {
            const jpeg_amd_extent &e = h_extents[i];
            if (e.width < 1 || e.height < 1) return JPEG_AMD_EINVAL;
            if (n_images > 1 && src_stride < (size_t)3 * e.width * e.height) return JPEG_AMD_EINVAL;
            JA_TRY(t.check_orientation(i));
            JA_TRY(t.window(i, e.width, e.height));
            const int verdict = t.record(rec, i, i, (uint64_t)i * src_stride, e.width, e.height);
            if (taps == JPEG_AMD_OK) taps = verdict;
        }
    }
    JA_TRY(taps);
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;
    JA_TRY(upload_records(ctx, rec));
    JA_HIP(ctx, t.launch(ctx->stream, n_images, d_src, ctx->resize_rec.ptr, 0));
    return JPEG_AMD_OK;
}

// jpeg_amd_decode_resized_batch and jpeg_amd_decode_tensor_batch, and their forms with a filter; c.d_pixels is t.d_dst, and its stride is not looked at.
int decode_resampled(jpeg_amd_ctx *ctx, const DecodeCall &c, const jpeg_amd_view *h_views, const ResampleRequest &rq)
{
    ResampleTarget t(rq);
    // everything the view call refuses is refused here, before its first chunk is enqueued (the intermediate's stride is
    // ours and always large enough), then what the target refuses
    DecodeCall views = c;
    views.pixel_stride = ~(size_t)0;
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(views, h_views, S, count, &whole, &cs));
    JA_TRY(t.check(c.n_images));
    const ResizePlan plan = plan_resize_chunks(c.n_images, h_views, t);
    JA_TRY(plan.status);
    JA_TRY(bind(ctx));
    if (c.n_images == 0) return JPEG_AMD_OK;
    return resample_chunks(ctx, plan, t, [&](size_t, const ResizeChunk &k, uint8_t *d_views) {
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall part = c.images(k.i0, k.m, coef);
        return jpeg_amd_decode_view_batch(ctx, c.L, k.m, coef, c.coef_stride, part.d_quanta, c.quanta_stride, c.ntables, c.cosited,
                                          c.color, h_views + k.i0, d_views, k.stride);
    });
}

}  // namespace

int jpeg_amd_resize_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                          const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride)
{
    return jpeg_amd_resize_filter_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, JPEG_AMD_FILTER_BILINEAR, d_dst, dst_stride);
}

int jpeg_amd_decode_resized_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                  const int16_t *const d_coef[], const size_t coef_stride[],
                                  const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                  int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                  int32_t out_w, int32_t out_h, uint8_t *d_pixels, size_t pixel_stride)
{
    return jpeg_amd_decode_resized_filter_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, h_views,
                                                out_w, out_h, JPEG_AMD_FILTER_BILINEAR, d_pixels, pixel_stride);
}

int jpeg_amd_decode_resized(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                            const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                            const jpeg_amd_view *view, int32_t out_w, int32_t out_h, uint8_t *d_pixels)
{
    // as jpeg_amd_decode_view: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY(ResampleTarget(ResampleRequest::bytes(out_w, out_h, d_pixels, 0)).check(1));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_resized_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, out_w, out_h, d_pixels,
                                         0);
}

int jpeg_amd_tensor_extent(const jpeg_amd_tensor_spec *spec, int32_t out_w, int32_t out_h, size_t *elem_bytes, size_t *image_elems)
{
    if (!spec) return JPEG_AMD_EINVAL;
    if (spec->dtype != JPEG_AMD_F32 && spec->dtype != JPEG_AMD_F16 && spec->dtype != JPEG_AMD_BF16) return JPEG_AMD_EINVAL;
    if (spec->layout != JPEG_AMD_TENSOR_HWC && spec->layout != JPEG_AMD_TENSOR_CHW) return JPEG_AMD_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(spec->mean[c]) || !std::isfinite(spec->scale[c])) return JPEG_AMD_EINVAL;
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    if (resize_tiles(out_w, out_h) > 0x7fffffffu) return JPEG_AMD_EINVAL;   // more workgroups than a grid holds
    if (elem_bytes) *elem_bytes = spec->dtype == JPEG_AMD_F32 ? 4 : 2;
    if (image_elems) *image_elems = (size_t)3 * out_w * out_h;
    return JPEG_AMD_OK;
}

int jpeg_amd_resize_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
{
    return jpeg_amd_resize_filter_tensor_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, JPEG_AMD_FILTER_BILINEAR, spec, h_flip,
                                               d_dst, dst_stride);
}

int jpeg_amd_decode_tensor_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                 int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                 void *d_dst, size_t dst_stride)
{
    return jpeg_amd_decode_tensor_filter_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, h_views,
                                               out_w, out_h, JPEG_AMD_FILTER_BILINEAR, spec, h_flip, d_dst, dst_stride);
}

int jpeg_amd_decode_tensor(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_view *view, int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec,
                           int flip, void *d_dst)
{
    // as jpeg_amd_decode_resized: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY(ResampleTarget(ResampleRequest::elements(out_w, out_h, spec, nullptr, d_dst, 0)).check(1));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    const uint8_t h_flip = flip ? 1 : 0;
    return jpeg_amd_decode_tensor_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, out_w, out_h, spec,
                                        &h_flip, d_dst, 0);
}

namespace {

constexpr int kMixedGroups = 2 * kViewDenoms;   // group 2 k + (three planes): the images of N = 8 >> k with that many planes

// Images [0, m) of a mixed call, or of a chunk of one, sorted into the launches of k_view_decode_mixed and the images that
// take the uniform call.
struct MixedPlan {
    std::vector<uint32_t> members[kMixedGroups];   // the group's images, in index order
    std::vector<int> fallback;                     // no tile kernel for the layout: the uniform call, image by image
};

// What the uniform view call with n_images = 1 judges of image `im` with view `v`, in its order (check_views itself), then the
// stride that the mixed call's placement needs.
int check_mixed_image(const jpeg_amd_image &im, int n_images, int cosited, jpeg_amd_color color, const jpeg_amd_view &v,
                      const void *d_out, size_t pixel_stride)
{
    const DecodeCall c{&im.layout, 1, im.d_coef, kOneImage, im.d_quanta, 0, im.ntables, cosited, color,
                       static_cast<uint8_t *>(const_cast<void *>(d_out)), 0};
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(c, &v, S, count, &whole, &cs));
    if (n_images > 1 && pixel_stride < (size_t)3 * v.region.width * v.region.height) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// The plan of m checked images; EINVAL: a launch of more workgroups than a grid holds (refused here, before the context is
// looked at, and so never by run_mixed).
int plan_mixed(const jpeg_amd_image *im, const jpeg_amd_view *v, int m, int cosited, MixedPlan *plan)
{
    uint64_t acc[kMixedGroups] = {};
    for (int i = 0; i < m; ++i) {
        if (!fused_decode_supported(im[i].layout, cosited != 0)) {
            plan->fallback.push_back(i);
            continue;
        }
        const int k = view_slot(v[i].denom), g = 2 * k + (im[i].layout.nplanes == 3 ? 1 : 0);
        plan->members[g].push_back((uint32_t)i);
        acc[g] += rect_tiles(8 >> k, kViewTileH, v[i].region);
    }
    for (int g = 0; g < kMixedGroups; ++g)
        if (acc[g] > 0x7fffffffu) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// The planned images into d_pixels, image i at i * pixel_stride: one copy of the records [m], then per group its index list
// and tile prefix (tile_staging.hpp), into the context's `mixed` buffer (from a pageable host buffer, so the copy has taken it when
// the call returns -- as stage_quanta); a launch per group; the uniform call for each of the others.
int run_mixed(jpeg_amd_ctx *ctx, const jpeg_amd_image *im, const jpeg_amd_view *v, int m, const MixedPlan &plan, int cosited,
              jpeg_amd_color color, uint8_t *d_pixels, size_t pixel_stride)
{
    if ((size_t)m != plan.fallback.size()) {
        TileStaging st((size_t)m, mixed_record_bytes(), kMixedGroups);   // the records of the uniform call's images stay zero: no list names them
        TileGroup group[kMixedGroups];
        for (int g = 0; g < kMixedGroups; ++g) {
            const std::vector<uint32_t> &mem = plan.members[g];
            if (mem.empty()) continue;
            const int n = 8 >> (g / 2);
            for (const uint32_t i : mem)
                mixed_record(st.payload(i), im[i].layout, n, im[i].d_coef, im[i].d_quanta, v[i].region, d_pixels + (size_t)i * pixel_stride);
            JA_TRY(st.group(mem, [&](uint32_t i) { return rect_tiles(n, kViewTileH, v[i].region); }, &group[g]));
        }
        JA_TRY(ensure_buffer(ctx, ctx->mixed, 4 * st.words.size()));
        JA_HIP(ctx, hipMemcpyAsync(ctx->mixed.ptr, st.words.data(), 4 * st.words.size(), hipMemcpyHostToDevice, ctx->stream));
        for (int g = 0; g < kMixedGroups; ++g) {
            if (plan.members[g].empty()) continue;
            TileLaunch l{};
            l.kernel = TileKernel::Mixed;
            l.n = 8 >> (g / 2);
            l.nplanes = g % 2 ? 3 : 1;
            l.rgb = color == JPEG_AMD_COLOR_RGB8;
            staged(l, ctx->mixed.ptr, group[g]);
            JA_HIP(ctx, launch_tile_decode(ctx->stream, l));
        }
    }
    for (const int i : plan.fallback)
        JA_TRY(jpeg_amd_decode_view_batch(ctx, &im[i].layout, 1, im[i].d_coef, kOneImage, im[i].d_quanta, 0, im[i].ntables, cosited,
                                          color, &v[i], d_pixels + (size_t)i * pixel_stride, 0));
    return JPEG_AMD_OK;
}

// What jpeg_amd_decode_resized_mixed and jpeg_amd_decode_tensor_mixed judge of a call of n_images images before they look at
// the context, the tap limit (plan->status) aside; the target is judged where the uniform call judges it: behind the first
// image.  judged < n_images (the file calls, whose image `judged` is already refused): only the images in front of it, and
// nothing that comes behind the images -- no plan.
int judge_resized_mixed(int n_images, int judged, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                        const jpeg_amd_view *h_views, ResampleTarget &t, ResizePlan *plan, std::vector<MixedPlan> *plans)
{
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_images || !h_views)) return JPEG_AMD_EINVAL;
    for (int i = 0; i < judged; ++i) {
        JA_TRY(check_mixed_image(h_images[i], 1, cosited, color, h_views[i], t.d_dst, 0));   // the views' stride is ours
        JA_TRY(t.check_orientation(i));
        if (i == 0) JA_TRY(t.check(n_images));
        JA_TRY(t.window(i, h_views[i].region.width, h_views[i].region.height));
    }
    if (n_images == 0) JA_TRY(t.check(n_images));
    if (judged < n_images) return JPEG_AMD_OK;
    *plan = plan_resize_chunks(n_images, h_views, t);
    plans->resize(plan->chunks.size());
    for (size_t c = 0; c < plans->size(); ++c)
        JA_TRY(plan_mixed(h_images + plan->chunks[c].i0, h_views + plan->chunks[c].i0, plan->chunks[c].m, cosited, &(*plans)[c]));
    return JPEG_AMD_OK;
}

}  // namespace

// The route of the mixed resample calls: decode_resampled's with the mixed view decode.
int jpeg_amd::capi::decode_views_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                       jpeg_amd_color color, const jpeg_amd_view *h_views, const ResampleRequest &rq)
try {
    // every argument first, the context last
    ResampleTarget t(rq);
    ResizePlan plan;
    std::vector<MixedPlan> plans;
    JA_TRY(judge_resized_mixed(n_images, n_images, h_images, cosited, color, h_views, t, &plan, &plans));
    JA_TRY(plan.status);
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    JA_TRY(bind(ctx));
    return resample_chunks(ctx, plan, t, [&](size_t c, const ResizeChunk &k, uint8_t *d_views) {
        return run_mixed(ctx, h_images + k.i0, h_views + k.i0, k.m, plans[c], cosited, color, d_views, k.stride);
    });
}
JA_NOTHROW_TAIL

int jpeg_amd::capi::check_resampled_mixed(int n_images, int judged, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                                          const jpeg_amd_view *h_views, const ResampleRequest &rq, int *taps)
{
    ResampleTarget t(rq);
    ResizePlan plan;
    std::vector<MixedPlan> plans;
    JA_TRY(judge_resized_mixed(n_images, judged, h_images, cosited, color, h_views, t, &plan, &plans));
    *taps = plan.status;
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_view_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                               jpeg_amd_color color, const jpeg_amd_view *h_views, uint8_t *d_pixels, size_t pixel_stride)
try {
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_images || !h_views)) return JPEG_AMD_EINVAL;
    for (int i = 0; i < n_images; ++i) JA_TRY(check_mixed_image(h_images[i], n_images, cosited, color, h_views[i], d_pixels, pixel_stride));
    MixedPlan plan;
    JA_TRY(plan_mixed(h_images, h_views, n_images, cosited, &plan));
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    JA_TRY(bind(ctx));
    return run_mixed(ctx, h_images, h_views, n_images, plan, cosited, color, d_pixels, pixel_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                  jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                  uint8_t *d_pixels, size_t pixel_stride)
{
    return jpeg_amd_decode_resized_filter_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, JPEG_AMD_FILTER_BILINEAR,
                                                d_pixels, pixel_stride);
}

int jpeg_amd_decode_tensor_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                 jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
{
    return jpeg_amd_decode_tensor_filter_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, JPEG_AMD_FILTER_BILINEAR, spec,
                                               h_flip, d_dst, dst_stride);
}

// The six resample calls with the filter chosen by the caller ("antialiased resample"); their forms without a filter argument,
// above, are these with JPEG_AMD_FILTER_BILINEAR.
int jpeg_amd_resize_filter_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter, uint8_t *d_dst,
                                 size_t dst_stride)
try {
    return jpeg_amd_resize_oriented_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, filter, nullptr, d_dst, dst_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_resize_filter_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return jpeg_amd_resize_oriented_tensor_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, filter, spec, h_flip, nullptr,
                                                 d_dst, dst_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                         const int16_t *const d_coef[], const size_t coef_stride[],
                                         const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                         int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                         int32_t out_w, int32_t out_h, int filter, uint8_t *d_pixels, size_t pixel_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, 0},
                            h_views, ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride).through(filter));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                        int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                        const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            static_cast<uint8_t *>(d_dst), 0},
                            h_views, ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride).through(filter));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                         jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                         int filter, uint8_t *d_pixels, size_t pixel_stride)
try {
    return jpeg_amd_decode_resized_oriented_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, filter, nullptr, d_pixels,
                                                  pixel_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                        size_t dst_stride)
try {
    return jpeg_amd_decode_tensor_oriented_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, filter, spec, h_flip,
                                                 nullptr, d_dst, dst_stride);
}
JA_NOTHROW_TAIL

// The four resample calls above the file level with an orientation per image ("oriented resample"); their forms without one,
// above, are these with h_orient == nullptr.
int jpeg_amd_resize_oriented_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                   const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                   const uint8_t *h_orient, uint8_t *d_dst, size_t dst_stride)
try {
    return jpeg_amd_resize_placed_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, filter, h_orient, nullptr, nullptr, d_dst,
                                        dst_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_resize_oriented_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                          const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                          const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                          void *d_dst, size_t dst_stride)
try {
    return jpeg_amd_resize_placed_tensor_batch(ctx, n_images, d_src, src_stride, h_extents, out_w, out_h, filter, spec, h_flip, h_orient,
                                               nullptr, nullptr, d_dst, dst_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_oriented_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                           int filter, const uint8_t *h_orient, uint8_t *d_pixels, size_t pixel_stride)
try {
    return jpeg_amd_decode_resized_placed_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, filter, h_orient, nullptr,
                                                nullptr, d_pixels, pixel_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_oriented_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                          jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                          int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                          const uint8_t *h_orient, void *d_dst, size_t dst_stride)
try {
    return jpeg_amd_decode_tensor_placed_mixed(ctx, n_images, h_images, cosited, color, h_views, out_w, out_h, filter, spec, h_flip, h_orient,
                                               nullptr, nullptr, d_dst, dst_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_orient_region(int orientation, int32_t width, int32_t height, const jpeg_amd_region *oriented, jpeg_amd_region *stored)
{
    if (!stored || !orientation_valid(orientation) || width < 1 || height < 1) return JPEG_AMD_EINVAL;
    const OrientedSource s = oriented_source(orientation, 0, width, height);
    const jpeg_amd_region r = oriented ? *oriented : jpeg_amd_region{0, 0, s.w, s.h};
    if (r.x < 0 || r.y < 0 || r.width < 1 || r.height < 1 || r.x > s.w - r.width || r.y > s.h - r.height) return JPEG_AMD_EINVAL;
    const OrientRect m = oriented_rect_to_stored(orientation, width, height, OrientRect{r.x, r.y, r.width, r.height});
    *stored = jpeg_amd_region{m.x, m.y, m.width, m.height};
    return JPEG_AMD_OK;
}

// The four resample calls above the file level with a placement ("placed resample"); their forms without one, above, are
// these with place == nullptr.
int jpeg_amd_place_window(int mode, int anchor, int32_t src_w, int32_t src_h, int32_t out_w, int32_t out_h, jpeg_amd_region *window)
{
    if (!window || (mode != JPEG_AMD_PLACE_FIT && mode != JPEG_AMD_PLACE_FIT_DOWN)) return JPEG_AMD_EINVAL;
    if (anchor != JPEG_AMD_ANCHOR_CENTRE && anchor != JPEG_AMD_ANCHOR_TOP_LEFT) return JPEG_AMD_EINVAL;
    if (src_w < 1 || src_h < 1 || out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    const int64_t sw = src_w, sh = src_h, ow = out_w, oh = out_h;
    int64_t ww, wh;
    if (mode == JPEG_AMD_PLACE_FIT_DOWN && sw <= ow && sh <= oh) {
        ww = sw;
        wh = sh;
    } else if (ow * sh <= oh * sw) {   // the width binds
        ww = ow;
        wh = std::min(oh, std::max<int64_t>(1, (2 * sh * ow + sw) / (2 * sw)));
    } else {
        wh = oh;
        ww = std::min(ow, std::max<int64_t>(1, (2 * sw * oh + sh) / (2 * sh)));
    }
    const bool centre = anchor == JPEG_AMD_ANCHOR_CENTRE;
    *window = jpeg_amd_region{centre ? (int32_t)((ow - ww) / 2) : 0, centre ? (int32_t)((oh - wh) / 2) : 0, (int32_t)ww, (int32_t)wh};
    return JPEG_AMD_OK;
}

int jpeg_amd_resize_placed_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                 const uint8_t *h_orient, const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out,
                                 uint8_t *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::bytes(out_w, out_h, d_dst, dst_stride)
                             .through(filter).oriented(h_orient).placed(place, h_windows_out));
}
JA_NOTHROW_TAIL

int jpeg_amd_resize_placed_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                        const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out, void *d_dst,
                                        size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                             .through(filter).oriented(h_orient).placed(place, h_windows_out));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_placed_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                         jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                         int filter, const uint8_t *h_orient, const jpeg_amd_placement *place,
                                         jpeg_amd_region *h_windows_out, uint8_t *d_pixels, size_t pixel_stride)
try {
    return decode_views_mixed(ctx, n_images, h_images, cosited, color, h_views,
                              ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                                  .through(filter).oriented(h_orient).placed(place, h_windows_out));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_placed_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                        const uint8_t *h_orient, const jpeg_amd_placement *place,
                                        jpeg_amd_region *h_windows_out, void *d_dst, size_t dst_stride)
try {
    return decode_views_mixed(ctx, n_images, h_images, cosited, color, h_views,
                              ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                  .through(filter).oriented(h_orient).placed(place, h_windows_out));
}
JA_NOTHROW_TAIL

// ---- "warped resample" ----
namespace {

// What jpeg_amd_warp_view and jpeg_amd_project_view share.  The denominator of a map whose shorter Jacobian column has the
// squared length step2: the largest d of 8, 4, 2 with d * d <= step2, else 1.
int map_denom(double step2)
{
    for (int d = 8; d > 1; d /= 2)
        if ((double)(d * d) <= step2) return d;
    return 1;
}

// The rectangle of the scaled image S that holds the taps of a canvas whose footprint spans lo[a] .. hi[a] on axis a, clamped.
// wider: the pixels that the filter's taps reach beyond the two-tap filter's on each side ("bicubic warp": 1).
jpeg_amd_region footprint_view(const double lo[2], const double hi[2], const jpeg_amd_layout &S, int wider = 0)
{
    const auto clamp = [](double v, double last) { return (int32_t)std::min(std::max(v, 0.0), last); };
    const double before = 1.0 + (double)wider, after = 2.0 + (double)wider;
    const int32_t x0 = clamp(std::floor(lo[0] - 0.5) - before, S.width - 1), x1 = clamp(std::floor(hi[0] - 0.5) + after, S.width - 1);
    const int32_t y0 = clamp(std::floor(lo[1] - 0.5) - before, S.height - 1), y1 = clamp(std::floor(hi[1] - 0.5) + after, S.height - 1);
    return jpeg_amd_region{x0, y0, x1 - x0 + 1, y1 - y0 + 1};
}

// jpeg_amd_project_filter_view behind the verdict on its filter: `wider` as footprint_view's.
int project_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int32_t out_w, int32_t out_h, int wider,
                 jpeg_amd_view *view, float m_view[9]);

}  // namespace

int jpeg_amd_warp_view(const jpeg_amd_layout *layout, int orientation, const float m[6], int32_t out_w, int32_t out_h,
                       jpeg_amd_view *view, float m_view[6])
{
    if (!view || !m_view || !orientation_valid(orientation)) return JPEG_AMD_EINVAL;
    JA_TRY(check_warp_matrix(m));
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(layout, -1));
    // 1. the orientation composed into the matrix: output centres to STORED coordinates
    const Orientation b = orientation_bits(orientation);
    const double W = layout->width, H = layout->height;
    double s[6];
    for (int k = 0; k < 3; ++k) {
        s[k] = b.T ? m[3 + k] : m[k];
        s[3 + k] = b.T ? m[k] : m[3 + k];
    }
    if (b.fx) { s[0] = -s[0]; s[1] = -s[1]; s[2] = W - s[2]; }
    if (b.fy) { s[3] = -s[3]; s[4] = -s[4]; s[5] = H - s[5]; }
    // 2. the denominator
    const double m00 = m[0], m01 = m[1], m10 = m[3], m11 = m[4];
    const double step2 = std::min(m00 * m00 + m10 * m10, m01 * m01 + m11 * m11);
    const int denom = map_denom(step2);
    // 3. against the scaled image
    jpeg_amd_layout S;
    JA_TRY(jpeg_amd_scaled_layout(layout, denom, &S));
    const double f = (double)(8 / denom) / 8.0;
    for (int k = 0; k < 6; ++k) s[k] = s[k] * f;
    // 4. the footprint of the canvas
    const double cx[4] = {0.0, (double)out_w, 0.0, (double)out_w}, cy[4] = {0.0, 0.0, (double)out_h, (double)out_h};
    double lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        for (int c = 0; c < 4; ++c) {
            const double v = (s[3 * a] * cx[c] + s[3 * a + 1] * cy[c]) + s[3 * a + 2];
            lo[a] = c == 0 ? v : std::min(lo[a], v);
            hi[a] = c == 0 ? v : std::max(hi[a], v);
        }
    }
    const jpeg_amd_region r = footprint_view(lo, hi, S);
    *view = jpeg_amd_view{denom, r};
    // 5. against the view
    s[2] = s[2] - (double)r.x;
    s[5] = s[5] - (double)r.y;
    for (int k = 0; k < 6; ++k) m_view[k] = (float)s[k];
    return JPEG_AMD_OK;
}

int jpeg_amd_warp_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                        const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                        int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::bytes(out_w, out_h, d_dst, dst_stride).mapped(ResampleMap::Affine, h_matrices, warp));
}
JA_NOTHROW_TAIL

int jpeg_amd_warp_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                               const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                               int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                               void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                             .mapped(ResampleMap::Affine, h_matrices, warp));
}
JA_NOTHROW_TAIL

namespace {

// The mixed calls through a map (jpeg_amd_decode_warped_mixed, jpeg_amd_decode_projected_mixed, their tensor forms): rq carries
// the caller's matrices against the upright images and the orientations; every image's view and m_view from map_view, which
// takes the orientation into the matrix, then the route of the mixed calls with those.
int mapped_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                 const ResampleRequest &rq, jpeg_amd_view *h_views_out, float *h_matrices_out)
{
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_images || !rq.h_matrices)) return JPEG_AMD_EINVAL;
    const size_t n = (size_t)n_images, k = rq.matrix_floats();
    std::vector<jpeg_amd_view> views(n);
    std::vector<float> view_matrices(k * n);
    for (size_t i = 0; i < n; ++i) {
        JA_TRY(map_view(rq, &h_images[i].layout, rq.h_orient ? rq.h_orient[i] : 1, rq.h_matrices + k * i, &views[i], &view_matrices[k * i]));
        if (h_views_out) h_views_out[i] = views[i];
        if (h_matrices_out) std::memcpy(h_matrices_out + k * i, &view_matrices[k * i], k * sizeof(float));
    }
    ResampleRequest behind = rq;
    behind.oriented(nullptr).mapped(rq.map, view_matrices.data(), rq.warp);
    return decode_views_mixed(ctx, n_images, h_images, cosited, color, views.data(), behind);
}

}  // namespace

int jpeg_amd_decode_warped_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                 jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                 const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h, jpeg_amd_view *h_views_out,
                                 float *h_matrices_out, uint8_t *d_pixels, size_t pixel_stride)
try {
    return mapped_mixed(ctx, n_images, h_images, cosited, color,
                        ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                            .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp),
                        h_views_out, h_matrices_out);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_warped_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                        const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, jpeg_amd_view *h_views_out,
                                        float *h_matrices_out, void *d_dst, size_t dst_stride)
try {
    return mapped_mixed(ctx, n_images, h_images, cosited, color,
                        ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                            .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp),
                        h_views_out, h_matrices_out);
}
JA_NOTHROW_TAIL

// ---- "colour stage" ----
// The tensor calls with an affine map of (R, G, B) per image between the resample and the tensor output; with colour == nullptr
// each is the call it is named after, by delegation.
int jpeg_amd_resize_colour_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                        const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out,
                                        const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                             .through(filter).oriented(h_orient).placed(place, h_windows_out).coloured(colour));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_colour_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                        const uint8_t *h_orient, const jpeg_amd_placement *place,
                                        jpeg_amd_region *h_windows_out, const jpeg_amd_colour *colour, void *d_dst,
                                        size_t dst_stride)
try {
    return decode_views_mixed(ctx, n_images, h_images, cosited, color, h_views,
                              ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                  .through(filter).oriented(h_orient).placed(place, h_windows_out).coloured(colour));
}
JA_NOTHROW_TAIL

int jpeg_amd_warp_colour_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                      const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                                      int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                      const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                             .mapped(ResampleMap::Affine, h_matrices, warp).coloured(colour));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_warped_colour_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                               jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                               const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                               const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, jpeg_amd_view *h_views_out,
                                               float *h_matrices_out, const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
try {
    return mapped_mixed(ctx, n_images, h_images, cosited, color,
                        ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                            .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp).coloured(colour),
                        h_views_out, h_matrices_out);
}
JA_NOTHROW_TAIL

// ---- "projective resample" and "bicubic warp" ----
namespace {

int project_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int32_t out_w, int32_t out_h, int wider,
                 jpeg_amd_view *view, float m_view[9])
{
    if (!view || !m_view || !orientation_valid(orientation)) return JPEG_AMD_EINVAL;
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    JA_TRY(check_project_matrix(m, out_w, out_h));
    JA_TRY(check_layout(layout, -1));
    // 1. the orientation composed into the matrix: output centres to STORED coordinates, homogeneous
    const Orientation b = orientation_bits(orientation);
    const double W = layout->width, H = layout->height;
    double s[9];
    for (int k = 0; k < 3; ++k) {
        s[k] = b.T ? m[3 + k] : m[k];
        s[3 + k] = b.T ? m[k] : m[3 + k];
        s[6 + k] = m[6 + k];
    }
    for (int k = 0; b.fx && k < 3; ++k) s[k] = W * s[6 + k] - s[k];
    for (int k = 0; b.fy && k < 3; ++k) s[3 + k] = H * s[6 + k] - s[3 + k];
    // 2. the denominator: the shorter column of the Jacobian at the corners and the centre of the canvas (of the upright map:
    // the orientation permutes and negates its rows)
    const double px[5] = {0.0, (double)out_w, 0.0, (double)out_w, 0.5 * (double)out_w};
    const double py[5] = {0.0, 0.0, (double)out_h, (double)out_h, 0.5 * (double)out_h};
    double step2 = 0.0;
    for (int p = 0; p < 5; ++p) {
        const double nw = ((double)m[6] * px[p] + (double)m[7] * py[p]) + (double)m[8];
        const double X = (((double)m[0] * px[p] + (double)m[1] * py[p]) + (double)m[2]) / nw;
        const double Y = (((double)m[3] * px[p] + (double)m[4] * py[p]) + (double)m[5]) / nw;
        for (int c = 0; c < 2; ++c) {
            const double jx = ((double)m[c] - X * (double)m[6 + c]) / nw, jy = ((double)m[3 + c] - Y * (double)m[6 + c]) / nw;
            const double n2 = jx * jx + jy * jy;
            step2 = p == 0 && c == 0 ? n2 : std::min(step2, n2);
        }
    }
    const int denom = map_denom(step2);
    // 3. against the scaled image: the numerators' rows times 1 / d
    jpeg_amd_layout S;
    JA_TRY(jpeg_amd_scaled_layout(layout, denom, &S));
    const double f = (double)(8 / denom) / 8.0;
    for (int k = 0; k < 6; ++k) s[k] = s[k] * f;
    // 4. the footprint of the canvas: the denominator is positive on it, so it maps onto the quadrilateral of its corners' images
    const double cx[4] = {0.0, (double)out_w, 0.0, (double)out_w}, cy[4] = {0.0, 0.0, (double)out_h, (double)out_h};
    double lo[2], hi[2];
    for (int c = 0; c < 4; ++c) {
        const double nw = (s[6] * cx[c] + s[7] * cy[c]) + s[8];
        for (int a = 0; a < 2; ++a) {
            const double v = ((s[3 * a] * cx[c] + s[3 * a + 1] * cy[c]) + s[3 * a + 2]) / nw;
            lo[a] = c == 0 ? v : std::min(lo[a], v);
            hi[a] = c == 0 ? v : std::max(hi[a], v);
        }
    }
    const jpeg_amd_region r = footprint_view(lo, hi, S, wider);
    // 5. against the view: the view's origin times the denominator's row off the numerators' rows
    float mv[9];
    for (int k = 0; k < 3; ++k) {
        mv[k] = (float)(s[k] - (double)r.x * s[6 + k]);
        mv[3 + k] = (float)(s[3 + k] - (double)r.y * s[6 + k]);
        mv[6 + k] = m[6 + k];
    }
    JA_TRY(check_project_matrix(mv, out_w, out_h));   // (an entry past 2^30 behind the subtraction)
    *view = jpeg_amd_view{denom, r};
    std::memcpy(m_view, mv, sizeof mv);
    return JPEG_AMD_OK;
}

}  // namespace

// The view that the map of `rq` reads of an image, and the matrix against it: jpeg_amd_warp_view's, or jpeg_amd_project_filter_view's
// at the request's filter -- whose verdict is not given here but with the edge mode's (ResampleTarget::check): any filter
// but the bicubic one has the two-tap footprint.
int jpeg_amd::capi::map_view(const ResampleRequest &rq, const jpeg_amd_layout *layout, int orientation, const float *m, jpeg_amd_view *view,
                             float *m_view)
{
    if (rq.map != ResampleMap::Projective) return jpeg_amd_warp_view(layout, orientation, m, rq.out_w, rq.out_h, view, m_view);
    return project_view(layout, orientation, m, rq.out_w, rq.out_h, rq.filter == JPEG_AMD_FILTER_BICUBIC ? 1 : 0, view, m_view);
}

int jpeg_amd_project_filter_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int filter, int32_t out_w, int32_t out_h,
                                 jpeg_amd_view *view, float m_view[9])
{
    if (filter != JPEG_AMD_FILTER_BILINEAR && filter != JPEG_AMD_FILTER_BICUBIC) return JPEG_AMD_EINVAL;
    return project_view(layout, orientation, m, out_w, out_h, filter == JPEG_AMD_FILTER_BICUBIC ? 1 : 0, view, m_view);
}

int jpeg_amd_project_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int32_t out_w, int32_t out_h,
                          jpeg_amd_view *view, float m_view[9])
{
    return jpeg_amd_project_filter_view(layout, orientation, m, JPEG_AMD_FILTER_BILINEAR, out_w, out_h, view, m_view);
}

// The existing projective calls are the calls with a filter at JPEG_AMD_FILTER_BILINEAR.
int jpeg_amd_project_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                           const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                           int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride)
{
    return jpeg_amd_project_filter_batch(ctx, n_images, d_src, src_stride, h_extents, h_matrices, warp, JPEG_AMD_FILTER_BILINEAR, out_w, out_h,
                                         d_dst, dst_stride);
}

int jpeg_amd_project_filter_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                  const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp, int filter,
                                  int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::bytes(out_w, out_h, d_dst, dst_stride)
                             .through(filter).mapped(ResampleMap::Projective, h_matrices, warp));
}
JA_NOTHROW_TAIL

int jpeg_amd_project_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                  const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                                  int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                  const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
{
    return jpeg_amd_project_filter_tensor_batch(ctx, n_images, d_src, src_stride, h_extents, h_matrices, warp, JPEG_AMD_FILTER_BILINEAR, out_w,
                                                out_h, spec, h_flip, colour, d_dst, dst_stride);
}

int jpeg_amd_project_filter_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                         const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp, int filter,
                                         int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                         const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                             .through(filter).mapped(ResampleMap::Projective, h_matrices, warp).coloured(colour));
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_projected_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                    jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                    const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h, jpeg_amd_view *h_views_out,
                                    float *h_matrices_out, uint8_t *d_pixels, size_t pixel_stride)
{
    return jpeg_amd_decode_projected_filter_mixed(ctx, n_images, h_images, cosited, color, h_orient, h_matrices, warp, JPEG_AMD_FILTER_BILINEAR,
                                                  out_w, out_h, h_views_out, h_matrices_out, d_pixels, pixel_stride);
}

int jpeg_amd_decode_projected_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                           const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                           jpeg_amd_view *h_views_out, float *h_matrices_out, uint8_t *d_pixels, size_t pixel_stride)
try {
    return mapped_mixed(ctx, n_images, h_images, cosited, color,
                        ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                            .through(filter).oriented(h_orient).mapped(ResampleMap::Projective, h_matrices, warp),
                        h_views_out, h_matrices_out);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_projected_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                           const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                           const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, jpeg_amd_view *h_views_out,
                                           float *h_matrices_out, const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
{
    return jpeg_amd_decode_tensor_projected_filter_mixed(ctx, n_images, h_images, cosited, color, h_orient, h_matrices, warp,
                                                         JPEG_AMD_FILTER_BILINEAR, out_w, out_h, spec, h_flip, h_views_out, h_matrices_out,
                                                         colour, d_dst, dst_stride);
}

int jpeg_amd_decode_tensor_projected_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                                  jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                                  const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                                  const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, jpeg_amd_view *h_views_out,
                                                  float *h_matrices_out, const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride)
try {
    return mapped_mixed(ctx, n_images, h_images, cosited, color,
                        ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                            .through(filter).oriented(h_orient).mapped(ResampleMap::Projective, h_matrices, warp).coloured(colour),
                        h_views_out, h_matrices_out);
}
JA_NOTHROW_TAIL
