// kernels_tile.hip -- the tile decode family: the four kernels whose workgroup is tile_decode.hpp's tile body, their one
// launcher, and the two fallback kernels of the layouts without a tile kernel.  include/jpeg_amd.h holds the contracts
// ("scaled decode", "view decode"); the region decode is the full decode, cropped (decode.swift:4154-4165, 4182-4276,
// 4291-4298).  The four differ in how a workgroup finds its image and its tile:
//
// k_region_decode<planes, rgb> (jpeg_amd_decode_region_batch): the rectangle grid at N = 8 with tiles of 128 x 64 pixels
// (16 x 8 luma blocks at most), image i of the launch image i of the call.
//
// k_scaled_decode<N, planes, rgb> (jpeg_amd_decode_scaled_batch): whole images of one size on a static grid of (tiles per
// image) x (images).  A tile is 128 x 32 OUTPUT pixels -- 128 / N x 32 / N luma blocks, so that a workgroup's output rows
// are 384-byte runs whatever N is.
//
// k_view_decode<N, planes, rgb> (jpeg_amd_decode_view_batch): the rectangle grid for the images of a call that share
// N = 8 / denom, through an index list (index[i] = the image's place in the call), which makes a call of mixed denominators
// one launch per denominator.  The tile is the scaled kernel's.  N = 8 gives the bytes of k_region_decode, for the
// denominator-1 images of such a call.
//
// k_view_decode_mixed<N, planes, rgb> (jpeg_amd_decode_view_mixed): the same grid and body for images of DIFFERENT sizes
// and samplings: one launch per (N, planes) of the call, every image with a record of its own in device memory in the place
// of the kernel argument.
//
// k_region_crop: the region and view calls' fallback, whole decoded images cut to their rectangles.
// k_idct_scaled<N, T>: the scaled call's fallback, the transform of one plane into samples of T, padded to whole 8 x 8 blocks
// by edge replication, for the staged interleave kernel under jpeg_amd_scaled_layout's layout.
//
// Compile with -ffp-contract=off (see dct.hpp) and -fno-slp-vectorize (tile_decode.hpp).
#pragma clang fp contract(off)

#include <cstring>
#include <type_traits>
#include <utility>

#include "tile_decode.hpp"

namespace jpeg_amd {

namespace {

// The region kernel's chroma window of a tile: 1x1 chroma at scale 2 reads 64 + 2 samples per 128 pixels (10 blocks at most),
// at scale 1 (a full-factor axis of 4:2:2 / 4:4:0) the samples under the tile's pixels and the zero-weight neighbour one past
// them (17 blocks); vertically 34 (6 blocks) or 65 samples (9 blocks).  (The others: chroma_span<N> of their tile.)
constexpr int kRegionChromaW = 8 * 17, kRegionChromaH = 8 * 9;

struct RegionArgs {
    TileArgs t;
    RectArgs rect;
};

template <int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_region_decode(RegionArgs a)
{
    Tile tile;
    if (rect_tile<8, kRegionTileH>(a.rect, nullptr, a.t, tile))
        decode_tile<8, NP, RGB, kTileW, kRegionTileH, kRegionChromaW, kRegionChromaH>(a.t, tile);
}

struct ScaledArgs {
    TileArgs t;
    int width, height;            // W', H'
    int tiles_x;
};

template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_scaled_decode(ScaledArgs a)
{
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    Tile tile;
    tile.img = blockIdx.y;
    tile.px0 = kTileW * tx; tile.px1 = min(a.width, tile.px0 + kTileW);
    tile.py0 = kViewTileH * ty; tile.py1 = min(a.height, tile.py0 + kViewTileH);
    tile.row_bytes = 3 * (size_t)a.width;
    tile.out = a.t.pixels + (size_t)tile.img * a.t.pixel_stride + (size_t)tile.py0 * tile.row_bytes + 3 * (size_t)tile.px0;
    decode_tile<N, NP, RGB, kTileW, kViewTileH, chroma_span<N>(kTileW), chroma_span<N>(kViewTileH)>(a.t, tile);
}

struct ViewArgs {
    TileArgs t;
    RectArgs rect;                // regions: of the scaled image, [images of the call]
    const uint32_t *index;        // [n]: the launch's image i is image index[i] of the call
};

template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_view_decode(ViewArgs a)
{
    Tile tile;
    if (rect_tile<N, kViewTileH>(a.rect, a.index, a.t, tile))
        decode_tile<N, NP, RGB, kTileW, kViewTileH, chroma_span<N>(kTileW), chroma_span<N>(kViewTileH)>(a.t, tile);
}

// The same workgroup for the images of a mixed call (jpeg_amd_decode_view_mixed) that share N and the number of planes:
// sizes and samplings differ from image to image, so what decode_tile reads comes from the image's MixedRecord.
template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_view_decode_mixed(MixedArgs g)
{
    Tile tile;
    if (const MixedRecord *rec = mixed_tile<N, kViewTileH>(g, tile))
        decode_tile<N, NP, RGB, kTileW, kViewTileH, chroma_span<N>(kTileW), chroma_span<N>(kViewTileH)>(rec->t, tile);
}

// Fallback crop: image i of `full` (W x H RGB / YCbCr bytes, `full_stride` apart) cut to its rectangle.
__global__ __launch_bounds__(kThreads) void k_region_crop(const uint8_t *__restrict__ full, size_t full_stride, int width,
                                                        const int4 *__restrict__ regions, uint8_t *__restrict__ pixels,
                                                        size_t pixel_stride)
{
    const int img = blockIdx.y;
    const int4 r = regions[img];
    const size_t row = 3 * (size_t)r.z, n = row * r.w;
    const uint8_t *src = full + (size_t)img * full_stride + 3 * ((size_t)r.y * width + r.x);
    uint8_t *dst = pixels + (size_t)img * pixel_stride;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const size_t y = i / row, x = i - y * row;
        dst[i] = src[y * 3 * (size_t)width + x];
    }
}

// One block per work-item: N x N samples at (N bx, N by) of a plane of pitch 8 units_x'.  The blocks of the last column
// and the last row also write the padding next to them -- up to 7 more columns / rows, the edge sample repeated.
template <int N, typename T>
__global__ __launch_bounds__(kThreads) void k_idct_scaled(const int16_t *__restrict__ coef, size_t coef_stride,
                                                        const uint16_t *__restrict__ quanta, size_t quanta_stride, int qi,
                                                        int ux, int uy, int pitch, int rows, float level, float limit,
                                                        T *__restrict__ out, size_t out_stride)
{
    __shared__ float sq[N * N];
    const int img = blockIdx.y, t = threadIdx.x;
    if (t < N * N) sq[t] = modulate_entry_scaled<N>(t % N, t / N, quanta[(size_t)img * quanta_stride + 64 * qi + zigzag_of(t % N, t / N)]);
    __syncthreads();

    const int b = blockIdx.x * kThreads + t;
    if (b >= ux * uy) return;
    const int by = b / ux, bx = b - by * ux;
    uint32_t w[scaled_head_words<N>()];
    load_block_head<N>(coef + (size_t)img * coef_stride + (size_t)64 * b, w);
    float g[N * N];
    idct_block_scaled<N>(w, sq, level, g);

    // this block's extent with its share of the padding: N, or up to the plane's padded edge (at most N + 7)
    const int xe = bx == ux - 1 ? pitch - N * bx : N, ye = by == uy - 1 ? rows - N * by : N;
    T *dst = out + (size_t)img * out_stride + (size_t)N * by * pitch + N * bx;
#pragma unroll
    for (int y = 0; y < N + 7; ++y) {
#pragma unroll
        for (int x = 0; x < N + 7; ++x)
            if (y < ye && x < xe) dst[(size_t)y * pitch + x] = (T)clamp_trunc(g[N * (y < N ? y : N - 1) + (x < N ? x : N - 1)], limit);
    }
}

// ---- the launcher ----

// What decode_tile reads of images of one layout: interleave_axis with the padded edge of a plane of n x n samples per block
// (n = 8: interleave_axis's own value).
TileArgs tile_args(const jpeg_amd_layout &L, int n, const PlaneSet &coef, QuantaRef q, uint8_t *d_pixels, size_t pixel_stride)
{
    TileArgs a{};
    for (int p = 0; p < L.nplanes; ++p) {
        a.coef[p] = static_cast<const int16_t *>(coef.ptr[p]);
        a.coef_stride[p] = coef.stride[p];
        a.ux[p] = L.units_x[p];
        a.qi[p] = L.qi[p];
        a.ax[p] = interleave_axis(L, p, false, false);
        a.ay[p] = interleave_axis(L, p, false, true);
        a.ax[p].last = n * L.units_x[p] - 1;
        a.ay[p].last = n * L.units_y[p] - 1;
    }
    a.quanta = q.d_quanta;
    a.quanta_stride = q.image_stride;
    a.pixels = d_pixels;
    a.pixel_stride = pixel_stride;
    return a;
}

// f(N, NP, RGB) as integral constants for n among Ns, 1 or 3 planes and rgb; anything else: no kernel exists for it.
template <int... Ns, typename F>
hipError_t with_shape(std::integer_sequence<int, Ns...>, int n, int nplanes, bool rgb, F f)
{
    if (nplanes != 1 && nplanes != 3) return hipErrorInvalidValue;
    const auto at = [&](auto N) {
        if (nplanes == 1) return rgb ? f(N, std::integral_constant<int, 1>{}, std::true_type{}) : f(N, std::integral_constant<int, 1>{}, std::false_type{});
        return rgb ? f(N, std::integral_constant<int, 3>{}, std::true_type{}) : f(N, std::integral_constant<int, 3>{}, std::false_type{});
    };
    hipError_t e = hipErrorInvalidValue;
    ((n == Ns ? (void)(e = at(std::integral_constant<int, Ns>{})) : (void)0), ...);
    return e;
}

template <typename Kernel, typename Args>
hipError_t run(Kernel kernel, dim3 grid, hipStream_t stream, const Args &a)
{
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tile_decode(hipStream_t stream, const TileLaunch &l)
{
    // workgroups along x: a rectangle grid's are staged, the static grid's are the tiles of one image
    const int tiles_x = (l.width + kTileW - 1) / kTileW;
    const uint32_t nwg = l.kernel == TileKernel::Scaled ? (uint32_t)tiles_x * (uint32_t)((l.height + kViewTileH - 1) / kViewTileH) : l.nwg;
    if (l.n_images == 0 || nwg == 0) return hipSuccess;
    const dim3 grid(nwg, l.kernel == TileKernel::Scaled ? (unsigned)l.n_images : 1u);
    if (l.kernel == TileKernel::Mixed) {
        const MixedArgs a{static_cast<const MixedRecord *>(l.d_payload), l.d_tiles, l.d_index, l.n_images};
        return with_shape(std::integer_sequence<int, 8, 4, 2, 1>{}, l.n, l.nplanes, l.rgb, [&](auto N, auto NP, auto RGB) {
            return run(k_view_decode_mixed<decltype(N)::value, decltype(NP)::value, decltype(RGB)::value>, grid, stream, a);
        });
    }
    if (!l.layout || l.nplanes != l.layout->nplanes) return hipErrorInvalidValue;
    const TileArgs t = tile_args(*l.layout, l.n, l.coef, l.q, l.d_pixels, l.pixel_stride);
    const RectArgs rect{l.d_tiles, static_cast<const int4 *>(l.d_payload), l.n_images};
    switch (l.kernel) {
    case TileKernel::Region: {
        const RegionArgs a{t, rect};
        return with_shape(std::integer_sequence<int, 8>{}, l.n, l.nplanes, l.rgb, [&](auto, auto NP, auto RGB) {
            return run(k_region_decode<decltype(NP)::value, decltype(RGB)::value>, grid, stream, a);
        });
    }
    case TileKernel::Scaled: {
        const ScaledArgs a{t, l.width, l.height, tiles_x};
        return with_shape(std::integer_sequence<int, 4, 2, 1>{}, l.n, l.nplanes, l.rgb, [&](auto N, auto NP, auto RGB) {
            return run(k_scaled_decode<decltype(N)::value, decltype(NP)::value, decltype(RGB)::value>, grid, stream, a);
        });
    }
    case TileKernel::View: {
        const ViewArgs a{t, rect, l.d_index};
        return with_shape(std::integer_sequence<int, 8, 4, 2, 1>{}, l.n, l.nplanes, l.rgb, [&](auto N, auto NP, auto RGB) {
            return run(k_view_decode<decltype(N)::value, decltype(NP)::value, decltype(RGB)::value>, grid, stream, a);
        });
    }
    default: return hipErrorInvalidValue;
    }
}

size_t mixed_record_bytes() { return sizeof(MixedRecord); }

void mixed_record(void *dst, const jpeg_amd_layout &L, int n, const int16_t *const d_coef[], const uint16_t *d_quanta,
                  const jpeg_amd_region &r, uint8_t *d_pixels)
{
    PlaneSet coef{};
    for (int p = 0; p < L.nplanes; ++p) coef.ptr[p] = d_coef[p];
    const MixedRecord rec{tile_args(L, n, coef, QuantaRef{d_quanta, 0}, d_pixels, 0), int4{r.x, r.y, r.width, r.height}};
    memcpy(dst, &rec, sizeof rec);
}

hipError_t launch_region_crop(hipStream_t stream, int n_images, const uint8_t *d_full, size_t full_stride, int width,
                              const int32_t *d_regions, size_t max_bytes, uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0) return hipSuccess;
    const size_t blocks = (max_bytes + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < 4096 ? (blocks ? blocks : 1) : 4096), (unsigned)n_images);
    hipLaunchKernelGGL(k_region_crop, grid, dim3(kThreads), 0, stream, d_full, full_stride, width,
                       reinterpret_cast<const int4 *>(d_regions), d_pixels, pixel_stride);
    return hipGetLastError();
}

hipError_t launch_idct_scaled_plane(hipStream_t stream, int n_images, const int16_t *d_coef, size_t coef_stride, QuantaRef q,
                                    int qi, int ux, int uy, int n, int precision, void *d_plane, size_t plane_stride, bool out_u8)
{
    const int nblocks = ux * uy;
    if (nblocks == 0 || n_images == 0) return hipSuccess;
    const float level = ldexpf(1.0f, precision - 1) + 0.5f;
    const float limit = ldexpf(1.0f, precision) - 1.0f;
    const int pitch = 8 * ((n * ux + 7) / 8), rows = 8 * ((n * uy + 7) / 8);
    const dim3 grid((unsigned)((nblocks + kThreads - 1) / kThreads), (unsigned)n_images);
#define JA_LAUNCH(N, T)                                                                                                   \
    hipLaunchKernelGGL((k_idct_scaled<N, T>), grid, dim3(kThreads), 0, stream, d_coef, coef_stride, q.d_quanta, q.image_stride, \
                       qi, ux, uy, pitch, rows, level, limit, static_cast<T *>(d_plane), plane_stride)
    if (out_u8) {
        if (n == 4) JA_LAUNCH(4, uint8_t);
        else if (n == 2) JA_LAUNCH(2, uint8_t);
        else JA_LAUNCH(1, uint8_t);
    } else {
        if (n == 4) JA_LAUNCH(4, uint16_t);
        else if (n == 2) JA_LAUNCH(2, uint16_t);
        else JA_LAUNCH(1, uint16_t);
    }
#undef JA_LAUNCH
    return hipGetLastError();
}

}  // namespace jpeg_amd
