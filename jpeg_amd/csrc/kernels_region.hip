// kernels_region.hip -- region decode (jpeg_amd_decode_region_batch): the full decode of an image, cropped to a pixel
// rectangle, bit for bit, at the cost of the rectangle's blocks (decode.swift:4154-4165, 4182-4276, 4291-4298).
//
// k_region_decode<planes, rgb>: one launch for a batch of identically laid out images, each with its own rectangle, on
// tile_decode.hpp's rectangle grid and tile body at N = 8.  A tile is at most 16 x 8 luma blocks (128 x 64 pixels) of the
// rectangle's block window.
//
// k_region_crop: the fallback of every other layout, whole decoded images cut to their rectangles.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "tile_decode.hpp"

namespace jpeg_amd {

namespace {

constexpr int kTileH = 64;   // pixels
// The chroma window of a tile: 1x1 chroma at scale 2 reads 64 + 2 samples per 128 pixels (10 blocks at most), at scale 1
// (a full-factor axis of 4:2:2 / 4:4:0) the samples under the tile's pixels and the zero-weight neighbour one past them
// (17 blocks); vertically 34 (6 blocks) or 65 samples (9 blocks).
constexpr int kChromaW = 8 * 17, kChromaH = 8 * 9;

struct RegionArgs {
    TileArgs t;
    RectArgs rect;
};

template <int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_region_decode(RegionArgs a)
{
    Tile tile;
    if (rect_tile<8, kTileH>(a.rect, nullptr, a.t, tile)) decode_tile<8, NP, RGB, kTileW, kTileH, kChromaW, kChromaH>(a.t, tile);
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

}  // namespace

hipError_t launch_region_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &L, const PlaneSet &coef, QuantaRef q,
                                bool rgb, const uint32_t *d_tiles, const int32_t *d_regions, uint32_t nwg,
                                uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0 || nwg == 0) return hipSuccess;
    const RegionArgs a{tile_args(L, 8, coef, q, d_pixels, pixel_stride),
                       RectArgs{d_tiles, reinterpret_cast<const int4 *>(d_regions), n_images}};
    const dim3 grid(nwg);
    if (L.nplanes == 1) {
        if (rgb) hipLaunchKernelGGL((k_region_decode<1, true>), grid, dim3(kThreads), 0, stream, a);
        else hipLaunchKernelGGL((k_region_decode<1, false>), grid, dim3(kThreads), 0, stream, a);
    } else {
        if (rgb) hipLaunchKernelGGL((k_region_decode<3, true>), grid, dim3(kThreads), 0, stream, a);
        else hipLaunchKernelGGL((k_region_decode<3, false>), grid, dim3(kThreads), 0, stream, a);
    }
    return hipGetLastError();
}

uint32_t region_tiles(const jpeg_amd_region &r) { return rect_tiles(8, kTileH, r); }

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

}  // namespace jpeg_amd
