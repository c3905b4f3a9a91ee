// kernels_view.hip -- view decode (jpeg_amd_decode_view_batch): per image a denominator and a rectangle of the scaled
// image's pixels.  include/jpeg_amd.h ("view decode") points to the contract, which is the scaled decode's, cropped.
//
// k_view_decode<N, planes, rgb>: one launch for the images of a call that share N = 8 / denom, each with its own
// rectangle, on tile_decode.hpp's rectangle grid and tile body.  An index list (index[i] = the image's place in the call)
// makes a call of mixed denominators one launch per denominator.  The tile is the scaled kernel's: 128 x 32 output pixels.
// N = 8 gives the bytes of k_region_decode, for the denominator-1 images of a mixed call.
//
// k_view_decode_mixed<N, planes, rgb>: the same grid and body for images of DIFFERENT sizes and samplings
// (jpeg_amd_decode_view_mixed): one launch per (N, planes) of the call, every image with a record of its own in device
// memory in the place of the kernel argument.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include <cstring>

#include "tile_decode.hpp"

namespace jpeg_amd {

namespace {

constexpr int kTileH = 32;   // output pixels

struct ViewArgs {
    TileArgs t;
    RectArgs rect;                // regions: of the scaled image, [images of the call]
    const uint32_t *index;        // [n]: the launch's image i is image index[i] of the call
};

template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_view_decode(ViewArgs a)
{
    Tile tile;
    if (rect_tile<N, kTileH>(a.rect, a.index, a.t, tile))
        decode_tile<N, NP, RGB, kTileW, kTileH, chroma_span<N>(kTileW), chroma_span<N>(kTileH)>(a.t, tile);
}

template <int N>
void launch_view(dim3 grid, hipStream_t stream, int nplanes, bool rgb, const ViewArgs &a)
{
    if (nplanes == 1) {
        if (rgb) hipLaunchKernelGGL((k_view_decode<N, 1, true>), grid, dim3(kThreads), 0, stream, a);
        else hipLaunchKernelGGL((k_view_decode<N, 1, false>), grid, dim3(kThreads), 0, stream, a);
    } else {
        if (rgb) hipLaunchKernelGGL((k_view_decode<N, 3, true>), grid, dim3(kThreads), 0, stream, a);
        else hipLaunchKernelGGL((k_view_decode<N, 3, false>), grid, dim3(kThreads), 0, stream, a);
    }
}

// The same workgroup for the images of a mixed call (jpeg_amd_decode_view_mixed) that share N and the number of planes:
// sizes and samplings differ from image to image, so what decode_tile reads comes from the image's MixedRecord.
template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_view_decode_mixed(MixedArgs g)
{
    Tile tile;
    if (const MixedRecord *rec = mixed_tile<N, kTileH>(g, tile))
        decode_tile<N, NP, RGB, kTileW, kTileH, chroma_span<N>(kTileW), chroma_span<N>(kTileH)>(rec->t, tile);
}

template <int N>
void launch_mixed(dim3 grid, hipStream_t stream, int nplanes, bool rgb, const MixedArgs &g)
{
    if (nplanes == 1) {
        if (rgb) hipLaunchKernelGGL((k_view_decode_mixed<N, 1, true>), grid, dim3(kThreads), 0, stream, g);
        else hipLaunchKernelGGL((k_view_decode_mixed<N, 1, false>), grid, dim3(kThreads), 0, stream, g);
    } else {
        if (rgb) hipLaunchKernelGGL((k_view_decode_mixed<N, 3, true>), grid, dim3(kThreads), 0, stream, g);
        else hipLaunchKernelGGL((k_view_decode_mixed<N, 3, false>), grid, dim3(kThreads), 0, stream, g);
    }
}

}  // namespace

size_t mixed_record_bytes() { return sizeof(MixedRecord); }

void mixed_record(void *dst, const jpeg_amd_layout &L, int n, const int16_t *const d_coef[], const uint16_t *d_quanta,
                  const jpeg_amd_region &r, uint8_t *d_pixels)
{
    PlaneSet coef{};
    for (int p = 0; p < L.nplanes; ++p) coef.ptr[p] = d_coef[p];
    const MixedRecord rec{tile_args(L, n, coef, QuantaRef{d_quanta, 0}, d_pixels, 0), int4{r.x, r.y, r.width, r.height}};
    memcpy(dst, &rec, sizeof rec);
}

hipError_t launch_view_decode_mixed(hipStream_t stream, int n_images, int n, int nplanes, bool rgb, const void *d_records,
                                    const uint32_t *d_index, const uint32_t *d_tiles, uint32_t nwg)
{
    if (n_images == 0 || nwg == 0) return hipSuccess;
    if (nplanes != 1 && nplanes != 3) return hipErrorInvalidValue;
    const MixedArgs g{static_cast<const MixedRecord *>(d_records), d_tiles, d_index, n_images};
    const dim3 grid(nwg);
    if (n == 8) launch_mixed<8>(grid, stream, nplanes, rgb, g);
    else if (n == 4) launch_mixed<4>(grid, stream, nplanes, rgb, g);
    else if (n == 2) launch_mixed<2>(grid, stream, nplanes, rgb, g);
    else if (n == 1) launch_mixed<1>(grid, stream, nplanes, rgb, g);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

uint32_t view_tiles(int n, const jpeg_amd_region &r) { return rect_tiles(n, kTileH, r); }

hipError_t launch_view_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &L, int n, const PlaneSet &coef, QuantaRef q,
                              bool rgb, const uint32_t *d_index, const uint32_t *d_tiles, const int32_t *d_regions, uint32_t nwg,
                              uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0 || nwg == 0) return hipSuccess;
    const ViewArgs a{tile_args(L, n, coef, q, d_pixels, pixel_stride),
                     RectArgs{d_tiles, reinterpret_cast<const int4 *>(d_regions), n_images}, d_index};
    const dim3 grid(nwg);
    if (n == 8) launch_view<8>(grid, stream, L.nplanes, rgb, a);
    else if (n == 4) launch_view<4>(grid, stream, L.nplanes, rgb, a);
    else if (n == 2) launch_view<2>(grid, stream, L.nplanes, rgb, a);
    else if (n == 1) launch_view<1>(grid, stream, L.nplanes, rgb, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace jpeg_amd
