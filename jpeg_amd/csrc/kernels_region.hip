// kernels_region.hip -- region decode (jpeg_amd_decode_region_batch): the full decode of an image, cropped to a pixel
// rectangle, bit for bit, at the cost of the rectangle's blocks (decode.swift:4154-4165, 4182-4276, 4291-4298).
//
// k_region_decode: one launch for a batch of identically laid out images, each with its own rectangle.  The grid is the
// sum over images of the rectangle's tiles; the host stages a prefix of those counts (tiles[i] = first workgroup of image i)
// with the rectangles, and a workgroup finds its image by a binary search over the prefix.  No counter, no state shared
// between workgroups.
//
// A tile is at most 16 x 8 luma blocks (128 x 64 pixels) of the rectangle's block window, clipped to the rectangle.  Its
// workgroup
//   1. modulates the image's tables into LDS and writes the per-column / per-row interleave maps of its chroma planes
//      (the sample pair and the fraction of decode.swift:4240-4251, tile-local);
//   2. transforms every block of every plane that the tile's pixels read -- axis_span of interleave.hpp, the chroma
//      halo included, clamped at the chroma plane's padded edge -- one block per work-item into byte samples in LDS;
//   3. writes the tile's pixels: upsample from LDS, colour, three byte stores per pixel (the rows of a region have any
//      length and any alignment).
// Layouts: those of fused_decode_supported (y8; ycc8 with full-factor luma and 1x1 chroma at scale 1 or 2 per axis, centred).
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "dct.hpp"
#include "fused_common.hpp"
#include "interleave.hpp"
#include "kernels.hpp"

namespace jpeg_amd {

namespace {

constexpr int kTileBX = 16, kTileBY = 8;                  // luma blocks per tile
constexpr int kTileW = 8 * kTileBX, kTileH = 8 * kTileBY;  // pixels
// The chroma window of a tile: 1x1 chroma at scale 2 reads 64 + 2 samples per 128 pixels (10 blocks at most), at scale 1
// (a full-factor axis of 4:2:2 / 4:4:0) the samples under the tile's pixels and the zero-weight neighbour one past them
// (17 blocks); vertically 34 (6 blocks) or 65 samples (9 blocks).
constexpr int kChromaBX = 17, kChromaBY = 9;
constexpr int kLumaBytes = 64 * kTileBX * kTileBY;
constexpr int kChromaBytes = 64 * kChromaBX * kChromaBY;

struct RegionArgs {
    const int16_t *coef[3];
    size_t coef_stride[3];        // int16 elements between images
    int ux[3], qi[3];
    InterleaveAxis ax[3], ay[3];
    const uint16_t *quanta;
    size_t quanta_stride;         // uint16 elements between images' table sets
    const uint32_t *tiles;        // [n + 1]: first workgroup of image i; tiles[n] = the grid
    const int4 *regions;          // [n]: x, y, width, height in pixels
    int n_images;
    uint8_t *pixels;
    size_t pixel_stride;          // bytes between images
};

template <int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_region_decode(RegionArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t smp[kLumaBytes + (NP == 3 ? 2 * kChromaBytes : 0)];
    __shared__ float sq[NP][64];
    __shared__ uint32_t colmap[kTileW], rowmap[kTileH];   // chroma: sample i | neighbour j << 16, tile-local
    __shared__ float colt[kTileW], rowt[kTileH];          // chroma: the fractions tx, ty

    const uint32_t wg = blockIdx.x;
    int lo = 0, hi = a.n_images;                          // image: the last i with tiles[i] <= wg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.tiles[mid] <= wg) lo = mid; else hi = mid;
    }
    const int img = lo;
    const int4 r = a.regions[img];
    const int tile = (int)(wg - a.tiles[img]);
    const int bx0 = r.x >> 3, by0 = r.y >> 3;
    const int ntx = (((r.x + r.z - 1) >> 3) - bx0) / kTileBX + 1;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int px0 = max(r.x, 8 * (bx0 + kTileBX * tx)), px1 = min(r.x + r.z, 8 * (bx0 + kTileBX * (tx + 1)));
    const int py0 = max(r.y, 8 * (by0 + kTileBY * ty)), py1 = min(r.y + r.w, 8 * (by0 + kTileBY * (ty + 1)));

    // block window of each plane (plane 2 has plane 1's factors: the same window)
    int wx0[NP], wy0[NP], wbx[NP], wby[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        int slo, shi;
        axis_span(a.ax[p], px0, px1 - 1, slo, shi);
        wx0[p] = slo >> 3; wbx[p] = (shi >> 3) - wx0[p] + 1;
        axis_span(a.ay[p], py0, py1 - 1, slo, shi);
        wy0[p] = slo >> 3; wby[p] = (shi >> 3) - wy0[p] + 1;
    }
    // the LDS bounds above hold for every layout the host sends here; a window past them is a host bug -- stop, write nothing
    if (wbx[0] > kTileBX || wby[0] > kTileBY) return;
    if (NP == 3 && (wbx[1] > kChromaBX || wby[1] > kChromaBY)) return;

    const int t = threadIdx.x;
    if (t < 64 * NP) {
        const int p = t >> 6, k = t & 7, h = (t >> 3) & 7;
        const uint16_t *q = a.quanta + (size_t)img * a.quanta_stride + 64 * a.qi[p];
        sq[p][t & 63] = modulate_entry(k, h, 0.125f, q[zigzag_of(k, h)]);   // scale 0x1p-3, decode.swift:4107
    }
    if constexpr (NP == 3) {
        // interleave maps of the chroma planes, decode.swift:4240-4251 (tile-local sample indices)
        const InterleaveAxis &mx = a.ax[1], &my = a.ay[1];
        if (t < kTileW && t < px1 - px0) {
            const int x = px0 + t, i = axis_index(mx, x), j = axis_neighbour(mx, x);
            colmap[t] = (uint32_t)(i - 8 * wx0[1]) | (uint32_t)(j - 8 * wx0[1]) << 16;
            colt[t] = axis_fraction(mx, x);
        }
        const int u = t - kTileW;
        if (u >= 0 && u < kTileH && u < py1 - py0) {
            const int y = py0 + u, i = axis_index(my, y), j = axis_neighbour(my, y);
            rowmap[u] = (uint32_t)(i - 8 * wy0[1]) | (uint32_t)(j - 8 * wy0[1]) << 16;
            rowt[u] = axis_fraction(my, y);
        }
    }
    __syncthreads();

    // every block of the windows: Spectral.Plane.idct (decode.swift:4101-4133) into byte samples
    int base[NP], nblk[NP], total = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        base[p] = p == 0 ? 0 : kLumaBytes + (p - 1) * kChromaBytes;
        nblk[p] = wbx[p] * wby[p];
        total += nblk[p];
    }
    for (int b = t; b < total; b += kThreads) {
        int p = 0, k = b;
#pragma unroll
        for (int s = 0; s + 1 < NP; ++s)
            if (p == s && k >= nblk[s]) { k -= nblk[s]; p = s + 1; }
        const int ly = k / wbx[p], lx = k - ly * wbx[p];
        uint32_t w[32];
        load_block(a.coef[p] + (size_t)img * a.coef_stride[p] + (size_t)64 * ((size_t)(wy0[p] + ly) * a.ux[p] + wx0[p] + lx), w);
        float g[64];
        idct_block(w, &sq[p][0], 128.5f, g);                 // level 2^7 + 1/2 (decode.swift:4110-4111)
        const int pitch = 8 * wbx[p];
        uint8_t *dst = smp + base[p] + 8 * ly * pitch + 8 * lx;
#pragma unroll
        for (int y = 0; y < 8; ++y) store_sample_row(dst + y * pitch, g + 8 * y, 255.0f);
    }
    __syncthreads();

    // the tile's pixels: Planar.interleaved + Rectangular.unpack(as:), literal arithmetic (interleave.hpp)
    const int tw = px1 - px0, th = py1 - py0;
    FastDiv dw;
    dw.set((uint32_t)tw);
    const int pitch0 = 8 * wbx[0];
    const uint8_t *s0 = smp + (py0 - 8 * wy0[0]) * pitch0 + (px0 - 8 * wx0[0]);
    uint8_t *out = a.pixels + (size_t)img * a.pixel_stride + 3 * ((size_t)(py0 - r.y) * r.z + (px0 - r.x));
    const size_t row_bytes = 3 * (size_t)r.z;
    for (uint32_t i = t; i < (uint32_t)(tw * th); i += kThreads) {
        uint32_t c;
        const uint32_t rr = dw.div(i, c);
        const uint32_t yv = s0[rr * pitch0 + c];
        uint32_t cb = 128u, cr = 128u;                        // a grey image is (y, 128, 128), jpeg.swift:499-503, 557-561
        if constexpr (NP == 3) {
            const int pitch1 = 8 * wbx[1];
            const uint8_t *s1 = smp + kLumaBytes, *s2 = smp + kLumaBytes + kChromaBytes;
            const uint32_t cm = colmap[c], rm = rowmap[rr];
            const uint32_t i0 = cm & 0xffffu, j0 = cm >> 16, i1 = (rm & 0xffffu) * pitch1, j1 = (rm >> 16) * pitch1;
            if (a.ax[1].direct) {                            // 4:4:4: the sample under the pixel
                cb = s1[i1 + i0];
                cr = s2[i1 + i0];
            } else {
                const float fx = colt[c], fy = rowt[rr];
                cb = bilinear_sample((float)s1[i1 + i0], (float)s1[i1 + j0], (float)s1[j1 + i0], (float)s1[j1 + j0], fx, fy);
                cr = bilinear_sample((float)s2[i1 + i0], (float)s2[i1 + j0], (float)s2[j1 + i0], (float)s2[j1 + j0], fx, fy);
            }
        }
        uint32_t o0 = yv, o1 = cb, o2 = cr;
        if constexpr (RGB) ycc_to_rgb((float)yv, (float)cb, (float)cr, o0, o1, o2);
        uint8_t *o = out + rr * row_bytes + 3 * c;
        o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
    }
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
    RegionArgs a{};
    for (int p = 0; p < L.nplanes; ++p) {
        a.coef[p] = static_cast<const int16_t *>(coef.ptr[p]);
        a.coef_stride[p] = coef.stride[p];
        a.ux[p] = L.units_x[p];
        a.qi[p] = L.qi[p];
        a.ax[p] = interleave_axis(L, p, false, false);
        a.ay[p] = interleave_axis(L, p, false, true);
    }
    a.quanta = q.d_quanta;
    a.quanta_stride = q.image_stride;
    a.tiles = d_tiles;
    a.regions = reinterpret_cast<const int4 *>(d_regions);
    a.n_images = n_images;
    a.pixels = d_pixels;
    a.pixel_stride = pixel_stride;
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

uint32_t region_tiles(const jpeg_amd_region &r)
{
    const int bx0 = r.x >> 3, by0 = r.y >> 3;
    const uint32_t nbx = (uint32_t)(((r.x + r.width - 1) >> 3) - bx0 + 1), nby = (uint32_t)(((r.y + r.height - 1) >> 3) - by0 + 1);
    return ((nbx + kTileBX - 1) / kTileBX) * ((nby + kTileBY - 1) / kTileBY);
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

}  // namespace jpeg_amd
