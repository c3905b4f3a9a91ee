// kernels_view.hip -- view decode (jpeg_amd_decode_view_batch): per image a denominator and a rectangle of the scaled
// image's pixels.  include/jpeg_amd.h ("view decode") points to the contract, which is the scaled decode's, cropped; the
// butterflies and the tables are dct.hpp's, the interleave and colour arithmetic is interleave.hpp's, unchanged.
//
// k_view_decode<N, planes, rgb> is the product of k_region_decode and k_scaled_decode: one launch for the images of a
// call that share N = 8 / denom, each with its own rectangle.  From the region kernel it has the grid -- the sum over the
// launch's images of the rectangle's tiles, a host-staged prefix (tiles[i] = first workgroup of the launch's image i) and
// a binary search per workgroup; no counter, no state shared between workgroups -- and an index list (index[i] = the
// image's place in the call), so that a call of mixed denominators is one launch per denominator.  From the scaled kernel
// it has the tile: 128 x 32 output pixels, 128 / N x 32 / N luma blocks, anchored on the block grid of the rectangle's
// window and clipped to the rectangle.  Its workgroup
//   1. modulates the image's N x N tables into LDS and writes the per-column / per-row interleave maps of its chroma
//      planes (the sample pair and the fraction of decode.swift:4240-4251, tile-local), with last = N units - 1;
//   2. transforms every block of every plane that the tile's pixels read (axis_span, the chroma halo included), one
//      block per work-item and trip, into byte samples in LDS; a work-item fetches only the head of its block;
//   3. writes the tile's pixels: upsample from LDS, colour, three byte stores per pixel.
// N = 8 is the full-size transform (load_block, idct_block): the bytes of k_region_decode, for the denominator-1 images
// of a mixed call.  Layouts: those of fused_decode_supported.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "dct.hpp"
#include "fused_common.hpp"
#include "interleave.hpp"
#include "kernels.hpp"

namespace jpeg_amd {

namespace {

constexpr int kTileW = 128, kTileH = 32;   // output pixels per tile

// The chroma window of a tile in samples, as kernels_scaled.hip's: along an axis at the image's scale the samples under
// the tile's pixels and the zero-weight neighbour one past them, at half of it half as many plus one on each side; the
// window starts and ends on a block, which adds at most N - 1 samples at each end.
template <int N> constexpr int chroma_w() { return kTileW + 2 * N; }
template <int N> constexpr int chroma_h() { return kTileH + 2 * N; }

struct ViewArgs {
    const int16_t *coef[3];
    size_t coef_stride[3];        // int16 elements between images
    int ux[3], qi[3];
    InterleaveAxis ax[3], ay[3];  // of the SCALED image: last = N units - 1
    const uint16_t *quanta;
    size_t quanta_stride;         // uint16 elements between images' table sets
    const uint32_t *index;        // [n]: the launch's image i is image index[i] of the call
    const uint32_t *tiles;        // [n + 1]: first workgroup of the launch's image i; tiles[n] = the grid
    const int4 *regions;          // [images of the call]: x, y, width, height in pixels of the scaled image
    int n_images;                 // of the launch
    uint8_t *pixels;
    size_t pixel_stride;          // bytes between images
};

// One block of the window into N x N byte samples at dst (pitch bytes between rows; dst aligned to N): the contract's
// passes at level 2^7 + 1/2, from the head of the block that holds the coefficients they read.
template <int N>
__device__ __forceinline__ void block_to_samples(const int16_t *src, const float *q, uint8_t *dst, int pitch)
{
    if constexpr (N == 8) {
        uint32_t w[32];
        load_block(src, w);
        float g[64];
        idct_block(w, q, 128.5f, g);
#pragma unroll
        for (int y = 0; y < 8; ++y) store_sample_row(dst + y * pitch, g + 8 * y, 255.0f);
    } else {
        uint32_t w[scaled_head_words<N>()];
        load_block_head<N>(src, w);
        float g[N * N];
        idct_block_scaled<N>(w, q, 128.5f, g);
#pragma unroll
        for (int y = 0; y < N; ++y) {
            uint32_t v = 0;
#pragma unroll
            for (int x = 0; x < N; ++x) v |= clamp_trunc(g[N * y + x], 255.0f) << (8 * x);
            if constexpr (N == 4) *reinterpret_cast<uint32_t *>(dst + y * pitch) = v;
            else if constexpr (N == 2) *reinterpret_cast<uint16_t *>(dst + y * pitch) = (uint16_t)v;
            else dst[y * pitch] = (uint8_t)v;
        }
    }
}

template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_view_decode(ViewArgs a)
{
    constexpr int kLumaBytes = kTileW * kTileH;
    constexpr int kChromaBytes = chroma_w<N>() * chroma_h<N>();
    static_assert(kLumaBytes % 8 == 0 && kChromaBytes % N == 0 && N * N * NP <= kThreads && kTileW + kTileH <= kThreads, "LDS carve and roles");
    __shared__ __attribute__((aligned(16))) uint8_t smp[kLumaBytes + (NP == 3 ? 2 * kChromaBytes : 0)];
    __shared__ float sq[NP][N * N];
    __shared__ uint32_t colmap[kTileW], rowmap[kTileH];   // chroma: sample i | neighbour j << 16, tile-local
    __shared__ float colt[kTileW], rowt[kTileH];          // chroma: the fractions tx, ty

    const uint32_t wg = blockIdx.x;
    int lo = 0, hi = a.n_images;                          // the launch's image: the last i with tiles[i] <= wg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.tiles[mid] <= wg) lo = mid; else hi = mid;
    }
    const int img = (int)a.index[lo];
    const int4 r = a.regions[img];
    const int tile = (int)(wg - a.tiles[lo]);
    const int ax0 = N * (r.x / N), ay0 = N * (r.y / N);   // the tile grid's anchor: the first block of the luma window
    const int ntx = (r.x + r.z - 1 - ax0) / kTileW + 1;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int px0 = max(r.x, ax0 + kTileW * tx), px1 = min(r.x + r.z, ax0 + kTileW * (tx + 1));
    const int py0 = max(r.y, ay0 + kTileH * ty), py1 = min(r.y + r.w, ay0 + kTileH * (ty + 1));
    if (px1 <= px0 || py1 <= py0) return;                 // a prefix that is not this rectangle's: a host bug -- write nothing

    // block window of each plane (plane 2 has plane 1's factors: the same window)
    int wx0[NP], wy0[NP], wbx[NP], wby[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        int slo, shi;
        axis_span(a.ax[p], px0, px1 - 1, slo, shi);
        wx0[p] = slo / N; wbx[p] = shi / N - wx0[p] + 1;
        axis_span(a.ay[p], py0, py1 - 1, slo, shi);
        wy0[p] = slo / N; wby[p] = shi / N - wy0[p] + 1;
    }
    // the LDS bounds above hold for every layout the host sends here; a window past them is a host bug -- stop, write nothing
    if (N * wbx[0] > kTileW || N * wby[0] > kTileH) return;
    if (NP == 3 && (N * wbx[1] > chroma_w<N>() || N * wby[1] > chroma_h<N>())) return;

    const int t = threadIdx.x;
    if (t < N * N * NP) {
        const int p = t / (N * N), e = t - p * (N * N), k = e % N, h = e / N;
        const uint16_t *q = a.quanta + (size_t)img * a.quanta_stride + 64 * a.qi[p];
        sq[p][e] = modulate_entry_scaled<N>(k, h, q[zigzag_of(k, h)]);
    }
    if constexpr (NP == 3) {
        // interleave maps of the chroma planes, decode.swift:4240-4251 (tile-local sample indices)
        const InterleaveAxis &mx = a.ax[1], &my = a.ay[1];
        if (t < kTileW && t < px1 - px0) {
            const int x = px0 + t, i = axis_index(mx, x), j = axis_neighbour(mx, x);
            colmap[t] = (uint32_t)(i - N * wx0[1]) | (uint32_t)(j - N * wx0[1]) << 16;
            colt[t] = axis_fraction(mx, x);
        }
        const int u = t - kTileW;
        if (u >= 0 && u < kTileH && u < py1 - py0) {
            const int y = py0 + u, i = axis_index(my, y), j = axis_neighbour(my, y);
            rowmap[u] = (uint32_t)(i - N * wy0[1]) | (uint32_t)(j - N * wy0[1]) << 16;
            rowt[u] = axis_fraction(my, y);
        }
    }
    __syncthreads();

    // every block of the windows into byte samples
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
        const int pitch = N * wbx[p];
        block_to_samples<N>(a.coef[p] + (size_t)img * a.coef_stride[p] + (size_t)64 * ((size_t)(wy0[p] + ly) * a.ux[p] + wx0[p] + lx),
                            &sq[p][0], smp + base[p] + N * ly * pitch + N * lx, pitch);
    }
    __syncthreads();

    // the tile's pixels: Planar.interleaved + Rectangular.unpack(as:), literal arithmetic (interleave.hpp)
    const int tw = px1 - px0, th = py1 - py0;
    FastDiv dw;
    dw.set((uint32_t)tw);
    const int pitch0 = N * wbx[0];
    const uint8_t *s0 = smp + (py0 - N * wy0[0]) * pitch0 + (px0 - N * wx0[0]);
    const size_t row_bytes = 3 * (size_t)r.z;
    uint8_t *out = a.pixels + (size_t)img * a.pixel_stride + 3 * ((size_t)(py0 - r.y) * r.z + (px0 - r.x));
    for (uint32_t i = t; i < (uint32_t)(tw * th); i += kThreads) {
        uint32_t c;
        const uint32_t rr = dw.div(i, c);
        const uint32_t yv = s0[rr * pitch0 + c];
        uint32_t cb = 128u, cr = 128u;                        // a grey image is (y, 128, 128), jpeg.swift:499-503, 557-561
        if constexpr (NP == 3) {
            const int pitch1 = N * wbx[1];
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

}  // namespace

uint32_t view_tiles(int n, const jpeg_amd_region &r)
{
    const int ax0 = n * (r.x / n), ay0 = n * (r.y / n);
    return (uint32_t)((r.x + r.width - 1 - ax0) / kTileW + 1) * (uint32_t)((r.y + r.height - 1 - ay0) / kTileH + 1);
}

hipError_t launch_view_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &L, int n, const PlaneSet &coef, QuantaRef q,
                              bool rgb, const uint32_t *d_index, const uint32_t *d_tiles, const int32_t *d_regions, uint32_t nwg,
                              uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0 || nwg == 0) return hipSuccess;
    ViewArgs a{};
    for (int p = 0; p < L.nplanes; ++p) {
        a.coef[p] = static_cast<const int16_t *>(coef.ptr[p]);
        a.coef_stride[p] = coef.stride[p];
        a.ux[p] = L.units_x[p];
        a.qi[p] = L.qi[p];
        a.ax[p] = interleave_axis(L, p, false, false);
        a.ay[p] = interleave_axis(L, p, false, true);
        a.ax[p].last = n * L.units_x[p] - 1;              // the scaled plane's padded edge in the place of 8 units - 1
        a.ay[p].last = n * L.units_y[p] - 1;
    }
    a.quanta = q.d_quanta;
    a.quanta_stride = q.image_stride;
    a.index = d_index;
    a.tiles = d_tiles;
    a.regions = reinterpret_cast<const int4 *>(d_regions);
    a.n_images = n_images;
    a.pixels = d_pixels;
    a.pixel_stride = pixel_stride;
    const dim3 grid(nwg);
    if (n == 8) launch_view<8>(grid, stream, L.nplanes, rgb, a);
    else if (n == 4) launch_view<4>(grid, stream, L.nplanes, rgb, a);
    else if (n == 2) launch_view<2>(grid, stream, L.nplanes, rgb, a);
    else if (n == 1) launch_view<1>(grid, stream, L.nplanes, rgb, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace jpeg_amd
