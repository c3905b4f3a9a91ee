// tile_decode.hpp -- the workgroup body that k_region_decode, k_scaled_decode, k_view_decode and k_view_decode_mixed share:
// one tile of output pixels of one image, straight from the coefficients, at N x N samples per block (N = 8 / denom in
// {8, 4, 2, 1}; N = 8 is the full-size transform).  The kernels differ in how a workgroup finds its image and its tile, in
// where what it reads of the image comes from (the kernel's arguments, or a record per image in device memory), in the
// tile's height and in the set of N they are built for; what a workgroup then does is decode_tile, written once:
//   1. modulate the image's N x N tables into LDS and write the per-column / per-row interleave maps of its chroma planes
//      (the sample pair and the fraction of decode.swift:4240-4251, tile-local), with last = N units - 1;
//   2. transform every block of every plane that the tile's pixels read -- axis_span of interleave.hpp, the chroma halo
//      included, clamped at the chroma plane's padded edge -- one block per work-item and trip, into byte samples in LDS;
//      for N < 8 a work-item fetches only the head of its block;
//   3. write the tile's pixels: upsample from LDS, colour, three byte stores per pixel (the rows of a rectangle have any
//      length and any alignment).
// The butterflies and the tables are dct.hpp's, the interleave and colour arithmetic is interleave.hpp's.
// Layouts: those of fused_decode_supported (y8; ycc8 with full-factor luma and 1x1 chroma at scale 1 or 2 per axis, centred).
//
// Compile every translation unit that instantiates decode_tile with -ffp-contract=off (see dct.hpp) and -fno-slp-vectorize.
#pragma once
#pragma clang fp contract(off)

#include "dct.hpp"
#include "fused_common.hpp"
#include "interleave.hpp"
#include "kernels.hpp"
#include "tile_staging.hpp"

namespace jpeg_amd {

// What decode_tile reads of a launch; each kernel's own argument struct holds one next to what finds its tiles.
struct TileArgs {
    const int16_t *coef[3];
    size_t coef_stride[3];        // int16 elements between images
    int ux[3], qi[3];
    InterleaveAxis ax[3], ay[3];  // of the image at N samples per block: last = N units - 1
    const uint16_t *quanta;
    size_t quanta_stride;         // uint16 elements between images' table sets
    uint8_t *pixels;
    size_t pixel_stride;          // bytes between images
};

// One block of the window into N x N byte samples at dst (pitch bytes between rows; dst aligned to N): the contract's
// passes at level 2^7 + 1/2 (decode.swift:4110-4111), from the head of the block that holds the coefficients they read.
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

// i / N for a sample or pixel index, which is never negative: a shift, without a signed division's correction.
template <int N> __device__ constexpr int udiv(int i) { return (int)((uint32_t)i / (uint32_t)N); }

// A workgroup's work: pixels [px0, px1) x [py0, py1) of image `img` -- at most TW x TH of them, starting on the block grid of
// N or clipped to a rectangle -- to `out`, the tile's first pixel, rows row_bytes apart.
struct Tile {
    int img, px0, px1, py0, py1;
    uint8_t *out;
    size_t row_bytes;
};

// A bound of a chroma plane's window along an axis of `tile` pixels, in samples: at the image's scale (4:2:2 / 4:4:0) the
// samples under the tile's pixels and the zero-weight neighbour one past them, at half of it half as many plus one on
// each side; the window starts and ends on a block, which adds at most N - 1 samples at each end.
template <int N> constexpr int chroma_span(int tile) { return tile + 2 * N; }

// The tile body.  CW x CH: the LDS a chroma plane's window gets, in samples.
template <int N, int NP, bool RGB, int TW, int TH, int CW, int CH>
__device__ __forceinline__ void decode_tile(const TileArgs &a, const Tile &tile)
{
    const int img = tile.img, px0 = tile.px0, px1 = tile.px1, py0 = tile.py0, py1 = tile.py1;
    constexpr int kLumaBytes = TW * TH, kChromaBytes = CW * CH;
    static_assert(kLumaBytes % 8 == 0 && kChromaBytes % N == 0 && N * N * NP <= kThreads && TW + TH <= kThreads, "LDS carve and roles");
    __shared__ __attribute__((aligned(16))) uint8_t smp[kLumaBytes + (NP == 3 ? 2 * kChromaBytes : 0)];
    __shared__ float sq[NP][N * N];
    __shared__ uint32_t colmap[TW], rowmap[TH];   // chroma: sample i | neighbour j << 16, tile-local
    __shared__ float colt[TW], rowt[TH];          // chroma: the fractions tx, ty

    // block window of each plane (plane 2 has plane 1's factors: the same window)
    int wx0[NP], wy0[NP], wbx[NP], wby[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        int slo, shi;
        axis_span(a.ax[p], px0, px1 - 1, slo, shi);
        wx0[p] = udiv<N>(slo); wbx[p] = udiv<N>(shi) - wx0[p] + 1;
        axis_span(a.ay[p], py0, py1 - 1, slo, shi);
        wy0[p] = udiv<N>(slo); wby[p] = udiv<N>(shi) - wy0[p] + 1;
    }
    // the LDS bounds above hold for every layout the host sends here; a window past them is a host bug -- stop, write nothing
    if (N * wbx[0] > TW || N * wby[0] > TH) return;
    if (NP == 3 && (N * wbx[1] > CW || N * wby[1] > CH)) return;

    const int t = threadIdx.x;
    if (t < N * N * NP) {
        const int p = t / (N * N), e = t - p * (N * N), k = e % N, h = e / N;
        const uint16_t *q = a.quanta + (size_t)img * a.quanta_stride + 64 * a.qi[p];
        sq[p][e] = modulate_entry_scaled<N>(k, h, q[zigzag_of(k, h)]);   // N = 8: scale 0x1p-3, decode.swift:4107
    }
    if constexpr (NP == 3) {
        // interleave maps of the chroma planes, decode.swift:4240-4251 (tile-local sample indices)
        const InterleaveAxis &mx = a.ax[1], &my = a.ay[1];
        if (t < TW && t < px1 - px0) {
            const int x = px0 + t, i = axis_index(mx, x), j = axis_neighbour(mx, x);
            colmap[t] = (uint32_t)(i - N * wx0[1]) | (uint32_t)(j - N * wx0[1]) << 16;
            colt[t] = axis_fraction(mx, x);
        }
        const int u = t - TW;
        if (u >= 0 && u < TH && u < py1 - py0) {
            const int y = py0 + u, i = axis_index(my, y), j = axis_neighbour(my, y);
            rowmap[u] = (uint32_t)(i - N * wy0[1]) | (uint32_t)(j - N * wy0[1]) << 16;
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
        uint8_t *o = tile.out + rr * tile.row_bytes + 3 * c;
        o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
    }
}

// ---- the rectangle kernels: per image a pixel rectangle of the image at N samples per block ------------------------------
// The grid is the sum over the launch's images of each rectangle's tiles.  The host stages a prefix of those counts
// (tiles[i] = first workgroup of the launch's image i, tiles[n] = the grid) with the rectangles; a workgroup finds its image
// by a binary search over the prefix.  No counter, no state shared between workgroups.  Tiles are TW x TH pixels, anchored
// on the first block of the rectangle's luma window and clipped to the rectangle.
struct RectArgs {
    const uint32_t *tiles;        // [n + 1]
    const int4 *regions;          // [images of the call]: x, y, width, height in pixels
    int n_images;                 // of the launch
};

// The launch's image of workgroup wg: the last i with tiles[i] <= wg.
__device__ __forceinline__ int rect_image(const uint32_t *tiles, int n_images, uint32_t wg)
{
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tiles[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

// Tile number `tile` of rectangle r, whose first pixel is at `base`: everything of t but img; false: r has no such tile.
template <int N, int TH>
__device__ __forceinline__ bool tile_of_rect(const int4 &r, int tile, uint8_t *base, Tile &t)
{
    const int ax0 = N * udiv<N>(r.x), ay0 = N * udiv<N>(r.y);   // the tile grid's anchor: the luma window's first block
    const int ntx = udiv<kTileW>(r.x + r.z - 1 - ax0) + 1;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    t.px0 = max(r.x, ax0 + kTileW * tx); t.px1 = min(r.x + r.z, ax0 + kTileW * (tx + 1));
    t.py0 = max(r.y, ay0 + TH * ty); t.py1 = min(r.y + r.w, ay0 + TH * (ty + 1));
    t.row_bytes = 3 * (size_t)r.z;
    t.out = base + 3 * ((size_t)(t.py0 - r.y) * r.z + (t.px0 - r.x));
    return t.px1 > t.px0 && t.py1 > t.py0;                // a prefix that is not this rectangle's: a host bug -- write nothing
}

// Workgroup blockIdx.x's tile; false: it has none.  index: [n], the launch's image i is image index[i] of the call and has
// that image's rectangle, or nullptr: it is image i.
template <int N, int TH>
__device__ __forceinline__ bool rect_tile(const RectArgs &g, const uint32_t *index, const TileArgs &a, Tile &t)
{
    const uint32_t wg = blockIdx.x;
    const int lo = rect_image(g.tiles, g.n_images, wg);
    t.img = index ? (int)index[lo] : lo;
    const int4 r = g.regions[t.img];
    return tile_of_rect<N, TH>(r, (int)(wg - g.tiles[lo]), a.pixels + (size_t)t.img * a.pixel_stride, t);
}

// ---- the mixed rectangle kernel: every image of a launch with a geometry of its own ---------------------------------------
// The rectangle grid above, but what decode_tile reads of an image comes from device memory, not from the kernel's
// arguments: one record per image of the call, staged by the host with the prefix and the index list.  The record's
// pointers are the image's own (decode_tile runs with Tile::img = 0, the strides are not read), ux, qi, ax, ay with
// last = N units - 1 are its layout's, `region` is its rectangle of the scaled image.
struct MixedRecord {
    TileArgs t;
    int4 region;                  // x, y, width, height in pixels
};
static_assert(sizeof(MixedRecord) % 16 == 0, "records lie in an array that the host stages as bytes");

struct MixedArgs {
    const MixedRecord *records;   // [images of the call]
    const uint32_t *tiles;        // [n + 1]
    const uint32_t *index;        // [n]: the launch's image i is image index[i] of the call
    int n_images;                 // of the launch
};

// Workgroup blockIdx.x's image -- its record, which decode_tile then reads in place -- and tile; nullptr: it has none.
// The record's address is the same for every work-item of the workgroup.
template <int N, int TH>
__device__ __forceinline__ const MixedRecord *mixed_tile(const MixedArgs &g, Tile &t)
{
    const uint32_t wg = blockIdx.x;
    const int lo = rect_image(g.tiles, g.n_images, wg);
    const MixedRecord *rec = g.records + g.index[lo];
    t.img = 0;
    const int4 r = rec->region;
    return tile_of_rect<N, TH>(r, (int)(wg - g.tiles[lo]), rec->t.pixels, t) ? rec : nullptr;
}

}  // namespace jpeg_amd
