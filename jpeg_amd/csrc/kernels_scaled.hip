// kernels_scaled.hip -- scaled decode (jpeg_amd_decode_scaled_batch): 1/2, 1/4 and 1/8 size pixels straight from the
// coefficients.  include/jpeg_amd.h ("scaled decode") holds the contract; the reduced butterflies and the table are in
// dct.hpp next to idct8 and modulate_entry, the interleave and colour arithmetic is interleave.hpp's, unchanged.
//
// k_scaled_decode<N, planes, rgb>: one launch for a batch of identically laid out images on a static grid of
// (tiles per image) x (images).  A tile is 128 x 32 OUTPUT pixels -- 128 / N x 32 / N luma blocks, so that a workgroup's
// output rows are 384-byte runs whatever N is.  Its workgroup
//   1. modulates the image's N x N tables into LDS and writes the per-column / per-row interleave maps of its chroma
//      planes (the sample pair and the fraction of decode.swift:4240-4251, tile-local), with last = N units - 1;
//   2. transforms every block of every plane that the tile's pixels read (axis_span, the chroma halo included), one
//      block per work-item and trip, into byte samples in LDS; a work-item fetches only the head of its block;
//   3. writes the tile's pixels: upsample from LDS, colour, three byte stores per pixel.
// Layouts: those of fused_decode_supported (y8; ycc8 with full-factor luma and 1x1 chroma at scale 1 or 2 per axis, centred).
//
// k_idct_scaled<N, T>: the fallback's transform of one plane into samples of T, padded to whole 8 x 8 blocks by edge
// replication, for the staged interleave kernel under jpeg_amd_scaled_layout's layout.
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

// The chroma window of a tile in samples: along an axis at the image's scale (4:2:2 / 4:4:0) the samples under the
// tile's pixels and the zero-weight neighbour one past them, at half of it half as many plus one on each side; the
// window starts and ends on a block, which adds at most N - 1 samples at each end.
template <int N> constexpr int chroma_w() { return kTileW + 2 * N; }
template <int N> constexpr int chroma_h() { return kTileH + 2 * N; }

struct ScaledArgs {
    const int16_t *coef[3];
    size_t coef_stride[3];        // int16 elements between images
    int ux[3], qi[3];
    InterleaveAxis ax[3], ay[3];  // of the SCALED image: last = N units - 1
    const uint16_t *quanta;
    size_t quanta_stride;         // uint16 elements between images' table sets
    int width, height;            // W', H'
    int tiles_x;
    uint8_t *pixels;
    size_t pixel_stride;          // bytes between images
};

// N x N samples of one block, clamp_trunc'ed, as bytes at dst (pitch bytes between rows; dst aligned to N).
template <int N>
__device__ __forceinline__ void store_samples_lds(uint8_t *dst, int pitch, const float (&g)[N * N])
{
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

template <int N, int NP, bool RGB>
__global__ __launch_bounds__(kThreads) void k_scaled_decode(ScaledArgs a)
{
    constexpr int kLumaBytes = kTileW * kTileH;
    constexpr int kChromaBytes = chroma_w<N>() * chroma_h<N>();
    __shared__ __attribute__((aligned(16))) uint8_t smp[kLumaBytes + (NP == 3 ? 2 * kChromaBytes : 0)];
    __shared__ float sq[NP][N * N];
    __shared__ uint32_t colmap[kTileW], rowmap[kTileH];   // chroma: sample i | neighbour j << 16, tile-local
    __shared__ float colt[kTileW], rowt[kTileH];          // chroma: the fractions tx, ty

    const int img = blockIdx.y;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int px0 = kTileW * tx, px1 = min(a.width, px0 + kTileW);
    const int py0 = kTileH * ty, py1 = min(a.height, py0 + kTileH);

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

    // every block of the windows into byte samples (the contract's passes; level 2^7 + 1/2)
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
        uint32_t w[scaled_head_words<N>()];
        load_block_head<N>(a.coef[p] + (size_t)img * a.coef_stride[p] + (size_t)64 * ((size_t)(wy0[p] + ly) * a.ux[p] + wx0[p] + lx), w);
        float g[N * N];
        idct_block_scaled<N>(w, &sq[p][0], 128.5f, g);
        const int pitch = N * wbx[p];
        store_samples_lds<N>(smp + base[p] + N * ly * pitch + N * lx, pitch, g);
    }
    __syncthreads();

    // the tile's pixels: Planar.interleaved + Rectangular.unpack(as:), literal arithmetic (interleave.hpp)
    const int tw = px1 - px0, th = py1 - py0;
    FastDiv dw;
    dw.set((uint32_t)tw);
    const int pitch0 = N * wbx[0];
    const uint8_t *s0 = smp + (py0 - N * wy0[0]) * pitch0 + (px0 - N * wx0[0]);
    const size_t row_bytes = 3 * (size_t)a.width;
    uint8_t *out = a.pixels + (size_t)img * a.pixel_stride + (size_t)py0 * row_bytes + 3 * (size_t)px0;
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

template <int N, int NP>
void launch_scaled(dim3 grid, hipStream_t stream, bool rgb, const ScaledArgs &a)
{
    if (rgb) hipLaunchKernelGGL((k_scaled_decode<N, NP, true>), grid, dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL((k_scaled_decode<N, NP, false>), grid, dim3(kThreads), 0, stream, a);
}

// interleave_axis with the scaled plane's padded edge: last = N units - 1 in the place of 8 units - 1
InterleaveAxis scaled_interleave_axis(const jpeg_amd_layout &L, int p, bool cosited, bool vertical, int n)
{
    InterleaveAxis m = interleave_axis(L, p, cosited, vertical);
    m.last = n * (vertical ? L.units_y[p] : L.units_x[p]) - 1;
    return m;
}

}  // namespace

hipError_t launch_scaled_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &L, int n, int width, int height,
                                const PlaneSet &coef, QuantaRef q, bool rgb, uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0) return hipSuccess;
    ScaledArgs a{};
    for (int p = 0; p < L.nplanes; ++p) {
        a.coef[p] = static_cast<const int16_t *>(coef.ptr[p]);
        a.coef_stride[p] = coef.stride[p];
        a.ux[p] = L.units_x[p];
        a.qi[p] = L.qi[p];
        a.ax[p] = scaled_interleave_axis(L, p, false, false, n);
        a.ay[p] = scaled_interleave_axis(L, p, false, true, n);
    }
    a.quanta = q.d_quanta;
    a.quanta_stride = q.image_stride;
    a.width = width;
    a.height = height;
    a.tiles_x = (width + kTileW - 1) / kTileW;
    a.pixels = d_pixels;
    a.pixel_stride = pixel_stride;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)((height + kTileH - 1) / kTileH), (unsigned)n_images);
    if (L.nplanes == 1) {
        if (n == 4) launch_scaled<4, 1>(grid, stream, rgb, a);
        else if (n == 2) launch_scaled<2, 1>(grid, stream, rgb, a);
        else launch_scaled<1, 1>(grid, stream, rgb, a);
    } else {
        if (n == 4) launch_scaled<4, 3>(grid, stream, rgb, a);
        else if (n == 2) launch_scaled<2, 3>(grid, stream, rgb, a);
        else launch_scaled<1, 3>(grid, stream, rgb, a);
    }
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
