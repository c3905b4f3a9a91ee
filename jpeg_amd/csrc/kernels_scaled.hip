// kernels_scaled.hip -- scaled decode (jpeg_amd_decode_scaled_batch): 1/2, 1/4 and 1/8 size pixels straight from the
// coefficients.  include/jpeg_amd.h ("scaled decode") holds the contract; the reduced butterflies and the table are in
// dct.hpp next to idct8 and modulate_entry.
//
// k_scaled_decode<N, planes, rgb>: one launch for a batch of identically laid out images on a static grid of
// (tiles per image) x (images), each workgroup tile_decode.hpp's tile body.  A tile is 128 x 32 OUTPUT pixels -- 128 / N x
// 32 / N luma blocks, so that a workgroup's output rows are 384-byte runs whatever N is.
//
// k_idct_scaled<N, T>: the fallback's transform of one plane into samples of T, padded to whole 8 x 8 blocks by edge
// replication, for the staged interleave kernel under jpeg_amd_scaled_layout's layout.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "tile_decode.hpp"

namespace jpeg_amd {

namespace {

constexpr int kTileH = 32;   // output pixels

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
    tile.py0 = kTileH * ty; tile.py1 = min(a.height, tile.py0 + kTileH);
    tile.row_bytes = 3 * (size_t)a.width;
    tile.out = a.t.pixels + (size_t)tile.img * a.t.pixel_stride + (size_t)tile.py0 * tile.row_bytes + 3 * (size_t)tile.px0;
    decode_tile<N, NP, RGB, kTileW, kTileH, chroma_span<N>(kTileW), chroma_span<N>(kTileH)>(a.t, tile);
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

}  // namespace

hipError_t launch_scaled_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &L, int n, int width, int height,
                                const PlaneSet &coef, QuantaRef q, bool rgb, uint8_t *d_pixels, size_t pixel_stride)
{
    if (n_images == 0) return hipSuccess;
    const int tiles_x = (width + kTileW - 1) / kTileW;
    const ScaledArgs a{tile_args(L, n, coef, q, d_pixels, pixel_stride), width, height, tiles_x};
    const dim3 grid((unsigned)tiles_x * (unsigned)((height + kTileH - 1) / kTileH), (unsigned)n_images);
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
