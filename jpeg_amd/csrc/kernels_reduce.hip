// kernels_reduce.hip -- spectral reduce (jpeg_amd_spectral_reduce_batch): a Spectral at 1/2, 1/4 or 1/8 size, coefficients in
// and coefficients out, in ONE launch for every plane of a batch.  include/jpeg_amd.h ("spectral reduce") holds the contract:
// the scaled-decode samples of each plane (dct.hpp: load_block_head, idct_block_scaled), edge-replicated to the output's whole
// blocks, through Spectral.Plane.fdct (encode.swift:199-248: fdct_block, the x8 modulated table, the quotient rounded half
// away from zero -- k_fdct_plane's literal true division).  A per-plane operation: no interleave, no colour, no halo, so every
// layout takes this kernel.
//
// Work decomposition: a workgroup of T x T work-items owns a tile of T x T OUTPUT blocks of one plane = 8 T x 8 T samples, which
// are the N x N samples of T D x T D source blocks (D = 8 / N = denom).  T = 16 at N = 4 and 2; T = 8 (one wave) at N = 1, where
// a 16 x 16 tile is 16384 source blocks and an 8192 x 8192 4:2:0 image only 96 workgroups (tile_side; DESIGN.md 8f has the
// runs that tried both shapes at N = 2 and N = 1).
//   Phase A  one SOURCE block per work-item and step: head fetch, reduced transform, clamp and truncate into the uint16 sample
//            tile in LDS.  A wave's lanes take 64 consecutive source blocks of one row (at N = 1 that is one 2-byte read from
//            each of 64 consecutive 128-byte lines: no line is read twice, and they are read in address order).  Block
//            coordinates are clamped to the plane; a slot past the plane's edge then repeats the edge block's last column /
//            row, which is the contract's sample-wise replication.  Rows of source blocks under no output block are skipped.
//   Phase B  one OUTPUT block per work-item: eight 16-byte LDS reads (T consecutive lanes read one sample row; at T = 8 the row
//            pitch is padded by 16 bytes so that the lane groups of ds_read_b128 meet no bank twice), fdct_block, quantise,
//            zigzag pack; the packed blocks go back through LDS
//            so that every store instruction writes eight neighbouring blocks, one 1 KiB run (as k_spectral_transform).
//
// The plane of a workgroup is uniform: every plane's tiles start at a workgroup boundary; grid y carries the images.
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include "kernels.hpp"
#include "dct.hpp"

namespace jpeg_amd {

namespace {

// output blocks per tile side; the workgroup is tile_side^2 work-items
__host__ __device__ constexpr int tile_side(int n) { return n == 1 ? 8 : 16; }
constexpr int kSlot = 144;                // bytes per packed output block in LDS (128 + 16 of padding, as k_spectral_transform)

struct ReduceArgs {
    const int16_t *in[JPEG_AMD_MAX_PLANES];
    size_t in_stride[JPEG_AMD_MAX_PLANES];
    int16_t *out[JPEG_AMD_MAX_PLANES];
    size_t out_stride[JPEG_AMD_MAX_PLANES];
    int in_ux[JPEG_AMD_MAX_PLANES], in_uy[JPEG_AMD_MAX_PLANES];      // source plane units (>= 1)
    int out_ux[JPEG_AMD_MAX_PLANES], out_uy[JPEG_AMD_MAX_PLANES];    // output plane units
    int qi[JPEG_AMD_MAX_PLANES];
    uint32_t wg_first[JPEG_AMD_MAX_PLANES + 1];                      // first workgroup of each plane
    int nplanes;
    const uint16_t *q_in, *q_out;
    size_t q_stride;
    float level_in, level_out, limit;      // 2^(P-1) + 0.5; 8 * 2^(P-1); 2^P - 1
};

template <int N>
__global__ __launch_bounds__(tile_side(N) * tile_side(N)) void k_spectral_reduce(ReduceArgs a)
{
    constexpr int kTile = tile_side(N), kThreads = kTile * kTile;
    constexpr int kPitch = kTile == 8 ? 72 : 128;      // samples per row of the LDS sample tile
    constexpr int D = 8 / N, SW = kTile * D;           // source blocks per tile side
    static_assert(kThreads * kSlot >= 8 * kTile * kPitch * 2, "the packed blocks reuse the sample tile");
    __shared__ __attribute__((aligned(16))) uint8_t lds[kThreads * kSlot];
    __shared__ float sq_in[N * N], sq_out[64];
    uint16_t *samples = reinterpret_cast<uint16_t *>(lds);

    int p = 0;
    while (p + 1 < a.nplanes && blockIdx.x >= a.wg_first[p + 1]) ++p;
    const int ux = a.in_ux[p], uy = a.in_uy[p], oux = a.out_ux[p], ouy = a.out_uy[p];
    const size_t img = blockIdx.y;
    const int t = threadIdx.x;
    {
        const size_t tq = img * a.q_stride + (size_t)64 * a.qi[p];
        if (t < N * N) sq_in[t] = modulate_entry_scaled<N>(t % N, t / N, a.q_in[tq + zigzag_of(t % N, t / N)]);
        if (t < 64) sq_out[t] = modulate_entry(t & 7, t >> 3, 8.0f, a.q_out[tq + zigzag_of(t & 7, t >> 3)]);   // encode.swift:205-209
    }
    __syncthreads();

    const uint32_t w_in_plane = blockIdx.x - a.wg_first[p];
    const uint32_t tiles_x = ((uint32_t)oux + kTile - 1) / kTile;
    const int X0 = (int)(w_in_plane % tiles_x) * kTile, Y0 = (int)(w_in_plane / tiles_x) * kTile;   // output blocks
    const int vw = min(kTile, oux - X0), vh = min(kTile, ouy - Y0);                                 // the tile's blocks inside the plane

    // ---- phase A: source blocks -> samples ----
    // work-item t keeps its column sx of source blocks and walks rows r0, r0 + RS, ...; U rows per trip, their head loads
    // issued together (rows past the tile's last are loaded from a clamped, valid address and dropped)
    {
        constexpr int RS = kThreads / SW;                  // rows of source blocks per step: 8, 4, 1
        constexpr int U = N == 1 ? 16 : N == 2 ? 8 : 2;    // steps per trip: 16, 32 and 32 head dwords in flight
        static_assert(SW <= kThreads && kThreads % SW == 0, "whole rows per step");
        const int sx = t % SW, r0 = t / SW;
        const int rows = vh * D;
        if (sx < vw * D) {
            const int bx = X0 * D + sx;
            const bool px = bx >= ux;                      // past the plane: the edge block's last column
            const int16_t *src = a.in[p] + img * a.in_stride[p] + (size_t)64 * min(bx, ux - 1);
            for (int sy0 = r0; sy0 < rows; sy0 += RS * U) {
                uint32_t w[U][scaled_head_words<N>()];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    load_block_head<N>(src + (size_t)64 * ux * (size_t)min(Y0 * D + sy0 + u * RS, uy - 1), w[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int sy = sy0 + u * RS;
                    if (sy >= rows) continue;
                    const bool py = Y0 * D + sy >= uy;     // ... the edge block's last row
                    float g[N * N];
                    idct_block_scaled<N>(w[u], sq_in, a.level_in, g);
                    uint32_t s[N * N];
#pragma unroll
                    for (int i = 0; i < N * N; ++i) s[i] = clamp_trunc(g[i], a.limit);
                    uint16_t *dst = samples + (N * sy) * kPitch + N * sx;
#pragma unroll
                    for (int y = 0; y < N; ++y) {
                        uint32_t r[N];
#pragma unroll
                        for (int x = 0; x < N; ++x) {
                            const uint32_t inrow = py ? s[N * (N - 1) + x] : s[N * y + x];
                            const uint32_t last = py ? s[N * (N - 1) + N - 1] : s[N * y + N - 1];
                            r[x] = px ? last : inrow;
                        }
                        if constexpr (N == 4) *reinterpret_cast<uint2 *>(dst + y * kPitch) = uint2{r[0] | (r[1] << 16), r[2] | (r[3] << 16)};
                        else if constexpr (N == 2) *reinterpret_cast<uint32_t *>(dst + y * kPitch) = r[0] | (r[1] << 16);
                        else dst[y * kPitch] = (uint16_t)r[0];
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- phase B: samples -> one output block per work-item ----
    const int lx = t % kTile, ly = t / kTile;
    uint32_t o[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) o[i] = 0;
    if (lx < vw && ly < vh) {
        float g[64];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint4 v = *reinterpret_cast<const uint4 *>(samples + (8 * ly + y) * kPitch + 8 * lx);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const float s = (float)((w[x >> 1] >> (16 * (x & 1))) & 0xffffu);
                g[8 * y + x] = fminf(a.limit, s);          // pointwiseMin(limit, .)  encode.swift:85
            }
        }
        float H[64];
        fdct_block(g, a.level_out, H);
        // quantise (true division, round half away) and scatter to zigzag order  encode.swift:225-240
#pragma unroll
        for (int h = 0; h < 8; ++h) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = H[8 * h + k] / sq_out[8 * h + k];
                const int32_t c = (int32_t)round_half_away(v);
                const int z = zigzag_of(k, h);
                o[z >> 1] |= ((uint32_t)c & 0xffffu) << (16 * (z & 1));
            }
        }
    }
    __syncthreads();                               // every work-item has read its samples: the tile becomes the packed blocks
#pragma unroll
    for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint4 *>(lds + t * kSlot + 16 * i) = uint4{o[4 * i + 0], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
    __syncthreads();
    // store: 8 lanes per block, 8 neighbouring blocks of one tile row per instruction -- one 1 KiB run
    const int wave = t >> 6, lane = t & 63, piece = lane & 7;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int blk = 64 * wave + 8 * i + (lane >> 3);
        const int x = blk % kTile, y = blk / kTile;
        if (x < vw && y < vh)
            *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(a.out[p] + img * a.out_stride[p] +
                                                                   (size_t)64 * ((size_t)(Y0 + y) * oux + X0 + x)) + 16 * piece) =
                *reinterpret_cast<const uint4 *>(lds + blk * kSlot + 16 * piece);
    }
}

}  // namespace

hipError_t launch_spectral_reduce(hipStream_t stream, int n_images, int n, const jpeg_amd_layout &in, const jpeg_amd_layout &out,
                                  const PlaneSet &coef_in, QuantaRef q, const uint16_t *d_quanta_out, const PlaneSetMut &coef_out)
{
    ReduceArgs a{};
    a.nplanes = in.nplanes;
    const int tile = tile_side(n);
    uint64_t wg = 0;
    for (int p = 0; p < in.nplanes; ++p) {
        a.in[p] = static_cast<const int16_t *>(coef_in.ptr[p]);
        a.in_stride[p] = coef_in.stride[p];
        a.out[p] = static_cast<int16_t *>(coef_out.ptr[p]);
        a.out_stride[p] = coef_out.stride[p];
        a.in_ux[p] = in.units_x[p]; a.in_uy[p] = in.units_y[p];
        a.out_ux[p] = out.units_x[p]; a.out_uy[p] = out.units_y[p];
        a.qi[p] = in.qi[p];
        a.wg_first[p] = (uint32_t)wg;
        // a plane with no source block has no samples to replicate: capi.hip refuses it; here it gets no workgroup
        if (in.units_x[p] > 0 && in.units_y[p] > 0)
            wg += (uint64_t)((out.units_x[p] + tile - 1) / tile) * (uint64_t)((out.units_y[p] + tile - 1) / tile);
    }
    if (wg > 0x7fffffffull) return hipErrorInvalidValue;
    for (int p = in.nplanes; p <= JPEG_AMD_MAX_PLANES; ++p) a.wg_first[p] = (uint32_t)wg;
    a.q_in = q.d_quanta; a.q_out = d_quanta_out ? d_quanta_out : q.d_quanta; a.q_stride = q.image_stride;
    a.level_in = ldexpf(1.0f, in.precision - 1) + 0.5f;
    a.level_out = ldexpf(1.0f, in.precision - 1) * 8.0f;     // encode.swift:215-218: no +0.5 in the forward level shift
    a.limit = ldexpf(1.0f, in.precision) - 1.0f;
    if (wg == 0 || n_images == 0) return hipSuccess;
    // x: the workgroups of ONE image's planes; y: the images
    const dim3 grid((unsigned)wg, (unsigned)n_images);
    const dim3 block((unsigned)(tile * tile));
    if (n == 4) hipLaunchKernelGGL((k_spectral_reduce<4>), grid, block, 0, stream, a);
    else if (n == 2) hipLaunchKernelGGL((k_spectral_reduce<2>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_spectral_reduce<1>), grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace jpeg_amd
