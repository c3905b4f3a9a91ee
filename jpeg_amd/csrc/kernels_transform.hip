// kernels_transform.hip -- lossless spectral transforms (rotate, flip, crop, requantise) in ONE launch for every plane of a
// batch: examples/rotate/main.swift (Block.transform, matrix / offset) and examples/recompress/main.swift:52-56.
//
// Work decomposition: ONE OUTPUT BLOCK PER WORK-ITEM for the arithmetic; the op is a template parameter, so the in-block
// permutation is a compile-time register renaming (XformMap), plus the packing of int16 pairs and the sign flips.  A block is
// one contiguous, 128-byte aligned run in either plane, so remapping at block granularity wastes no cache line whatever the
// source position.  The memory side goes through LDS: a wave owns a tile of 64 output blocks (tile_width), loads their sources
// 8 lanes per block with every instruction reading 8 neighbouring source blocks (one 1 KiB run) and stores 1 KiB runs of the
// output.  The first form -- each lane streaming its own block in 16-byte pieces, as k_idct_plane does -- ran at 1.39-1.68x
// the time of a device copy of the same bytes at 8192 x 8192 4:2:0 (profiles/r07_transform.txt).
//
// The plane of a workgroup is uniform: every plane's tiles start at a workgroup boundary.
//
// Requantisation is the reference's literal expression in float64 (HIP's double division is correctly rounded; the build
// uses -ffp-contract=off).  Where the reference traps (a q_in above 32767, an Int16 product that overflows, q_out = 0), the
// kernel sets *overflow with an ordinary store; the value it writes for that coefficient is then unspecified.
#pragma clang fp contract(off)

#include "kernels.hpp"
#include "transform.hpp"

namespace jpeg_amd {

namespace {

constexpr int kThreads = 256;

struct TransformArgs {
    const int16_t *in[JPEG_AMD_MAX_PLANES];
    size_t in_stride[JPEG_AMD_MAX_PLANES];
    int16_t *out[JPEG_AMD_MAX_PLANES];
    size_t out_stride[JPEG_AMD_MAX_PLANES];
    int in_ux[JPEG_AMD_MAX_PLANES], in_uy[JPEG_AMD_MAX_PLANES];      // source plane units
    int out_ux[JPEG_AMD_MAX_PLANES], out_uy[JPEG_AMD_MAX_PLANES];    // output plane units
    int ox[JPEG_AMD_MAX_PLANES], oy[JPEG_AMD_MAX_PLANES];            // region origin, in the plane's blocks
    int qi[JPEG_AMD_MAX_PLANES];
    uint32_t wg_first[JPEG_AMD_MAX_PLANES + 1];                      // first workgroup of each plane
    int nplanes;
    const uint16_t *q_in, *q_out;                                    // q_out: requantising variant only
    size_t q_stride;
    int32_t *overflow;
};

__device__ __forceinline__ int32_t coef_of(const uint32_t (&w)[32], int z)
{
    const int32_t word = (int32_t)w[z >> 1];
    return (z & 1) ? (word >> 16) : (int32_t)(int16_t)word;
}

__device__ __forceinline__ uint32_t pack2(int32_t lo, int32_t hi)
{
    return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
}

__device__ __forceinline__ void load_table(const uint16_t *t, uint32_t (&w)[32])
{
    const uint4 *s = reinterpret_cast<const uint4 *>(t);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = s[i];
        w[4 * i + 0] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
}
__device__ __forceinline__ uint32_t table_of(const uint32_t (&w)[32], int z)
{
    return (z & 1) ? (w[z >> 1] >> 16) : (w[z >> 1] & 0xffffu);
}

// LDS staging: a wave's 64 output blocks, one 144-byte slot each (128 bytes + 16 of padding: a lane reading its own block
// with ds_read_b128 walks slots 36 dwords apart, which spreads the wave over the banks)
constexpr int kSlot = 144;

// The wave's tile of output blocks, TW x (64 / TW); a workgroup is 4 tiles side by side.  Ops that keep the axes take a run of
// 64 blocks of one row: source and output are both long runs.  Transposing ops take 8 x 8 tiles: a tile row is a 1 KiB run of
// the output, a tile column one of the source.  (8192 x 8192 4:2:0, time over a device copy of the same bytes: NONE 1.07 with
// runs, 1.08-1.13 with tiles; TRANSPOSE 1.21 with runs, 1.11-1.15 with tiles -- profiles/r07_transform.txt.)
__host__ __device__ constexpr int tile_width(int op) { return (op & JPEG_AMD_XFORM_TRANSPOSE) ? 8 : 64; }

template <int OP, bool REQUANT>
__global__ __launch_bounds__(kThreads) void k_spectral_transform(TransformArgs a)
{
    constexpr int TW = tile_width(OP), TH = 64 / TW, WGX = 4, WGY = 1;
    constexpr bool T = (OP & JPEG_AMD_XFORM_TRANSPOSE) != 0;
    constexpr bool FH = (OP & JPEG_AMD_XFORM_FLIP_H) != 0;
    constexpr bool FV = (OP & JPEG_AMD_XFORM_FLIP_V) != 0;
    constexpr XformMap<OP> map{};
    __shared__ __attribute__((aligned(16))) uint8_t lds[kThreads * kSlot];

    int p = 0;
    while (p + 1 < a.nplanes && blockIdx.x >= a.wg_first[p + 1]) ++p;
    const int oux = a.out_ux[p], ouy = a.out_uy[p];
    // the workgroup's (WGX TW) x (WGY TH) blocks of the output plane, the wave's TW x TH tile of them; lane l owns tile block
    // (l % TW, l / TW)
    const uint32_t w_in_plane = blockIdx.x - a.wg_first[p];
    const uint32_t tiles_x = ((uint32_t)oux + WGX * TW - 1) / (WGX * TW);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int X0 = (int)(w_in_plane % tiles_x) * (WGX * TW) + (wave % WGX) * TW;
    const int Y0 = (int)(w_in_plane / tiles_x) * (WGY * TH) + (wave / WGX) * TH;
    const int X = X0 + lane % TW, Y = Y0 + lane / TW;
    const size_t img = blockIdx.y;
    uint8_t *slots = lds + wave * 64 * kSlot;

    // the source block of this lane's output block: undo FLIP_V, FLIP_H, TRANSPOSE, then the region's origin
    const uint8_t *src = nullptr;                  // nullptr: past the plane (a new, zero block) or past the output
    if (X < oux && Y < ouy) {
        const int X1 = FH ? oux - 1 - X : X;
        const int Y1 = FV ? ouy - 1 - Y : Y;
        const int sx = (T ? Y1 : X1) + a.ox[p];
        const int sy = (T ? X1 : Y1) + a.oy[p];
        if (sx < a.in_ux[p] && sy < a.in_uy[p])
            src = reinterpret_cast<const uint8_t *>(a.in[p] + img * a.in_stride[p] + (size_t)64 * ((size_t)sy * a.in_ux[p] + sx));
    }

    // load: 8 lanes per block, 16 bytes each, 8 blocks per instruction that are neighbours in the SOURCE -- a tile row, or a
    // tile column for the transposing ops: every instruction reads one 1 KiB run
    const int piece = lane & 7;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int blk = (T && TW == 8) ? 8 * (lane >> 3) + i : 8 * i + (lane >> 3);
        const uint64_t sp = (uint64_t)__shfl(reinterpret_cast<uintptr_t>(src), blk);
        uint4 v = uint4{0, 0, 0, 0};
        if (sp) v = *reinterpret_cast<const uint4 *>(sp + 16 * piece);
        *reinterpret_cast<uint4 *>(slots + blk * kSlot + 16 * piece) = v;
    }
    __syncthreads();
    uint32_t w[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = *reinterpret_cast<const uint4 *>(slots + lane * kSlot + 16 * i);
        w[4 * i + 0] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }

    uint32_t o[32];
    bool bad = false;
    if constexpr (!REQUANT) {
#pragma unroll
        for (int z = 0; z < 64; z += 2) {
            int32_t c0 = coef_of(w, map.m[z]), c1 = coef_of(w, map.m[z + 1]);
            if (map.neg[z]) { bad |= c0 == -32768; c0 = -c0; }
            if (map.neg[z + 1]) { bad |= c1 == -32768; c1 = -c1; }
            o[z >> 1] = pack2(c0, c1);
        }
    } else {
        const size_t t = img * a.q_stride + (size_t)64 * a.qi[p];
        uint32_t qin[32], qout[32];
        load_table(a.q_in + t, qin);
        load_table(a.q_out + t, qout);
        int32_t r[64];
#pragma unroll
        for (int z = 0; z < 64; ++z) {
            // v = Int16(q_in[m]) * sign * in[m];  r = Double(v) / Double(q_out);  Int16(r + 0.3 * (r < 0 ? -1 : 1))
            const int32_t qi = (int32_t)table_of(qin, map.m[z]);
            const int32_t c = map.neg[z] ? -coef_of(w, map.m[z]) : coef_of(w, map.m[z]);
            const int32_t v = qi * c;
            const uint32_t qo = table_of(qout, z);
            bad |= qi > 32767 || v < -32768 || v > 32767 || qo == 0;
            const double q = (double)(qo == 0 ? 1u : qo);
            const double x = (double)(int16_t)v / q;
            const double y = x + (x < 0.0 ? -0.3 : 0.3);
            r[z] = (int32_t)y;
        }
#pragma unroll
        for (int z = 0; z < 64; z += 2) o[z >> 1] = pack2(r[z], r[z + 1]);
    }
    if (bad && X < oux && Y < ouy && a.overflow) *a.overflow = 1;

    __syncthreads();                               // every lane has read its slot
#pragma unroll
    for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint4 *>(slots + lane * kSlot + 16 * i) = uint4{o[4 * i + 0], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
    __syncthreads();
    // store: tile row i is 8 consecutive output blocks -- one 1 KiB run per instruction
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int blk = 8 * i + (lane >> 3);
        const int x = X0 + blk % TW, y = Y0 + blk / TW;
        if (x < oux && y < ouy)
            *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(a.out[p] + img * a.out_stride[p] +
                                                                   (size_t)64 * ((size_t)y * oux + x)) + 16 * piece) =
                *reinterpret_cast<const uint4 *>(slots + blk * kSlot + 16 * piece);
    }
}

template <int OP>
void launch_op(hipStream_t stream, dim3 grid, const TransformArgs &a, bool requant)
{
    if (requant)
        hipLaunchKernelGGL((k_spectral_transform<OP, true>), grid, dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((k_spectral_transform<OP, false>), grid, dim3(kThreads), 0, stream, a);
}

}  // namespace

hipError_t launch_transform(hipStream_t stream, int n_images, int op, const jpeg_amd_layout &in, const jpeg_amd_layout &out,
                            const int *ox, const int *oy, const PlaneSet &coef_in, QuantaRef q, const uint16_t *d_quanta_out,
                            const PlaneSetMut &coef_out, int32_t *d_overflow)
{
    TransformArgs a{};
    a.nplanes = in.nplanes;
    uint32_t wg = 0;
    for (int p = 0; p < in.nplanes; ++p) {
        a.in[p] = static_cast<const int16_t *>(coef_in.ptr[p]);
        a.in_stride[p] = coef_in.stride[p];
        a.out[p] = static_cast<int16_t *>(coef_out.ptr[p]);
        a.out_stride[p] = coef_out.stride[p];
        a.in_ux[p] = in.units_x[p]; a.in_uy[p] = in.units_y[p];
        a.out_ux[p] = out.units_x[p]; a.out_uy[p] = out.units_y[p];
        a.ox[p] = ox[p]; a.oy[p] = oy[p];
        a.qi[p] = in.qi[p];
        a.wg_first[p] = wg;
        const int gw = 4 * tile_width(op), gh = 64 / tile_width(op);
        const size_t tiles = (size_t)((out.units_x[p] + gw - 1) / gw) * ((out.units_y[p] + gh - 1) / gh);
        wg += out.units_x[p] && out.units_y[p] ? (uint32_t)tiles : 0u;
    }
    for (int p = in.nplanes; p <= JPEG_AMD_MAX_PLANES; ++p) a.wg_first[p] = wg;
    a.q_in = q.d_quanta; a.q_out = d_quanta_out; a.q_stride = q.image_stride;
    a.overflow = d_overflow;
    if (wg == 0 || n_images == 0) return hipSuccess;
    // x: the workgroups of ONE image's planes; y: the images (each image's blocks start at a workgroup boundary)
    const dim3 grid(wg, (unsigned)n_images);
    const bool rq = d_quanta_out != nullptr;
    switch (op) {
        case 0: launch_op<0>(stream, grid, a, rq); break;
        case 1: launch_op<1>(stream, grid, a, rq); break;
        case 2: launch_op<2>(stream, grid, a, rq); break;
        case 3: launch_op<3>(stream, grid, a, rq); break;
        case 4: launch_op<4>(stream, grid, a, rq); break;
        case 5: launch_op<5>(stream, grid, a, rq); break;
        case 6: launch_op<6>(stream, grid, a, rq); break;
        default: launch_op<7>(stream, grid, a, rq); break;
    }
    return hipGetLastError();
}

}  // namespace jpeg_amd
