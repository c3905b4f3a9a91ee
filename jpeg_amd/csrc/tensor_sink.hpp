// tensor_sink.hpp -- the output stage of include/jpeg_amd.h ("tensor output") for the kernels that end in it: k_resize_tensor
// (behind resample_walk) and k_tables_tensor (behind antialias_walk), both in kernels_resample.hip.  Both walks hand over a run
// of kRun pixels of one output row as bytes; tensor_sink turns them into elements,
//     t = (float)u - mean[c];  v = t * scale[c]          two binary32 operations, nothing contracted, no division
// which stay in registers and leave through store_elems: HWC one run of 12 consecutive elements, CHW three runs of 4.
// Element stores up to the first address that is a multiple of 4 elements, 4-element vector stores from there (16 bytes at
// binary32, 8 bytes at the 16-bit types; two of them merged into one 16-byte store where the address allows), element stores
// behind the last whole vector.  Any element-aligned base and any stride are correct; where out_w is a multiple of 4 and d_dst
// and dst_stride are multiples of 4 elements -- 224 x 224 into a dense tensor -- every run leaves in vector stores only.
// Conversions: binary16 is the compiler's float -> _Float16 conversion of the finished binary32 product (round to nearest even
// in the default mode; see to_element).  bfloat16 is INTEGER ARITHMETIC ON THE BITS, bits + 0x7fff + ((bits >> 16) & 1), the
// upper half kept -- not the packed hardware convert: it is the contract's own formula, it needs no inline assembly, and every
// value here is finite.
// tensor_sink itself is also the text of the sink that k_resize_tensor keeps in its body for the stored records
// (kernels_resample.hip says why): a change to one is made to the other.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma once
#pragma clang fp contract(off)

#include <type_traits>

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

enum class bf16_t : uint16_t {};   // bfloat16 as its bit pattern (a scalar type: arrays of it stay in registers)
static_assert(sizeof(bf16_t) == 2 && sizeof(_Float16) == 2, "element sizes");

template <typename T>
struct TensorArgs : ResampleArgs {
    float mean[3], scale[3];
    T *dst;
    size_t dst_stride;   // elements between output images
};

template <typename T>
__device__ __forceinline__ T to_element(float v)
{
    if constexpr (std::is_same<T, float>::value) {
        return v;
    } else if constexpr (std::is_same<T, _Float16>::value) {
        // v is pinned as a binary32 value first: left alone, the compiler folds the multiply that made it into the conversion
        // (v_fma_mixlo_f16 a, b, 0), which is not the contract's product rounded to binary32 and turns a product of -0 into +0
        asm("" : "+v"(v));
        return (_Float16)v;
    } else {
        const uint32_t bits = __float_as_uint(v);
        return (bf16_t)(uint16_t)((bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16);
    }
}

__device__ __forceinline__ uint32_t bits16(_Float16 v) { return __builtin_bit_cast(uint16_t, v); }
__device__ __forceinline__ uint32_t bits16(bf16_t v) { return (uint16_t)v; }

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// 4 elements to an address that is a multiple of 4 elements.
template <typename T>
__device__ __forceinline__ void store4(T *p, const T *v)
{
    if constexpr (sizeof(T) == 4)
        *reinterpret_cast<f32x4_t *>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
    else
        *reinterpret_cast<u32x2_t *>(p) = u32x2_t{bits16(v[0]) | (bits16(v[1]) << 16), bits16(v[2]) | (bits16(v[3]) << 16)};
}

// 8 elements of 2 bytes to an address that is a multiple of 16 bytes.
template <typename T>
__device__ __forceinline__ void store8(T *p, const T *v)
{
    *reinterpret_cast<u32x4_t *>(p) = u32x4_t{bits16(v[0]) | (bits16(v[1]) << 16), bits16(v[2]) | (bits16(v[3]) << 16),
                                              bits16(v[4]) | (bits16(v[5]) << 16), bits16(v[6]) | (bits16(v[7]) << 16)};
}

// The first n of v's N elements to p, whose first multiple of 4 elements is H elements ahead (H static, so that every
// register index is): elements up to it, vectors of 4 from there, elements behind the last whole vector.
template <typename T, int N, int H>
__device__ __forceinline__ void store_from(T *p, const T (&v)[N], int n)
{
#pragma unroll
    for (int k = 0; k < H; ++k)
        if (k < n) p[k] = v[k];
    if constexpr (H == 0 && N == 12 && sizeof(T) == 2) {
        if (n == N) {   // 24 bytes: 16 + 8 or 8 + 16
            if (((uint32_t)(uintptr_t)p & 15u) == 0) {
                store8(p, &v[0]);
                store4(p + 8, &v[8]);
            } else {
                store4(p, &v[0]);
                store8(p + 4, &v[4]);
            }
            return;
        }
    }
#pragma unroll
    for (int b = H; b < N; b += 4) {
        if (b + 4 <= N && b + 4 <= n) {
            store4(p + b, &v[b]);
        } else {
#pragma unroll
            for (int k = b; k < b + 4 && k < N; ++k)
                if (k < n) p[k] = v[k];
        }
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_elems(T *p, const T (&v)[N], int n)
{
    switch (((0u - (uint32_t)(uintptr_t)p) / (uint32_t)sizeof(T)) & 3u) {
    case 0: store_from<T, N, 0>(p, v, n); break;
    case 1: store_from<T, N, 1>(p, v, n); break;
    case 2: store_from<T, N, 2>(p, v, n); break;
    default: store_from<T, N, 3>(p, v, n); break;
    }
}

// The sink of both walks: the run o of npix pixels stored at (x, y) of the image at dst, `plane` = out_w out_h.
template <typename T, bool CHW>
__device__ __forceinline__ void tensor_sink(const TensorArgs<T> &a, T *dst, size_t plane, const uint32_t (&o)[kRun][3], int y,
                                            int x, int npix)
{
    T e[CHW ? 3 : 1][CHW ? kRun : 3 * kRun];   // CHW: three runs of kRun, HWC: one run of 3 kRun
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = (float)o[k][c] - a.mean[c];
            e[CHW ? c : 0][CHW ? k : 3 * k + c] = to_element<T>(d * a.scale[c]);
        }
    }
    const size_t at = (size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x;
    if constexpr (CHW) {
#pragma unroll
        for (int c = 0; c < 3; ++c) store_elems<T, kRun>(dst + c * plane + at, e[c], npix);
    } else {
        store_elems<T, 3 * kRun>(dst + 3 * at, e[0], 3 * npix);
    }
}

// The colour sink ("colour stage" of include/jpeg_amd.h): tensor_sink with image i's affine map of (R, G, B) and the clamp
// between the byte and the mean.  Per channel c, every statement ONE binary32 operation:
//     p = ((k[c][0] * r) + (k[c][1] * g)) + (k[c][2] * b);  q = p + k[c][3];  q = q < lo ? lo : q;  q = q > hi ? hi : q
// then tensor_sink's t = q - mean[c], v = t * scale[c] and its conversion and stores.  The clamp is two compares and selects,
// not v_max / v_min: those may return either zero for max(-0, +0), and the sign of q = -0 shows in q - mean where mean is 0.
// There is no branch: the two infinities leave every q, which is finite, as it is.  k is the workgroup's record, read by the
// kernel in front of the walk (blockIdx.y indexes it: scalar loads into SGPRs); lo and hi are kernel arguments.
// The conversion loop and the stores repeat tensor_sink's text instead of sharing a helper with it, so that nothing of the
// existing kernels' text moves (they are to stay the code they are): a change to one is made to the other.
template <typename T, bool CHW>
__device__ __forceinline__ void colour_sink(const TensorArgs<T> &a, const ColourRecord &k, float lo, float hi, T *dst, size_t plane,
                                            const uint32_t (&o)[kRun][3], int y, int x, int npix)
{
    T e[CHW ? 3 : 1][CHW ? kRun : 3 * kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        const float r = (float)o[j][0], g = (float)o[j][1], b = (float)o[j][2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p = ((k.k[c][0] * r) + (k.k[c][1] * g)) + (k.k[c][2] * b);
            float q = p + k.k[c][3];
            q = q < lo ? lo : q;
            q = q > hi ? hi : q;
            const float d = q - a.mean[c];
            e[CHW ? c : 0][CHW ? j : 3 * j + c] = to_element<T>(d * a.scale[c]);
        }
    }
    const size_t at = (size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x;
    if constexpr (CHW) {
#pragma unroll
        for (int c = 0; c < 3; ++c) store_elems<T, kRun>(dst + c * plane + at, e[c], npix);
    } else {
        store_elems<T, 3 * kRun>(dst + 3 * at, e[0], 3 * npix);
    }
}

}  // namespace jpeg_amd
