// tensor_source.hpp -- the input stage of include/jpeg_amd.h ("tensor sources") for k_tensor_pixels (kernels_pixels.hip): the
// counterpart of tensor_sink.hpp.  A work-item takes a run of kRun pixels of one row as elements -- HWC one run of 12
// consecutive elements, CHW three runs of 4 -- through load_elems, and to_byte turns an element into the contract's byte,
//     f = e as binary32;  p = f * scale[c];  s = p + offset[c];  b = fminf(fmaxf(s, 0), 255);  u = (uint8_t)(int)(b + 0.5f)
// every line one binary32 operation, nothing contracted, no division; a uint8 element is the byte itself.
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma once
#pragma clang fp contract(off)

#include <type_traits>

#include "tensor_sink.hpp"

namespace jpeg_amd {

// 4 elements from an address that is a multiple of 4 elements.
template <typename T>
__device__ __forceinline__ void load4(const T *p, T *v)
{
    if constexpr (sizeof(T) == 4) {
        const f32x4_t q = *reinterpret_cast<const f32x4_t *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (sizeof(T) == 2) {
        const u32x2_t q = *reinterpret_cast<const u32x2_t *>(p);
        v[0] = __builtin_bit_cast(T, (uint16_t)q.x); v[1] = __builtin_bit_cast(T, (uint16_t)(q.x >> 16));
        v[2] = __builtin_bit_cast(T, (uint16_t)q.y); v[3] = __builtin_bit_cast(T, (uint16_t)(q.y >> 16));
    } else {
        const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (T)(q >> (8 * k));
    }
}

// The first n of N elements at p into v, the rest of v left as it is; p's first multiple of 4 elements is H elements ahead
// (H static, so that every register index is): elements up to it, vectors of 4 from there, elements behind the last whole
// vector.  Nothing at or behind p + n is read.
template <typename T, int N, int H>
__device__ __forceinline__ void load_from(const T *p, T (&v)[N], int n)
{
#pragma unroll
    for (int k = 0; k < H; ++k)
        if (k < n) v[k] = p[k];
#pragma unroll
    for (int b = H; b < N; b += 4) {
        if (b + 4 <= N && b + 4 <= n) {
            load4(p + b, &v[b]);
        } else {
#pragma unroll
            for (int k = b; k < b + 4 && k < N; ++k)
                if (k < n) v[k] = p[k];
        }
    }
}

template <typename T, int N>
__device__ __forceinline__ void load_elems(const T *p, T (&v)[N], int n)
{
    switch (((0u - (uint32_t)(uintptr_t)p) / (uint32_t)sizeof(T)) & 3u) {
    case 0: load_from<T, N, 0>(p, v, n); break;
    case 1: load_from<T, N, 1>(p, v, n); break;
    case 2: load_from<T, N, 2>(p, v, n); break;
    default: load_from<T, N, 3>(p, v, n); break;
    }
}

template <typename T>
__device__ __forceinline__ float element_value(T e)
{
    if constexpr (std::is_same<T, float>::value) {
        return e;
    } else if constexpr (std::is_same<T, _Float16>::value) {
        // f is pinned as a binary32 value: left alone, the compiler may fold the conversion into the multiply that follows
        // (v_fma_mix_f32 e, scale, 0), which is not the contract's conversion followed by its product
        float f = (float)e;
        asm("" : "+v"(f));
        return f;
    } else {
        return __uint_as_float((uint32_t)(uint16_t)e << 16);
    }
}

// The contract's byte of an element of channel scale / offset.
template <typename T>
__device__ __forceinline__ uint32_t to_byte(T e, float scale, float offset)
{
    if constexpr (std::is_same<T, uint8_t>::value) {
        return e;
    } else {
        const float p = element_value<T>(e) * scale;
        const float s = p + offset;
        return (uint32_t)(int)(fminf(fmaxf(s, 0.0f), 255.0f) + 0.5f);
    }
}

}  // namespace jpeg_amd
