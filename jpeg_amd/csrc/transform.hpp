// transform.hpp -- the in-block half of the lossless spectral transforms (include/jpeg_amd.h, JPEG_AMD_XFORM_*), shared by
// the kernel (kernels_transform.hip) and the host's table mapping (capi.hip, jpeg_amd_transform_quanta).
//
// examples/rotate/main.swift, Block.transform: output zigzag index z takes sign(z) * in[m(z)].  With (k, h) the output
// frequencies of z, a transpose reads the input at (h, k); a horizontal mirror negates odd k, a vertical mirror odd h
// (the mirrors act in the output frame, after the transpose).
#pragma once

#include "dct.hpp"

namespace jpeg_amd {

// (k, h) of zigzag index z: the inverse of zigzag_of
__host__ __device__ constexpr int zigzag_k(int z)
{
    for (int i = 0; i < 64; ++i)
        if (zigzag_of(i & 7, i >> 3) == z) return i & 7;
    return 0;
}
__host__ __device__ constexpr int zigzag_h(int z)
{
    for (int i = 0; i < 64; ++i)
        if (zigzag_of(i & 7, i >> 3) == z) return i >> 3;
    return 0;
}

// m(z): the input zigzag index output index z reads
__host__ __device__ constexpr int xform_source(int op, int z)
{
    const int k = zigzag_k(z), h = zigzag_h(z);
    return (op & 1) ? zigzag_of(h, k) : zigzag_of(k, h);
}
// sign(z) < 0
__host__ __device__ constexpr bool xform_negates(int op, int z)
{
    const int k = zigzag_k(z), h = zigzag_h(z);
    return (((op & 2) != 0) && (k & 1)) != (((op & 4) != 0) && (h & 1));
}

// The whole map as a compile-time table (the kernel unrolls over it: a register renaming)
template <int OP>
struct XformMap {
    int m[64];
    bool neg[64];
    constexpr XformMap() : m(), neg()
    {
        for (int z = 0; z < 64; ++z) {
            m[z] = xform_source(OP, z);
            neg[z] = xform_negates(OP, z);
        }
    }
};

}  // namespace jpeg_amd
