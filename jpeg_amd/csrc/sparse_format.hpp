// sparse_format.hpp -- the sparse record of a frame's coefficients, stated once: what the host entropy coders (entropy.cpp,
// entropy_encode.cpp), the device kernels (k_sparsify, k_expand_sparse, k_expand_mixed) and the batch file paths agree on.
// Free of HIP: the entropy coders are also built with a plain C++ compiler.
//
// Instead of int16 planes -- 128 bytes per block, of which a typical file fills three or four coefficients -- a frame travels
// as [descriptors][entries]:
//   descriptor, one per block, planes in frame order: the index of the block's first entry; kAbsent = no block (all zero)
//   entry, one per nonzero coefficient (the DC always has one): value | zigzag index << 16 | last-of-block << 31
//
// THE ORDER OF A BLOCK'S ENTRIES.  A block's entries lie in a row, in ASCENDING zigzag order, the DC first.  Both writers keep
// it -- jpeg_amd_jpeg_decode_sparse (the DC, then every AC coefficient as the scan's run lengths reach it, k only ever growing)
// and k_sparsify (i = 0 .. 31, low half before high half) -- and both readers rely on it: the octet walk of k_expand_mixed stops at the first
// entry at or behind its head (k_expand_sparse walks the same way to the last-entry flag; each kernel keeps its own text of
// the walk: shared as one device function, in any of five forms, it was laid out another way and k_expand_mixed lost 0.3 to 1 %), jpeg_amd_jpeg_encode_sparse takes the runs from the indices and ends a block whose indices do not
// ascend.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/jpeg_amd.h"

#ifdef __HIP__
#define JA_SPARSE_FN __host__ __device__ constexpr
#else
#define JA_SPARSE_FN constexpr
#endif

namespace jpeg_amd {
namespace sparse {

constexpr uint32_t kAbsent = 0xffffffffu;      // descriptor: no scan reached the block
constexpr uint32_t kLast = 0x80000000u;        // entry: the last of its block
constexpr int kZigzagShift = 16;               // entry: where the zigzag index begins (6 bits)
constexpr uint32_t kValueMask = 0xffffu;       // entry: the coefficient, as uint16

JA_SPARSE_FN uint32_t make(uint32_t value16, uint32_t zigzag) { return value16 | zigzag << kZigzagShift; }   // (| kLast on a block's last)
JA_SPARSE_FN uint32_t value(uint32_t entry) { return entry & kValueMask; }
JA_SPARSE_FN uint32_t zigzag(uint32_t entry) { return (entry >> kZigzagShift) & 63; }
JA_SPARSE_FN bool is_last(uint32_t entry) { return (entry >> 31) != 0; }

}  // namespace sparse

// The record of one frame in the batch paths (jpeg_amd_jpeg_decode_sparse, k_sparsify): a descriptor per block and an arena of
// kSparseEntriesPerBlock entries per block (3/4 of the planes' bytes at most; only what is used travels).  Descriptors are 32-bit
// indices into the arena: a frame whose record would not be addressable that way (25 * blocks >= 2^32 - 1: beyond 60 000 x
// 60 000 4:4:4) travels as planes (ok = false).
constexpr size_t kSparseEntriesPerBlock = 24;
// jpeg_amd_jpeg_decode_sparse wants room for a whole block -- 72 entries -- in front of every block it starts.  A budget with
// this headroom lets a file of a few blocks travel sparse (the mixed calls); without, such a file travels as planes.
constexpr size_t kSparseDecoderHeadroom = 72;

struct SparseBudget {
    size_t blocks, arena, elems;   // elems: uint32 per image, [descriptors][entries]
    bool ok;
};

inline SparseBudget sparse_budget(const jpeg_amd_layout &L, size_t headroom = 0)
{
    size_t blocks = 0;
    for (int c = 0; c < L.nplanes; ++c) blocks += (size_t)L.units_x[c] * L.units_y[c];
    const size_t arena = kSparseEntriesPerBlock * blocks;
    return {blocks, arena + headroom, blocks + arena + headroom, blocks + arena < sparse::kAbsent};
}

}  // namespace jpeg_amd
