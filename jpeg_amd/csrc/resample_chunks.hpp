// resample_chunks.hpp -- the chunk rule of the resized and tensor decodes: how a call's views are cut into chunks of
// consecutive images that are decoded into one buffer of the context and resampled by one launch each (capi_view.hip,
// plan_resize_chunks and resample_chunks).  Host text only, nothing but the public header behind it: a stand-alone program can
// include it (tests/cpp/resample_chunks_test.cpp does, under AddressSanitizer and UndefinedBehaviorSanitizer).
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "jpeg_amd.h"

namespace jpeg_amd {
namespace capi {

constexpr size_t kResizeChunkBytes = (size_t)1 << 30;   // decoded views per chunk of the resized and tensor decodes

// Images [i0, i0 + m) of a call, each view compact (3 * width * height bytes), image i0 + j at j * stride of the chunk's buffer.
struct ResizeChunk { int i0, m; size_t stride; };

// The chunks of n_images views, in order: each takes the consecutive images that fit -- m images at a stride of the chunk's
// largest view, stride * m <= limit -- and at least one, so that a single view above the limit is a chunk alone.  A view of
// the public header's largest size (65 535 x 65 535: 12.9 GB) and 65 535 images stay far inside 64 bits.
inline std::vector<ResizeChunk> split_resize_chunks(int n_images, const jpeg_amd_view *h_views, size_t limit = kResizeChunkBytes)
{
    static_assert(sizeof(size_t) >= 8, "the products of a view's bytes and a chunk's images are taken in size_t");
    std::vector<ResizeChunk> chunks;
    for (int i0 = 0; i0 < n_images;) {
        int m = 0;
        size_t stride = 0;
        for (; i0 + m < n_images; ++m) {
            const jpeg_amd_region &r = h_views[i0 + m].region;
            const size_t s = std::max(stride, (size_t)3 * r.width * r.height);
            if (m > 0 && s * ((size_t)m + 1) > limit) break;
            stride = s;
        }
        chunks.push_back(ResizeChunk{i0, m, stride});
        i0 += m;
    }
    return chunks;
}

}  // namespace capi
}  // namespace jpeg_amd
