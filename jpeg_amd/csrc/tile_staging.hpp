// tile_staging.hpp -- what the host stages for the launches of the tile decode kernels (kernels_tile.hip), and the tile grid's
// constants that the host's counts and the kernels must agree on.  No HIP in here: tests/cpp/tile_staging_test.cpp builds it
// with plain g++ under AddressSanitizer and UndefinedBehaviorSanitizer, as worker_pool.hpp is built for its tests.
//
// The words of one call, uploaded in one copy:
//   [payload: one per image of the call][per launch of the call, its group: index list [m], tile prefix [m + 1]]
// payload: the image's rectangle (x, y, width, height: 4 words) or, for k_view_decode_mixed, its record.  index[j]: the
// launch's image j is image index[j] of the call (k_region_decode, whose launch is the whole call in order, does not read
// it).  prefix[j]: the first workgroup of the launch's image j; prefix[m]: the launch's grid.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jpeg_amd.h"

namespace jpeg_amd {

constexpr int kTileW = 128;        // output pixels per tile row, every kernel's: a workgroup's rows are runs of up to 384 bytes
constexpr int kRegionTileH = 64;   // rows per tile of k_region_decode
constexpr int kViewTileH = 32;     // ... of k_scaled_decode, k_view_decode and k_view_decode_mixed

static_assert(sizeof(jpeg_amd_region) == 16, "a rectangle is staged as the kernels' int4");

// Tiles of a rectangle at n samples per block and tile_h rows per tile: the host's count, which the kernels take apart.
inline uint32_t rect_tiles(int n, int tile_h, const jpeg_amd_region &r)
{
    const int ax0 = n * (r.x / n), ay0 = n * (r.y / n);
    return (uint32_t)((r.x + r.width - 1 - ax0) / kTileW + 1) * (uint32_t)((r.y + r.height - 1 - ay0) / tile_h + 1);
}

// One launch's part of the staged words, in words from their start.
struct TileGroup {
    size_t index = 0, tiles = 0;   // the index list [n_images], the prefix [n_images + 1]
    int n_images = 0;
    uint32_t nwg = 0;              // the launch's workgroups: prefix[n_images]
};

struct TileStaging {
    std::vector<uint32_t> words;
    size_t payload_words;          // per image

    // The payloads of n_images images, zeroed; room for `groups` groups that hold every image once at most.
    TileStaging(size_t n_images, size_t payload_bytes, size_t groups) : payload_words(payload_bytes / 4)
    {
        words.reserve(n_images * (payload_words + 2) + groups);
        words.resize(n_images * payload_words);
    }
    void *payload(size_t i) { return words.data() + i * payload_words; }   // (until the next group())
    void rect(size_t i, const jpeg_amd_region &r) { memcpy(payload(i), &r, sizeof r); }

    // Appends the group of `members` -- images of the call, in the launch's order; tiles(i): the workgroups of image i.
    // EINVAL: more workgroups than a grid holds.
    template <typename Tiles>
    int group(const std::vector<uint32_t> &members, Tiles tiles, TileGroup *g)
    {
        g->index = words.size();
        g->tiles = g->index + members.size();
        g->n_images = (int)members.size();
        words.insert(words.end(), members.begin(), members.end());
        uint64_t acc = 0;
        for (const uint32_t i : members) {
            words.push_back((uint32_t)acc);
            acc += tiles(i);
        }
        if (acc > 0x7fffffffu) return JPEG_AMD_EINVAL;
        words.push_back((uint32_t)acc);
        g->nwg = (uint32_t)acc;
        return JPEG_AMD_OK;
    }
};

}  // namespace jpeg_amd
