// TileStaging (jpeg_amd/csrc/tile_staging.hpp), what the host stages for the launches of the tile decode kernels, under
// AddressSanitizer and UndefinedBehaviorSanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I jpeg_amd/csrc
//       tests/cpp/tile_staging_test.cpp -o t && ./t
// The three callers' shapes -- the region call's one group, the view call's four denominator groups, the mixed call's eight
// (denominator, planes) groups over records -- against a restatement that counts tiles by walking them:
//  a. the words are [payload per image][per group: index list, prefix], the groups in the order they were added, and each
//     TileGroup names its own part of them;
//  b. prefix[j] is the sum of the tiles of the group's images before j, prefix[m] the returned workgroup count;
//  c. payloads written before a group was added are still there after the last one (the vector has grown in between);
//  d. a group whose counts sum to 0x80000000, or past 2^32, is refused with EINVAL; 0x7fffffff is not.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "tile_staging.hpp"

using jpeg_amd::TileGroup;
using jpeg_amd::TileStaging;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); ++g_failures; } } while (0)

// Tiles of r by walking them: from the block of n that holds the first pixel, in steps of the tile, while inside r.
static uint32_t walk_tiles(int n, int tile_h, const jpeg_amd_region &r)
{
    uint32_t cols = 0, rows = 0;
    for (long long x = r.x - r.x % n; x < (long long)r.x + r.width; x += 128) ++cols;
    for (long long y = r.y - r.y % n; y < (long long)r.y + r.height; y += tile_h) ++rows;
    return cols * rows;
}

static uint32_t draw(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static jpeg_amd_region some_region(uint32_t &s)
{
    return jpeg_amd_region{(int32_t)(draw(s) % 700), (int32_t)(draw(s) % 500), (int32_t)(1 + draw(s) % 900), (int32_t)(1 + draw(s) % 400)};
}

// One call of n_images images, payload_bytes each, whose image i belongs to group group_of[i] (or to none: -1) at n_of[g]
// samples per block and tile_h rows per tile.
static void run_case(const char *name, size_t n_images, size_t payload_bytes, int groups, const std::vector<int> &group_of,
                     const std::vector<int> &n_of, int tile_h, uint32_t seed)
{
    std::vector<jpeg_amd_region> rects(n_images);
    for (auto &r : rects) r = some_region(seed);
    const size_t pw = payload_bytes / 4;

    TileStaging st(n_images, payload_bytes, (size_t)groups);
    CHECK(st.words.size() == n_images * pw, "%s: payload size", name);
    for (size_t i = 0; i < n_images; ++i) {
        if (payload_bytes == sizeof(jpeg_amd_region)) {
            st.rect(i, rects[i]);
        } else {   // a record: a pattern of the image in every byte
            std::memset(st.payload(i), (int)(0x30 + i), payload_bytes);
        }
    }
    std::vector<uint32_t> want(st.words);   // (a), (c): the payloads as they were written
    std::vector<TileGroup> got((size_t)groups);
    for (int g = 0; g < groups; ++g) {
        std::vector<uint32_t> members;
        for (size_t i = 0; i < n_images; ++i)
            if (group_of[i] == g) members.push_back((uint32_t)i);
        const int n = n_of[(size_t)g];
        const int status = st.group(members, [&](uint32_t i) { return jpeg_amd::rect_tiles(n, tile_h, rects[i]); }, &got[(size_t)g]);
        CHECK(status == JPEG_AMD_OK, "%s: group %d refused", name, g);
        // the restatement
        const size_t at = want.size();
        want.insert(want.end(), members.begin(), members.end());
        uint32_t acc = 0;
        for (const uint32_t i : members) {
            want.push_back(acc);
            acc += walk_tiles(n, tile_h, rects[i]);
        }
        want.push_back(acc);
        const TileGroup &t = got[(size_t)g];
        CHECK(t.index == at && t.tiles == at + members.size() && t.n_images == (int)members.size(), "%s: group %d offsets", name, g);
        CHECK(t.nwg == acc && st.words[t.tiles + members.size()] == t.nwg, "%s: group %d workgroups %u, want %u", name, g, t.nwg, acc);   // (b)
    }
    CHECK(st.words == want, "%s: the staged words", name);
    CHECK(st.words.size() == n_images * pw + 2 * (size_t)std::count_if(group_of.begin(), group_of.end(), [](int g) { return g >= 0; }) + (size_t)groups,
          "%s: word count", name);
}

int main()
{
    // the region call: one group of every image in order, N = 8, tiles of 64 rows
    run_case("region", 7, 16, 1, std::vector<int>(7, 0), {8}, jpeg_amd::kRegionTileH, 1);
    // the view call: a group per denominator, the images of each scattered over the call
    run_case("view", 13, 16, 4, {2, 0, 1, 3, 0, 0, 2, 1, 3, 3, 0, 2, 1}, {8, 4, 2, 1}, jpeg_amd::kViewTileH, 2);
    // the mixed call: a group per (denominator, planes) over records of 208 bytes; image 5 and 11 take the uniform call
    run_case("mixed", 18, 208, 8, {7, 0, 3, 4, 1, -1, 6, 2, 5, 0, 7, -1, 3, 1, 4, 2, 6, 5}, {8, 8, 4, 4, 2, 2, 1, 1}, jpeg_amd::kViewTileH, 3);
    // a call without groups (the crop fallback): the payloads alone
    run_case("no groups", 4, 16, 0, std::vector<int>(4, -1), {}, jpeg_amd::kViewTileH, 4);

    // (d) the limit of a grid
    const std::vector<uint32_t> two = {0, 1}, three = {0, 1, 2};
    {
        TileStaging st(3, 16, 1);
        TileGroup g;
        CHECK(st.group(two, [](uint32_t i) { return i == 0 ? 0x40000000u : 0x3fffffffu; }, &g) == JPEG_AMD_OK, "0x7fffffff is refused");
        CHECK(g.nwg == 0x7fffffffu && st.words[g.tiles] == 0 && st.words[g.tiles + 1] == 0x40000000u && st.words[g.tiles + 2] == 0x7fffffffu,
              "0x7fffffff: prefix");
    }
    {
        TileStaging st(3, 16, 1);
        TileGroup g;
        CHECK(st.group(two, [](uint32_t) { return 0x40000000u; }, &g) == JPEG_AMD_EINVAL, "0x80000000 is not refused");
    }
    {
        TileStaging st(3, 16, 1);
        TileGroup g;
        CHECK(st.group(three, [](uint32_t) { return 0x60000000u; }, &g) == JPEG_AMD_EINVAL, "a sum past 2^32 is not refused");
    }
    if (g_failures) std::printf("FAILED: %d\n", g_failures);
    else std::printf("ok\n");
    return g_failures ? 1 : 0;
}
