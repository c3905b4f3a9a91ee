// split_resize_chunks (jpeg_amd/csrc/resample_chunks.hpp), the chunk rule of the resized and tensor decodes, under
// AddressSanitizer and UndefinedBehaviorSanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -I jpeg_amd/csrc
//       tests/cpp/resample_chunks_test.cpp -o t && ./t
// Without arguments it checks, for random view lists under a small limit and for constructed ones under the real limit:
//  a. the chunks partition [0, n) in order, every chunk has m >= 1, and n = 0 gives no chunks;
//  b. a chunk's stride is the largest 3 * w * h among its views;
//  c. m == 1 or stride * m <= limit;
//  d. every chunk but the last is maximal: max(stride, the next view) * (m + 1) > limit;
//  e. the split is the one a brute-force restatement finds (the longest prefix that fits, by trying every length);
//  f. the boundaries: stride * m == limit keeps the image, one byte over cuts it; a single view above the limit (65 535 x
//     65 535, 12.9 GB) is a chunk alone and nothing wraps; a late large view raises the stride of the whole chunk it joins.
// With arguments -- [--limit BYTES] WxH ... -- it prints the chunks of those views, one "i0 m stride" per line: the pytest wrapper
// compares them with what the GPU tests of the chunk seam assume.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "resample_chunks.hpp"

using jpeg_amd::capi::kResizeChunkBytes;
using jpeg_amd::capi::ResizeChunk;
using jpeg_amd::capi::split_resize_chunks;

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); ++g_failures; } } while (0)

static uint32_t draw(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static jpeg_amd_view view(int32_t w, int32_t h) { return jpeg_amd_view{1, jpeg_amd_region{0, 0, w, h}}; }

// 128-bit where the compiler has it, so that the restatement cannot wrap where the header might
static unsigned __int128 bytes_of(const jpeg_amd_view &v) { return (unsigned __int128)3 * (unsigned)v.region.width * (unsigned)v.region.height; }

// (a) .. (d) of a split, and (e): the restatement tries every length m from the chunk's first image and keeps the longest
// prefix-closed one (a length fits when the largest view of the first m, times m, is within the limit; one image always fits).
static void check_split(const char *name, const std::vector<jpeg_amd_view> &views, size_t limit)
{
    const int n = (int)views.size();
    const std::vector<ResizeChunk> got = split_resize_chunks(n, views.data(), limit);
    CHECK((n == 0) == got.empty(), "%s: n = %d gives %zu chunks", name, n, got.size());
    int at = 0;
    for (size_t c = 0; c < got.size(); ++c) {
        const ResizeChunk &k = got[c];
        CHECK(k.i0 == at && k.m >= 1 && k.i0 + k.m <= n, "%s: chunk %zu is [%d, %d + %d), expected from %d", name, c, k.i0, k.i0, k.m, at);
        if (k.m < 1 || k.i0 != at || k.i0 + k.m > n) return;
        unsigned __int128 largest = 0;
        for (int j = 0; j < k.m; ++j) largest = std::max(largest, bytes_of(views[(size_t)(k.i0 + j)]));
        CHECK((unsigned __int128)k.stride == largest, "%s: chunk %zu stride %zu", name, c, k.stride);                          // (b)
        CHECK(k.m == 1 || largest * (unsigned)k.m <= limit, "%s: chunk %zu of %d images is over the limit", name, c, k.m);     // (c)
        if (k.i0 + k.m < n) {                                                                                                 // (d)
            const unsigned __int128 next = std::max(largest, bytes_of(views[(size_t)(k.i0 + k.m)]));
            CHECK(next * (unsigned)(k.m + 1) > limit, "%s: chunk %zu is not maximal", name, c);
        }
        int want = 1;                                                                                                         // (e)
        unsigned __int128 run = bytes_of(views[(size_t)at]);
        for (int m = 2; at + m <= n; ++m) {
            run = std::max(run, bytes_of(views[(size_t)(at + m - 1)]));
            if (run * (unsigned)m > limit) break;
            want = m;
        }
        CHECK(k.m == want, "%s: chunk %zu has %d images, the restatement %d", name, c, k.m, want);
        at += k.m;
    }
    CHECK(at == n, "%s: the chunks end at %d of %d", name, at, n);
}

static void self_test()
{
    // random lists under small limits: many chunks, strides of every order
    uint32_t seed = 7;
    for (int round = 0; round < 400; ++round) {
        const size_t limit = 1 + draw(seed) % 5000;
        std::vector<jpeg_amd_view> views((size_t)(draw(seed) % 40));
        for (auto &v : views) v = view((int32_t)(1 + draw(seed) % 30), (int32_t)(1 + draw(seed) % 30));
        check_split("random", views, limit);
    }
    check_split("none", {}, 100);
    CHECK(split_resize_chunks(0, nullptr).empty(), "n = 0 with the default limit");

    // (f) exactly the limit keeps the image; one byte over cuts it
    {
        const std::vector<jpeg_amd_view> four(4, view(5, 5));                       // 75 bytes each
        std::vector<ResizeChunk> k = split_resize_chunks(4, four.data(), 300);
        CHECK(k.size() == 1 && k[0].m == 4 && k[0].stride == 75, "75 * 4 == 300 is one chunk");
        k = split_resize_chunks(4, four.data(), 299);
        CHECK(k.size() == 2 && k[0].m == 3 && k[1].i0 == 3 && k[1].m == 1, "75 * 4 == 299 + 1 is cut behind three");
        check_split("exact", four, 300);
        check_split("one over", four, 299);
    }
    // ... and at the real size: the scenario of the GPU tests under the real limit
    {
        const size_t whole = (size_t)3 * 2048 * 1536;                              // 9 437 184: 113 fit, 114 do not
        CHECK(whole * 113 <= kResizeChunkBytes && whole * 114 > kResizeChunkBytes, "113 whole views of 2048 x 1536 fit");
        const std::vector<jpeg_amd_view> many(230, view(2048, 1536));
        const std::vector<ResizeChunk> k = split_resize_chunks(230, many.data());
        CHECK(k.size() == 3 && k[0].m == 113 && k[1].i0 == 113 && k[1].m == 113 && k[2].i0 == 226 && k[2].m == 4 && k[2].stride == whole,
              "230 views of 2048 x 1536 are [0, 113) [113, 226) [226, 230)");
        check_split("230 whole", many, kResizeChunkBytes);
        // the exact boundary at that order of size (3 * w * h is never 2^30, so under a limit of its own): two views of 3 * 2^28 bytes
        const std::vector<jpeg_amd_view> big(2, view(16384, 16384));
        CHECK(split_resize_chunks(2, big.data(), (size_t)3 << 29).size() == 1, "two views of 3 * 2^28 under 3 * 2^29 are one chunk");
        CHECK(split_resize_chunks(2, big.data(), ((size_t)3 << 29) - 1).size() == 2, "... and one byte less cuts them");
    }
    // a single view above the limit is a chunk alone, at any place; 65 535 x 65 535 x 3 = 12 884 508 675 does not wrap
    {
        const std::vector<jpeg_amd_view> v = {view(4, 4), view(65535, 65535), view(4, 4), view(65535, 65535), view(65535, 65535)};
        const std::vector<ResizeChunk> k = split_resize_chunks(5, v.data());
        const size_t huge = (size_t)12884508675ull;
        CHECK(k.size() == 5, "a view above the limit: %zu chunks", k.size());
        for (size_t c = 0; c < k.size() && k.size() == 5; ++c)
            CHECK(k[c].i0 == (int)c && k[c].m == 1 && k[c].stride == (c % 2 == 1 || c == 4 ? huge : (size_t)48), "a view above the limit: chunk %zu stride %zu", c, k[c].stride);
        check_split("huge", v, kResizeChunkBytes);
        // 65 535 of them, the most a call takes: the products stay inside 64 bits whatever m the loop tries
        const std::vector<jpeg_amd_view> all(65535, view(65535, 65535));
        CHECK(split_resize_chunks(65535, all.data()).size() == 65535, "65 535 views of 65 535 x 65 535");
    }
    // a late large view raises the stride of the whole chunk it joins: 100 views of 48 bytes, then one of 3 * 2048 * 1536
    {
        std::vector<jpeg_amd_view> v(100, view(4, 4));
        v.push_back(view(2048, 1536));
        v.insert(v.end(), 30, view(4, 4));
        const std::vector<ResizeChunk> k = split_resize_chunks((int)v.size(), v.data());
        CHECK(k.size() == 2 && k[0].m == 113 && k[0].stride == (size_t)3 * 2048 * 1536 && k[1].i0 == 113 && k[1].m == 18 && k[1].stride == 48,
              "a late large view: the chunk's stride is its, and the chunk ends where 114 of it would not fit");
        check_split("late large", v, kResizeChunkBytes);
        // ... and where it does not fit any more behind the images in front of it, it is cut off
        std::vector<jpeg_amd_view> w(113, view(4, 4));
        w.push_back(view(2048, 1536));
        const std::vector<ResizeChunk> q = split_resize_chunks(114, w.data());
        CHECK(q.size() == 2 && q[0].m == 113 && q[0].stride == 48 && q[1].m == 1 && q[1].stride == (size_t)3 * 2048 * 1536,
              "a large view behind 113 small ones starts a chunk");
        check_split("cut off", w, kResizeChunkBytes);
    }
}

int main(int argc, char **argv)
{
    if (argc > 1) {
        size_t limit = kResizeChunkBytes;
        std::vector<jpeg_amd_view> views;
        for (int a = 1; a < argc; ++a) {
            if (!std::strcmp(argv[a], "--limit") && a + 1 < argc) {
                limit = (size_t)std::strtoull(argv[++a], nullptr, 10);
                continue;
            }
            long w = 0, h = 0;
            if (std::sscanf(argv[a], "%ldx%ld", &w, &h) != 2 || w < 1 || h < 1 || w > 65535 || h > 65535) {
                std::fprintf(stderr, "%s: not WxH\n", argv[a]);
                return 2;
            }
            views.push_back(view((int32_t)w, (int32_t)h));
        }
        for (const ResizeChunk &k : split_resize_chunks((int)views.size(), views.data(), limit)) std::printf("%d %d %zu\n", k.i0, k.m, k.stride);
        return 0;
    }
    self_test();
    if (g_failures) std::printf("FAILED: %d\n", g_failures);
    else std::printf("ok\n");
    return g_failures ? 1 : 0;
}
