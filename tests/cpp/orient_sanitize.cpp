// orient_sanitize.cpp -- csrc/orient.hpp and jpeg_amd_jpeg_orientation (csrc/entropy.cpp) under AddressSanitizer + UBSan,
// CPU only.  Built and run by tests/test_orient_sanitize.py; never loaded into Python.
//   1. For all 8 orientations and every stored extent up to 6 x 5, at two offsets: oriented_source()'s base and steps give
//      offset + 3 (ys w + xs) for every pixel of the oriented image, with (xs, ys) written out here from the definition, every
//      stored pixel is reached exactly once, and every address lies inside [offset, offset + 3 w h).  The rectangle mapping of
//      every rectangle covers exactly the stored pixels its oriented pixels come from.
//   2. The parser over Exif segments of every shape the Python tests build, a few thousand seeded truncations and byte mutations
//      of them, and every file given on the command line cut at every length below 4 KiB: each input lies in a heap buffer of
//      EXACTLY its size (the sanitizer sees a read one byte past it), and the answer is always OK with a value in 1 .. 8.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "jpeg_amd.h"
#include "orient.hpp"

using namespace jpeg_amd;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                    \
    } while (0)

static void stored_of(int o, int w, int h, int xo, int yo, int &xs, int &ys)
{
    static const int bits[9][3] = {{0, 0, 0}, {0, 0, 0}, {0, 1, 0}, {0, 1, 1}, {0, 0, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 1}, {1, 1, 0}};
    const int T = bits[o][0], fx = bits[o][1], fy = bits[o][2];
    if (!T) {
        xs = fx ? w - 1 - xo : xo;
        ys = fy ? h - 1 - yo : yo;
    } else {
        xs = fx ? w - 1 - yo : yo;
        ys = fy ? h - 1 - xo : xo;
    }
}

static void check_addresses()
{
    for (int o = 1; o <= 8; ++o)
        for (int w = 1; w <= 6; ++w)
            for (int h = 1; h <= 5; ++h)
                for (uint64_t offset : {(uint64_t)0, (uint64_t)0x1234567890ull}) {
                    EXPECT(orientation_valid(o));
                    const OrientedSource s = oriented_source(o, offset, w, h);
                    const bool T = o >= 5;
                    EXPECT(s.w == (T ? h : w) && s.h == (T ? w : h));
                    std::vector<int> hits((size_t)w * h, 0);
                    for (int yo = 0; yo < s.h; ++yo)
                        for (int xo = 0; xo < s.w; ++xo) {
                            int xs, ys;
                            stored_of(o, w, h, xo, yo, xs, ys);
                            const uint64_t at = s.base + (uint64_t)(xo * s.step_x) + (uint64_t)(yo * s.step_y);
                            EXPECT(at == offset + 3u * ((uint64_t)ys * w + xs));
                            EXPECT(at >= offset && at + 2 < offset + 3u * (uint64_t)w * h);
                            if (xs >= 0 && xs < w && ys >= 0 && ys < h) ++hits[(size_t)ys * w + xs];
                        }
                    for (int v : hits) EXPECT(v == 1);
                    // every rectangle of the oriented image
                    for (int x = 0; x < s.w; ++x)
                        for (int y = 0; y < s.h; ++y)
                            for (int rw = 1; x + rw <= s.w; ++rw)
                                for (int rh = 1; y + rh <= s.h; ++rh) {
                                    const OrientRect m = oriented_rect_to_stored(o, w, h, OrientRect{x, y, rw, rh});
                                    EXPECT(m.x >= 0 && m.y >= 0 && m.width >= 1 && m.height >= 1 && m.x + m.width <= w && m.y + m.height <= h);
                                    EXPECT(m.width * m.height == rw * rh);
                                    for (int yo = y; yo < y + rh; ++yo)
                                        for (int xo = x; xo < x + rw; ++xo) {
                                            int xs, ys;
                                            stored_of(o, w, h, xo, yo, xs, ys);
                                            EXPECT(xs >= m.x && xs < m.x + m.width && ys >= m.y && ys < m.y + m.height);
                                        }
                                }
                }
    EXPECT(!orientation_valid(0) && !orientation_valid(9) && !orientation_valid(-1));
}

// ---- the parser ------------------------------------------------------------------------------------------------------------

typedef std::vector<uint8_t> Bytes;

static void put16(Bytes &b, bool big, uint32_t v)
{
    b.push_back((uint8_t)(big ? v >> 8 : v));
    b.push_back((uint8_t)(big ? v : v >> 8));
}
static void put32(Bytes &b, bool big, uint32_t v)
{
    put16(b, big, big ? v >> 16 : v & 0xffff);
    put16(b, big, big ? v & 0xffff : v >> 16);
}

// SOI, an APP1 Exif segment with `before` other entries, the orientation entry, one more entry; then a frame-less tail.
static Bytes file_with(bool big, int type, uint32_t count, uint32_t value, int before, uint32_t ifd = 8)
{
    Bytes t;
    t.insert(t.end(), big ? "MM" : "II", (big ? "MM" : "II") + 2);
    put16(t, big, 42);
    put32(t, big, ifd);
    t.resize(ifd, 0);
    put16(t, big, (uint32_t)before + 2);
    for (int i = 0; i < before; ++i) { put16(t, big, 0x0100 + i); put16(t, big, 3); put32(t, big, 1); put16(t, big, 7); put16(t, big, 0); }
    put16(t, big, 0x0112); put16(t, big, (uint32_t)type); put32(t, big, count);
    if (type == 3) { put16(t, big, value); put16(t, big, 0); } else put32(t, big, value);
    put16(t, big, 0x011a); put16(t, big, 4); put32(t, big, 1); put32(t, big, 72);
    put32(t, big, 0);
    Bytes f = {0xFF, 0xD8, 0xFF, 0xE1};
    const size_t n = 2 + 6 + t.size();
    f.push_back((uint8_t)(n >> 8)); f.push_back((uint8_t)n);
    f.insert(f.end(), {'E', 'x', 'i', 'f', 0, 0});
    f.insert(f.end(), t.begin(), t.end());
    f.insert(f.end(), {0xFF, 0xDB, 0x00, 0x04, 1, 2, 0xFF, 0xDA, 0x00, 0x02, 0x12, 0x34, 0xFF, 0xD9});
    return f;
}

// The parser on a heap copy of exactly n bytes of `data`.
static int parsed(const uint8_t *data, size_t n, int expect = 0)
{
    uint8_t *exact = new uint8_t[n ? n : 1];
    if (n) std::memcpy(exact, data, n);
    int32_t o = -7;
    const int st = jpeg_amd_jpeg_orientation(exact, n, &o);
    delete[] exact;
    EXPECT(st == JPEG_AMD_OK && o >= 1 && o <= 8);
    if (expect) EXPECT(o == expect);
    return o;
}

static Bytes slurp(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return Bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    check_addresses();

    int32_t o = 0;
    EXPECT(jpeg_amd_jpeg_orientation(nullptr, 4, &o) == JPEG_AMD_EINVAL);
    const uint8_t soi[2] = {0xFF, 0xD8};
    EXPECT(jpeg_amd_jpeg_orientation(soi, 2, nullptr) == JPEG_AMD_EINVAL);

    std::vector<Bytes> seeds;
    const auto seed = [&](Bytes file, int expect) {
        parsed(file.data(), file.size(), expect);
        seeds.push_back(std::move(file));
    };
    for (int big = 0; big < 2; ++big) {
        for (int type = 3; type <= 4; ++type)
            for (uint32_t v = 1; v <= 8; ++v) seed(file_with(big, type, 1, v, (int)v % 3), (int)v);
        for (uint32_t v : {0u, 9u, 65535u}) seed(file_with(big, 3, 1, v, 1), 1);   // values that are no orientation
        seed(file_with(big, 3, 2, 6, 1), 1);                                       // count 2
        seed(file_with(big, 2, 1, 6, 1), 1);                                       // ASCII
        seed(file_with(big, 4, 1, 0x60000, 0), 1);                                 // 6 in the other half of a LONG
        seed(file_with(big, 3, 1, 6, 2, 40), 6);                                   // IFD0 further in
    }

    // every truncation of every seed, then seeded mutations: bytes set, bytes flipped, a cut
    size_t runs = 0;
    for (const Bytes &s : seeds)
        for (size_t n = 0; n <= s.size(); ++n, ++runs) parsed(s.data(), n);
    std::mt19937 rng(20240607);
    for (int round = 0; round < 6000; ++round, ++runs) {
        Bytes m = seeds[rng() % seeds.size()];
        const int edits = 1 + (int)(rng() % 4);
        for (int e = 0; e < edits; ++e) {
            const size_t at = rng() % m.size();
            switch (rng() % 4) {
            case 0: m[at] = (uint8_t)rng(); break;
            case 1: m[at] ^= (uint8_t)(1u << (rng() % 8)); break;
            case 2: m[at] = 0xFF; break;
            default: m[at] = rng() % 2 ? 0x00 : 0x7F; break;
            }
        }
        if (rng() % 3 == 0) m.resize(rng() % (m.size() + 1));
        parsed(m.data(), m.size());
    }

    // the files of the command line, cut at every length below 4 KiB, and whole
    for (int i = 1; i < argc; ++i) {
        const Bytes f = slurp(argv[i]);
        EXPECT(!f.empty());
        const int whole = parsed(f.data(), f.size());
        EXPECT(whole == 1);   // (the fixtures' Exif segments say 1, or carry no orientation)
        for (size_t n = 0; n < 4096 && n <= f.size(); ++n, ++runs) parsed(f.data(), n);
    }
    std::printf("%zu parser runs, %d failures\n", runs, failures);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
