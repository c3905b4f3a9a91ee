// entropy_device_host.cpp -- the device entropy decoder's host instantiation (csrc/huffman_interval.hpp through
// jpeg_amd_jpeg_decode_intervals_host) and its planner under AddressSanitizer + UBSan, CPU only.  Every file given on the
// command line is read into a heap allocation of EXACTLY its size -- the decoder documents no padding, so it gets none -- and
// decoded into planes of exactly their size; where the planner takes the file, status and planes must be
// jpeg_amd_jpeg_decode_spectral's.  Then 100 seeded corruptions of every file (any status is fine, a sanitizer report is
// not).  Built and run by tests/test_entropy_device_cpu.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <random>
#include <vector>

#include "jpeg_amd.h"

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

struct Planes {
    std::vector<std::unique_ptr<int16_t[]>> own;
    std::vector<size_t> count;
    int16_t *ptr[JPEG_AMD_MAX_PLANES] = {};
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64];
    explicit Planes(const jpeg_amd_frame_info &fi)
    {
        std::memset(quanta, 0, sizeof quanta);
        for (int c = 0; c < fi.ncomponents; ++c) {
            count.push_back((size_t)64 * fi.units_x[c] * fi.units_y[c]);
            own.emplace_back(new int16_t[count.back()]);
            std::fill(own.back().get(), own.back().get() + count.back(), (int16_t)0x5a5a);
            ptr[c] = own.back().get();
        }
    }
};

// -> false when the two decoders disagree
static bool check(const uint8_t *bytes, size_t n)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);      // exactly n bytes: one read past the end is a report
    std::memcpy(exact.get(), bytes, n);
    jpeg_amd_frame_info fi{};
    if (jpeg_amd_jpeg_inspect(exact.get(), n, &fi) != JPEG_AMD_OK) return true;
    size_t blocks = 0;
    for (int c = 0; c < fi.ncomponents; ++c) blocks += (size_t)fi.units_x[c] * fi.units_y[c];
    if (blocks > (1u << 20)) return true;
    jpeg_amd_frame_info pi{};
    int32_t nscans = 0;
    int64_t nintervals = 0;
    const int verdict = jpeg_amd_jpeg_plan_intervals(exact.get(), n, &pi, &nscans, &nintervals);
    Planes dev(fi), host(fi);
    const int ds = jpeg_amd_jpeg_decode_intervals_host(exact.get(), n, dev.ptr, dev.quanta, nullptr);
    if (verdict != JPEG_AMD_OK) return ds == verdict;
    const int hs = jpeg_amd_jpeg_decode_spectral(exact.get(), n, host.ptr, host.quanta, nullptr);
    if (ds != hs) return false;
    if (hs != JPEG_AMD_OK) return true;
    for (int c = 0; c < fi.ncomponents; ++c)
        if (std::memcmp(dev.ptr[c], host.ptr[c], dev.count[c] * 2) != 0 || std::memcmp(dev.quanta[c], host.quanta[c], 128) != 0) return false;
    return true;
}

int main(int argc, char **argv)
{
    std::mt19937 rng(20261021);
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        if (!check(file.data(), file.size())) { std::printf("%s: the decoders disagree\n", argv[a]); ++failures; }
        for (int it = 0; it < 100; ++it) {
            std::vector<uint8_t> bad = file;
            const int edits = 1 + (int)(rng() % 4);
            for (int e = 0; e < edits && bad.size() > 8; ++e) {
                const size_t pos = 2 + rng() % (bad.size() - 2);
                switch (rng() % 4) {
                    case 0: bad[pos] = (uint8_t)rng(); break;
                    case 1: bad[pos] ^= (uint8_t)(1u << (rng() % 8)); break;
                    case 2: bad.erase(bad.begin() + (long)pos, bad.begin() + (long)std::min(bad.size(), pos + 1 + rng() % 40)); break;
                    default: bad.resize(pos); break;
                }
            }
            if (!check(bad.data(), bad.size())) { std::printf("%s: the decoders disagree on corruption %d\n", argv[a], it); ++failures; }
        }
    }
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
