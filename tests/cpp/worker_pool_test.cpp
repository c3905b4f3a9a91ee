// WorkerPool, FileQueue and PixelDrain (jpeg_amd/csrc/worker_pool.hpp) under ThreadSanitizer: every item of every region runs exactly once,
// a region uses no more threads than it was given, begin() returns before the work is done and finish() joins it, regions of
// every size follow each other on one pool; the file queue of jpeg_amd_decompress_batch decodes every file exactly once and
// every chunk completely, on the calling thread when the pool has no helper, and a call that fails in chunk 0 while chunk 1 is
// being decoded stops its threads before it trims their records and never starts a chunk that was not opened; the pixel drain
// of that call: drain_failures() below.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <random>
#include <set>
#include <thread>
#include <vector>
#include "worker_pool.hpp"

using jpeg_amd::FileQueue;
using jpeg_amd::PixelDrain;
using jpeg_amd::WorkerPool;

// The pixel drain of jpeg_amd_decompress_batch (PixelDrain): m images of 1, 3 and 33 pieces (and of 33 pieces and a rest) to
// a destination with a pitch, on pools of 1, 2, 5 and 16 threads, several drains back to back on each pool.  A drain whose
// pixels arrive: the callable runs exactly once, held for a few milliseconds it still finds the destination untouched when it
// answers, and afterwards every byte of every image is there and the pitch's gaps are not written (two threads copying one
// piece would be a data race, which ThreadSanitizer reports).  A drain whose callable answers false copies nothing and end()
// says so.  A drain that is begun and then abandoned is joined by its destructor, with the pixels copied.
static int drain_failures()
{
    int failures = 0;
    const size_t piece = 64, gap = 24;
    const int m = 5;
    for (int pool_threads : {1, 2, 5, 16}) {
        WorkerPool pool(pool_threads);
        for (size_t bytes : {piece, 3 * piece, 33 * piece, 33 * piece + 7}) {
            const size_t pitch = bytes + gap;
            std::vector<uint8_t> src(bytes * m), dst;
            for (size_t b = 0; b < src.size(); ++b) src[b] = (uint8_t)(1 + b % 251);   // never the 0 the destination starts from
            for (int mode = 0; mode < 3; ++mode) {                                     // 0: arrives, 1: fails, 2: arrives, abandoned
                dst.assign(pitch * m, 0);
                std::atomic<int> calls{0};
                bool early = false, ended = true;
                auto arrived = [&]() -> bool {
                    calls.fetch_add(1);
                    std::this_thread::sleep_for(std::chrono::milliseconds(3));
                    for (uint8_t v : dst) early = early || v != 0;                     // (a copy under way here is a race for TSan too)
                    return mode != 1;
                };
                {
                    PixelDrain drain(&pool, pool_threads, piece);
                    if (!drain.end()) { std::printf("drain: end() without begin() failed\n"); ++failures; }
                    drain.begin(m, src.data(), bytes, dst.data(), pitch, arrived);
                    if (mode != 2) ended = drain.end();
                }
                const char *what = mode == 0 ? "arrives" : mode == 1 ? "fails" : "abandoned";
                if (calls.load() != 1) { std::printf("drain %s, pool %d, %zu bytes: the callable ran %d times\n", what, pool_threads, bytes, calls.load()); ++failures; }
                if (early) { std::printf("drain %s, pool %d, %zu bytes: copied before the callable answered\n", what, pool_threads, bytes); ++failures; }
                if (ended != (mode != 1)) { std::printf("drain %s, pool %d, %zu bytes: end() returned %d\n", what, pool_threads, bytes, (int)ended); ++failures; }
                size_t wrong = 0;
                for (size_t b = 0; b < dst.size(); ++b) {
                    const size_t i = b / pitch, at = b % pitch;
                    const uint8_t want = mode != 1 && at < bytes ? src[i * bytes + at] : 0;
                    wrong += dst[b] != want;
                }
                if (wrong) { std::printf("drain %s, pool %d, %zu bytes: %zu bytes of the destination are wrong\n", what, pool_threads, bytes, wrong); ++failures; }
            }
        }
    }
    return failures;
}

int main()
{
    std::mt19937 rng(7);
    int failures = 0;
    for (int pool_threads : {1, 2, 5, 16}) {
        WorkerPool pool(pool_threads);
        for (int round = 0; round < 300; ++round) {
            const int count = (int)(rng() % 70), limit = 1 + (int)(rng() % (unsigned)(pool_threads + 2));
            std::vector<std::atomic<int>> hits((size_t)std::max(count, 1));
            for (auto &h : hits) h.store(0);
            std::mutex m;
            std::set<std::thread::id> who;
            const bool split = rng() & 1;
            auto job = [&](int i) {
                hits[(size_t)i].fetch_add(1);
                std::lock_guard<std::mutex> g(m);
                who.insert(std::this_thread::get_id());
            };
            if (split) { pool.begin(count, job, limit); pool.finish(); }
            else pool.run(count, job, limit);
            for (int i = 0; i < count; ++i) if (hits[(size_t)i].load() != 1) { std::printf("pool %d round %d: item %d ran %d times\n", pool_threads, round, i, hits[(size_t)i].load()); ++failures; }
            if ((int)who.size() > std::min(limit, pool_threads)) { std::printf("pool %d round %d: %zu threads worked, limit %d\n", pool_threads, round, who.size(), limit); ++failures; }
        }
        // the directing thread of jpeg_amd_decompress_batch: chunk k + 1 opened before chunk k is waited for (a pool without a
        // helper: chunk k opened, then decoded in wait(k))
        for (int round = 0; round < 20; ++round) {
            const int files = 1 + (int)(rng() % 200), chunk = 1 + (int)(rng() % 32), nchunks = (files + chunk - 1) / chunk;
            std::vector<std::atomic<int>> hits((size_t)files);
            for (auto &h : hits) h.store(0);
            std::vector<std::vector<uint32_t>> records;
            FileQueue queue(pool, records, files, chunk, std::min(pool_threads, files), [&](int f, std::vector<uint32_t> &) {
                hits[(size_t)f].fetch_add(1);
                return 0;
            }, 1 << 10);
            for (int k = 0; k < nchunks; ++k) {
                queue.open(std::min(queue.threaded() ? k + 2 : k + 1, nchunks));
                if (queue.wait(k) != 0) { std::printf("pool %d: chunk %d failed\n", pool_threads, k); ++failures; }
                for (int f = k * chunk; f < std::min(files, (k + 1) * chunk); ++f)
                    if (hits[(size_t)f].load() != 1) { std::printf("pool %d: chunk %d is back, file %d ran %d times\n", pool_threads, k, f, hits[(size_t)f].load()); ++failures; }
            }
        }
    }
    // abort mid-call: files 3 and 5 of chunk 0 fail (wait(0) reports the last one); the director leaves after wait(0) while chunk 1's files are being decoded into
    // records grown past the trim threshold.  The queue must stop and join the threads before it trims (TSan: a record freed under
    // a thread that still writes it), and no file of chunks 2 and 3 (never opened) may run.
    for (int round = 0; round < 5; ++round) {
        WorkerPool pool(5);
        const int files = 32, chunk = 8;
        std::vector<std::atomic<int>> hits((size_t)files);
        for (auto &h : hits) h.store(0);
        std::vector<std::vector<uint32_t>> records;
        int st = 0;
        {
            FileQueue queue(pool, records, files, chunk, 4, [&](int f, std::vector<uint32_t> &record) {
                hits[(size_t)f].fetch_add(1);
                record.resize(4096);
                record[(size_t)f] = (uint32_t)f;
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
                record[(size_t)f + 1] = (uint32_t)f;
                return f == 3 ? -7 : f == 5 ? -9 : 0;
            }, 1024);
            queue.open(2);
            st = queue.wait(0);
        }
        if (st != -9) { std::printf("abort: chunk 0 returned %d\n", st); ++failures; }
        for (int f = 0; f < files; ++f) {
            const int want = f < chunk ? 1 : f < 2 * chunk ? -1 : 0;   // (-1: chunk 1, at most once)
            if (want >= 0 ? hits[(size_t)f].load() != want : hits[(size_t)f].load() > 1) {
                std::printf("abort: file %d ran %d times\n", f, hits[(size_t)f].load());
                ++failures;
            }
        }
        for (const auto &r : records) if (r.capacity() > 1024) { std::printf("abort: a record of %zu kept\n", r.capacity()); ++failures; }
    }
    // no helper thread: every file on the calling thread, exactly once
    {
        WorkerPool pool(1);
        const int files = 100, chunk = 32;
        std::vector<int> hits((size_t)files, 0);
        std::vector<std::vector<uint32_t>> records;
        const std::thread::id self = std::this_thread::get_id();
        FileQueue queue(pool, records, files, chunk, 8, [&](int f, std::vector<uint32_t> &) {
            ++hits[(size_t)f];
            return std::this_thread::get_id() == self ? 0 : -1;
        }, 1024);
        if (queue.threaded()) { std::printf("a pool of one has a helper thread\n"); ++failures; }
        for (int k = 0; k < (files + chunk - 1) / chunk; ++k) {
            queue.open(k + 1);
            if (queue.wait(k) != 0) { std::printf("no helper: chunk %d ran off the calling thread\n", k); ++failures; }
        }
        for (int f = 0; f < files; ++f) if (hits[(size_t)f] != 1) { std::printf("no helper: file %d ran %d times\n", f, hits[(size_t)f]); ++failures; }
    }
    failures += drain_failures();
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
