// WorkerPool and FileQueue (jpeg_amd/csrc/worker_pool.hpp) under ThreadSanitizer: every item of every region runs exactly once,
// a region uses no more threads than it was given, begin() returns before the work is done and finish() joins it, regions of
// every size follow each other on one pool; the file queue of jpeg_amd_decompress_batch decodes every file exactly once and
// every chunk completely, on the calling thread when the pool has no helper, and a call that fails in chunk 0 while chunk 1 is
// being decoded stops its threads before it trims their records and never starts a chunk that was not opened.
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
using jpeg_amd::WorkerPool;

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
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
