// FileQueue (jpeg_amd/csrc/worker_pool.hpp) with chunks of DIFFERENT sizes, as jpeg_amd_decompress_tensor_mixed cuts them,
// under ThreadSanitizer: every file exactly once, none before its chunk is opened, a chunk complete when wait() returns; and
// the way out of a failed call -- per-file state that the threads write into must outlive the queue, which stops and joins them.
//   g++ -std=c++17 -O1 -g -fsanitize=thread -I jpeg_amd/csrc tests/cpp/file_queue_chunks_test.cpp -o t -lpthread && ./t
#include <cstdio>
#include <random>

#include "worker_pool.hpp"

using jpeg_amd::FileQueue;
using jpeg_amd::WorkerPool;

int main()
{
    int failures = 0;
    std::mt19937 rng(20241019);
    for (int pool_threads : {1, 2, 5, 16}) {
        WorkerPool pool(pool_threads);
        for (int round = 0; round < 20; ++round) {
            // chunks of 1 .. 32 files, consecutive
            const int files = 1 + (int)(rng() % 200);
            std::vector<int> first{0};
            while (first.back() < files) first.push_back(std::min(files, first.back() + 1 + (int)(rng() % 32)));
            const int nchunks = (int)first.size() - 1;
            std::vector<int> chunk_of((size_t)files);
            for (int k = 0; k < nchunks; ++k)
                for (int f = first[(size_t)k]; f < first[(size_t)k + 1]; ++f) chunk_of[(size_t)f] = k;
            std::vector<std::atomic<int>> hits((size_t)files);
            for (auto &h : hits) h.store(0);
            std::atomic<int> opened{0}, early{0};
            std::vector<std::vector<uint32_t>> records;
            FileQueue queue(pool, records, first, std::min(pool_threads, files), [&](int f, std::vector<uint32_t> &) {
                hits[(size_t)f].fetch_add(1);
                if (chunk_of[(size_t)f] >= opened.load()) early.fetch_add(1);
                return 0;
            }, 1 << 10);
            for (int k = 0; k < nchunks; ++k) {
                const int upto = std::min(queue.threaded() ? k + 2 : k + 1, nchunks);
                opened.store(std::max(opened.load(), upto));
                queue.open(upto);
                if (queue.wait(k) != 0) { std::printf("pool %d: chunk %d failed\n", pool_threads, k); ++failures; }
                for (int f = first[(size_t)k]; f < first[(size_t)k + 1]; ++f)
                    if (hits[(size_t)f].load() != 1) { std::printf("pool %d: chunk %d is back, file %d ran %d times\n", pool_threads, k, f, hits[(size_t)f].load()); ++failures; }
            }
            if (early.load()) { std::printf("pool %d: %d files ran before their chunk was opened\n", pool_threads, early.load()); ++failures; }
        }
    }
    // a failed call: file 2 of chunk 0 (3 files) fails; the director leaves after wait(0) while chunk 1 (9 files) is being decoded
    // into the per-file state, which is declared BEFORE the queue and so destroyed after it has joined the threads; chunk 2 was
    // never opened
    for (int round = 0; round < 5; ++round) {
        WorkerPool pool(5);
        const std::vector<int> first{0, 3, 12, 20};
        std::vector<std::atomic<int>> hits(20);
        for (auto &h : hits) h.store(0);
        std::vector<std::vector<uint32_t>> records;
        int st = 0;
        {
            std::vector<std::vector<int>> state(20);
            FileQueue queue(pool, records, first, 4, [&](int f, std::vector<uint32_t> &record) {
                hits[(size_t)f].fetch_add(1);
                record.resize(4096);
                state[(size_t)f].assign(64, f);
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
                state[(size_t)f][63] = -f;
                return f == 2 ? -7 : 0;
            }, 1024);
            queue.open(2);
            st = queue.wait(0);
        }
        if (st != -7) { std::printf("abort: chunk 0 returned %d\n", st); ++failures; }
        for (int f = 0; f < 20; ++f) {
            const int n = hits[(size_t)f].load();
            if (f < 3 ? n != 1 : f < 12 ? n > 1 : n != 0) { std::printf("abort: file %d ran %d times\n", f, n); ++failures; }
        }
        for (const auto &r : records) if (r.capacity() > 1024) { std::printf("abort: a record of %zu kept\n", r.capacity()); ++failures; }
    }
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
