// ChunkLoop (jpeg_amd/csrc/worker_pool.hpp), the chunk loop of the batch decodes, under ThreadSanitizer with a fake device:
//   g++ -std=c++17 -O1 -g -fsanitize=thread -I jpeg_amd/csrc tests/cpp/chunk_loop_test.cpp -o t -lpthread && ./t
// Pools of 1, 2, 5 and 16 threads, uniform and ragged chunkings of 1 to 7 chunks, with and without a drain, with and without
// the wait for the pixels of a direct download; every fake sleeps 0 to 2 ms at random.  What is asserted, by letter:
//  a. no file of chunk j >= 2 is decoded before slot_free(j & 1) has returned true after submit(j - 2);
//  b. packed_end of a slot is 0 when the first file of a chunk packs into it (the chunk's records lie one behind the other from
//     0), and is the sum of the chunk's records when submit reads it;
//  c. submit(k) runs after every file of chunk k has returned, in order of k, on the calling thread;
//  d. the drain of chunk k - 1 is begun after submit(k) and ended before submit(k + 1), the last chunk is drained before the
//     loop returns;
//  e. a decode failure in chunk 1 of 4, a submit failure and a slot_free that answers false each end the loop with that status;
//  f. after such a failure no later submit runs, no file of an unopened chunk is ever decoded, and the threads are joined before
//     the per-file state, declared before the loop, is destroyed (TSan: a write into freed memory);
//  g. with a pool of one thread everything runs on the caller.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <numeric>
#include <thread>
#include <vector>
#include "worker_pool.hpp"

using jpeg_amd::ChunkDevice;
using jpeg_amd::ChunkLoop;
using jpeg_amd::WorkerPool;

static std::atomic<uint32_t> g_nap{1};
static uint32_t draw() { return (g_nap.fetch_add(1) * 2654435761u) >> 8; }
static void nap() { std::this_thread::sleep_for(std::chrono::microseconds(draw() % 2001)); }

static int g_failures = 0;
static std::atomic<int> g_thread_failures{0};
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); ++g_failures; } } while (0)
#define CHECK_T(cond) do { if (!(cond)) g_thread_failures.fetch_add(1); } while (0)   // on any thread

enum Fault { kNone, kDecode, kSubmit, kSlot };
constexpr int kDecodeFailed = -7, kSubmitFailed = -9, kDeviceFailed = -3;

// What the files of one call leave behind; it lives in a scope of its own, which ends right behind the loop.
struct PerFile {
    std::atomic<int> hits{0}, done{0};
    size_t size = 0, where = ~(size_t)0;
    std::thread::id who;
    uint32_t scribble[2] = {0, 0};
};

// One call.  -> the loop's status
static int one_call(const char *what, int pool_threads, const std::vector<int> &first, bool drain, bool direct, Fault fault)
{
    const int nchunks = (int)first.size() - 1, files = first.back();
    const std::thread::id self = std::this_thread::get_id();
    WorkerPool pool(pool_threads);
    std::vector<std::vector<uint32_t>> records;
    int status = 0, submitted = 0, freed_next = 2, drains_begun = 0, drains_ended = 0, last_drained = -1;
    bool draining = false, finished = false;
    std::vector<int> hits((size_t)files, 0);
    {
        std::unique_ptr<PerFile[]> state(new PerFile[(size_t)files]);
        std::vector<std::atomic<int>> slot_freed((size_t)nchunks + 2);
        for (auto &f : slot_freed) f.store(0);
        std::atomic<int> submitted_seen{0};
        for (int f = 0; f < files; ++f) state[(size_t)f].size = 1 + draw() % 100;
        ChunkLoop loop;
        auto chunk_of = [&](int file) { return (int)(std::upper_bound(first.begin(), first.end(), file) - first.begin()) - 1; };
        ChunkDevice dev;
        dev.failure = kDeviceFailed;
        dev.slot_free = [&](int slot) {
            const int j = freed_next++;
            CHECK(std::this_thread::get_id() == self, "%s: slot_free off the calling thread", what);
            CHECK(slot == (j & 1) && submitted >= j - 1, "%s: slot_free(%d) for chunk %d with %d chunks submitted", what, slot, j, submitted);   // (a)
            nap();
            if (fault == kSlot) return false;
            slot_freed[(size_t)j].store(1);
            return true;
        };
        dev.submit = [&](int k) {
            CHECK(std::this_thread::get_id() == self && k == submitted, "%s: submit(%d) is submission %d, or off the calling thread", what, k, submitted);   // (c)
            size_t sum = 0;
            std::vector<std::pair<size_t, size_t>> packed;
            for (int f = first[(size_t)k]; f < first[(size_t)k + 1]; ++f) {
                PerFile &p = state[(size_t)f];
                CHECK(p.done.load() == 1, "%s: submit(%d) before file %d has returned", what, k, f);                                  // (c)
                sum += p.size;
                packed.emplace_back(p.where, p.size);
            }
            CHECK(loop.packed_end[k & 1].load() == sum, "%s: submit(%d) reads packed_end %zu, the records are %zu", what, k, loop.packed_end[k & 1].load(), sum);   // (b)
            std::sort(packed.begin(), packed.end());
            size_t at = 0;
            for (const auto &p : packed) { CHECK(p.first == at, "%s: chunk %d: a record at %zu, not %zu", what, k, p.first, at); at += p.second; }   // (b): from 0, no gap
            CHECK(!draining, "%s: submit(%d) while chunk %d is being drained", what, k, last_drained);                                  // (d)
            if (drain && k >= 2) CHECK(last_drained == k - 2, "%s: submit(%d) and the last chunk drained is %d", what, k, last_drained);  // (d)
            nap();
            ++submitted;
            submitted_seen.store(submitted);
            return fault == kSubmit && k == 1 ? kSubmitFailed : 0;
        };
        dev.finished = [&](int slot) {
            CHECK(slot == ((nchunks - 1) & 1) && submitted == nchunks, "%s: finished(%d) with %d of %d submitted", what, slot, submitted, nchunks);
            nap();
            finished = true;
            return true;
        };
        if (direct)
            dev.pixels_gone = [&](int slot) {
                CHECK(slot == (submitted & 1) && submitted >= 2, "%s: pixels_gone(%d) in front of submit(%d)", what, slot, submitted);
                nap();
                return true;
            };
        if (drain) {
            dev.begin_drain = [&](int k) {
                CHECK(!draining && k == last_drained + 1, "%s: drain of chunk %d begun behind chunk %d", what, k, last_drained);
                CHECK(k == nchunks - 1 ? finished : submitted == k + 2, "%s: drain of chunk %d begun with %d submitted", what, k, submitted);   // (d)
                draining = true;
                last_drained = k;
                ++drains_begun;
            };
            dev.end_drain = [&] {
                if (draining) { nap(); ++drains_ended; }
                draining = false;
                return true;
            };
        }
        status = loop.run(pool, records, first, std::min(pool_threads, files), [&](int file, std::vector<uint32_t> &record) {
            PerFile &p = state[(size_t)file];
            const int j = chunk_of(file);
            p.hits.fetch_add(1);
            p.who = std::this_thread::get_id();
            if (j >= 2) CHECK_T(slot_freed[(size_t)j].load() == 1);                                                                       // (a)
            CHECK_T(submitted_seen.load() >= j - 1);                                                                                      // (a): submit(j - 2) has run
            record.resize(128);
            p.scribble[0] = (uint32_t)file;
            nap();
            p.where = loop.packed_end[j & 1].fetch_add(p.size);
            p.scribble[1] = (uint32_t)file;                                                                                               // (f): still alive?
            p.done.store(1);
            return fault == kDecode && j == 1 && file == first[1] ? kDecodeFailed : 0;
        }, 1 << 10, dev);
        for (int f = 0; f < files; ++f) {
            hits[(size_t)f] = state[(size_t)f].hits.load();
            if (pool_threads == 1) CHECK(hits[(size_t)f] == 0 || state[(size_t)f].who == self, "%s: file %d ran off the calling thread", what, f);   // (g)
        }
    }   // (f): the per-file state goes here; a thread that still ran would write into freed memory
    if (fault == kNone) {
        CHECK(status == 0 && submitted == nchunks && finished, "%s: status %d, %d of %d chunks submitted", what, status, submitted, nchunks);
        for (int f = 0; f < files; ++f) CHECK(hits[(size_t)f] == 1, "%s: file %d ran %d times", what, f, hits[(size_t)f]);
        if (drain) CHECK(drains_begun == nchunks && drains_ended == nchunks && last_drained == nchunks - 1, "%s: %d drains begun, %d ended", what, drains_begun, drains_ended);   // (d)
    } else {
        // (e), (f): of 4 chunks, the decode and the submit fault are chunk 1's -- chunk 3 was never opened; the slot that is not
        // freed is chunk 2's first wait -- chunk 2 was never opened either
        const int want = fault == kDecode ? kDecodeFailed : fault == kSubmit ? kSubmitFailed : kDeviceFailed;
        CHECK(status == want, "%s: status %d, not %d", what, status, want);
        CHECK(submitted <= (fault == kDecode ? 1 : 2) && !finished, "%s: %d chunks submitted after the failure", what, submitted);
        for (int f = first[fault == kSlot ? 2 : 3]; f < files; ++f) CHECK(hits[(size_t)f] == 0, "%s: file %d of an unopened chunk ran", what, f);
        for (int f = 0; f < files; ++f) CHECK(hits[(size_t)f] <= 1, "%s: file %d ran %d times", what, f, hits[(size_t)f]);
        CHECK(!draining, "%s: a drain was left running", what);
    }
    return status;
}

int main()
{
    char what[128];
    for (int pool_threads : {1, 2, 5, 16})
        for (int nchunks = 1; nchunks <= 7; ++nchunks)
            for (int ragged = 0; ragged < 2; ++ragged)
                for (int mode = 0; mode < 3; ++mode) {                     // 0: device output, 1: a drain, 2: a direct download
                    std::vector<int> first{0};
                    const int chunk = 1 + (int)(draw() % 6);
                    for (int k = 0; k < nchunks; ++k) {
                        const int m = ragged ? 1 + (int)(draw() % 9) : k + 1 < nchunks ? chunk : 1 + (int)(draw() % (unsigned)chunk);
                        first.push_back(first.back() + m);
                    }
                    std::snprintf(what, sizeof what, "pool %d, %d %s chunks, mode %d", pool_threads, nchunks, ragged ? "ragged" : "uniform", mode);
                    one_call(what, pool_threads, first, mode == 1, mode == 2, kNone);
                }
    for (int pool_threads : {1, 2, 5, 16})
        for (Fault fault : {kDecode, kSubmit, kSlot})
            for (int mode = 0; mode < 2; ++mode) {
                std::snprintf(what, sizeof what, "pool %d, fault %d, %s", pool_threads, (int)fault, mode ? "drain" : "no drain");
                one_call(what, pool_threads, {0, 5, 9, 16, 20}, mode == 1, false, fault);
            }
    if (g_thread_failures.load()) { std::printf("%d files were decoded before their slot was free\n", g_thread_failures.load()); ++g_failures; }
    std::printf("%s\n", g_failures ? "FAILED" : "ok");
    return g_failures ? 1 : 0;
}
