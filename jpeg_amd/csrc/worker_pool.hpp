// worker_pool.hpp -- the host threads of the batch file paths (capi_file.hip, capi_files.hip): the pool, the file queue of the
// batch decodes, the drain of their pixels and the chunk loop that directs them.  Header-only and free of HIP so that
// tests/cpp/worker_pool_test.cpp and chunk_loop_test.cpp can run it under ThreadSanitizer on a machine without a GPU.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace jpeg_amd {

// The host threads of the batch file paths, kept in the context between calls and handed one parallel region after the other.
// (Starting 32 threads per chunk cost more than half of what a chunk of 32 1080p files takes them; starting and ending them
// per CALL still meant 32 stacks unmapped per call, and an munmap is what the GPU driver's MMU notifier answers by stopping
// the queues: every other batch of 512 files took 50 instead of 20 ms.)  Items are drawn from a counter (files differ in length); the calling thread works too.  Not re-entrant:
// one region at a time.
class WorkerPool {
public:
    explicit WorkerPool(int nthreads)
    {
        try {
            threads_.reserve((size_t)std::max(0, nthreads - 1));
            for (int t = 1; t < nthreads; ++t) threads_.emplace_back([this, t] { work(t - 1); });
        } catch (...) {      // fewer threads than asked for: the ones that did start (and the caller) do the work
        }
    }
    ~WorkerPool()
    {
        finish();
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        go_.notify_all();
        for (std::thread &t : threads_) t.join();
    }
    int size() const { return (int)threads_.size() + 1; }      // the calling thread included
    WorkerPool(const WorkerPool &) = delete;
    WorkerPool &operator=(const WorkerPool &) = delete;
    // fn(i) for i in [0, count); fn does not throw.  begin() hands the region to the workers and returns; finish() has the
    // calling thread take its share and waits for the rest.
    // `threads`: how many threads may work on the region, the calling one (in finish()) included; the pool may be larger
    void begin(int count, std::function<void(int)> fn, int threads = 1 << 30)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = std::move(fn); count_ = std::max(0, count); next_.store(0);
            limit_ = std::max(0, threads - 1);
            busy_ = (int)threads_.size();
            ++generation_;
            open_ = true;
        }
        go_.notify_all();
    }
    void finish()
    {
        if (!open_) return;
        for (int i; (i = next_.fetch_add(1)) < count_;) job_(i);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return busy_ == 0; });
        open_ = false;
    }
    void run(int count, std::function<void(int)> fn, int threads = 1 << 30)
    {
        begin(count, std::move(fn), threads);
        finish();
    }

private:
    void work(int id)
    {
        unsigned long seen = 0;
        for (;;) {
            int count;
            {
                std::unique_lock<std::mutex> g(m_);
                go_.wait(g, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                count = id < limit_ ? count_ : -1;             // (a thread beyond the region's limit only reports back: it must not draw an item)
            }
            if (count >= 0)
                for (int i; (i = next_.fetch_add(1)) < count;) job_(i);   // (job_ is not touched until every worker has reported back)
            std::lock_guard<std::mutex> g(m_);
            if (--busy_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable go_, done_;
    std::function<void(int)> job_;
    std::atomic<int> next_{0};
    int count_ = 0, busy_ = 0, limit_ = 0;
    bool open_ = false;
    unsigned long generation_ = 0;
    bool stop_ = false;
};

// The host-thread side of a batch decode (jpeg_amd_decompress_batch, jpeg_amd_decompress_tensor_mixed): `files` files in chunks
// of `chunk` -- or in chunks of sizes of the caller's, given by their first files -- drawn from ONE
// counter for the whole call by `threads` threads of the pool, each with its own record (records[index], kept by the caller
// between calls).  No barrier between chunks: a thread that is done with its file of chunk k goes on with chunk k + 1 while a
// slower one still works on chunk k -- but a file is not started before its chunk is opened.  The calling thread directs:
// open(j) lets chunks [0, j) be decoded, wait(k) returns once chunk k is.  A pool without a helper thread decodes nothing by
// itself: wait(k) decodes chunk k on the calling thread.  decode(file, record) returns 0 or an error status and does not throw.
class FileQueue {
public:
    using Decode = std::function<int(int, std::vector<uint32_t> &)>;
    FileQueue(WorkerPool &pool, std::vector<std::vector<uint32_t>> &records, int files, int chunk, int threads, Decode decode,
              size_t trim_above)
        : FileQueue(pool, records, uniform_chunks(files, chunk), threads, std::move(decode), trim_above)
    {
    }
    // Chunks of different sizes: chunk k is files [first[k], first[k + 1]), first.back() the number of files.
    FileQueue(WorkerPool &pool, std::vector<std::vector<uint32_t>> &records, std::vector<int> first, int threads, Decode decode,
              size_t trim_above)
        : pool_(pool), records_(records), decode_(std::move(decode)), first_(std::move(first)), files_(first_.back()),
          trim_above_(trim_above), inline_(pool.size() < 2), status_((size_t)files_, 0), left_(first_.size() - 1)
    {
        for (size_t k = 0; k < left_.size(); ++k) left_[k] = first_[k + 1] - first_[k];
        if (records_.size() < (size_t)std::max(1, threads)) records_.resize((size_t)std::max(1, threads));
        if (!inline_) pool_.begin(threads, [this](int index) { work(records_[(size_t)index]); }, threads + 1);
    }
    // Every way out of a call comes through here, a failed chunk included, while threads may still be decoding later chunks into
    // their records: they are stopped and joined BEFORE the records a call on huge frames left behind (hundreds of MB each) are
    // trimmed -- never the other way round.
    ~FileQueue()
    {
        { std::lock_guard<std::mutex> g(m_); abort_ = true; }
        cv_.notify_all();
        pool_.finish();
        for (std::vector<uint32_t> &r : records_)
            if (r.capacity() > trim_above_) std::vector<uint32_t>().swap(r);
    }
    bool threaded() const { return !inline_; }
    void open(int chunks)
    {
        { std::lock_guard<std::mutex> g(m_); open_ = std::max(open_, chunks); }
        cv_.notify_all();
    }
    // chunk k must have been opened; returns the status of its last failing file (0: every file decoded)
    int wait(int k)
    {
        const int end = first_[(size_t)k + 1];
        if (inline_)
            while (next_.load() < end) run(next_.fetch_add(1), records_[0]);
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return left_[(size_t)k] == 0; });
        int st = 0;
        for (int file = first_[(size_t)k]; file < end; ++file)
            if (status_[(size_t)file] != 0) st = status_[(size_t)file];
        return st;
    }

    static std::vector<int> uniform_chunks(int files, int chunk)
    {
        std::vector<int> first;
        for (int f = 0; f < files; f += chunk) first.push_back(f);
        first.push_back(files);
        return first;
    }

private:
    int chunk_of(int file) const { return (int)(std::upper_bound(first_.begin(), first_.end(), file) - first_.begin()) - 1; }
    void run(int file, std::vector<uint32_t> &record)
    {
        status_[(size_t)file] = decode_(file, record);
        std::lock_guard<std::mutex> g(m_);
        if (--left_[(size_t)chunk_of(file)] == 0) cv_.notify_all();
    }
    void work(std::vector<uint32_t> &record)
    {
        for (;;) {
            const int file = next_.fetch_add(1);
            if (file >= files_) return;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return abort_ || open_ > chunk_of(file); });
                if (abort_) return;
            }
            run(file, record);
        }
    }
    WorkerPool &pool_;
    std::vector<std::vector<uint32_t>> &records_;
    const Decode decode_;
    const std::vector<int> first_;   // chunk k: files [first_[k], first_[k + 1])
    const int files_;
    const size_t trim_above_;
    const bool inline_;
    std::vector<int> status_;        // per file, read by wait() once the file's chunk is complete
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<int> left_;          // files of chunk k not decoded yet
    std::atomic<int> next_{0};
    int open_ = 0;
    bool abort_ = false;
};

// m images of `bytes` bytes each, cut into pieces of at most `piece` bytes so that one huge image is shared by the threads of
// a region too: item j of count(m) is bytes [lo, lo + len) of image i.
struct Pieces {
    size_t bytes, piece, per_image;
    Pieces(size_t bytes_, size_t piece_) : bytes(bytes_), piece(piece_), per_image((bytes_ + piece_ - 1) / piece_) {}
    int count(int m) const { return (int)(per_image * (size_t)m); }
    struct At { size_t i, lo, len; };
    At at(size_t j) const
    {
        const size_t lo = (j % per_image) * piece;
        return At{j / per_image, lo, std::min(piece, bytes - lo)};
    }
};

// The way back of a chunk's pixels in jpeg_amd_decompress_batch: m images of `bytes` bytes, one behind the other at `src`, are
// copied to `dst` at a pitch of `dst_stride` by the threads of a pool (pieces of <= 8 MiB; the test takes smaller ones) once
// their download is complete.
// `arrived` waits for the download and says whether the pixels are there: the first thread to get to the region runs it,
// exactly once, and the others wait for that thread; nothing is copied before it has answered true, and nothing at all once it
// has answered false.  begin() returns at once; end() has the calling thread copy too, joins the region and reports whether
// the pixels arrived (true as well when nothing was begun).  The destructor joins: no region outlives its drain.
class PixelDrain {
public:
    PixelDrain(WorkerPool *pool, int threads, size_t piece = (size_t)8 << 20) : pool_(pool), threads_(threads), piece_(piece) {}
    ~PixelDrain() { (void)end(); }
    PixelDrain(const PixelDrain &) = delete;
    PixelDrain &operator=(const PixelDrain &) = delete;
    void begin(int m, const uint8_t *src, size_t bytes, uint8_t *dst, size_t dst_stride, std::function<bool()> arrived)
    {
        const Pieces pieces(bytes, piece_);
        state_.store(0);
        draining_ = true;
        pool_->begin(pieces.count(m), [this, pieces, src, dst, dst_stride, arrived](int j) {
            int zero = 0;
            if (state_.compare_exchange_strong(zero, 1)) state_.store(arrived() ? 2 : 3);
            while (state_.load() < 2) std::this_thread::sleep_for(std::chrono::microseconds(50));
            if (state_.load() != 2) return;
            const Pieces::At p = pieces.at((size_t)j);
            std::memcpy(dst + p.i * dst_stride + p.lo, src + pieces.bytes * p.i + p.lo, p.len);
        }, threads_);
    }
    bool end()
    {
        if (!draining_) return true;
        pool_->finish();
        draining_ = false;
        return state_.load() == 2;
    }

private:
    WorkerPool *pool_;
    const int threads_;
    const size_t piece_;
    std::atomic<int> state_{0};      // 0: nobody has looked yet, 1: a thread is waiting, 2: the pixels are there, 3: failed
    bool draining_ = false;
};

// The device side of a batch decode, as the chunk loop sees it.  Chunk k is decoded into pinned slot k & 1 and submitted from
// there; a callable that answers false has failed (and has noted why), and the loop ends with `failure`.
struct ChunkDevice {
    std::function<bool(int)> slot_free;      // (slot) wait until the chunk last submitted from the slot has been read out of it
    std::function<int(int)> submit;          // (k) enqueue chunk k, whose files are all decoded; a status
    std::function<bool(int)> finished;       // (slot) wait until the chunk last submitted from the slot is where the call leaves it
    // a call whose pixels go straight from the device slot to the caller: (slot) wait until the pixels of the chunk last
    // submitted from the slot have left, in front of the next submission from it (empty: nothing of the kind)
    std::function<bool(int)> pixels_gone;
    // a call whose pixels are copied out of the pinned slot by host threads (PixelDrain): begin(k) starts the copy of chunk k
    // once it has arrived, end() joins it and says whether it arrived (empty: no copy)
    std::function<void(int)> begin_drain;
    std::function<bool()> end_drain;
    int failure;
};

// The chunk loop of the batch decodes (jpeg_amd_decompress_batch[_device], jpeg_amd_decompress_tensor_mixed, _resized_mixed):
// ONE queue of files for the whole call (FileQueue), decoded on `threads` host threads beside the calling one, which directs and
// submits a chunk to the device as soon as its last file is in.
//  - With threads, chunk k + 1 is opened while they are in chunk k: a thread that is through with chunk k goes straight on, and
//    the director waits for chunk k - 1's kernels where it has nothing else to do.  Without, it decodes chunk k itself, in
//    wait(k), in front of the chunk's submission.
//  - Chunk j is decoded into pinned slot j & 1, which is opened again only after slot_free(j & 1): the uploads of chunk j - 2
//    have read it.  packed_end[j & 1] -- the elements of the sparse records that the files of a chunk have packed one behind
//    the other into the slot, drawn by each with one fetch_add -- is reset then, and read by submit(j).
//  - The drain of chunk k - 1 runs beside the decoding of chunk k + 1 and is joined before chunk k + 1 is submitted: its download
//    lands in the same pinned slot.  The copy only reads the slot's pixels, which the decoders do not touch.
//  - The last chunk is waited for (and drained) on the way out.
// Returns the first failing status: of a file (the last failing one of its chunk), of submit, or `failure`.  On a failure copies
// and kernels may be in flight: the caller waits for its streams.  The queue dies in here, so the threads are stopped and
// joined before run() returns: what decode() writes into must have been declared before the call, nothing more.
struct ChunkLoop {
    std::atomic<size_t> packed_end[2];

    int run(WorkerPool &pool, std::vector<std::vector<uint32_t>> &records, const std::vector<int> &first, int threads,
            FileQueue::Decode decode, size_t trim_above, const ChunkDevice &dev)
    {
        const int nchunks = (int)first.size() - 1, ok = 0;
        int result = ok;
        packed_end[0].store(0); packed_end[1].store(0);
        auto end_drain = [&] { return !dev.end_drain || dev.end_drain() ? ok : dev.failure; };
        {
            FileQueue queue(pool, records, first, threads, std::move(decode), trim_above);
            for (int k = 0; k < nchunks && result == ok; ++k) {
                const int j = queue.threaded() ? k + 1 : k;
                if (j >= 2 && j < nchunks) {
                    if (!dev.slot_free(j & 1)) { result = dev.failure; break; }
                    packed_end[j & 1].store(0);                       // (chunks 0 and 1 start from the initial zeros)
                }
                queue.open(std::min(j + 1, nchunks));
                result = queue.wait(k);
                if (end_drain() != ok) result = dev.failure;          // chunk k - 1 is out of its pinned slot: chunk k + 1's download may land there
                if (result == ok && dev.pixels_gone && k >= 2 && !dev.pixels_gone(k & 1)) result = dev.failure;
                if (result == ok) result = dev.submit(k);
                if (result == ok && k >= 1 && dev.begin_drain) dev.begin_drain(k - 1);
            }
            const int drained = end_drain();
            if (result == ok) result = drained;
        }
        if (result != ok) return result;
        if (!dev.finished((nchunks - 1) & 1)) return dev.failure;
        if (dev.begin_drain) dev.begin_drain(nchunks - 1);
        return end_drain();
    }
};

}  // namespace jpeg_amd
