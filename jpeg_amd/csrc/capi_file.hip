// capi_file.hip -- the C ABI, file unit: JPEG bytes to pixels and back (one file, and the two batch pipelines), and the
// file-to-file calls of the coefficient domain.  The host threads and the pixel drain are in worker_pool.hpp; the files of
// mixed sizes to one tensor are in capi_files.hip, which shares the staging helpers at the head of this file.
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace jpeg_amd {
namespace capi {

// The staging the two batch entry points for files share, kept in the context between calls: two pinned host slots (the host
// threads work in one while the device works from / into the other), two device slots, two events per slot and a second
// stream so that uploads and downloads overlap (full-duplex PCIe).
int ensure_file_staging(jpeg_amd_ctx *ctx, size_t slot_bytes, size_t device_slot_bytes)
{
    if (ctx->file_pinned_bytes < slot_bytes) {
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 2; ++i) {
            if (ctx->file_pinned[i]) { (void)hipHostFree(ctx->file_pinned[i]); ctx->file_pinned[i] = nullptr; }
            ctx->file_pinned_bytes = 0;
            JA_HIP(ctx, hipHostMalloc(&ctx->file_pinned[i], slot_bytes, hipHostMallocDefault));
            if (!ctx->file_done[i]) JA_HIP(ctx, hipEventCreateWithFlags(&ctx->file_done[i], hipEventDisableTiming));
            if (!ctx->file_decoded[i]) JA_HIP(ctx, hipEventCreateWithFlags(&ctx->file_decoded[i], hipEventDisableTiming));
            if (!ctx->file_fetched[i]) JA_HIP(ctx, hipEventCreateWithFlags(&ctx->file_fetched[i], hipEventDisableTiming));
        }
        ctx->file_pinned_bytes = slot_bytes;
    }
    if (!ctx->file_d2h) JA_HIP(ctx, hipStreamCreateWithFlags(&ctx->file_d2h, hipStreamNonBlocking));
    if (ctx->file_device_bytes < 2 * device_slot_bytes) {           // two device slots as well
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        JA_HIP(ctx, hipStreamSynchronize(ctx->file_d2h));
        if (ctx->file_device) { (void)hipFree(ctx->file_device); ctx->file_device = nullptr; ctx->file_device_bytes = 0; }
        JA_HIP(ctx, hipMalloc(&ctx->file_device, 2 * device_slot_bytes));
        ctx->file_device_bytes = 2 * device_slot_bytes;
    }
    return JPEG_AMD_OK;
}

// How many host threads "all cores" means: the hardware's, capped by the CPU bandwidth the process's control group grants
// (cgroup v2 cpu.max / v1 cfs quota: a container limited to 16 CPUs on a 256-thread host runs 32 busy threads for a few
// milliseconds and is then stopped until the period ends -- seen as every other batch taking 40 ms longer).
int default_host_threads()
{
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    auto read_two = [](const char *path, long long &a, long long &b) -> bool {
        FILE *f = std::fopen(path, "r");
        if (!f) return false;
        char first[32] = {0};
        const bool ok = std::fscanf(f, "%31s %lld", first, &b) == 2;
        std::fclose(f);
        if (!ok || std::strcmp(first, "max") == 0) return false;
        a = std::atoll(first);
        return a > 0 && b > 0;
    };
    long long quota = 0, period = 0;
    if (read_two("/sys/fs/cgroup/cpu.max", quota, period)) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
    else {
        FILE *q = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"), *p = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
        if (q && p && std::fscanf(q, "%lld", &quota) == 1 && std::fscanf(p, "%lld", &period) == 1 && quota > 0 && period > 0)
            n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
        if (q) std::fclose(q);
        if (p) std::fclose(p);
    }
    return n;
}

// Wait for an event of the file pipelines by POLLING it (a yield between polls, a short sleep once the wait is long).
// hipEventSynchronize on an event recorded a millisecond ago sleeps on an interrupt, and on this stack that wake-up takes
// tens of milliseconds every few calls: a batch of 512 1080p files alternated between 19.5 and 50 ms.
hipError_t wait_event(hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) std::this_thread::sleep_for(std::chrono::microseconds(50));
        else std::this_thread::yield();
    }
}

// the context's pool, with at least `threads` threads (the calling one included)
WorkerPool &pool_with(std::unique_ptr<WorkerPool> &pool, int threads)
{
    if (!pool || pool->size() < threads) pool.reset(new WorkerPool(threads));
    return *pool;
}

// The way out of both pipelines: a failure leaves copies and kernels in flight, so both streams are waited for.
int after_both_streams(jpeg_amd_ctx *ctx, int result)
{
    if (result != JPEG_AMD_OK) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->file_d2h); }
    return result;
}

// The `nthreads` argument of the batch file calls: <= 0 leaves the number to the library.
int host_threads(int nthreads, bool *auto_threads)
{
    if (auto_threads) *auto_threads = nthreads <= 0;
    return std::max(1, nthreads <= 0 ? default_host_threads() : nthreads);
}

// (the infos are the parser's: the units follow from the size and the factors, so this is "one geometry" and no more)
static bool same_frame(const jpeg_amd_frame_info &a, const jpeg_amd_frame_info &b)
{
    bool same = a.width == b.width && a.height == b.height && a.precision == b.precision && a.ncomponents == b.ncomponents;
    for (int c = 0; same && c < a.ncomponents; ++c)
        same = a.factor_x[c] == b.factor_x[c] && a.factor_y[c] == b.factor_y[c] && a.units_x[c] == b.units_x[c] && a.units_y[c] == b.units_y[c];
    return same;
}

int FileBatch::decode_to_slot(int file, const Into &to, const jpeg_amd_frame_info &frame, const SparseBudget &sb, bool inspect_dense,
                              std::vector<uint32_t> &record, uint64_t *where, bool *dense)
try {
    const uint8_t *data = h_jpeg[file];
    *dense = true;
    if (!data) return JPEG_AMD_EINVAL;
    jpeg_amd_frame_info seen{};
    if (to.device) to.device->on = false;
    if ((ctx->flags & JPEG_AMD_CTX_DEVICE_ENTROPY) && to.device) {
        namespace iv = jpeg_amd::interval;
        iv::FilePlan plan;
        const int ps = iv::plan_file(data, nbytes[file], &plan);
        if (ps != JPEG_AMD_OK && ps != JPEG_AMD_ENOSUP) return ps;          // malformed: the host decoder says the same
        if (ps == JPEG_AMD_OK) {
            if (!same_frame(plan.info, frame)) return JPEG_AMD_EINVAL;
            const iv::FileBlock b = iv::file_block(plan);
            bool fits = b.size <= to.room;                                   // (or its bytes and list exceed its plane: the host route)
            for (const iv::IntervalWork &w : plan.work) fits = fits && iv::work_fits(w, plan.scans[w.scan], nbytes[file]);
            if (fits) {
                iv::write_file_block(plan, b, data, reinterpret_cast<char *>(to.planes[0]));
                for (int c = 0; c < plan.info.ncomponents; ++c) std::memcpy(to.quanta[c], plan.quanta[c], 128);
                int16_t *const none[JPEG_AMD_MAX_PLANES] = {nullptr, nullptr, nullptr, nullptr};
                to.device->record = iv::file_record(plan, b, 0, none);
                to.device->bytes = b.size;
                to.device->on = true;
                return JPEG_AMD_OK;                                          // (*dense: the expand leaves its planes alone)
            }
        }
    }
    // Sparse first, without a look at the headers beforehand: the decoder itself refuses a frame with more blocks than the
    // descriptor array holds and never writes past the arena, so a file of another geometry is caught afterwards.
    if (sb.ok) {
        if (record.size() < sb.elems) record.resize(sb.elems);          // (this thread's; kept in the context between calls, trimmed on the way out when huge)
        size_t n = 0;
        const int ss = jpeg_amd_jpeg_decode_sparse(data, nbytes[file], record.data(), sb.blocks, record.data() + sb.blocks, sb.arena, &n, to.quanta, &seen);
        if (ss == JPEG_AMD_OK) {
            if (!same_frame(seen, frame)) return JPEG_AMD_EINVAL;       // (mixed calls: the bytes changed under the call)
            // the record goes behind the ones already in the slot (the records of a chunk, of at most sb.elems each, always fit)
            *where = loop.packed_end[to.slot].fetch_add(sb.blocks + n);
            std::memcpy(to.packed + *where, record.data(), (sb.blocks + n) * 4);
            *dense = false;
            return JPEG_AMD_OK;
        }
        if (ss != JPEG_AMD_ENOSUP) return ss;                           // (EINVAL may be "more blocks than the frame": the same verdict either way)
    }
    // progressive, a missing restart marker, too dense, or not tried: planes (fewer files than threads: the spare threads go to
    // the file's restart intervals)
    if (inspect_dense) {
        JA_TRY(jpeg_amd_jpeg_inspect(data, nbytes[file], &seen));
        if (!same_frame(seen, frame)) return JPEG_AMD_EINVAL;
    }
    const int inner = std::max(1, nthreads / to.m);
    return jpeg_amd_jpeg_decode_spectral_mt(data, nbytes[file], to.planes, to.quanta, nullptr, inner > 1 && auto_threads ? 0 : inner);
}
catch (...) { return JPEG_AMD_ENOMEM; }   // (the record's growth: nothing may be thrown on a thread of the queue)

// The loop's device side on the context's stream and events: file_decoded[slot] is recorded behind the uploads and kernels of
// a chunk, file_done[slot] where its pixels are where the call leaves them (submit records both); a failure is JPEG_AMD_EHIP
// with the context's last_hip set.
ChunkDevice FileBatch::device(std::function<int(int)> submit)
{
    jpeg_amd_ctx *c = ctx;
    auto reached = [c](hipEvent_t ev) {
        const hipError_t w = wait_event(ev);
        if (w != hipSuccess) c->last_hip = (int)w;
        return w == hipSuccess;
    };
    ChunkDevice dev;
    dev.slot_free = [c, reached](int slot) { return reached(c->file_decoded[slot]); };
    dev.finished = [c, reached](int slot) { return reached(c->file_done[slot]); };
    dev.submit = std::move(submit);
    dev.failure = JPEG_AMD_EHIP;
    return dev;
}

// (the threads' sparse records stay in the context between calls -- a batch of 1080p files: 5 MB per thread -- unless huge)
int FileBatch::run_chunks(const std::vector<int> &first, const FileQueue::Decode &decode, const ChunkDevice &dev)
{
    const int t_n = std::min(nthreads, n_images);
    return after_both_streams(ctx, loop.run(pool_with(ctx->workers, t_n + 1), ctx->records, first, t_n, decode, (size_t)16 << 20, dev));
}

}  // namespace capi
}  // namespace jpeg_amd

namespace {

// Is [p, p + bytes) page-locked host memory (hipHostMalloc / hipHostRegister) that a copy engine reaches directly?  Then the
// batch entry points move the caller's buffer itself instead of staging it through their own pinned slots.
bool is_pinned_host(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return false;
    const char *ends[2] = {static_cast<const char *>(p), static_cast<const char *>(p) + bytes - 1};
    for (const char *q : ends) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }   // (unregistered memory: an error, cleared)
        if (at.type != hipMemoryTypeHost || at.isManaged) return false;
    }
    return true;
}

// m images of npx bytes between host and device, image i at i * stride on either side: one copy when both sides are
// contiguous (a staging slot always is; a caller's buffer with a stride of npx), else a copy per image.
hipError_t copy_images(hipStream_t stream, hipMemcpyKind kind, void *dst, size_t dst_stride, const void *src, size_t src_stride, size_t npx,
                       int m)
{
    if (dst_stride == npx && src_stride == npx) return hipMemcpyAsync(dst, src, npx * m, kind, stream);
    for (int i = 0; i < m; ++i) {
        const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + dst_stride * i, static_cast<const char *>(src) + src_stride * i, npx, kind, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Host memory for the coefficient planes of a layout, and the array of pointers into them that the entry points take.
struct HostPlanes {
    std::vector<std::vector<int16_t>> planes;
    int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
    explicit HostPlanes(const jpeg_amd_layout &L) : planes((size_t)L.nplanes)
    {
        for (int c = 0; c < L.nplanes; ++c) {
            planes[c].resize(plane_samples(&L, c));
            coef[c] = planes[c].data();
        }
    }
};

}  // namespace

// ---- JPEG bytes -> pixels (host entropy decode + the fused device path) ----------------------
namespace {
// (defined with the batch pipeline below; device_route: whether JPEG_AMD_CTX_DEVICE_ENTROPY applies to this call)
int decompress_batch_impl(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                          int cosited, jpeg_amd_color color, uint8_t *h_pixels, uint8_t *d_pixels_out, size_t pixel_stride,
                          jpeg_amd_frame_info *info_out, bool device_route);
}  // namespace

int jpeg_amd_decompress(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int cosited,
                        jpeg_amd_color color, uint8_t *h_pixels, size_t pixel_capacity,
                        jpeg_amd_frame_info *info_out)
try {
    JA_TRY(bind(ctx));
    if (!h_jpeg) return JPEG_AMD_EINVAL;
    jpeg_amd_frame_info fi;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg, nbytes, &fi));
    if (info_out) *info_out = fi;
    if (!jpeg_common(fi.precision, fi.ncomponents)) return JPEG_AMD_ENOSUP;
    const size_t need = (size_t)fi.width * fi.height * 3;
    if (!h_pixels || pixel_capacity < need) return JPEG_AMD_EINVAL;
    // a batch of one: pinned staging kept in the context, restart intervals and the copy-out on
    // host threads (their number left to the library)
    // (one file stays on the host route whatever the context's flags say: a lone stream is a lone lane on the device)
    return decompress_batch_impl(ctx, &h_jpeg, &nbytes, 1, 0, cosited, color, h_pixels, nullptr, need, nullptr, false);
}
JA_NOTHROW_TAIL


// Rectangular<Format>.decompress(stream:cosite:) for any format (decode.swift:4367-4374): the one-call form of
// jpeg_amd_jpeg_decode_spectral_mt + jpeg_amd_host_spectral_rectangular.
int jpeg_amd_decompress_rectangular(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int cosited, int nrecognized,
                                    int nthreads, uint16_t *h_rect, size_t rect_capacity, jpeg_amd_frame_info *info_out)
try {
    JA_TRY(bind(ctx));
    if (!h_jpeg) return JPEG_AMD_EINVAL;
    jpeg_amd_frame_info fi;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg, nbytes, &fi));
    if (info_out) *info_out = fi;
    const int nc = fi.ncomponents;
    if (nc < 1 || nc > JPEG_AMD_MAX_PLANES || fi.precision < 1 || fi.precision > 16) return JPEG_AMD_ENOSUP;
    if (nrecognized < 0 || nrecognized > nc) return JPEG_AMD_EINVAL;
    const int np = nrecognized == 0 ? nc : nrecognized;
    const size_t need = (size_t)fi.width * fi.height * np;
    if (!h_rect || rect_capacity < need) return JPEG_AMD_EINVAL;
    // every component is entropy-decoded (a scan may interleave recognised and non-recognised ones); only the recognised
    // planes go to the device
    HostPlanes in(layout_of_info(fi, nc));
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64];
    JA_TRY(jpeg_amd_jpeg_decode_spectral_mt(h_jpeg, nbytes, in.coef, quanta, &fi, nthreads));
    if (info_out) *info_out = fi;
    const jpeg_amd_layout L = layout_of_info(fi, np);
    return jpeg_amd_host_spectral_rectangular(ctx, &L, in.coef, &quanta[0][0], np, cosited, h_rect);
}
JA_NOTHROW_TAIL

// ---- many JPEG files of one geometry -> pixels: host threads entropy-decode a chunk into
//      pinned memory while the device (H2D, fused decode, D2H on the context's stream) works on
//      the previous chunk ----------------------------------------------------------------------
namespace {

// One call of jpeg_amd_decompress_batch[_device] behind its checks: what is constant for the call (set by
// decompress_batch_impl), and the parts of the pipeline.
struct BatchDecode : FileBatch {
    uint8_t *h_pixels, *d_pixels_out;          // in host memory, or left on the device
    size_t pixel_stride, npx, plane[JPEG_AMD_MAX_PLANES] = {};
    jpeg_amd_frame_info fi;                    // image 0's: one geometry per batch
    jpeg_amd_layout L;
    int nc, chunk, nchunks;
    SparseBudget sb;
    SlotLayout at;
    bool to_host, direct_out, copies_out, device_route;
    std::vector<DeviceEntropyFile> device_files;   // per file (JPEG_AMD_CTX_DEVICE_ENTROPY)

    int images(int k) const { return std::min(chunk, n_images - k * chunk); }
    int decode_file(int file, std::vector<uint32_t> &record);
    int submit(int k);
    int run();
};

// The entropy decoding of one file, on a thread of the file queue, into pinned slot k & 1 of its chunk k.
int BatchDecode::decode_file(int file, std::vector<uint32_t> &record)
{
    const int k = file / chunk, i = file - k * chunk, m = images(k);
    char *host = static_cast<char *>(ctx->file_pinned[k & 1]);
    Into to{k & 1, m, reinterpret_cast<uint32_t *>(host + at.sparse_off), reinterpret_cast<uint16_t(*)[64]>(host + at.quanta_off + (size_t)i * kQSlotElems * 2), {}};
    for (int c = 0; c < nc; ++c) to.planes[c] = reinterpret_cast<int16_t *>(host + at.coef_off[c]) + plane[c] * i;
    to.room = plane[0] * 2;
    to.device = device_route ? &device_files[(size_t)file] : nullptr;
    // spare threads only help a file that has restart intervals, and the sparse form is written by one thread per file: with
    // fewer files than threads a batch of such files travels as planes
    SparseBudget mine = sb;
    mine.ok = sb.ok && (nthreads / m <= 1 || fi.restart_interval == 0);
    bool dense = true;
    // (one geometry per batch, image 0's: the buffers are sized for it, and no other file has been looked at)
    const int st = decode_to_slot(file, to, fi, mine, true, record, reinterpret_cast<uint64_t *>(host + at.where_off) + i, &dense);
    reinterpret_cast<uint8_t *>(host + at.skip_off)[i] = dense;
    return st;
}

// the device side of chunk k (asynchronous); the host moves on to chunk k + 1 meanwhile.
// Device slot `slot` was last read by the download of chunk k - 2, finished before drain(k - 2)
// returned.  Upload + kernels on the context's stream, download on the second one.
// (a failure in here leaves copies and kernels in flight: run_chunks() waits for both streams on the way out)
int BatchDecode::submit(int k)
{
    const int slot = k & 1, base = k * chunk, m = images(k);
    char *host = static_cast<char *>(ctx->file_pinned[slot]);
    const uint8_t *skip = reinterpret_cast<const uint8_t *>(host + at.skip_off);
    char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * at.slot_bytes;
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) d_coef[c] = reinterpret_cast<int16_t *>(dev + at.coef_off[c]);
    bool any_sparse = false;
    std::vector<DeviceEntropyJob> jobs;
    for (int i = 0; i < m; ++i) {
        any_sparse = any_sparse || !skip[i];
        const DeviceEntropyFile &df = device_files[(size_t)(base + i)];
        if (df.on) {                                 // its planes are produced on the device, from its block
            DeviceEntropyJob job{&df, host + at.coef_off[0] + plane[0] * 2 * i, {}};
            for (int c = 0; c < nc; ++c) job.d_planes[c] = d_coef[c] + plane[c] * i;
            jobs.push_back(job);
        } else if (skip[i])                          // planes, this image only (progressive, damaged, too dense)
            for (int c = 0; c < nc; ++c)
                JA_HIP(ctx, hipMemcpyAsync(dev + at.coef_off[c] + plane[c] * 2 * i, host + at.coef_off[c] + plane[c] * 2 * i, plane[c] * 2,
                                           hipMemcpyHostToDevice, ctx->stream));
    }
    // tables, flags, record offsets and the packed records: one copy
    JA_HIP(ctx, hipMemcpyAsync(dev + at.quanta_off, host + at.quanta_off, at.sparse_off - at.quanta_off + loop.packed_end[slot].load() * 4, hipMemcpyHostToDevice, ctx->stream));
    JA_TRY(decode_blocks_on_device(ctx, jobs.data(), (int)jobs.size()));
    if (any_sparse) {
        PlaneSetMut cs{};
        for (int c = 0; c < nc; ++c) { cs.ptr[c] = d_coef[c]; cs.stride[c] = plane[c]; }
        JA_HIP(ctx, launch_expand_sparse(ctx->stream, m, L, reinterpret_cast<const uint32_t *>(dev + at.sparse_off), 0, nullptr, 0,
                                         reinterpret_cast<const uint8_t *>(dev + at.skip_off), cs, reinterpret_cast<const uint64_t *>(dev + at.where_off)));
    }
    uint8_t *d_px = to_host ? reinterpret_cast<uint8_t *>(dev + at.px_off) : d_pixels_out + (size_t)base * pixel_stride;
    JA_TRY(jpeg_amd_decode_batch(ctx, &L, m, d_coef, plane, reinterpret_cast<const uint16_t *>(dev + at.quanta_off), kQSlotElems,
                                 JPEG_AMD_MAX_PLANES, cosited, color, d_px, to_host ? npx : pixel_stride));
    JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
    if (!to_host) {                                  // the pixels stay where they are: done when the kernels are
        JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->stream));
        return JPEG_AMD_OK;
    }
    JA_HIP(ctx, hipStreamWaitEvent(ctx->file_d2h, ctx->file_decoded[slot], 0));
    // into the pinned slot, or straight into the caller's page-locked buffer
    if (!direct_out) JA_HIP(ctx, copy_images(ctx->file_d2h, hipMemcpyDeviceToHost, host + at.px_off, npx, dev + at.px_off, npx, npx, m));
    else JA_HIP(ctx, copy_images(ctx->file_d2h, hipMemcpyDeviceToHost, h_pixels + (size_t)base * pixel_stride, pixel_stride, dev + at.px_off, npx, npx, m));
    JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->file_d2h));
    return JPEG_AMD_OK;
}

// The chunk loop is worker_pool.hpp's (ChunkLoop); this is its device side.  The helper threads that copy chunk k - 2's pixels
// out of a pinned slot may still be running while chunk k is decoded into it: they only read the pixel region, which the
// decoders do not touch.
int BatchDecode::run()
{
    WorkerPool *copiers = copies_out ? &pool_with(ctx->copiers, std::min(nthreads, 16) + 1) : nullptr;
    PixelDrain drain(copiers, std::min(nthreads, 16) + 1);
    ChunkDevice dev = device([this](int k) { return submit(k); });
    // (downloads that go straight into the caller's buffer are not waited for by a copy out: the device slot's pixels of chunk
    // k - 2 must have left before chunk k's kernels write there)
    if (direct_out) dev.pixels_gone = dev.finished;
    // Chunk k on its way back: its pixels are copied out of the pinned slot by the context's copy threads once the download is
    // complete (PixelDrain: the first thread to get there waits for it, the others for that thread).
    if (copies_out) {
        dev.begin_drain = [this, &drain](int k) {
            const int device = ctx->device;
            hipEvent_t done = ctx->file_done[k & 1];
            drain.begin(images(k), static_cast<const uint8_t *>(ctx->file_pinned[k & 1]) + at.px_off, npx, h_pixels + (size_t)k * chunk * pixel_stride,
                        pixel_stride, [device, done] {
                            (void)hipSetDevice(device);
                            return wait_event(done) == hipSuccess;
                        });
        };
        dev.end_drain = [this, &drain] {
            const bool arrived = drain.end();
            if (!arrived) ctx->last_hip = (int)hipErrorUnknown;
            return arrived;
        };
    }
    return run_chunks(FileQueue::uniform_chunks(n_images, chunk), [this](int file, std::vector<uint32_t> &record) { return decode_file(file, record); }, dev);
}

// Files -> pixels, in host memory (h_pixels) or left on the device (d_pixels_out): see jpeg_amd_decompress_batch[_device].
int decompress_batch_impl(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                          int cosited, jpeg_amd_color color, uint8_t *h_pixels, uint8_t *d_pixels_out, size_t pixel_stride,
                          jpeg_amd_frame_info *info_out, bool device_route)
{
    JA_TRY(bind(ctx));
    if (!h_jpeg || !nbytes || (!h_pixels && !d_pixels_out) || n_images < 0) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!h_jpeg[0]) return JPEG_AMD_EINVAL;
    BatchDecode d;
    d.ctx = ctx; d.h_jpeg = h_jpeg; d.nbytes = nbytes; d.n_images = n_images; d.cosited = cosited; d.color = color;
    d.h_pixels = h_pixels; d.d_pixels_out = d_pixels_out;
    d.to_host = h_pixels != nullptr;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg[0], nbytes[0], &d.fi));
    if (info_out) *info_out = d.fi;
    if (!jpeg_common(d.fi.precision, d.fi.ncomponents)) return JPEG_AMD_ENOSUP;
    d.nc = d.fi.ncomponents;
    d.npx = (size_t)d.fi.width * d.fi.height * 3;
    if (pixel_stride == 0) pixel_stride = d.npx;
    if (pixel_stride < d.npx) return JPEG_AMD_EINVAL;
    d.pixel_stride = pixel_stride;

    d.L = layout_of_info(d.fi, d.nc);
    for (int c = 0; c < d.nc; ++c) d.plane[c] = plane_samples(&d.L, c);
    d.chunk = std::min(n_images, 32);
    // Sequential files travel as SPARSE coefficients (jpeg_amd_jpeg_decode_sparse: a descriptor per block + an entry per
    // nonzero coefficient, an eighth of the planes for a typical file) and are expanded on the device; an image that does not
    // fit its arena, a progressive or a damaged one is decoded into planes and uploaded whole, like every image of a frame too
    // large for 32-bit descriptors (sparse_budget).
    d.sb = sparse_budget(d.L);
    // slot layout: [coef plane 0 x chunk][plane 1 x chunk][plane 2 x chunk] [quanta x chunk][skip flags][record offsets][records ...] [pixels x chunk]
    // The middle part goes up in ONE copy per chunk: the tables, the per-image flags, where each image's sparse record
    // [descriptors][entries in use] begins, and the records themselves, packed one behind the other in the order the threads
    // finish (a copy per image is 32 more commands per chunk, and every ~2 000 commands the runtime stops for 30 ms).
    for (int c = 0; c < d.nc; ++c) d.at.coef_off[c] = d.at.take(d.plane[c] * 2 * d.chunk);
    d.at.quanta_off = d.at.take((size_t)d.chunk * kQSlotElems * 2);
    d.at.skip_off = d.at.take((size_t)d.chunk);
    d.at.where_off = d.at.take((size_t)d.chunk * 8);
    d.at.sparse_off = d.at.take(d.sb.elems * 4 * d.chunk);
    d.at.px_off = d.at.take(d.to_host ? d.npx * d.chunk : 0);
    JA_TRY(ensure_file_staging(ctx, d.at.slot_bytes, d.at.slot_bytes));
    d.nthreads = host_threads(nthreads, &d.auto_threads);
    d.device_route = device_route;
    d.device_files.resize((size_t)n_images);

    d.nchunks = (n_images + d.chunk - 1) / d.chunk;
    // a caller whose pixel buffer is page-locked gets the download straight into it: no copy out of the pinned slot
    d.direct_out = d.to_host && is_pinned_host(h_pixels, (size_t)(n_images - 1) * pixel_stride + d.npx);
    d.copies_out = d.to_host && !d.direct_out;
    return d.run();
}

}  // namespace

int jpeg_amd_decompress_batch(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                              int n_images, int nthreads, int cosited, jpeg_amd_color color,
                              uint8_t *h_pixels, size_t pixel_stride, jpeg_amd_frame_info *info_out)
try {
    if (!h_pixels) return JPEG_AMD_EINVAL;
    return decompress_batch_impl(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_pixels, nullptr, pixel_stride, info_out, true);
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_batch_device(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                     int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                     uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *info_out)
try {
    if (!d_pixels) return JPEG_AMD_EINVAL;
    return decompress_batch_impl(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr, d_pixels, pixel_stride, info_out, true);
}
JA_NOTHROW_TAIL

// ---- pixels -> JPEG bytes (the fused device path + host entropy encode) ----------------------
int jpeg_amd_compress(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels,
                      jpeg_amd_color color, const int32_t *quanta_key, const uint16_t *h_quanta,
                      const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                      int nscans, const jpeg_amd_metadata *metadata, int nmetadata, uint8_t *h_out, size_t capacity,
                      size_t *nbytes)
try {
    JA_TRY(bind(ctx));
    if (!frame || !h_pixels || !quanta_key || !h_quanta || !h_quanta_keys || !scans || !nbytes) return JPEG_AMD_EINVAL;
    const int nc = frame->ncomponents;
    if (!jpeg_common(frame->precision, nc)) return JPEG_AMD_ENOSUP;
    jpeg_amd_layout L;
    JA_TRY(layout_of_frame(frame, quanta_key, h_quanta_keys, ntables, &L));
    HostPlanes out(L);
    JA_TRY(jpeg_amd_host_encode(ctx, &L, h_pixels, color, h_quanta, ntables, out.coef));
    return jpeg_amd_jpeg_encode_spectral(frame, quanta_key, out.coef, h_quanta, h_quanta_keys, ntables, scans, nscans,
                                         metadata, nmetadata, h_out, capacity, nbytes);
}
JA_NOTHROW_TAIL


// Rectangular<Format>.compress(stream:quanta:) for any format (encode.swift:2031): the one-call form of
// jpeg_amd_host_rectangular_spectral + jpeg_amd_jpeg_encode_spectral.
int jpeg_amd_compress_rectangular(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint16_t *h_rect,
                                  const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys, int ntables,
                                  const jpeg_amd_scan *scans, int nscans, const jpeg_amd_metadata *metadata, int nmetadata,
                                  uint8_t *h_out, size_t capacity, size_t *nbytes)
try {
    JA_TRY(bind(ctx));
    if (!frame || !h_rect || !quanta_key || !h_quanta || !h_quanta_keys || !scans || !nbytes) return JPEG_AMD_EINVAL;
    const int nc = frame->ncomponents;
    if (nc < 1 || nc > JPEG_AMD_MAX_PLANES || frame->precision < 1 || frame->precision > 16) return JPEG_AMD_ENOSUP;
    jpeg_amd_layout L;
    JA_TRY(layout_of_frame(frame, quanta_key, h_quanta_keys, ntables, &L));
    HostPlanes out(L);
    JA_TRY(jpeg_amd_host_rectangular_spectral(ctx, &L, h_rect, h_quanta, ntables, out.coef));
    return jpeg_amd_jpeg_encode_spectral(frame, quanta_key, out.coef, h_quanta, h_quanta_keys, ntables, scans, nscans,
                                         metadata, nmetadata, h_out, capacity, nbytes);
}
JA_NOTHROW_TAIL

// ---- many pictures of one geometry -> JPEG files: one fused encode launch per chunk, the host
//      threads entropy-code the planes of a chunk as soon as they are back ------------------------
namespace {

// One call of jpeg_amd_compress_batch[_device] behind its checks: what is constant for the call (set by
// compress_batch_impl), and the parts of the pipeline.
struct BatchEncode {
    jpeg_amd_ctx *ctx;
    jpeg_amd_frame_info *frame;
    const uint8_t *h_pixels, *d_pixels_in;     // in host memory, or already on the device
    size_t pixel_stride;
    int n_images;
    jpeg_amd_color color;
    const int32_t *quanta_key;
    const uint16_t *h_quanta;
    const int32_t *h_quanta_keys;
    int ntables;
    const jpeg_amd_scan *scans;
    int nscans;
    const jpeg_amd_metadata *metadata;
    int nmetadata, nthreads;
    uint8_t *h_out;
    size_t out_stride, *nbytes;
    int nc;
    size_t npx, plane[JPEG_AMD_MAX_PLANES] = {};
    jpeg_amd_layout L;
    int chunk, nchunks;
    const uint16_t *d_q;
    SparseBudget sb;
    bool sparse_down, on_device, direct_in;
    SlotLayout at;
    Pieces staging{1, 1};                      // pixels are staged in pieces of <= 4 MiB
    WorkerPool *pool;
    // jpeg_amd_compress_tensor_batch_device: the pictures are tensors on the device (include/jpeg_amd.h, "tensor sources"),
    // image i at d_tensor + i * tensor_stride elements of elem_bytes; source == nullptr: they are pixels
    const void *d_tensor = nullptr;
    size_t tensor_stride = 0, elem_bytes = 1;
    const jpeg_amd_tensor_source *source = nullptr;

    int images(int k) const { return std::min(chunk, n_images - k * chunk); }
    int submit(int k);
    int fetch(int k);
    int host_region(int code, int stage, int fetch_chunk);
    int run();
};

// The device side of chunk k, asynchronous: pixels up and kernels on the context's stream; on the second stream, behind
// them, the first stage of the download -- the entry counts (or, for a progressive frame, the planes).  Device slot and
// pinned slot k & 1 were last used by chunk k - 2, whose download was waited for before its files were written.
int BatchEncode::submit(int k)
{
    const int slot = k & 1, m = images(k);
    char *host = static_cast<char *>(ctx->file_pinned[slot]);
    char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * at.slot_bytes;
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) d_coef[c] = reinterpret_cast<int16_t *>(dev + at.coef_off[c]);
    const uint8_t *d_px = reinterpret_cast<const uint8_t *>(dev);
    size_t d_px_stride = npx;
    // tensors: the front launch writes the chunk's bytes into the slot's pixel area, where uploaded pixels would lie
    if (source)
        JA_HIP(ctx, launch_tensor_pixels(ctx->stream, m, static_cast<const char *>(d_tensor) + (size_t)k * chunk * tensor_stride * elem_bytes,
                                         tensor_stride, L.width, L.height, *source, reinterpret_cast<uint8_t *>(dev), npx));
    else if (on_device) { d_px = d_pixels_in + (size_t)k * chunk * pixel_stride; d_px_stride = pixel_stride; }   // encoded where they are
    // from the pinned slot, or from the caller's page-locked buffer where they are
    else if (!direct_in) JA_HIP(ctx, copy_images(ctx->stream, hipMemcpyHostToDevice, dev, npx, host, npx, npx, m));
    else JA_HIP(ctx, copy_images(ctx->stream, hipMemcpyHostToDevice, dev, npx, h_pixels + (size_t)k * chunk * pixel_stride, pixel_stride, npx, m));
    JA_TRY(jpeg_amd_encode_batch(ctx, &L, m, d_px, d_px_stride, color, d_q, 0, ntables, d_coef, plane));
    if (sparse_down) {
        PlaneSet cs{};
        for (int c = 0; c < nc; ++c) { cs.ptr[c] = d_coef[c]; cs.stride[c] = plane[c]; }
        uint32_t *sp = reinterpret_cast<uint32_t *>(dev + at.sparse_off);
        JA_HIP(ctx, launch_sparsify(ctx->stream, m, L, cs, sp, sb.elems, sp + sb.blocks, sb.elems, (uint32_t)sb.arena,
                                    reinterpret_cast<uint32_t *>(dev + at.count_off)));
    }
    JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
    JA_HIP(ctx, hipStreamWaitEvent(ctx->file_d2h, ctx->file_decoded[slot], 0));
    if (sparse_down) JA_HIP(ctx, hipMemcpyAsync(host + at.count_off, dev + at.count_off, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->file_d2h));
    else
        for (int c = 0; c < nc; ++c)
            JA_HIP(ctx, hipMemcpyAsync(host + at.coef_off[c], dev + at.coef_off[c], plane[c] * 2 * m, hipMemcpyDeviceToHost, ctx->file_d2h));
    JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->file_d2h));
    return JPEG_AMD_OK;
}

// The second stage of chunk k's download, once its counts are in: per picture the descriptors and the entries in use --
// or its planes, where the entries did not fit.  Issued BEFORE chunk k + 1 is submitted, so that it does not queue up
// behind that chunk's kernels on the download stream.
int BatchEncode::fetch(int k)
{
    const int slot = k & 1, m = images(k);
    char *host = static_cast<char *>(ctx->file_pinned[slot]);
    char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * at.slot_bytes;
    if (sparse_down) {
        JA_HIP(ctx, wait_event(ctx->file_done[slot]));
        const uint32_t *count = reinterpret_cast<const uint32_t *>(host + at.count_off);
        for (int i = 0; i < m; ++i) {
            if (count[i] <= sb.arena) {
                const size_t where = at.sparse_off + sb.elems * 4 * (size_t)i;
                JA_HIP(ctx, hipMemcpyAsync(host + where, dev + where, (sb.blocks + count[i]) * 4, hipMemcpyDeviceToHost, ctx->file_d2h));
            } else {
                for (int c = 0; c < nc; ++c)
                    JA_HIP(ctx, hipMemcpyAsync(host + at.coef_off[c] + plane[c] * 2 * i, dev + at.coef_off[c] + plane[c] * 2 * i, plane[c] * 2,
                                               hipMemcpyDeviceToHost, ctx->file_d2h));
            }
        }
    }
    JA_HIP(ctx, hipEventRecord(ctx->file_fetched[slot], ctx->file_d2h));
    return JPEG_AMD_OK;
}

// One parallel region of the host threads: the files of chunk `code` are written from what came down into its pinned slot
// (code >= 0) and the pixels of chunk `stage` are copied into its pinned slot (stage < nchunks).  The caller's pixels
// are pageable memory: copying them to pinned memory on all threads and uploading from there is what keeps the upload
// asynchronous and at the speed of the link.
int BatchEncode::host_region(int code, int stage, int fetch_chunk)
{
    int m_code = 0, m_stage = 0;
    const char *down = nullptr;
    char *stage_host = nullptr;
    if (code >= 0) {
        m_code = images(code);
        JA_HIP(ctx, wait_event(ctx->file_fetched[code & 1]));
        down = static_cast<const char *>(ctx->file_pinned[code & 1]);
    }
    if (stage < nchunks && !direct_in) {
        m_stage = images(stage);
        stage_host = static_cast<char *>(ctx->file_pinned[stage & 1]);   // (its last upload, chunk stage - 2, is long complete)
    }
    std::vector<int> status((size_t)std::max(m_code, 1), JPEG_AMD_OK);
    pool->begin(m_code + staging.count(m_stage), [&](int j) {
        if (j < m_code) {
            const size_t image = (size_t)code * chunk + (size_t)j;
            const uint32_t count = sparse_down ? reinterpret_cast<const uint32_t *>(down + at.count_off)[j] : 0;
            if (sparse_down && count <= sb.arena) {
                const uint32_t *sp = reinterpret_cast<const uint32_t *>(down + at.sparse_off) + sb.elems * (size_t)j;
                status[(size_t)j] = jpeg_amd_jpeg_encode_sparse(frame, quanta_key, sp, sp + sb.blocks, count, h_quanta, h_quanta_keys, ntables, scans,
                                                                nscans, metadata, nmetadata, h_out + image * out_stride, out_stride, &nbytes[image]);
            } else {
                const int16_t *planes[JPEG_AMD_MAX_PLANES] = {};
                for (int c = 0; c < nc; ++c) planes[c] = reinterpret_cast<const int16_t *>(down + at.coef_off[c]) + plane[c] * j;
                status[(size_t)j] = jpeg_amd_jpeg_encode_spectral(frame, quanta_key, planes, h_quanta, h_quanta_keys, ntables, scans, nscans,
                                                                  metadata, nmetadata, h_out + image * out_stride, out_stride, &nbytes[image]);
            }
        } else {
            const Pieces::At p = staging.at((size_t)(j - m_code));
            std::memcpy(stage_host + npx * p.i + p.lo, h_pixels + ((size_t)stage * chunk + p.i) * pixel_stride + p.lo, p.len);
        }
    }, nthreads);
    // while the other threads are at it, this one waits for the kernels of the chunk on the device and starts the second
    // stage of its download, which then runs beside the rest of the region
    const int fetched_status = fetch_chunk >= 0 ? fetch(fetch_chunk) : JPEG_AMD_OK;
    pool->finish();
    if (fetched_status != JPEG_AMD_OK) return fetched_status;
    for (int st : status) if (st != JPEG_AMD_OK) return st;   // EINVAL with nbytes[i] > out_stride: buffer too small
    return JPEG_AMD_OK;
}

int BatchEncode::run()
{
    struct Finish { WorkerPool &p; ~Finish() { p.finish(); } } finish_on_exit{*pool};
    int result = host_region(-1, 0, -1);
    if (result == JPEG_AMD_OK) result = submit(0);
    for (int k = 0; k < nchunks && result == JPEG_AMD_OK; ++k) {
        result = host_region(k - 1, k + 1, k);                    // ... while the device works on chunk k
        if (result == JPEG_AMD_OK && k + 1 < nchunks) result = submit(k + 1);
    }
    if (result == JPEG_AMD_OK) result = host_region(nchunks - 1, nchunks, -1);
    return after_both_streams(ctx, result);
}

// Pixels -> files; the pixels in host memory (h_pixels) or already on the device (d_pixels_in): jpeg_amd_compress_batch[_device];
// or tensors on the device (d_tensor, tensor_stride in elements, source): jpeg_amd_compress_tensor_batch_device.
int compress_batch_impl(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels, const uint8_t *d_pixels_in,
                        size_t pixel_stride, const void *d_tensor, size_t tensor_stride, const jpeg_amd_tensor_source *source,
                        int n_images, jpeg_amd_color color,
                        const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys,
                        int ntables, const jpeg_amd_scan *scans, int nscans,
                        const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                        uint8_t *h_out, size_t out_stride, size_t nbytes[])
{
    JA_TRY(bind(ctx));
    const bool on_device = d_pixels_in != nullptr || d_tensor != nullptr;
    if (!frame || (!h_pixels && !on_device) || !quanta_key || !h_quanta || !h_quanta_keys || !scans || !h_out || !nbytes || n_images < 0)
        return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    const int nc = frame->ncomponents;
    if (!jpeg_common(frame->precision, nc)) return JPEG_AMD_ENOSUP;
    const size_t npx = (size_t)frame->width * frame->height * 3;
    if (pixel_stride == 0) pixel_stride = npx;
    if (pixel_stride < npx) return JPEG_AMD_EINVAL;
    BatchEncode e{ctx, frame, h_pixels, d_pixels_in, pixel_stride, n_images, color, quanta_key, h_quanta, h_quanta_keys, ntables, scans, nscans,
                  metadata, nmetadata, nthreads, h_out, out_stride, nbytes, nc, npx};
    JA_TRY(layout_of_frame(frame, quanta_key, h_quanta_keys, ntables, &e.L));
    for (int c = 0; c < nc; ++c) e.plane[c] = plane_samples(&e.L, c);
    if (d_tensor) {   // behind everything the pixel call refuses
        if (tensor_stride == 0) tensor_stride = npx;
        JA_TRY(check_tensor_source(n_images, d_tensor, tensor_stride, frame->width, frame->height, source, &e.elem_bytes));
        e.d_tensor = d_tensor; e.tensor_stride = tensor_stride; e.source = source;
    }
    e.chunk = std::min(n_images, 32);
    e.nthreads = host_threads(e.nthreads, nullptr);

    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &e.d_q));
    // Sequential scans: the coefficients come down as SPARSE entries (k_sparsify: a descriptor per block + an entry per
    // nonzero coefficient, an eighth of the planes for a typical picture) and go to the writer in that form
    // (jpeg_amd_jpeg_encode_sparse); a picture whose entries do not fit its arena comes down as planes, like every picture of a
    // progressive frame, or of a frame too large for 32-bit descriptors (sparse_budget).
    e.sb = sparse_budget(e.L);
    // (... or of 2^26 blocks or more: k_sparsify's uint32 cursor could wrap, and the host would read a small count)
    e.sparse_down = frame->process != 2 && e.sb.ok && sparsify_count_fits(e.sb.blocks);
    // slot layout (pinned and device alike): [pixels x chunk][coef plane 0 x chunk][plane 1 x chunk][plane 2 x chunk][sparse x chunk][counts]
    e.at.px_off = e.at.take(npx * e.chunk);
    for (int c = 0; c < nc; ++c) e.at.coef_off[c] = e.at.take(e.plane[c] * 2 * e.chunk);
    e.at.sparse_off = e.at.take(e.sparse_down ? e.sb.elems * 4 * e.chunk : 0);
    e.at.count_off = e.at.take((size_t)e.chunk * 4);
    JA_TRY(ensure_file_staging(ctx, e.at.slot_bytes, e.at.slot_bytes));

    e.nchunks = (n_images + e.chunk - 1) / e.chunk;
    // a caller whose pixels are page-locked gets them uploaded from where they are: nothing to stage
    e.on_device = on_device;
    e.direct_in = on_device || is_pinned_host(h_pixels, (size_t)(n_images - 1) * pixel_stride + npx);
    e.staging = Pieces(npx, (size_t)4 << 20);
    e.pool = &pool_with(ctx->workers, std::min(e.nthreads, 2 * e.chunk));   // (kept in the context between calls)
    return e.run();
}

}  // namespace

int jpeg_amd_compress_batch(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels,
                            size_t pixel_stride, int n_images, jpeg_amd_color color,
                            const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys,
                            int ntables, const jpeg_amd_scan *scans, int nscans,
                            const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                            uint8_t *h_out, size_t out_stride, size_t nbytes[])
try {
    if (!h_pixels) return JPEG_AMD_EINVAL;
    return compress_batch_impl(ctx, frame, h_pixels, nullptr, pixel_stride, nullptr, 0, nullptr, n_images, color, quanta_key, h_quanta, h_quanta_keys, ntables,
                               scans, nscans, metadata, nmetadata, nthreads, h_out, out_stride, nbytes);
}
JA_NOTHROW_TAIL

int jpeg_amd_compress_batch_device(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *d_pixels,
                                   size_t pixel_stride, int n_images, jpeg_amd_color color,
                                   const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys,
                                   int ntables, const jpeg_amd_scan *scans, int nscans,
                                   const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                                   uint8_t *h_out, size_t out_stride, size_t nbytes[])
try {
    if (!d_pixels) return JPEG_AMD_EINVAL;
    return compress_batch_impl(ctx, frame, nullptr, d_pixels, pixel_stride, nullptr, 0, nullptr, n_images, color, quanta_key, h_quanta, h_quanta_keys, ntables,
                               scans, nscans, metadata, nmetadata, nthreads, h_out, out_stride, nbytes);
}
JA_NOTHROW_TAIL

int jpeg_amd_compress_tensor_batch_device(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const void *d_src, size_t src_stride,
                                          const jpeg_amd_tensor_source *src, int n_images, jpeg_amd_color color,
                                          const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys,
                                          int ntables, const jpeg_amd_scan *scans, int nscans,
                                          const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                                          uint8_t *h_out, size_t out_stride, size_t nbytes[])
try {
    if (!d_src) return JPEG_AMD_EINVAL;
    // bytes in the encoder's own order are the pixel call: no launch
    if (src && src->dtype == JPEG_AMD_U8 && src->layout == JPEG_AMD_TENSOR_HWC)
        return compress_batch_impl(ctx, frame, nullptr, static_cast<const uint8_t *>(d_src), src_stride, nullptr, 0, nullptr, n_images, color,
                                   quanta_key, h_quanta, h_quanta_keys, ntables, scans, nscans, metadata, nmetadata, nthreads, h_out,
                                   out_stride, nbytes);
    return compress_batch_impl(ctx, frame, nullptr, nullptr, 0, d_src, src_stride, src, n_images, color, quanta_key, h_quanta, h_quanta_keys,
                               ntables, scans, nscans, metadata, nmetadata, nthreads, h_out, out_stride, nbytes);
}
JA_NOTHROW_TAIL

// ---- file to file in the coefficient domain: what jpeg_amd_transform and jpeg_amd_reduce share ---------------------------
namespace {

// Host entropy decoding, one device step on the planes, the host writer with the input's script (scans, table keys, restart
// interval, metadata segments).  plan(L, &O): the output layout; device(L, d_in, quanta, nc, d_out): the step, synchronised on
// return; table(c, quanta[c], t): the output table of component c when h_requant is NULL.
template <typename Plan, typename Device, typename Table>
int file_to_file(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, const uint16_t *h_requant, int nthreads, Plan plan,
                 Device device, Table table, uint8_t *h_out, size_t capacity, size_t *nbytes_out, jpeg_amd_frame_info *out_info)
{
    jpeg_amd_frame_info fi;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg, nbytes, &fi));
    const int nc = fi.ncomponents;
    if (nc < 1 || nc > JPEG_AMD_MAX_PLANES) return JPEG_AMD_ENOSUP;
    // the script: scans, table keys, metadata segments (pointing into h_jpeg)
    int nscans = 0, nmeta = 0;
    int32_t keys[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(jpeg_amd_jpeg_script(h_jpeg, nbytes, nullptr, 0, &nscans, keys, nullptr, 0, &nmeta));
    std::vector<jpeg_amd_scan> scans((size_t)std::max(nscans, 1));
    std::vector<jpeg_amd_metadata> meta((size_t)std::max(nmeta, 1));
    JA_TRY(jpeg_amd_jpeg_script(h_jpeg, nbytes, scans.data(), nscans, &nscans, keys, meta.data(), nmeta, &nmeta));
    // entropy decoding on the host
    HostPlanes in(layout_of_info(fi, nc));
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64];
    JA_TRY(jpeg_amd_jpeg_decode_spectral_mt(h_jpeg, nbytes, in.coef, quanta, &fi, nthreads));
    const jpeg_amd_layout L = layout_of_info(fi, nc);
    jpeg_amd_layout O;
    JA_TRY(plan(L, &O));
    // components that share a key share a table, in the file and after requantisation
    if (h_requant)
        for (int c = 0; c < nc; ++c)
            for (int d = 0; d < c; ++d)
                if (keys[c] == keys[d] && std::memcmp(h_requant + 64 * c, h_requant + 64 * d, 64 * sizeof(uint16_t)))
                    return JPEG_AMD_EINVAL;
    // the device: upload, the step, download
    HostPlanes out(O);
    {
        DeviceBag bag(ctx);
        const int16_t *d_in[JPEG_AMD_MAX_PLANES] = {};
        int16_t *d_out[JPEG_AMD_MAX_PLANES] = {};
        JA_TRY(bag.upload_planes<int16_t>(&L, in.coef, d_in));
        JA_TRY(bag.alloc_planes(&O, d_out));
        JA_TRY(device(L, d_in, &quanta[0][0], nc, d_out));
        JA_TRY(bag.download_planes(&O, out.coef, d_out));
        JA_TRY(bag.finish());
    }
    // one table per distinct key, ascending
    std::vector<int32_t> tkeys;
    std::vector<uint16_t> tables;
    for (int c = 0; c < nc; ++c)
        if (std::find(tkeys.begin(), tkeys.end(), keys[c]) == tkeys.end()) tkeys.push_back(keys[c]);
    std::sort(tkeys.begin(), tkeys.end());
    for (int32_t k : tkeys) {
        const int c = (int)(std::find(keys, keys + nc, k) - keys);
        uint16_t t[64];
        if (h_requant) std::memcpy(t, h_requant + 64 * c, sizeof t);
        else JA_TRY(table(c, quanta[c], t));
        tables.insert(tables.end(), t, t + 64);
    }
    jpeg_amd_frame_info of = fi;
    of.width = O.width; of.height = O.height;
    of.scale_x = O.scale_x; of.scale_y = O.scale_y;
    for (int c = 0; c < nc; ++c) {
        of.factor_x[c] = O.factor_x[c]; of.factor_y[c] = O.factor_y[c];
        of.units_x[c] = O.units_x[c];   of.units_y[c] = O.units_y[c];
    }
    if (out_info) *out_info = of;
    return jpeg_amd_jpeg_encode_spectral(&of, keys, out.coef, tables.data(), tkeys.data(), (int)tkeys.size(), scans.data(), nscans,
                                         meta.data(), nmeta, h_out, capacity, nbytes_out);
}

}  // namespace

// File to file: host entropy decoding, the transform on the device, the host writer with the input's script; the tables in
// output orientation.
int jpeg_amd_transform(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int op, const jpeg_amd_region *region,
                       const uint16_t *h_requant, int nthreads, uint8_t *h_out, size_t capacity, size_t *nbytes_out,
                       jpeg_amd_frame_info *out_info)
try {
    JA_TRY(bind(ctx));
    if (!h_jpeg || !nbytes_out || op < 0 || op > 7) return JPEG_AMD_EINVAL;
    return file_to_file(
        ctx, h_jpeg, nbytes, h_requant, nthreads,
        [&](const jpeg_amd_layout &L, jpeg_amd_layout *O) { return jpeg_amd_transform_layout(&L, op, region, O); },
        [&](const jpeg_amd_layout &L, const int16_t *const d_in[], const uint16_t *quanta, int nc, int16_t *const d_out[]) {
            return jpeg_amd_spectral_transform(ctx, &L, op, region, d_in, quanta, nc, h_requant, d_out);
        },
        [&](int, const uint16_t *q, uint16_t *t) { return jpeg_amd_transform_quanta(op, q, t); },
        h_out, capacity, nbytes_out, out_info);
}
JA_NOTHROW_TAIL

// File to file: host entropy decoding, one reduce launch on the device, the host writer with the input's script.
int jpeg_amd_reduce(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int denom, const uint16_t *h_requant,
                    int nthreads, uint8_t *h_out, size_t capacity, size_t *nbytes_out, jpeg_amd_frame_info *out_info)
try {
    JA_TRY(bind(ctx));
    if (!h_jpeg || !nbytes_out || reduce_n(denom) == 0) return JPEG_AMD_EINVAL;
    return file_to_file(
        ctx, h_jpeg, nbytes, h_requant, nthreads,
        [&](const jpeg_amd_layout &L, jpeg_amd_layout *O) { return jpeg_amd_reduce_layout(&L, denom, O); },
        [&](const jpeg_amd_layout &L, const int16_t *const d_in[], const uint16_t *quanta, int nc, int16_t *const d_out[]) {
            return jpeg_amd_spectral_reduce(ctx, &L, denom, d_in, quanta, nc, h_requant, d_out);
        },
        [&](int, const uint16_t *q, uint16_t *t) { std::memcpy(t, q, 64 * sizeof(uint16_t)); return (int)JPEG_AMD_OK; },
        h_out, capacity, nbytes_out, out_info);
}
JA_NOTHROW_TAIL
