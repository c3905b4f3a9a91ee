// capi.hip -- the C ABI declared in include/jpeg_amd.h: argument validation, context /
// stream / scratch management, table staging and the host-buffer conveniences.
// No arithmetic on samples happens here; all of it is in kernels_*.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <atomic>
#include <memory>
#include <chrono>
#include <system_error>
#include <thread>
#include <vector>

#include "interleave.hpp"
#include "kernels.hpp"
#include "transform.hpp"
#include "worker_pool.hpp"

using namespace jpeg_amd;

// Device memory a context keeps between calls and grows on demand (ensure_buffer).
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
};

struct jpeg_amd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    DeviceBuffer scratch;          // the planes of the staged paths, the whole images of the fallbacks
    uint16_t *d_qstage = nullptr;  // ring of staged host tables
    uint32_t *d_walk = nullptr;    // the ticket counter of the 4:2:0 walk of long calls (kernels_quad.hip)
    int32_t *d_flag = nullptr;     // the overflow dword of jpeg_amd_spectral_transform (allocated on first use)
    DeviceBuffer region;           // staged regions + tile prefix of jpeg_amd_decode_region_batch / _view_batch
    // jpeg_amd_decode_resized_batch / jpeg_amd_resize_batch: the decoded views of a chunk and the resample's per-image records.
    // Buffers of their own: the view call in between regrows `scratch` and overwrites `region`.
    DeviceBuffer resize_src, resize_rec;
    // the mixed calls (jpeg_amd_decode_view_mixed, ...): the per-image records, index lists and tile prefixes of their launches.
    // A buffer of its own: the uniform calls of a mixed call's fallback images rewrite `region`, the resample rewrites the others.
    DeviceBuffer mixed;
    int qslot = 0;
    int last_hip = 0;
    // staging of the batch file paths (jpeg_amd_decompress_batch, jpeg_amd_compress_batch), kept between calls: two pinned
    // host slots (the host threads work in one while the device works from / into the other) and two device slots
    void *file_pinned[2] = {nullptr, nullptr};
    void *file_device = nullptr;                      // both device slots
    size_t file_pinned_bytes = 0, file_device_bytes = 0;
    hipEvent_t file_done[2] = {nullptr, nullptr};     // chunk's pixels (decode) / first stage of its download (encode) are back
    hipEvent_t file_decoded[2] = {nullptr, nullptr};  // chunk's kernels are done (device -> host copy may start)
    hipEvent_t file_fetched[2] = {nullptr, nullptr};  // encode: the second stage of the chunk's download is back
    hipStream_t file_d2h = nullptr;                   // downloads overlap the next chunk's uploads (full-duplex PCIe)
    std::unique_ptr<WorkerPool> workers, copiers;     // host threads of the batch file paths: entropy coding; copies out of the pinned slots
    std::vector<std::vector<uint32_t>> records;       // a sparse record per entropy-decoding thread
};

namespace {

constexpr int kQSlots = 32;                                   // staged table sets in flight
constexpr size_t kQSlotElems = JPEG_AMD_MAX_PLANES * 64;      // uint16 per slot

#define JA_HIP(ctx, expr)                                         \
    do {                                                          \
        const hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) {                                   \
            (ctx)->last_hip = (int)e_;                            \
            return e_ == hipErrorOutOfMemory ? JPEG_AMD_ENOMEM : JPEG_AMD_EHIP; \
        }                                                         \
    } while (0)

// Function-try-block tail of the entry points that allocate host memory or start threads: the header promises plain
// C, so no C++ exception (std::bad_alloc, std::system_error from a thread that cannot be started) leaves the library.
#define JA_NOTHROW_TAIL                                               \
    catch (const std::bad_alloc &) { return JPEG_AMD_ENOMEM; }        \
    catch (...) { return JPEG_AMD_ENOMEM; }

#define JA_TRY(expr)                          \
    do {                                      \
        const int s_ = (expr);                \
        if (s_ != JPEG_AMD_OK) return s_;     \
    } while (0)

int bind(jpeg_amd_ctx *ctx)
{
    if (!ctx) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipSetDevice(ctx->device));
    return JPEG_AMD_OK;
}

int units_of(int size, int stride) { return size / stride + (size % stride != 0 ? 1 : 0); }

// The preconditions the reference traps on (decode.swift:1710-1712, 2227, 2599) plus the
// bounds this ABI needs.
int check_layout(const jpeg_amd_layout *L, int ntables)
{
    if (!L) return JPEG_AMD_EINVAL;
    if (L->width <= 0 || L->height <= 0) return JPEG_AMD_EINVAL;
    if (L->precision < 1 || L->precision > 16) return JPEG_AMD_EINVAL;
    if (L->nplanes < 1 || L->nplanes > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (L->scale_x < 1 || L->scale_y < 1) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p) {
        if (L->factor_x[p] < 1 || L->factor_y[p] < 1) return JPEG_AMD_EINVAL;
        if (L->factor_x[p] > L->scale_x || L->factor_y[p] > L->scale_y) return JPEG_AMD_EINVAL;
        if (L->units_x[p] < 0 || L->units_y[p] < 0) return JPEG_AMD_EINVAL;
        if ((long long)L->units_x[p] * L->units_y[p] > (1LL << 30)) return JPEG_AMD_EINVAL;
        if (ntables >= 0 && (L->qi[p] < 0 || L->qi[p] >= ntables)) return JPEG_AMD_EINVAL;
    }
    return JPEG_AMD_OK;
}

// Planar.interleaved reads plane samples up to the image size (crop copy) or up to the
// padded plane (bilinear): the planes must cover the image (decode.swift:4190-4215).
int check_planes_cover_image(const jpeg_amd_layout *L)
{
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_is_direct(*L, p)) {
            if (8 * L->units_x[p] < L->width || 8 * L->units_y[p] < L->height) return JPEG_AMD_EINVAL;
        } else {
            // bilinear: the sample index of the last pixel (decode.swift:4223-4246; its neighbour i + 1 is clamped to the
            // plane, i itself is not) must lie inside the plane.  The cosited form is the larger of the two.
            if (L->units_x[p] < 1 || L->units_y[p] < 1) return JPEG_AMD_EINVAL;
            const long long ix = axis_index(interleave_axis(*L, p, true, false), L->width - 1);
            const long long iy = axis_index(interleave_axis(*L, p, true, true), L->height - 1);
            if (ix >= 8LL * L->units_x[p] || iy >= 8LL * L->units_y[p]) return JPEG_AMD_EINVAL;
        }
    }
    return JPEG_AMD_OK;
}

size_t plane_samples(const jpeg_amd_layout *L, int p)
{
    return (size_t)64 * L->units_x[p] * L->units_y[p];
}

// One of the context's buffers with room for `bytes`, grown with an eighth to spare.  The one place that frees such a
// buffer between calls: the previous call's kernels may still use it, so the stream is synchronised first.
// (C linkage, as the helpers inside the extern "C" block have: the library's dynamic symbol list keeps the name.)
extern "C" int ensure_buffer(jpeg_amd_ctx *ctx, DeviceBuffer &buf, size_t bytes)
{
    if (bytes <= buf.bytes) return JPEG_AMD_OK;
    if (buf.ptr) {
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        JA_HIP(ctx, hipFree(buf.ptr));
        buf = DeviceBuffer{};
    }
    const size_t want = bytes + bytes / 8 + 4096;
    JA_HIP(ctx, hipMalloc(&buf.ptr, want));
    buf.bytes = want;
    return JPEG_AMD_OK;
}

// Copy host tables [ntables][64] into the next ring slot; returns the device pointer.
int stage_quanta(jpeg_amd_ctx *ctx, const uint16_t *h_quanta, int ntables, const uint16_t **d_out)
{
    if (!h_quanta || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    uint16_t *slot = ctx->d_qstage + (size_t)ctx->qslot * kQSlotElems;
    ctx->qslot = (ctx->qslot + 1) % kQSlots;
    JA_HIP(ctx, hipMemcpyAsync(slot, h_quanta, (size_t)ntables * 64 * sizeof(uint16_t),
                               hipMemcpyHostToDevice, ctx->stream));
    *d_out = slot;
    return JPEG_AMD_OK;
}

// The single-image forms are their batch forms with one image, staged tables and these strides.
constexpr size_t kOneImage[JPEG_AMD_MAX_PLANES] = {0, 0, 0, 0};

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Bytes of scratch_planes's planes: they take [0, this) of the scratch.
size_t scratch_planes_bytes(const jpeg_amd_layout *L, int n_images, size_t sample_bytes)
{
    size_t total = 0;
    for (int p = 0; p < L->nplanes; ++p) total += align256(plane_samples(L, p) * (size_t)n_images * sample_bytes);
    return total;
}

// The planes of the staged paths in the context's scratch: n_images images of every plane, `sample_bytes` per sample.
int scratch_planes(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, size_t sample_bytes, PlaneSetMut *ps)
{
    size_t offset[JPEG_AMD_MAX_PLANES], total = 0;
    for (int p = 0; p < L->nplanes; ++p) {
        offset[p] = total;
        total += align256(plane_samples(L, p) * (size_t)n_images * sample_bytes);
    }
    JA_TRY(ensure_buffer(ctx, ctx->scratch, total));
    *ps = PlaneSetMut{};
    for (int p = 0; p < L->nplanes; ++p) {
        ps->ptr[p] = static_cast<uint8_t *>(ctx->scratch.ptr) + offset[p];
        ps->stride[p] = plane_samples(L, p);
    }
    return JPEG_AMD_OK;
}

// The ABI's per-plane pointer (and stride: nullptr = one image) arrays as a PlaneSet / PlaneSetMut.  Decode inputs
// (need_all) reject any null plane pointer, encode outputs only where the plane has samples.
template <typename Set, typename T>
int plane_set(const jpeg_amd_layout *L, T *const d_planes[], const size_t stride[], bool need_all, Set *ps)
{
    *ps = Set{};
    for (int p = 0; p < L->nplanes; ++p) {
        if (!d_planes[p] && (need_all || plane_samples(L, p))) return JPEG_AMD_EINVAL;
        ps->ptr[p] = d_planes[p];
        ps->stride[p] = stride ? stride[p] : 0;
    }
    return JPEG_AMD_OK;
}

// What the batch entry points of the built-in 8-bit colour formats require, in the order that decides the status of a
// call that is wrong twice (EINVAL against ENOSUP).
int check_batch8(const jpeg_amd_layout *L, int n_images, jpeg_amd_color color)
{
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (L->nplanes != 1 && L->nplanes != 3) return JPEG_AMD_EINVAL;   // built-in colour formats
    if (L->precision != 8) return JPEG_AMD_ENOSUP;                   // JPEG.Common is 8-bit
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// The arguments the batch decode entry points (whole, region, scaled, view, resized) share, as the caller gave them.
struct DecodeCall {
    const jpeg_amd_layout *L;
    int n_images;
    const int16_t *const *d_coef;
    const size_t *coef_stride;
    const uint16_t *d_quanta;
    size_t quanta_stride;
    int ntables, cosited;
    jpeg_amd_color color;
    uint8_t *d_pixels;
    size_t pixel_stride;

    // What is judged before the image count may end the call, in the order that decides the status of a call that is wrong
    // twice.  The context is no part of it: every entry point binds where it always did.
    int check() const
    {
        JA_TRY(check_layout(L, ntables));
        JA_TRY(check_planes_cover_image(L));
        return check_batch8(L, n_images, color);
    }
    // ... and of a call with images: no null pointer (per_image: the entry point's regions or views are there, where it
    // has any) and the coefficient planes as a PlaneSet.
    int planes(PlaneSet *cs, bool per_image = true) const
    {
        if (!d_coef || !coef_stride || !d_quanta || !d_pixels || !per_image) return JPEG_AMD_EINVAL;
        return plane_set(L, d_coef, coef_stride, true, cs);
    }
    // Images [i0, i0 + m) of this call; `coef` is the caller's room for their plane pointers.
    DecodeCall images(int i0, int m, const int16_t *coef[JPEG_AMD_MAX_PLANES]) const
    {
        for (int p = 0; p < L->nplanes; ++p) coef[p] = d_coef[p] + (size_t)i0 * coef_stride[p];
        return DecodeCall{L, m, coef, coef_stride, d_quanta + (size_t)i0 * quanta_stride, quanta_stride, ntables, cosited, color,
                          d_pixels + (size_t)i0 * pixel_stride, pixel_stride};
    }
    QuantaRef quanta() const { return QuantaRef{d_quanta, quanta_stride}; }
    bool rgb() const { return color == JPEG_AMD_COLOR_RGB8; }
};

// The staged decode (any factors): IDCT every plane into scratch planes of bytes or halfwords, then upsample + interleave
// (+ colour) into `kind` pixels.
int staged_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const PlaneSet &coef, QuantaRef q, bool cosited,
                  bool planes_u8, PixelKind kind, void *d_out, size_t out_stride_bytes)
{
    PlaneSetMut scratch;
    JA_TRY(scratch_planes(ctx, L, n_images, planes_u8 ? sizeof(uint8_t) : sizeof(uint16_t), &scratch));
    PlaneSet ps{};
    for (int p = 0; p < L->nplanes; ++p) {
        JA_HIP(ctx, launch_idct_plane(ctx->stream, n_images, static_cast<const int16_t *>(coef.ptr[p]), coef.stride[p], q, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, scratch.ptr[p], scratch.stride[p], planes_u8));
        ps.ptr[p] = scratch.ptr[p];
        ps.stride[p] = scratch.stride[p];
    }
    JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, n_images, *L, ps, planes_u8, cosited, kind, d_out, out_stride_bytes));
    return JPEG_AMD_OK;
}

// The staged encode (any factors): decomposed() into uint16 scratch planes, then fdct(quanta:) plane by plane.
int staged_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const void *d_in, size_t in_stride_bytes,
                  PixelKind kind, QuantaRef q, const PlaneSetMut &coef)
{
    PlaneSetMut ps;
    JA_TRY(scratch_planes(ctx, L, n_images, sizeof(uint16_t), &ps));
    JA_HIP(ctx, launch_decompose(ctx->stream, n_images, *L, d_in, in_stride_bytes, kind, ps));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        JA_HIP(ctx, launch_fdct_plane(ctx->stream, n_images, static_cast<const uint16_t *>(ps.ptr[p]), ps.stride[p], q, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, static_cast<int16_t *>(coef.ptr[p]),
                                      coef.stride[p]));
    }
    return JPEG_AMD_OK;
}

// A decoded frame's layout: its first `nplanes` components, table c for component c.
jpeg_amd_layout layout_of_info(const jpeg_amd_frame_info &fi, int nplanes)
{
    jpeg_amd_layout L{};
    L.width = fi.width; L.height = fi.height; L.precision = fi.precision; L.nplanes = nplanes;
    L.scale_x = fi.scale_x; L.scale_y = fi.scale_y;          // the scale of ALL components (decode.swift:2181-2190)
    for (int c = 0; c < nplanes; ++c) {
        L.factor_x[c] = fi.factor_x[c]; L.factor_y[c] = fi.factor_y[c];
        L.units_x[c] = fi.units_x[c];   L.units_y[c] = fi.units_y[c];
        L.qi[c] = c;
    }
    return L;
}

// The layout of a frame to be encoded: scale and units from its factors (both written back into the frame), each
// component's table found by its key.  Precision and component count are the caller's to check.
int layout_of_frame(jpeg_amd_frame_info *frame, const int32_t *quanta_key, const int32_t *h_quanta_keys, int ntables,
                    jpeg_amd_layout *L)
{
    if (frame->width < 1 || frame->height < 1 || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    const int nc = frame->ncomponents;
    *L = jpeg_amd_layout{};
    L->width = frame->width; L->height = frame->height; L->precision = frame->precision; L->nplanes = nc;
    L->scale_x = L->scale_y = 1;
    for (int c = 0; c < nc; ++c) {
        if (frame->factor_x[c] < 1 || frame->factor_y[c] < 1) return JPEG_AMD_EINVAL;
        L->factor_x[c] = frame->factor_x[c]; L->factor_y[c] = frame->factor_y[c];
        L->scale_x = std::max(L->scale_x, L->factor_x[c]); L->scale_y = std::max(L->scale_y, L->factor_y[c]);
        L->qi[c] = -1;
        for (int t = 0; t < ntables; ++t) if (h_quanta_keys[t] == quanta_key[c]) L->qi[c] = t;
        if (L->qi[c] < 0) return JPEG_AMD_EINVAL;   // missing quantization table (decode.swift:2527)
    }
    JA_TRY(jpeg_amd_layout_units(L));
    frame->scale_x = L->scale_x; frame->scale_y = L->scale_y;
    for (int c = 0; c < nc; ++c) { frame->units_x[c] = L->units_x[c]; frame->units_y[c] = L->units_y[c]; }
    return JPEG_AMD_OK;
}

// The sparse form of a frame's coefficients in the batch paths (jpeg_amd_jpeg_decode_sparse, k_sparsify): per image a
// descriptor per block and an arena of 24 entries per block (3/4 of the planes' bytes at most; only what is used travels).
// Descriptors are 32-bit indices into the arena: a frame whose record would not be addressable that way (25 * blocks >= 2^32:
// beyond 60 000 x 60 000 4:4:4) travels as planes (ok = false).
struct SparseBudget {
    size_t blocks, arena, elems;   // elems: uint32 per image, [descriptors][entries]
    bool ok;
};
SparseBudget sparse_budget(const jpeg_amd_layout &L)
{
    size_t blocks = 0;
    for (int c = 0; c < L.nplanes; ++c) blocks += (size_t)L.units_x[c] * L.units_y[c];
    const size_t arena = 24 * blocks;
    return {blocks, arena, blocks + arena, blocks + arena < 0xffffffffull};
}

// The staging the two batch entry points for files share, kept in the context between calls: two pinned host slots (the host
// threads work in one while the device works from / into the other), two device slots, two events per slot and a second
// stream so that uploads and downloads overlap (full-duplex PCIe).
int ensure_file_staging(jpeg_amd_ctx *ctx, size_t slot_bytes)
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
    if (ctx->file_device_bytes < 2 * slot_bytes) {           // two device slots as well
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        JA_HIP(ctx, hipStreamSynchronize(ctx->file_d2h));
        if (ctx->file_device) { (void)hipFree(ctx->file_device); ctx->file_device = nullptr; ctx->file_device_bytes = 0; }
        JA_HIP(ctx, hipMalloc(&ctx->file_device, 2 * slot_bytes));
        ctx->file_device_bytes = 2 * slot_bytes;
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

// the context's pool, with at least `threads` threads (the calling one included)
WorkerPool &pool_with(std::unique_ptr<WorkerPool> &pool, int threads)
{
    if (!pool || pool->size() < threads) pool.reset(new WorkerPool(threads));
    return *pool;
}

}  // namespace

extern "C" {

int jpeg_amd_version(void) { return JPEG_AMD_VERSION; }

const char *jpeg_amd_strerror(int status)
{
    switch (status) {
        case JPEG_AMD_OK: return "ok";
        case JPEG_AMD_EINVAL: return "invalid argument (violated precondition)";
        case JPEG_AMD_ENOMEM: return "out of memory";
        case JPEG_AMD_EHIP: return "HIP runtime error";
        case JPEG_AMD_ENODEV: return "no such device";
        case JPEG_AMD_ENOSUP: return "not supported";
        default: return "unknown status";
    }
}

int jpeg_amd_device_count(int *count)
{
    if (!count) return JPEG_AMD_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return JPEG_AMD_ENODEV; }
    *count = n;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_create(int device, void *stream, int flags, jpeg_amd_ctx **out)
{
    if (!out) return JPEG_AMD_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return JPEG_AMD_ENODEV;
    jpeg_amd_ctx *ctx = new (std::nothrow) jpeg_amd_ctx();
    if (!ctx) return JPEG_AMD_ENOMEM;
    ctx->device = device;
    int status = JPEG_AMD_OK;
    do {
        if (hipSetDevice(device) != hipSuccess) { status = JPEG_AMD_ENODEV; break; }
        if (flags & JPEG_AMD_CTX_OWN_STREAM) {
            if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
            ctx->own_stream = true;
        } else {
            ctx->stream = static_cast<hipStream_t>(stream);  // NULL = the default stream
        }
        if (hipEventCreate(&ctx->ev_begin) != hipSuccess || hipEventCreate(&ctx->ev_end) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_qstage), kQSlots * kQSlotElems * sizeof(uint16_t)) != hipSuccess) { status = JPEG_AMD_ENOMEM; break; }
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_walk), 256) != hipSuccess) { status = JPEG_AMD_ENOMEM; break; }
        if (hipMemset(ctx->d_walk, 0, 256) != hipSuccess) { status = JPEG_AMD_EHIP; break; }
    } while (0);
    if (status != JPEG_AMD_OK) {
        jpeg_amd_ctx_destroy(ctx);
        return status;
    }
    *out = ctx;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_destroy(jpeg_amd_ctx *ctx)
{
    if (!ctx) return JPEG_AMD_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->workers.reset();
    ctx->copiers.reset();
    for (DeviceBuffer *buf : {&ctx->scratch, &ctx->region, &ctx->resize_src, &ctx->resize_rec, &ctx->mixed})
        if (buf->ptr) (void)hipFree(buf->ptr);
    if (ctx->d_qstage) (void)hipFree(ctx->d_qstage);
    if (ctx->d_walk) (void)hipFree(ctx->d_walk);
    if (ctx->d_flag) (void)hipFree(ctx->d_flag);
    for (int i = 0; i < 2; ++i) {
        if (ctx->file_pinned[i]) (void)hipHostFree(ctx->file_pinned[i]);
        if (ctx->file_done[i]) (void)hipEventDestroy(ctx->file_done[i]);
        if (ctx->file_decoded[i]) (void)hipEventDestroy(ctx->file_decoded[i]);
        if (ctx->file_fetched[i]) (void)hipEventDestroy(ctx->file_fetched[i]);
    }
    if (ctx->file_d2h) (void)hipStreamDestroy(ctx->file_d2h);
    if (ctx->file_device) (void)hipFree(ctx->file_device);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_synchronize(jpeg_amd_ctx *ctx)
{
    JA_TRY(bind(ctx));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_last_hip_error(const jpeg_amd_ctx *ctx) { return ctx ? ctx->last_hip : 0; }

int jpeg_amd_layout_units(jpeg_amd_layout *L)
{
    if (!L || L->nplanes < 1 || L->nplanes > JPEG_AMD_MAX_PLANES || L->scale_x < 1 ||
        L->scale_y < 1 || L->width <= 0 || L->height <= 0)
        return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p) {
        if (L->factor_x[p] < 1 || L->factor_y[p] < 1) return JPEG_AMD_EINVAL;
        L->units_x[p] = units_of(L->width * L->factor_x[p], 8 * L->scale_x);
        L->units_y[p] = units_of(L->height * L->factor_y[p], 8 * L->scale_y);
    }
    return JPEG_AMD_OK;
}

// ---- memory + timing --------------------------------------------------------------------

int jpeg_amd_malloc(jpeg_amd_ctx *ctx, size_t bytes, void **d_ptr)
{
    JA_TRY(bind(ctx));
    if (!d_ptr) return JPEG_AMD_EINVAL;
    *d_ptr = nullptr;
    if (bytes == 0) return JPEG_AMD_OK;
    JA_HIP(ctx, hipMalloc(d_ptr, bytes));
    return JPEG_AMD_OK;
}

int jpeg_amd_free(jpeg_amd_ctx *ctx, void *d_ptr)
{
    JA_TRY(bind(ctx));
    if (!d_ptr) return JPEG_AMD_OK;
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    JA_HIP(ctx, hipFree(d_ptr));
    return JPEG_AMD_OK;
}

int jpeg_amd_memcpy_h2d(jpeg_amd_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    JA_TRY(bind(ctx));
    if (bytes == 0) return JPEG_AMD_OK;
    if (!d_dst || !h_src) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_memcpy_d2h(jpeg_amd_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    JA_TRY(bind(ctx));
    if (bytes == 0) return JPEG_AMD_OK;
    if (!h_dst || !d_src) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_timer_begin(jpeg_amd_ctx *ctx)
{
    JA_TRY(bind(ctx));
    JA_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
    return JPEG_AMD_OK;
}

int jpeg_amd_timer_end(jpeg_amd_ctx *ctx, float *elapsed_ms)
{
    JA_TRY(bind(ctx));
    if (!elapsed_ms) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
    // poll instead of sleeping on the event: a blocked host thread takes tens of microseconds to wake up, which a caller
    // that brackets a short timed region with its own clock would charge to the region
    // -- but only for a bounded time (200 us): a long region (the PCIe-bound file paths, a rank per core) must not burn a host
    // core, so after that the thread sleeps on the event like everybody else
    hipError_t q = hipErrorNotReady;
    const auto give_up = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
    while ((q = hipEventQuery(ctx->ev_end)) == hipErrorNotReady && std::chrono::steady_clock::now() < give_up) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    if (q == hipErrorNotReady) q = hipEventSynchronize(ctx->ev_end);
    JA_HIP(ctx, q);
    JA_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev_begin, ctx->ev_end));
    return JPEG_AMD_OK;
}

// ---- decode stages ----------------------------------------------------------------------

int jpeg_amd_idct_plane(jpeg_amd_ctx *ctx, const int16_t *d_coef, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision, uint16_t *d_plane)
{
    JA_TRY(bind(ctx));
    if (units_x < 0 || units_y < 0 || precision < 1 || precision > 16) return JPEG_AMD_EINVAL;
    if ((long long)units_x * units_y > (1LL << 30)) return JPEG_AMD_EINVAL;
    if (units_x == 0 || units_y == 0) return JPEG_AMD_OK;
    if (!d_coef || !d_plane) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta_zigzag, 1, &d_q));
    JA_HIP(ctx, launch_idct_plane(ctx->stream, 1, d_coef, 0, QuantaRef{d_q, 0}, 0, units_x,
                                  units_y, precision, d_plane, 0, false));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                           const int16_t *const d_coef[], const uint16_t *h_quanta, int ntables,
                           uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!d_coef || !d_planes) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        if (!d_coef[p] || !d_planes[p]) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, launch_idct_plane(ctx->stream, 1, d_coef[p], 0, QuantaRef{d_q, 0}, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, d_planes[p],
                                      0, false));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                const uint16_t *const d_planes[], int cosited, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    if (!d_planes || !d_rect) return JPEG_AMD_EINVAL;
    PlaneSet ps;
    JA_TRY(plane_set(L, d_planes, nullptr, true, &ps));
    JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, 1, *L, ps, false, cosited != 0,
                                        PixelKind::Rect16, d_rect, 0));
    return JPEG_AMD_OK;
}

int jpeg_amd_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *d_rect, size_t npixels,
                                int nplanes, jpeg_amd_color color, uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    if (npixels == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_pixels) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, launch_unpack(ctx->stream, d_rect, npixels, nplanes, color, d_pixels));
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                          const int16_t *const d_coef[], const size_t coef_stride[],
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int cosited, jpeg_amd_color color, uint8_t *d_pixels,
                          size_t pixel_stride)
{
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs));
    const QuantaRef q = c.quanta();
    const bool rgb = c.rgb();
    if (fused_decode_supported(*L, cosited != 0)) {
        JA_HIP(ctx, launch_fused_decode(ctx->stream, n_images, *L, cs, q, rgb, ctx->d_walk, d_pixels, pixel_stride));
        return JPEG_AMD_OK;
    }
    return staged_decode(ctx, L, n_images, cs, q, cosited != 0, true, rgb ? PixelKind::RGB8 : PixelKind::YCC8, d_pixels, pixel_stride);
}

int jpeg_amd_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                    const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                    uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, d_pixels, 0);
}

namespace {

// A pixel region of jpeg_amd_decode_region_batch / jpeg_amd_region_window: inside the image, not empty.
int check_region(const jpeg_amd_layout *L, const jpeg_amd_region &r)
{
    if (r.x < 0 || r.y < 0 || r.width <= 0 || r.height <= 0) return JPEG_AMD_EINVAL;
    if ((long long)r.x + r.width > L->width || (long long)r.y + r.height > L->height) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

bool whole_image(const jpeg_amd_layout *L, const jpeg_amd_region &r)
{
    return r.x == 0 && r.y == 0 && r.width == L->width && r.height == L->height;
}

// `buf` into the context's region buffer (grown on demand), one copy from a host buffer (pageable, so the copy has taken
// it when the call returns -- as stage_quanta).
int upload_regions(jpeg_amd_ctx *ctx, const std::vector<uint32_t> &buf)
{
    const size_t bytes = 4 * buf.size();
    JA_TRY(ensure_buffer(ctx, ctx->region, bytes));
    JA_HIP(ctx, hipMemcpyAsync(ctx->region.ptr, buf.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    return JPEG_AMD_OK;
}

// One launch of a view decode kernel, appended to the words that are staged for it: the index list [m] of its images, then the
// prefix [m + 1] of their tiles at n samples per block.  *nwg: the launch's workgroups; EINVAL: more of them than a grid holds.
int stage_group(std::vector<uint32_t> &buf, const std::vector<uint32_t> &members, int n, const jpeg_amd_view *h_views, uint32_t *nwg)
{
    buf.insert(buf.end(), members.begin(), members.end());
    uint64_t acc = 0;
    for (const uint32_t i : members) {
        buf.push_back((uint32_t)acc);
        acc += view_tiles(n, h_views[i].region);
    }
    if (acc > 0x7fffffffu) return JPEG_AMD_EINVAL;
    buf.push_back((uint32_t)acc);
    *nwg = (uint32_t)acc;
    return JPEG_AMD_OK;
}

// The regions (int32 [n][4]) and their tile prefix (uint32 [n + 1]) in the context's region buffer, one copy from a host
// buffer (pageable, so the copy has taken it when the call returns -- as stage_quanta).  Returns the workgroup count.
int stage_regions(jpeg_amd_ctx *ctx, const jpeg_amd_region *h, int n, const int32_t **d_regions, const uint32_t **d_tiles,
                  uint32_t *nwg)
{
    const size_t bytes = (size_t)16 * n + 4 * ((size_t)n + 1);
    std::vector<uint32_t> buf(bytes / 4);
    uint32_t acc = 0;
    for (int i = 0; i < n; ++i) {
        std::memcpy(&buf[4 * (size_t)i], &h[i], 16);
        buf[4 * (size_t)n + i] = acc;
        acc += region_tiles(h[i]);
    }
    buf[4 * (size_t)n + n] = acc;
    JA_TRY(upload_regions(ctx, buf));
    *d_regions = static_cast<const int32_t *>(ctx->region.ptr);
    *d_tiles = reinterpret_cast<const uint32_t *>(*d_regions + 4 * (size_t)n);
    *nwg = acc;
    return JPEG_AMD_OK;
}

constexpr size_t kFallbackChunkBytes = (size_t)1 << 30;   // scratch per chunk of a fallback's whole-image decodes or planes

constexpr int kViewDenoms = 4;   // slot k: denom 1 << k
int view_slot(int denom) { return denom == 1 ? 0 : denom == 2 ? 1 : denom == 4 ? 2 : denom == 8 ? 3 : -1; }

// The region and the view call's fallback for the layouts without a tile kernel: the whole scaled images of a run of
// consecutive images of one denominator into scratch behind the staged paths' planes (S's planes are no larger than L's),
// then one crop launch; a run is at most a chunk.  S[k]: the image at denominator 1 << k, for every k among the views.
int crop_fallback(jpeg_amd_ctx *ctx, const DecodeCall &c, const jpeg_amd_view *h_views, const jpeg_amd_layout S[kViewDenoms])
{
    const jpeg_amd_layout *L = c.L;
    const int n_images = c.n_images;
    const size_t n = (size_t)n_images;
    size_t full_max = 0;
    std::vector<uint32_t> buf(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const jpeg_amd_layout &Si = S[view_slot(h_views[i].denom)];
        full_max = std::max(full_max, (size_t)3 * Si.width * Si.height);
        std::memcpy(&buf[4 * i], &h_views[i].region, 16);
    }
    const size_t per_image = full_max + scratch_planes_bytes(L, 1, sizeof(uint8_t));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(n, kFallbackChunkBytes / per_image));
    const size_t planes_bytes = scratch_planes_bytes(L, chunk, sizeof(uint8_t));
    JA_TRY(ensure_buffer(ctx, ctx->scratch, planes_bytes + align256(full_max * chunk)));
    uint8_t *d_full = static_cast<uint8_t *>(ctx->scratch.ptr) + planes_bytes;   // the staged paths' planes stay below it
    JA_TRY(upload_regions(ctx, buf));
    const int32_t *d_regions = static_cast<const int32_t *>(ctx->region.ptr);
    for (int i0 = 0; i0 < n_images;) {
        const int denom = h_views[i0].denom;
        const jpeg_amd_layout &Sd = S[view_slot(denom)];
        int m = 0;
        size_t max_bytes = 0;
        for (; i0 + m < n_images && m < chunk && h_views[i0 + m].denom == denom; ++m)
            max_bytes = std::max(max_bytes, (size_t)3 * h_views[i0 + m].region.width * h_views[i0 + m].region.height);
        const size_t full = (size_t)3 * Sd.width * Sd.height;
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall run = c.images(i0, m, coef);
        JA_TRY(jpeg_amd_decode_scaled_batch(ctx, L, m, coef, c.coef_stride, run.d_quanta, c.quanta_stride, c.ntables, c.cosited, c.color,
                                            denom, d_full, full));
        JA_HIP(ctx, launch_region_crop(ctx->stream, m, d_full, full, Sd.width, d_regions + 4 * (size_t)i0, max_bytes, run.d_pixels,
                                       c.pixel_stride));
        i0 += m;
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_decode_region_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_region *h_regions,
                                 uint8_t *d_pixels, size_t pixel_stride)
try {
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs, h_regions != nullptr));
    bool whole = true;
    for (int i = 0; i < n_images; ++i) {
        JA_TRY(check_region(L, h_regions[i]));
        if (n_images > 1 && pixel_stride < (size_t)3 * h_regions[i].width * h_regions[i].height) return JPEG_AMD_EINVAL;
        whole = whole && whole_image(L, h_regions[i]);
    }
    if (whole)
        return jpeg_amd_decode_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                     d_pixels, pixel_stride);

    if (fused_decode_supported(*L, cosited != 0)) {
        const int32_t *d_regions = nullptr;
        const uint32_t *d_tiles = nullptr;
        uint32_t nwg = 0;
        JA_TRY(stage_regions(ctx, h_regions, n_images, &d_regions, &d_tiles, &nwg));
        JA_HIP(ctx, launch_region_decode(ctx->stream, n_images, *L, cs, c.quanta(), c.rgb(), d_tiles, d_regions, nwg, d_pixels,
                                         pixel_stride));
        return JPEG_AMD_OK;
    }

    // the crop fallback at denominator 1, where the scaled image is the image
    std::vector<jpeg_amd_view> views((size_t)n_images);
    for (int i = 0; i < n_images; ++i) views[(size_t)i] = jpeg_amd_view{1, h_regions[i]};
    const jpeg_amd_layout S[kViewDenoms] = {*L};
    return crop_fallback(ctx, c, views.data(), S);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_region(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_region *region, uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!region) return JPEG_AMD_EINVAL;
    JA_TRY(check_region(L, *region));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_region_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, region, d_pixels, 0);
}

int jpeg_amd_region_window(const jpeg_amd_layout *L, int cosited, const jpeg_amd_region *region,
                           jpeg_amd_region windows[JPEG_AMD_MAX_PLANES])
{
    if (!region || !windows) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    JA_TRY(check_region(L, *region));
    const jpeg_amd_region &r = *region;
    for (int p = 0; p < JPEG_AMD_MAX_PLANES; ++p) {
        windows[p] = jpeg_amd_region{0, 0, 0, 0};
        if (p >= L->nplanes) continue;
        int32_t x0, x1, y0, y1;
        axis_span(interleave_axis(*L, p, cosited != 0, false), r.x, r.x + r.width - 1, x0, x1);
        axis_span(interleave_axis(*L, p, cosited != 0, true), r.y, r.y + r.height - 1, y0, y1);
        windows[p] = jpeg_amd_region{x0 >> 3, y0 >> 3, (x1 >> 3) - (x0 >> 3) + 1, (y1 >> 3) - (y0 >> 3) + 1};
    }
    return JPEG_AMD_OK;
}

namespace {

// N = 8 / denom for a denom of the contract, else 0.
int scaled_n(int denom) { return denom == 1 || denom == 2 || denom == 4 || denom == 8 ? 8 / denom : 0; }

// The planes, N x N samples per block, must cover the scaled image as check_planes_cover_image asks of the full-size one:
// with units = ceil(size factor / (8 scale)) they always do (include/jpeg_amd.h has the proof); units given by hand may not.
int check_planes_cover_scaled(const jpeg_amd_layout *L, const jpeg_amd_layout *S, int n)
{
    for (int p = 0; p < L->nplanes; ++p) {
        const long long sx = (long long)n * L->units_x[p], sy = (long long)n * L->units_y[p];
        if (plane_is_direct(*L, p)) {
            if (sx < S->width || sy < S->height) return JPEG_AMD_EINVAL;
        } else {
            if (sx < 1 || sy < 1) return JPEG_AMD_EINVAL;
            if (axis_index(interleave_axis(*L, p, true, false), S->width - 1) >= sx) return JPEG_AMD_EINVAL;
            if (axis_index(interleave_axis(*L, p, true, true), S->height - 1) >= sy) return JPEG_AMD_EINVAL;
        }
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_scaled_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out)
{
    if (!out) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(in, -1));
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout s = *in;
    s.width = (int32_t)(((long long)in->width * n + 7) / 8);
    s.height = (int32_t)(((long long)in->height * n + 7) / 8);
    for (int p = 0; p < in->nplanes; ++p) {
        s.units_x[p] = (int32_t)(((long long)in->units_x[p] * n + 7) / 8);
        s.units_y[p] = (int32_t)(((long long)in->units_y[p] * n + 7) / 8);
    }
    *out = s;
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_scaled_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, int denom,
                                 uint8_t *d_pixels, size_t pixel_stride)
{
    if (denom == 1)
        return jpeg_amd_decode_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                     d_pixels, pixel_stride);
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    JA_TRY(bind(ctx));
    JA_TRY(c.check());
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout S;
    JA_TRY(jpeg_amd_scaled_layout(L, denom, &S));
    JA_TRY(check_planes_cover_scaled(L, &S, n));
    if (n_images == 0) return JPEG_AMD_OK;
    PlaneSet cs;
    JA_TRY(c.planes(&cs));
    if (n_images > 1 && pixel_stride < (size_t)3 * S.width * S.height) return JPEG_AMD_EINVAL;
    const QuantaRef q = c.quanta();
    const bool rgb = c.rgb();
    if (fused_decode_supported(*L, cosited != 0)) {
        JA_HIP(ctx, launch_scaled_decode(ctx->stream, n_images, *L, n, S.width, S.height, cs, q, rgb, d_pixels, pixel_stride));
        return JPEG_AMD_OK;
    }

    // fallback: every plane N x N per block into byte planes in scratch, padded to S's whole blocks by edge replication, then
    // the staged interleave + colour kernel under S, chunk by chunk
    const size_t per_image = std::max<size_t>(1, scratch_planes_bytes(&S, 1, sizeof(uint8_t)));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_images, kFallbackChunkBytes / per_image));
    PlaneSetMut scratch;
    JA_TRY(scratch_planes(ctx, &S, chunk, sizeof(uint8_t), &scratch));
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int m = std::min(chunk, n_images - i0);
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall part = c.images(i0, m, coef);
        PlaneSet ps{};
        for (int p = 0; p < L->nplanes; ++p) {
            JA_HIP(ctx, launch_idct_scaled_plane(ctx->stream, m, coef[p], coef_stride[p], part.quanta(), L->qi[p], L->units_x[p],
                                                 L->units_y[p], n, L->precision, scratch.ptr[p], scratch.stride[p], true));
            ps.ptr[p] = scratch.ptr[p];
            ps.stride[p] = scratch.stride[p];
        }
        JA_HIP(ctx, launch_planar_to_pixels(ctx->stream, m, S, ps, true, cosited != 0, rgb ? PixelKind::RGB8 : PixelKind::YCC8,
                                            part.d_pixels, pixel_stride));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_decode_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color, int denom,
                           uint8_t *d_pixels)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (scaled_n(denom) == 0) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_scaled_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, denom, d_pixels, 0);
}

int jpeg_amd_spectral_idct_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                                  const uint16_t *h_quanta, int ntables, int denom, uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (denom == 1) return jpeg_amd_spectral_idct(ctx, L, d_coef, h_quanta, ntables, d_planes);
    const int n = scaled_n(denom);
    if (n == 0 || !d_coef || !d_planes) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) != 0 && (!d_coef[p] || !d_planes[p])) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p)
        JA_HIP(ctx, launch_idct_scaled_plane(ctx->stream, 1, d_coef[p], 0, QuantaRef{d_q, 0}, L->qi[p], L->units_x[p], L->units_y[p], n,
                                             L->precision, d_planes[p], 0, false));
    return JPEG_AMD_OK;
}

namespace {

// The image at `denom` as the scaled contract defines it: *S is jpeg_amd_scaled_layout's, and the planes cover it.
int scaled_image(const jpeg_amd_layout *L, int denom, jpeg_amd_layout *S)
{
    const int n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    JA_TRY(jpeg_amd_scaled_layout(L, denom, S));
    return denom == 1 ? JPEG_AMD_OK : check_planes_cover_scaled(L, S, n);
}

// Every argument of jpeg_amd_decode_view_batch but the context, in the order that decides the status of a call that is wrong
// twice.  S[k] / count[k]: the scaled image and the number of views of denominator 1 << k; *whole: every view a whole image.
int check_views(const DecodeCall &c, const jpeg_amd_view *h_views, jpeg_amd_layout S[kViewDenoms], int count[kViewDenoms], bool *whole,
                PlaneSet *cs)
{
    const jpeg_amd_layout *L = c.L;
    const int n_images = c.n_images;
    JA_TRY(c.check());
    if (n_images == 0) return JPEG_AMD_OK;
    JA_TRY(c.planes(cs, h_views != nullptr));
    for (int i = 0; i < n_images; ++i) {
        const int k = view_slot(h_views[i].denom);
        if (k < 0) return JPEG_AMD_EINVAL;
        if (count[k]++ == 0) JA_TRY(scaled_image(L, h_views[i].denom, &S[k]));
        const jpeg_amd_region &r = h_views[i].region;
        JA_TRY(check_region(&S[k], r));
        if (n_images > 1 && c.pixel_stride < (size_t)3 * r.width * r.height) return JPEG_AMD_EINVAL;
        *whole = *whole && whole_image(&S[k], r);
    }
    return JPEG_AMD_OK;
}

// What jpeg_amd_decode_view and jpeg_amd_decode_resized refuse before a table is staged: check_views for their one view.
// (C++ linkage: a function of an unnamed namespace inside the extern "C" block is exported under its plain name.)
extern "C++" int check_one_view(const jpeg_amd_layout *L, int ntables, jpeg_amd_color color, const jpeg_amd_view *view)
{
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_planes_cover_image(L));
    JA_TRY(check_batch8(L, 1, color));
    if (!view) return JPEG_AMD_EINVAL;
    jpeg_amd_layout S;
    JA_TRY(scaled_image(L, view->denom, &S));
    return check_region(&S, view->region);
}

}  // namespace

int jpeg_amd_decode_view_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                               const int16_t *const d_coef[], const size_t coef_stride[],
                               const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                               int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                               uint8_t *d_pixels, size_t pixel_stride)
try {
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    const DecodeCall c{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, pixel_stride};
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(c, h_views, S, count, &whole, &cs));
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;

    const int denom0 = h_views[0].denom;
    if (whole && count[view_slot(denom0)] == n_images)
        return jpeg_amd_decode_scaled_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            denom0, d_pixels, pixel_stride);
    if (count[0] == n_images) {   // every view a region of the full-size image
        std::vector<jpeg_amd_region> regions((size_t)n_images);
        for (int i = 0; i < n_images; ++i) regions[(size_t)i] = h_views[i].region;
        return jpeg_amd_decode_region_batch(ctx, L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            regions.data(), d_pixels, pixel_stride);
    }

    const size_t n = (size_t)n_images;
    if (fused_decode_supported(*L, cosited != 0)) {
        // staged in one copy: the rectangles [n][4], then per denominator of the call its group (stage_group)
        std::vector<uint32_t> buf(4 * n), members;
        for (size_t i = 0; i < n; ++i) std::memcpy(&buf[4 * i], &h_views[i].region, 16);
        size_t at[kViewDenoms];
        uint32_t nwg[kViewDenoms];
        for (int k = 0; k < kViewDenoms; ++k) {
            at[k] = buf.size();
            nwg[k] = 0;
            if (count[k] == 0) continue;
            members.clear();
            for (size_t i = 0; i < n; ++i)
                if (view_slot(h_views[i].denom) == k) members.push_back((uint32_t)i);
            JA_TRY(stage_group(buf, members, 8 >> k, h_views, &nwg[k]));
        }
        JA_TRY(upload_regions(ctx, buf));
        const uint32_t *d_buf = static_cast<const uint32_t *>(ctx->region.ptr);
        for (int k = 0; k < kViewDenoms; ++k) {
            if (count[k] == 0) continue;
            JA_HIP(ctx, launch_view_decode(ctx->stream, count[k], *L, 8 >> k, cs, c.quanta(), c.rgb(), d_buf + at[k],
                                           d_buf + at[k] + count[k], reinterpret_cast<const int32_t *>(d_buf), nwg[k], d_pixels,
                                           pixel_stride));
        }
        return JPEG_AMD_OK;
    }

    return crop_fallback(ctx, c, h_views, S);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_view(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                         const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                         const jpeg_amd_view *view, uint8_t *d_pixels)
{
    // as the batch call: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_view_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, d_pixels, 0);
}

int jpeg_amd_view_window(const jpeg_amd_layout *L, int cosited, int denom, const jpeg_amd_region *region,
                         jpeg_amd_region windows[JPEG_AMD_MAX_PLANES])
{
    if (!region || !windows) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    JA_TRY(check_planes_cover_image(L));
    jpeg_amd_layout S;
    JA_TRY(scaled_image(L, denom, &S));
    JA_TRY(check_region(&S, *region));
    const jpeg_amd_region &r = *region;
    const int32_t n = scaled_n(denom);
    for (int p = 0; p < JPEG_AMD_MAX_PLANES; ++p) {
        windows[p] = jpeg_amd_region{0, 0, 0, 0};
        if (p >= L->nplanes) continue;
        InterleaveAxis mx = interleave_axis(*L, p, cosited != 0, false), my = interleave_axis(*L, p, cosited != 0, true);
        mx.last = n * L->units_x[p] - 1;   // the scaled plane's padded edge
        my.last = n * L->units_y[p] - 1;
        int32_t x0, x1, y0, y1;
        axis_span(mx, r.x, r.x + r.width - 1, x0, x1);
        axis_span(my, r.y, r.y + r.height - 1, y0, y1);
        windows[p] = jpeg_amd_region{x0 / n, y0 / n, x1 / n - x0 / n + 1, y1 / n - y0 / n + 1};
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_view_of_source(const jpeg_amd_layout *L, int denom, const jpeg_amd_region *source_region, jpeg_amd_region *region)
{
    if (!source_region || !region) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(L, -1));
    const long long n = scaled_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    JA_TRY(check_region(L, *source_region));
    const jpeg_amd_region &s = *source_region;
    const long long w1 = ((long long)L->width * n + 7) / 8, h1 = ((long long)L->height * n + 7) / 8;
    const long long x0 = s.x * n / 8, x1 = std::min(w1, (((long long)s.x + s.width) * n + 7) / 8);
    const long long y0 = s.y * n / 8, y1 = std::min(h1, (((long long)s.y + s.height) * n + 7) / 8);
    *region = jpeg_amd_region{(int32_t)x0, (int32_t)y0, (int32_t)(x1 - x0), (int32_t)(y1 - y0)};
    return JPEG_AMD_OK;
}

int jpeg_amd_view_denom(int32_t src_w, int32_t src_h, int32_t want_w, int32_t want_h)
{
    for (int denom = 8; denom > 1; denom /= 2) {
        const long long n = 8 / denom;
        if (src_w * n / 8 >= want_w && src_h * n / 8 >= want_h) return denom;
    }
    return 1;
}

namespace {

constexpr size_t kResizeChunkBytes = (size_t)1 << 30;   // decoded views per chunk of the resized and tensor decodes

// The records into the context's record buffer, one copy from a host buffer (pageable, so the copy has taken it when the call
// returns -- as stage_quanta).
int upload_records(jpeg_amd_ctx *ctx, const std::vector<uint8_t> &rec)
{
    JA_TRY(ensure_buffer(ctx, ctx->resize_rec, rec.size()));
    JA_HIP(ctx, hipMemcpyAsync(ctx->resize_rec.ptr, rec.data(), rec.size(), hipMemcpyHostToDevice, ctx->stream));
    return JPEG_AMD_OK;
}

// What both resample calls require of the output.
int check_resize_target(int n_images, int32_t out_w, int32_t out_h, const void *d_dst, size_t dst_stride)
{
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    if (resize_tiles(out_w, out_h) > 0x7fffffffu) return JPEG_AMD_EINVAL;   // more workgroups than a grid holds
    if (n_images > 0 && !d_dst) return JPEG_AMD_EINVAL;
    if (n_images > 1 && dst_stride < (size_t)3 * out_w * out_h) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// What the tensor calls require of the output, beyond jpeg_amd_tensor_extent.
int check_tensor_target(int n_images, int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const void *d_dst,
                        size_t dst_stride, size_t *elem_bytes)
{
    size_t image_elems = 0;
    JA_TRY(jpeg_amd_tensor_extent(spec, out_w, out_h, elem_bytes, &image_elems));
    if (n_images > 0 && !d_dst) return JPEG_AMD_EINVAL;
    if ((uintptr_t)d_dst % *elem_bytes != 0) return JPEG_AMD_EINVAL;
    if (n_images > 1 && dst_stride < image_elems) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// Where the resampled images of a call go, and through which filter: bytes (k_resize_bilinear, k_antialias_bytes) or, in a
// tensor call, elements of `spec` (k_resize_tensor, k_antialias_tensor).  `tensor` is not `spec != nullptr`: a tensor call
// without a spec is jpeg_amd_tensor_extent's to refuse.  The records of a call are bytes on the host, record_bytes() per image:
// ResizeRecord for the bilinear kernels, as ever, AntialiasRecord for the others.
struct ResampleTarget {
    int32_t out_w, out_h;
    int filter;              // JPEG_AMD_FILTER_*
    bool tensor;
    const jpeg_amd_tensor_spec *spec;
    const uint8_t *h_flip;   // per image, or nullptr: none is mirrored
    void *d_dst;
    size_t stride;           // between images, in elements
    size_t elem_bytes = 1;   // of a tensor call: check() sets it

    bool antialias() const { return filter == JPEG_AMD_FILTER_ANTIALIAS; }
    int check(int n_images)
    {
        if (filter != JPEG_AMD_FILTER_BILINEAR && filter != JPEG_AMD_FILTER_ANTIALIAS) return JPEG_AMD_EINVAL;
        return tensor ? check_tensor_target(n_images, out_w, out_h, spec, d_dst, stride, &elem_bytes)
                      : check_resize_target(n_images, out_w, out_h, d_dst, stride);
    }
    // Image i of the call, w x h at `offset` bytes from the launch's source.  The scale factors of the contract: divided here,
    // in binary32, never on the device.
    // ENOSUP: the antialiasing filter's tap limit, kx or ky above kAntialiasMaxScale.  The record is written either way, and
    // the caller keeps the verdict of the first such image until everything else of the call has been judged.
    size_t record_bytes() const { return antialias() ? sizeof(AntialiasRecord) : sizeof(ResizeRecord); }
    int record(std::vector<uint8_t> &rec, int at, int i, uint64_t offset, int32_t w, int32_t h) const
    {
        const float kx = (float)w / (float)out_w, ky = (float)h / (float)out_h;
        const uint32_t flip = h_flip && h_flip[i] ? 1u : 0u;
        if (!antialias()) {
            const ResizeRecord r{offset, w, h, kx, ky, flip, 0u};
            std::memcpy(rec.data() + (size_t)at * sizeof r, &r, sizeof r);
            return JPEG_AMD_OK;
        }
        const float sx = std::max(kx, 1.0f), sy = std::max(ky, 1.0f);
        const AntialiasRecord r{offset, w, h, kx, sx, 1.0f / sx, ky, sy, 1.0f / sy, flip, 0u};
        std::memcpy(rec.data() + (size_t)at * sizeof r, &r, sizeof r);
        return kx > kAntialiasMaxScale || ky > kAntialiasMaxScale ? JPEG_AMD_ENOSUP : JPEG_AMD_OK;
    }
    // Images [i0, i0 + m) of the call, from their records: record i0 of d_rec onwards.
    hipError_t launch(hipStream_t stream, int m, const uint8_t *d_src, const void *d_rec, int i0) const
    {
        uint8_t *d_out = static_cast<uint8_t *>(d_dst) + (size_t)i0 * stride * elem_bytes;
        if (antialias()) {
            const AntialiasRecord *rec = static_cast<const AntialiasRecord *>(d_rec) + i0;
            return tensor ? launch_antialias_tensor(stream, m, d_src, rec, out_w, out_h, *spec, d_out, stride)
                          : launch_antialias_bytes(stream, m, d_src, rec, out_w, out_h, d_out, stride);
        }
        const ResizeRecord *rec = static_cast<const ResizeRecord *>(d_rec) + i0;
        return tensor ? launch_resize_tensor(stream, m, d_src, rec, out_w, out_h, *spec, d_out, stride)
                      : launch_resize_bilinear(stream, m, d_src, rec, out_w, out_h, d_out, stride);
    }
};

// The chunks of the resized and tensor decodes: consecutive images, m images at a stride of the chunk's largest view, at most
// kResizeChunkBytes in all; rec holds image i's record inside its chunk (the target's kind of record); need: the bytes the
// largest chunk takes; status: what the target's record() says of the first image it refuses.
struct ResizeChunk { int i0, m; size_t stride; };
struct ResizePlan {
    std::vector<ResizeChunk> chunks;
    std::vector<uint8_t> rec;
    size_t need = 0;
    int status = JPEG_AMD_OK;
};
extern "C++" ResizePlan plan_resize_chunks(int n_images, const jpeg_amd_view *h_views, const ResampleTarget &t)
{
    ResizePlan plan;
    plan.rec.resize((size_t)n_images * t.record_bytes());
    for (int i0 = 0; i0 < n_images;) {
        int m = 0;
        size_t stride = 0;
        for (; i0 + m < n_images; ++m) {
            const jpeg_amd_region &r = h_views[i0 + m].region;
            const size_t s = std::max(stride, (size_t)3 * r.width * r.height);
            if (m > 0 && s * ((size_t)m + 1) > kResizeChunkBytes) break;
            stride = s;
        }
        for (int j = 0; j < m; ++j) {
            const jpeg_amd_region &r = h_views[i0 + j].region;
            const int verdict = t.record(plan.rec, i0 + j, i0 + j, (uint64_t)j * stride, r.width, r.height);
            if (plan.status == JPEG_AMD_OK) plan.status = verdict;
        }
        plan.chunks.push_back(ResizeChunk{i0, m, stride});
        plan.need = std::max(plan.need, stride * (size_t)m);
        i0 += m;
    }
    return plan;
}

// The route of every resized and tensor decode, behind its checks and on a bound context: chunk by chunk,
// decode(c, chunk, d_views) puts the views of chunk c into the context's buffer at the chunk's stride, and the target's launch
// resamples them from there.  (C++ linkage, here and above: see check_one_view.)
extern "C++" template <typename Decode>
int resample_chunks(jpeg_amd_ctx *ctx, const ResizePlan &plan, const ResampleTarget &t, Decode decode)
{
    JA_TRY(ensure_buffer(ctx, ctx->resize_src, plan.need));
    JA_TRY(upload_records(ctx, plan.rec));
    uint8_t *d_views = static_cast<uint8_t *>(ctx->resize_src.ptr);
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const ResizeChunk &k = plan.chunks[c];
        JA_TRY(decode(c, k, d_views));
        JA_HIP(ctx, t.launch(ctx->stream, k.m, d_views, ctx->resize_rec.ptr, k.i0));
    }
    return JPEG_AMD_OK;
}

// jpeg_amd_resize_batch and jpeg_amd_resize_tensor_batch, and their forms with a filter.
int resize_images(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride, const jpeg_amd_extent *h_extents,
                  ResampleTarget t)
{
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    JA_TRY(t.check(n_images));
    std::vector<uint8_t> rec((size_t)n_images * t.record_bytes());
    int taps = JPEG_AMD_OK;   // the tap limit: judged last, by the first image over it
    if (n_images > 0) {
        if (!d_src || !h_extents) return JPEG_AMD_EINVAL;
        for (int i = 0; i < n_images; ++i) {
            const jpeg_amd_extent &e = h_extents[i];
            if (e.width < 1 || e.height < 1) return JPEG_AMD_EINVAL;
            if (n_images > 1 && src_stride < (size_t)3 * e.width * e.height) return JPEG_AMD_EINVAL;
            const int verdict = t.record(rec, i, i, (uint64_t)i * src_stride, e.width, e.height);
            if (taps == JPEG_AMD_OK) taps = verdict;
        }
    }
    JA_TRY(taps);
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;
    JA_TRY(upload_records(ctx, rec));
    JA_HIP(ctx, t.launch(ctx->stream, n_images, d_src, ctx->resize_rec.ptr, 0));
    return JPEG_AMD_OK;
}

// jpeg_amd_decode_resized_batch and jpeg_amd_decode_tensor_batch, and their forms with a filter; c.d_pixels is t.d_dst, and its stride is not looked at.
int decode_resampled(jpeg_amd_ctx *ctx, const DecodeCall &c, const jpeg_amd_view *h_views, ResampleTarget t)
{
    // everything the view call refuses is refused here, before its first chunk is enqueued (the intermediate's stride is
    // ours and always large enough), then what the target refuses
    DecodeCall views = c;
    views.pixel_stride = ~(size_t)0;
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(views, h_views, S, count, &whole, &cs));
    JA_TRY(t.check(c.n_images));
    const ResizePlan plan = plan_resize_chunks(c.n_images, h_views, t);
    JA_TRY(plan.status);
    JA_TRY(bind(ctx));
    if (c.n_images == 0) return JPEG_AMD_OK;
    return resample_chunks(ctx, plan, t, [&](size_t, const ResizeChunk &k, uint8_t *d_views) {
        const int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
        const DecodeCall part = c.images(k.i0, k.m, coef);
        return jpeg_amd_decode_view_batch(ctx, c.L, k.m, coef, c.coef_stride, part.d_quanta, c.quanta_stride, c.ntables, c.cosited,
                                          c.color, h_views + k.i0, d_views, k.stride);
    });
}

}  // namespace

int jpeg_amd_resize_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                          const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents, ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, false, nullptr, nullptr, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                  const int16_t *const d_coef[], const size_t coef_stride[],
                                  const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                  int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                  int32_t out_w, int32_t out_h, uint8_t *d_pixels, size_t pixel_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, 0},
                            h_views, ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, false, nullptr, nullptr, d_pixels, pixel_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                            const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                            const jpeg_amd_view *view, int32_t out_w, int32_t out_h, uint8_t *d_pixels)
{
    // as jpeg_amd_decode_view: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY((ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, false, nullptr, nullptr, d_pixels, 0}.check(1)));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_decode_resized_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, out_w, out_h, d_pixels,
                                         0);
}

int jpeg_amd_tensor_extent(const jpeg_amd_tensor_spec *spec, int32_t out_w, int32_t out_h, size_t *elem_bytes, size_t *image_elems)
{
    if (!spec) return JPEG_AMD_EINVAL;
    if (spec->dtype != JPEG_AMD_F32 && spec->dtype != JPEG_AMD_F16 && spec->dtype != JPEG_AMD_BF16) return JPEG_AMD_EINVAL;
    if (spec->layout != JPEG_AMD_TENSOR_HWC && spec->layout != JPEG_AMD_TENSOR_CHW) return JPEG_AMD_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(spec->mean[c]) || !std::isfinite(spec->scale[c])) return JPEG_AMD_EINVAL;
    if (out_w < 1 || out_h < 1 || out_w > kResizeMaxSide || out_h > kResizeMaxSide) return JPEG_AMD_EINVAL;
    if (resize_tiles(out_w, out_h) > 0x7fffffffu) return JPEG_AMD_EINVAL;   // more workgroups than a grid holds
    if (elem_bytes) *elem_bytes = spec->dtype == JPEG_AMD_F32 ? 4 : 2;
    if (image_elems) *image_elems = (size_t)3 * out_w * out_h;
    return JPEG_AMD_OK;
}

int jpeg_amd_resize_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents, ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                 int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                 void *d_dst, size_t dst_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            static_cast<uint8_t *>(d_dst), 0},
                            h_views, ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_view *view, int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec,
                           int flip, void *d_dst)
{
    // as jpeg_amd_decode_resized: what can be refused is refused before a table is staged
    JA_TRY(check_one_view(L, ntables, color, view));
    JA_TRY((ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, true, spec, nullptr, d_dst, 0}.check(1)));
    JA_TRY(bind(ctx));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    const uint8_t h_flip = flip ? 1 : 0;
    return jpeg_amd_decode_tensor_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, color, view, out_w, out_h, spec,
                                        &h_flip, d_dst, 0);
}

namespace {

constexpr int kMixedGroups = 2 * kViewDenoms;   // group 2 k + (three planes): the images of N = 8 >> k with that many planes

// Images [0, m) of a mixed call, or of a chunk of one, sorted into the launches of k_view_decode_mixed and the images that
// take the uniform call.
struct MixedPlan {
    std::vector<uint32_t> members[kMixedGroups];   // the group's images, in index order
    std::vector<int> fallback;                     // no tile kernel for the layout: the uniform call, image by image
};

// What the uniform view call with n_images = 1 judges of image `im` with view `v`, in its order (check_views itself), then the
// stride that the mixed call's placement needs.
int check_mixed_image(const jpeg_amd_image &im, int n_images, int cosited, jpeg_amd_color color, const jpeg_amd_view &v,
                      const void *d_out, size_t pixel_stride)
{
    const DecodeCall c{&im.layout, 1, im.d_coef, kOneImage, im.d_quanta, 0, im.ntables, cosited, color,
                       static_cast<uint8_t *>(const_cast<void *>(d_out)), 0};
    jpeg_amd_layout S[kViewDenoms];
    int count[kViewDenoms] = {0, 0, 0, 0};
    bool whole = true;
    PlaneSet cs{};
    JA_TRY(check_views(c, &v, S, count, &whole, &cs));
    if (n_images > 1 && pixel_stride < (size_t)3 * v.region.width * v.region.height) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// The plan of m checked images; EINVAL: a launch of more workgroups than a grid holds (refused here, before the context is
// looked at, and so never by run_mixed).
int plan_mixed(const jpeg_amd_image *im, const jpeg_amd_view *v, int m, int cosited, MixedPlan *plan)
{
    uint64_t acc[kMixedGroups] = {};
    for (int i = 0; i < m; ++i) {
        if (!fused_decode_supported(im[i].layout, cosited != 0)) {
            plan->fallback.push_back(i);
            continue;
        }
        const int k = view_slot(v[i].denom), g = 2 * k + (im[i].layout.nplanes == 3 ? 1 : 0);
        plan->members[g].push_back((uint32_t)i);
        acc[g] += view_tiles(8 >> k, v[i].region);
    }
    for (int g = 0; g < kMixedGroups; ++g)
        if (acc[g] > 0x7fffffffu) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

// The planned images into d_pixels, image i at i * pixel_stride: one copy of the records [m], then per group its index list
// and tile prefix (stage_group), into the context's `mixed` buffer (from a pageable host buffer, so the copy has taken it when
// the call returns -- as stage_quanta); a launch per group; the uniform call for each of the others.
int run_mixed(jpeg_amd_ctx *ctx, const jpeg_amd_image *im, const jpeg_amd_view *v, int m, const MixedPlan &plan, int cosited,
              jpeg_amd_color color, uint8_t *d_pixels, size_t pixel_stride)
{
    const size_t rec_bytes = mixed_record_bytes(), lists = rec_bytes * (size_t)m / 4;
    size_t words = 0;
    for (int g = 0; g < kMixedGroups; ++g)
        if (!plan.members[g].empty()) words += 2 * plan.members[g].size() + 1;
    if (words != 0) {
        std::vector<uint32_t> buf;
        buf.reserve(lists + words);
        buf.resize(lists);   // the records of the uniform call's images stay zero: no list names them
        size_t at[kMixedGroups] = {};
        uint32_t nwg[kMixedGroups] = {};
        for (int g = 0; g < kMixedGroups; ++g) {
            const std::vector<uint32_t> &mem = plan.members[g];
            if (mem.empty()) continue;
            const int n = 8 >> (g / 2);
            for (const uint32_t i : mem)
                mixed_record(reinterpret_cast<uint8_t *>(buf.data()) + rec_bytes * i, im[i].layout, n, im[i].d_coef, im[i].d_quanta,
                             v[i].region, d_pixels + (size_t)i * pixel_stride);
            at[g] = buf.size();
            JA_TRY(stage_group(buf, mem, n, v, &nwg[g]));
        }
        JA_TRY(ensure_buffer(ctx, ctx->mixed, 4 * buf.size()));
        JA_HIP(ctx, hipMemcpyAsync(ctx->mixed.ptr, buf.data(), 4 * buf.size(), hipMemcpyHostToDevice, ctx->stream));
        const uint32_t *d_w = static_cast<const uint32_t *>(ctx->mixed.ptr);
        for (int g = 0; g < kMixedGroups; ++g) {
            const int count = (int)plan.members[g].size();
            if (count == 0) continue;
            JA_HIP(ctx, launch_view_decode_mixed(ctx->stream, count, 8 >> (g / 2), g % 2 ? 3 : 1, color == JPEG_AMD_COLOR_RGB8,
                                                 ctx->mixed.ptr, d_w + at[g], d_w + at[g] + count, nwg[g]));
        }
    }
    for (const int i : plan.fallback)
        JA_TRY(jpeg_amd_decode_view_batch(ctx, &im[i].layout, 1, im[i].d_coef, kOneImage, im[i].d_quanta, 0, im[i].ntables, cosited,
                                          color, &v[i], d_pixels + (size_t)i * pixel_stride, 0));
    return JPEG_AMD_OK;
}

// jpeg_amd_decode_resized_mixed and jpeg_amd_decode_tensor_mixed: decode_resampled's route with the mixed view decode.
int resized_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                  const jpeg_amd_view *h_views, ResampleTarget t)
{
    // every argument first, the context last; the target is judged where the uniform call judges it: behind the first image
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_images || !h_views)) return JPEG_AMD_EINVAL;
    for (int i = 0; i < n_images; ++i) {
        JA_TRY(check_mixed_image(h_images[i], 1, cosited, color, h_views[i], t.d_dst, 0));   // the views' stride is ours
        if (i == 0) JA_TRY(t.check(n_images));
    }
    if (n_images == 0) JA_TRY(t.check(n_images));
    const ResizePlan plan = plan_resize_chunks(n_images, h_views, t);
    std::vector<MixedPlan> plans(plan.chunks.size());
    for (size_t c = 0; c < plans.size(); ++c)
        JA_TRY(plan_mixed(h_images + plan.chunks[c].i0, h_views + plan.chunks[c].i0, plan.chunks[c].m, cosited, &plans[c]));
    JA_TRY(plan.status);
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    JA_TRY(bind(ctx));
    return resample_chunks(ctx, plan, t, [&](size_t c, const ResizeChunk &k, uint8_t *d_views) {
        return run_mixed(ctx, h_images + k.i0, h_views + k.i0, k.m, plans[c], cosited, color, d_views, k.stride);
    });
}

}  // namespace

int jpeg_amd_decode_view_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                               jpeg_amd_color color, const jpeg_amd_view *h_views, uint8_t *d_pixels, size_t pixel_stride)
try {
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_images || !h_views)) return JPEG_AMD_EINVAL;
    for (int i = 0; i < n_images; ++i) JA_TRY(check_mixed_image(h_images[i], n_images, cosited, color, h_views[i], d_pixels, pixel_stride));
    MixedPlan plan;
    JA_TRY(plan_mixed(h_images, h_views, n_images, cosited, &plan));
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    JA_TRY(bind(ctx));
    return run_mixed(ctx, h_images, h_views, n_images, plan, cosited, color, d_pixels, pixel_stride);
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                  jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                  uint8_t *d_pixels, size_t pixel_stride)
try {
    return resized_mixed(ctx, n_images, h_images, cosited, color, h_views,
                         ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, false, nullptr, nullptr, d_pixels, pixel_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                 jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return resized_mixed(ctx, n_images, h_images, cosited, color, h_views,
                         ResampleTarget{out_w, out_h, JPEG_AMD_FILTER_BILINEAR, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

// The six calls above with the filter chosen by the caller ("antialiased resample"): the same routes, the filter in the target.
int jpeg_amd_resize_filter_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter, uint8_t *d_dst,
                                 size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleTarget{out_w, out_h, filter, false, nullptr, nullptr, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_resize_filter_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return resize_images(ctx, n_images, d_src, src_stride, h_extents,
                         ResampleTarget{out_w, out_h, filter, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                         const int16_t *const d_coef[], const size_t coef_stride[],
                                         const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                         int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                         int32_t out_w, int32_t out_h, int filter, uint8_t *d_pixels, size_t pixel_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color, d_pixels, 0},
                            h_views, ResampleTarget{out_w, out_h, filter, false, nullptr, nullptr, d_pixels, pixel_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                        int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                        const uint8_t *h_flip, void *d_dst, size_t dst_stride)
try {
    return decode_resampled(ctx, DecodeCall{L, n_images, d_coef, coef_stride, d_quanta, quanta_stride, ntables, cosited, color,
                                            static_cast<uint8_t *>(d_dst), 0},
                            h_views, ResampleTarget{out_w, out_h, filter, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_resized_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                         jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                         int filter, uint8_t *d_pixels, size_t pixel_stride)
try {
    return resized_mixed(ctx, n_images, h_images, cosited, color, h_views,
                         ResampleTarget{out_w, out_h, filter, false, nullptr, nullptr, d_pixels, pixel_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_decode_tensor_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                        size_t dst_stride)
try {
    return resized_mixed(ctx, n_images, h_images, cosited, color, h_views,
                         ResampleTarget{out_w, out_h, filter, true, spec, h_flip, d_dst, dst_stride});
}
JA_NOTHROW_TAIL

int jpeg_amd_spectral_expand_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const uint32_t *d_desc,
                                   size_t desc_stride, const uint32_t *d_entries, size_t entries_stride, const uint8_t *d_skip,
                                   int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_desc || !d_entries || !d_coef || !coef_stride) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, true, &cs));
    JA_HIP(ctx, launch_expand_sparse(ctx->stream, n_images, *L, d_desc, desc_stride, d_entries, entries_stride, d_skip, cs));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_rectangular_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, uint16_t *d_rect, size_t rect_stride)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_planes_cover_image(L));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef || !coef_stride || !d_quanta || !d_rect) return JPEG_AMD_EINVAL;
    PlaneSet cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, true, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    if (generic_fused_supported(*L)) {
        JA_HIP(ctx, launch_generic_fused(ctx->stream, n_images, *L, cs, q, cosited != 0,
                                         ctx->d_walk ? ctx->d_walk + 16 : nullptr, d_rect, rect_stride));   // (dword 16: the 4:2:0 walk owns dword 0)
        return JPEG_AMD_OK;
    }
    return staged_decode(ctx, L, n_images, cs, q, cosited != 0, false, PixelKind::Rect16, d_rect, rect_stride * sizeof(uint16_t));
}

int jpeg_amd_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const int16_t *const d_coef[],
                                  const uint16_t *h_quanta, int ntables, int cosited, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_spectral_rectangular_batch(ctx, L, 1, d_coef, kOneImage, d_q, 0, ntables, cosited, d_rect, 0);
}

// ---- encode stages ----------------------------------------------------------------------

int jpeg_amd_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *d_pixels, size_t npixels,
                              int nplanes, jpeg_amd_color color, uint16_t *d_rect)
{
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    if (color != JPEG_AMD_COLOR_YCC8 && color != JPEG_AMD_COLOR_RGB8) return JPEG_AMD_EINVAL;
    if (npixels == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_pixels) return JPEG_AMD_EINVAL;
    JA_HIP(ctx, launch_pack(ctx->stream, d_pixels, npixels, nplanes, color, d_rect));
    return JPEG_AMD_OK;
}

int jpeg_amd_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                    const uint16_t *d_rect, uint16_t *const d_planes[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!d_rect || !d_planes) return JPEG_AMD_EINVAL;
    PlaneSetMut ps;
    JA_TRY(plane_set(L, d_planes, nullptr, false, &ps));
    JA_HIP(ctx, launch_decompose(ctx->stream, 1, *L, d_rect, 0, PixelKind::Rect16, ps));
    return JPEG_AMD_OK;
}

int jpeg_amd_fdct_plane(jpeg_amd_ctx *ctx, const uint16_t *d_plane, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision, int16_t *d_coef)
{
    JA_TRY(bind(ctx));
    if (units_x < 0 || units_y < 0 || precision < 1 || precision > 16) return JPEG_AMD_EINVAL;
    if ((long long)units_x * units_y > (1LL << 30)) return JPEG_AMD_EINVAL;
    if (units_x == 0 || units_y == 0) return JPEG_AMD_OK;
    if (!d_coef || !d_plane) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta_zigzag, 1, &d_q));
    JA_HIP(ctx, launch_fdct_plane(ctx->stream, 1, d_plane, 0, QuantaRef{d_q, 0}, 0, units_x,
                                  units_y, precision, d_coef, 0));
    return JPEG_AMD_OK;
}

int jpeg_amd_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                         const uint16_t *const d_planes[], const uint16_t *h_quanta, int ntables,
                         int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!d_coef || !d_planes) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    for (int p = 0; p < L->nplanes; ++p) {
        if (plane_samples(L, p) == 0) continue;
        if (!d_coef[p] || !d_planes[p]) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, launch_fdct_plane(ctx->stream, 1, d_planes[p], 0, QuantaRef{d_q, 0}, L->qi[p],
                                      L->units_x[p], L->units_y[p], L->precision, d_coef[p], 0));
    }
    return JPEG_AMD_OK;
}

int jpeg_amd_encode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images,
                          const uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_color color,
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    JA_TRY(check_batch8(L, n_images, color));
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef || !coef_stride || !d_quanta || !d_pixels) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, false, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    const bool rgb = color == JPEG_AMD_COLOR_RGB8;
    if (fused_encode_supported(*L)) {
        JA_HIP(ctx, launch_fused_encode(ctx->stream, n_images, *L, d_pixels, pixel_stride, rgb, q, cs));
        return JPEG_AMD_OK;
    }
    return staged_encode(ctx, L, n_images, d_pixels, pixel_stride, rgb ? PixelKind::RGB8 : PixelKind::YCC8, q, cs);
}

int jpeg_amd_rectangular_spectral_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, const uint16_t *d_rect,
                                        size_t rect_stride, const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int16_t *const d_coef[], const size_t coef_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_rect || !d_quanta || !d_coef || !coef_stride) return JPEG_AMD_EINVAL;
    PlaneSetMut cs;
    JA_TRY(plane_set(L, d_coef, coef_stride, false, &cs));
    const QuantaRef q{d_quanta, quanta_stride};
    if (generic_encode_supported(*L)) {
        JA_HIP(ctx, launch_generic_encode(ctx->stream, n_images, *L, d_rect, rect_stride, q, cs));
        return JPEG_AMD_OK;
    }
    return staged_encode(ctx, L, n_images, d_rect, rect_stride * sizeof(uint16_t), PixelKind::Rect16, q, cs);
}

int jpeg_amd_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint16_t *d_rect,
                                  const uint16_t *h_quanta, int ntables, int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_rectangular_spectral_batch(ctx, L, 1, d_rect, 0, d_q, 0, ntables, d_coef, kOneImage);
}

int jpeg_amd_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint8_t *d_pixels,
                    jpeg_amd_color color, const uint16_t *h_quanta, int ntables,
                    int16_t *const d_coef[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    return jpeg_amd_encode_batch(ctx, L, 1, d_pixels, 0, color, d_q, 0, ntables, d_coef, kOneImage);
}

// ---- host-buffer conveniences -------------------------------------------------------------

namespace {

// Small RAII bag of device buffers for the host wrappers: single buffers, or every plane of a layout (T: the 16-bit sample;
// a plane without samples gets the 16 bytes of an empty buffer and no copy).  (C++ linkage for the member templates.)
extern "C++" struct DeviceBag {
    jpeg_amd_ctx *ctx;
    std::vector<void *> ptrs;
    explicit DeviceBag(jpeg_amd_ctx *c) : ctx(c) {}
    ~DeviceBag()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : ptrs) (void)hipFree(p);
    }
    int alloc(size_t bytes, void **out)
    {
        *out = nullptr;
        if (bytes == 0) bytes = 16;
        const hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) { ctx->last_hip = (int)e; return JPEG_AMD_ENOMEM; }
        ptrs.push_back(*out);
        return JPEG_AMD_OK;
    }
    int upload(const void *h, size_t bytes, void **out)
    {
        JA_TRY(alloc(bytes, out));
        if (bytes == 0) return JPEG_AMD_OK;
        if (!h) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, hipMemcpyAsync(*out, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        return JPEG_AMD_OK;
    }
    int download(void *h, const void *d, size_t bytes)
    {
        if (bytes == 0) return JPEG_AMD_OK;
        if (!h) return JPEG_AMD_EINVAL;
        JA_HIP(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return JPEG_AMD_OK;
    }
    template <typename T>
    int alloc_planes(const jpeg_amd_layout *L, T *d[])
    {
        for (int p = 0; p < L->nplanes; ++p) JA_TRY(alloc(plane_samples(L, p) * sizeof(T), (void **)&d[p]));
        return JPEG_AMD_OK;
    }
    template <typename T>
    int upload_planes(const jpeg_amd_layout *L, const T *const h[], const T *d[])
    {
        for (int p = 0; p < L->nplanes; ++p) JA_TRY(upload(h[p], plane_samples(L, p) * sizeof(T), (void **)&d[p]));
        return JPEG_AMD_OK;
    }
    template <typename T>
    int download_planes(const jpeg_amd_layout *L, T *const h[], T *const d[])
    {
        for (int p = 0; p < L->nplanes; ++p) JA_TRY(download(h[p], d[p], plane_samples(L, p) * sizeof(T)));
        return JPEG_AMD_OK;
    }
    // the downloads have arrived in the caller's memory
    int finish()
    {
        JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return JPEG_AMD_OK;
    }
};

size_t rect_samples(const jpeg_amd_layout *L) { return (size_t)L->width * L->height * L->nplanes; }

}  // namespace

int jpeg_amd_host_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                const int16_t *const h_coef[], const uint16_t *h_quanta,
                                int ntables, uint16_t *const h_planes[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    JA_TRY(bag.alloc_planes(L, d_planes));
    JA_TRY(jpeg_amd_spectral_idct(ctx, L, d_coef, h_quanta, ntables, d_planes));
    JA_TRY(bag.download_planes(L, h_planes, d_planes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                     const uint16_t *const h_planes[], int cosited,
                                     uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!h_planes || !h_rect) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_planes, d_planes));
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.alloc(rect_samples(L) * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_planar_interleaved(ctx, L, d_planes, cosited, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, rect_samples(L) * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *h_rect, size_t npixels,
                                     int nplanes, jpeg_amd_color color, uint8_t *h_pixels)
try {
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_rect, npixels * nplanes * 2, (void **)&d_rect));
    JA_TRY(bag.alloc(npixels * 3, (void **)&d_px));
    JA_TRY(jpeg_amd_rectangular_unpack(ctx, d_rect, npixels, nplanes, color, d_px));
    JA_TRY(bag.download(h_pixels, d_px, npixels * 3));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                         const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                         int cosited, jpeg_amd_color color, uint8_t *h_pixels)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_pixels) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    uint8_t *d_px = nullptr;
    const size_t nbytes = (size_t)L->width * L->height * 3;
    JA_TRY(bag.alloc(nbytes, (void **)&d_px));
    JA_TRY(jpeg_amd_decode(ctx, L, d_coef, h_quanta, ntables, cosited, color, d_px));
    JA_TRY(bag.download(h_pixels, d_px, nbytes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                       const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                                       int cosited, uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_rect) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_coef, d_coef));
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.alloc(rect_samples(L) * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_spectral_rectangular(ctx, L, d_coef, h_quanta, ntables, cosited, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, rect_samples(L) * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint16_t *h_rect,
                                       const uint16_t *h_quanta, int ntables, int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_rect || !h_coef) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.upload(h_rect, rect_samples(L) * 2, (void **)&d_rect));
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_rectangular_spectral(ctx, L, d_rect, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *h_pixels, size_t npixels,
                                   int nplanes, jpeg_amd_color color, uint16_t *h_rect)
try {
    JA_TRY(bind(ctx));
    if (nplanes != 1 && nplanes != 3) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_pixels, npixels * 3, (void **)&d_px));
    JA_TRY(bag.alloc(npixels * nplanes * 2, (void **)&d_rect));
    JA_TRY(jpeg_amd_rectangular_pack(ctx, d_px, npixels, nplanes, color, d_rect));
    JA_TRY(bag.download(h_rect, d_rect, npixels * nplanes * 2));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                                         const uint16_t *h_rect, uint16_t *const h_planes[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, -1));
    if (!h_rect || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint16_t *d_rect = nullptr;
    JA_TRY(bag.upload(h_rect, rect_samples(L) * 2, (void **)&d_rect));
    uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_planes));
    JA_TRY(jpeg_amd_rectangular_decomposed(ctx, L, d_rect, d_planes));
    JA_TRY(bag.download_planes(L, h_planes, d_planes));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L,
                              const uint16_t *const h_planes[], const uint16_t *h_quanta,
                              int ntables, int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_planes) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    const uint16_t *d_planes[JPEG_AMD_MAX_PLANES] = {};
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.upload_planes(L, h_planes, d_planes));
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_planar_fdct(ctx, L, d_planes, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL

int jpeg_amd_host_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, const uint8_t *h_pixels,
                         jpeg_amd_color color, const uint16_t *h_quanta, int ntables,
                         int16_t *const h_coef[])
try {
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (!h_coef || !h_pixels) return JPEG_AMD_EINVAL;
    DeviceBag bag(ctx);
    uint8_t *d_px = nullptr;
    JA_TRY(bag.upload(h_pixels, (size_t)L->width * L->height * 3, (void **)&d_px));
    int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
    JA_TRY(bag.alloc_planes(L, d_coef));
    JA_TRY(jpeg_amd_encode(ctx, L, d_px, color, h_quanta, ntables, d_coef));
    JA_TRY(bag.download_planes(L, h_coef, d_coef));
    return bag.finish();
}
JA_NOTHROW_TAIL

// ---- JPEG bytes -> pixels (host entropy decode + the fused device path) ----------------------
int jpeg_amd_decompress(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int cosited,
                        jpeg_amd_color color, uint8_t *h_pixels, size_t pixel_capacity,
                        jpeg_amd_frame_info *info_out)
try {
    JA_TRY(bind(ctx));
    if (!h_jpeg) return JPEG_AMD_EINVAL;
    jpeg_amd_frame_info fi;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg, nbytes, &fi));
    if (info_out) *info_out = fi;
    // JPEG.Common recognises 8-bit images of arity 1 or 3 (jpeg.swift:357-424)
    if (fi.precision != 8 || (fi.ncomponents != 1 && fi.ncomponents != 3)) return JPEG_AMD_ENOSUP;
    const size_t need = (size_t)fi.width * fi.height * 3;
    if (!h_pixels || pixel_capacity < need) return JPEG_AMD_EINVAL;
    // a batch of one: pinned staging kept in the context, restart intervals and the copy-out on
    // host threads (their number left to the library)
    return jpeg_amd_decompress_batch(ctx, &h_jpeg, &nbytes, 1, 0, cosited, color, h_pixels, need, nullptr);
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
    std::vector<std::vector<int16_t>> planes((size_t)nc);
    int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) {
        planes[c].resize((size_t)64 * fi.units_x[c] * fi.units_y[c]);
        coef[c] = planes[c].data();
    }
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64];
    JA_TRY(jpeg_amd_jpeg_decode_spectral_mt(h_jpeg, nbytes, coef, quanta, &fi, nthreads));
    if (info_out) *info_out = fi;
    const jpeg_amd_layout L = layout_of_info(fi, np);
    return jpeg_amd_host_spectral_rectangular(ctx, &L, coef, &quanta[0][0], np, cosited, h_rect);
}
JA_NOTHROW_TAIL

// ---- many JPEG files of one geometry -> pixels: host threads entropy-decode a chunk into
//      pinned memory while the device (H2D, fused decode, D2H on the context's stream) works on
//      the previous chunk ----------------------------------------------------------------------
namespace {

// Files -> pixels, in host memory (h_pixels) or left on the device (d_pixels_out): see jpeg_amd_decompress_batch[_device].
int decompress_batch_impl(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                          int cosited, jpeg_amd_color color, uint8_t *h_pixels, uint8_t *d_pixels_out, size_t pixel_stride,
                          jpeg_amd_frame_info *info_out)
{
    JA_TRY(bind(ctx));
    if (!h_jpeg || !nbytes || (!h_pixels && !d_pixels_out) || n_images < 0) return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    if (!h_jpeg[0]) return JPEG_AMD_EINVAL;
    const bool to_host = h_pixels != nullptr;
    jpeg_amd_frame_info fi;
    JA_TRY(jpeg_amd_jpeg_inspect(h_jpeg[0], nbytes[0], &fi));
    if (info_out) *info_out = fi;
    if (fi.precision != 8 || (fi.ncomponents != 1 && fi.ncomponents != 3)) return JPEG_AMD_ENOSUP;
    const int nc = fi.ncomponents;
    const size_t npx = (size_t)fi.width * fi.height * 3;
    if (pixel_stride == 0) pixel_stride = npx;
    if (pixel_stride < npx) return JPEG_AMD_EINVAL;

    const jpeg_amd_layout L = layout_of_info(fi, nc);
    size_t plane[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) plane[c] = plane_samples(&L, c);
    const int chunk = std::min(n_images, 32);
    // Sequential files travel as SPARSE coefficients (jpeg_amd_jpeg_decode_sparse: a descriptor per block + an entry per
    // nonzero coefficient, an eighth of the planes for a typical file) and are expanded on the device; an image that does not
    // fit its arena, a progressive or a damaged one is decoded into planes and uploaded whole, like every image of a frame too
    // large for 32-bit descriptors (sparse_budget).
    const SparseBudget sb = sparse_budget(L);
    const size_t blocks = sb.blocks, arena = sb.arena, sparse_elems = sb.elems;
    // slot layout: [coef plane 0 x chunk][plane 1 x chunk][plane 2 x chunk] [quanta x chunk][skip flags][record offsets][records ...] [pixels x chunk]
    // The middle part goes up in ONE copy per chunk: the tables, the per-image flags, where each image's sparse record
    // [descriptors][entries in use] begins, and the records themselves, packed one behind the other in the order the threads
    // finish (a copy per image is 32 more commands per chunk, and every ~2 000 commands the runtime stops for 30 ms).
    size_t coef_off[JPEG_AMD_MAX_PLANES] = {}, off = 0;
    for (int c = 0; c < nc; ++c) { coef_off[c] = off; off += align256(plane[c] * 2 * chunk); }
    const size_t quanta_off = off;  off += align256((size_t)chunk * kQSlotElems * 2);
    const size_t skip_off = off;    off += align256((size_t)chunk);
    const size_t where_off = off;   off += align256((size_t)chunk * 8);
    const size_t sparse_off = off;  off += align256(sparse_elems * 4 * chunk);
    const size_t px_off = off;      off += to_host ? align256(npx * chunk) : 0;
    const size_t slot_bytes = off;
    JA_TRY(ensure_file_staging(ctx, slot_bytes));
    const bool auto_threads = nthreads <= 0;
    if (auto_threads) nthreads = default_host_threads();
    nthreads = std::max(1, nthreads);

    const int nchunks = (n_images + chunk - 1) / chunk;
    int result = JPEG_AMD_OK;
    // a caller whose pixel buffer is page-locked gets the download straight into it: no copy out of the pinned slot
    const bool direct_out = to_host && is_pinned_host(h_pixels, (size_t)(n_images - 1) * pixel_stride + npx);
    const bool copies_out = to_host && !direct_out;
    // Chunk k on its way back: its pixels are copied out of the pinned slot by the context's copy threads (pieces of <= 8 MiB, so
    // that one huge image is shared by the threads too) once the download is complete -- the first thread to get there waits for
    // it, the others for that thread.  begin_drain returns at once; end_drain waits (the calling thread copies too).
    WorkerPool *copiers = copies_out ? &pool_with(ctx->copiers, std::min(nthreads, 16) + 1) : nullptr;
    std::atomic<int> arrived{0};                             // 0: nobody has looked yet, 1: a thread is waiting, 2: the pixels are there, 3: failed
    bool draining = false;
    auto begin_drain = [&](int k) {
        const int slot = k & 1, base = k * chunk, m = std::min(chunk, n_images - base);
        const uint8_t *src = static_cast<const uint8_t *>(ctx->file_pinned[slot]) + px_off;
        const size_t piece = (size_t)8 << 20, per_image = (npx + piece - 1) / piece;
        arrived.store(0);
        draining = true;
        hipEvent_t done = ctx->file_done[slot];
        const int device = ctx->device;
        copiers->begin((int)(per_image * m), [=, &arrived](int j) {
            int zero = 0;
            if (arrived.compare_exchange_strong(zero, 1)) {
                (void)hipSetDevice(device);
                arrived.store(wait_event(done) == hipSuccess ? 2 : 3);
            }
            while (arrived.load() < 2) std::this_thread::sleep_for(std::chrono::microseconds(50));
            if (arrived.load() != 2) return;
            const size_t i = (size_t)j / per_image, lo = ((size_t)j % per_image) * piece, len = std::min(piece, npx - lo);
            std::memcpy(h_pixels + (size_t)(base + i) * pixel_stride + lo, src + npx * i + lo, len);
        }, std::min(nthreads, 16) + 1);
    };
    auto end_drain = [&]() -> int {
        if (!draining) return JPEG_AMD_OK;
        copiers->finish();
        draining = false;
        if (arrived.load() != 2) { ctx->last_hip = (int)hipErrorUnknown; return JPEG_AMD_EHIP; }
        return JPEG_AMD_OK;
    };
    struct DrainGuard { decltype(end_drain) &f; ~DrainGuard() { (void)f(); } } drain_guard{end_drain};   // joined on every way out
    // The entropy decoding: ONE queue of files for the whole call (FileQueue), decoded on t_n host threads beside this one, which
    // directs; this thread submits a chunk to the device as soon as its last file is in.  Chunk j is decoded into pinned slot
    // j & 1, which is free once the kernels of chunk j - 2 are done (its uploads read the slot's coefficient, sparse and table
    // regions; file_decoded[slot] is recorded behind them).  The helper thread that copies chunk j - 2's pixels out of the same
    // slot may still be running; it only reads the pixel region, which the decoders do not touch.
    std::atomic<size_t> packed_end[2];                       // per slot: elements of the records packed so far
    packed_end[0].store(0); packed_end[1].store(0);
    auto decode_file = [&](int file, std::vector<uint32_t> &record) -> int {
        const int k = file / chunk, i = file - k * chunk, slot = k & 1, m = std::min(chunk, n_images - k * chunk);
        char *host = static_cast<char *>(ctx->file_pinned[slot]);
        uint8_t *skip = reinterpret_cast<uint8_t *>(host + skip_off);
        // fewer files than threads: the spare threads go to the restart intervals of each file (planes: the sparse form
        // is written by one thread per file)
        const int inner = std::max(1, nthreads / m);
        int16_t *planes[JPEG_AMD_MAX_PLANES] = {};
        for (int c = 0; c < nc; ++c) planes[c] = reinterpret_cast<int16_t *>(host + coef_off[c]) + plane[c] * i;
        uint16_t(*quanta)[64] = reinterpret_cast<uint16_t(*)[64]>(host + quanta_off + (size_t)i * kQSlotElems * 2);
        jpeg_amd_frame_info f{};
        skip[i] = 1;
        if (!h_jpeg[file]) return JPEG_AMD_EINVAL;
        auto same_geometry = [&]() {                         // one geometry per batch: the buffers are sized for image 0
            bool same = f.width == fi.width && f.height == fi.height && f.precision == 8 && f.ncomponents == nc;
            for (int c = 0; same && c < nc; ++c)
                same = f.factor_x[c] == fi.factor_x[c] && f.factor_y[c] == fi.factor_y[c];
            return same;
        };
        int st = JPEG_AMD_OK;
        // Sparse first, without a look at the headers beforehand: the decoder itself refuses a frame with more blocks than the
        // descriptor array holds and never writes past the arena, so a file of another geometry is caught afterwards.
        // (spare threads only help a file that has restart intervals; such a file is decoded into planes on `inner` threads)
        bool sparse_done = false;
        if ((inner == 1 || fi.restart_interval == 0) && sb.ok) {
            if (record.size() < sparse_elems) record.resize(sparse_elems);      // (this thread's; kept in the context between calls, trimmed on the way out when huge)
            size_t n = 0;
            const int ss = jpeg_amd_jpeg_decode_sparse(h_jpeg[file], nbytes[file], record.data(), blocks, record.data() + blocks, arena, &n, quanta, &f);
            if (ss == JPEG_AMD_OK) {
                if (!same_geometry()) return JPEG_AMD_EINVAL;
                // the record goes behind the ones already in the slot (m records of at most sparse_elems always fit)
                const size_t at = packed_end[slot].fetch_add(blocks + n);
                std::memcpy(reinterpret_cast<uint32_t *>(host + sparse_off) + at, record.data(), (blocks + n) * 4);
                reinterpret_cast<uint64_t *>(host + where_off)[i] = at;
                skip[i] = 0;
                sparse_done = true;
            } else if (ss != JPEG_AMD_ENOSUP) {
                // (EINVAL may be "more blocks than image 0": the same verdict either way)
                return ss;
            }
        }
        if (!sparse_done) {
            st = jpeg_amd_jpeg_inspect(h_jpeg[file], nbytes[file], &f);
            if (st == JPEG_AMD_OK && !same_geometry()) st = JPEG_AMD_EINVAL;
        }
        if (st == JPEG_AMD_OK && skip[i])
            st = jpeg_amd_jpeg_decode_spectral_mt(h_jpeg[file], nbytes[file], planes, quanta, nullptr, inner > 1 && auto_threads ? 0 : inner);
        return st;
    };
    const int t_n = std::min(nthreads, n_images);
    // (the threads' sparse records stay in the context between calls -- a batch of 1080p files: 5 MB per thread -- unless huge)
    FileQueue queue(pool_with(ctx->workers, t_n + 1), ctx->records, n_images, chunk, t_n, [&](int file, std::vector<uint32_t> &record) {
        try { return decode_file(file, record); } catch (...) { return (int)JPEG_AMD_ENOMEM; }
    }, (size_t)16 << 20);
    for (int k = 0; k < nchunks && result == JPEG_AMD_OK; ++k) {
        const int slot = k & 1, base = k * chunk, m = std::min(chunk, n_images - base);
        char *host = static_cast<char *>(ctx->file_pinned[slot]);
        const uint8_t *skip = reinterpret_cast<const uint8_t *>(host + skip_off);
        // (like every failure inside this loop it leaves through the common tail below, which waits for both streams)
        // With threads, chunk k + 1 is opened while they are in chunk k: a thread that is through with chunk k goes straight on,
        // and this thread waits for chunk k - 1's kernels here, where it has nothing else to do.  Without, this thread decodes
        // chunk k itself (in wait(k)), in front of the chunk's submission.
        const int j = queue.threaded() ? k + 1 : k;
        if (j >= 2 && j < nchunks) {
            const hipError_t w = wait_event(ctx->file_decoded[j & 1]);
            if (w != hipSuccess) { ctx->last_hip = (int)w; result = JPEG_AMD_EHIP; break; }
            packed_end[j & 1].store(0);                       // (chunks 0 and 1 start from the initial zeros)
        }
        queue.open(std::min(j + 1, nchunks));
        result = queue.wait(k);
        { const int ds = end_drain(); if (ds != JPEG_AMD_OK) result = ds; }   // chunk k - 1 is out of its pinned slot: chunk k + 1's download may land there
        // (downloads that go straight into the caller's buffer are not waited for by a copy out: the device slot's pixels of
        // chunk k - 2 must have left before chunk k's kernels write there)
        if (result == JPEG_AMD_OK && direct_out && k >= 2) {
            const hipError_t w = wait_event(ctx->file_done[slot]);
            if (w != hipSuccess) { ctx->last_hip = (int)w; result = JPEG_AMD_EHIP; }
        }
        if (result != JPEG_AMD_OK) break;
        // the device side of chunk k (asynchronous); the host moves on to chunk k + 1 meanwhile.
        // Device slot `slot` was last read by the download of chunk k - 2, finished before drain(k - 2)
        // returned.  Upload + kernels on the context's stream, download on the second one.
        // (a failure in here leaves copies and kernels in flight: no early return, the common tail below waits for both streams)
        auto submit = [&]() -> int {
            char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * slot_bytes;
            int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
            for (int c = 0; c < nc; ++c) d_coef[c] = reinterpret_cast<int16_t *>(dev + coef_off[c]);
            bool any_sparse = false;
            for (int i = 0; i < m; ++i) {
                any_sparse = any_sparse || !skip[i];
                if (skip[i])                                 // planes, this image only (progressive, damaged, too dense)
                    for (int c = 0; c < nc; ++c)
                        JA_HIP(ctx, hipMemcpyAsync(dev + coef_off[c] + plane[c] * 2 * i, host + coef_off[c] + plane[c] * 2 * i, plane[c] * 2,
                                                   hipMemcpyHostToDevice, ctx->stream));
            }
            // tables, flags, record offsets and the packed records: one copy
            JA_HIP(ctx, hipMemcpyAsync(dev + quanta_off, host + quanta_off, sparse_off - quanta_off + packed_end[slot].load() * 4, hipMemcpyHostToDevice, ctx->stream));
            if (any_sparse) {
                PlaneSetMut cs{};
                for (int c = 0; c < nc; ++c) { cs.ptr[c] = d_coef[c]; cs.stride[c] = plane[c]; }
                JA_HIP(ctx, launch_expand_sparse(ctx->stream, m, L, reinterpret_cast<const uint32_t *>(dev + sparse_off), 0, nullptr, 0,
                                                 reinterpret_cast<const uint8_t *>(dev + skip_off), cs, reinterpret_cast<const uint64_t *>(dev + where_off)));
            }
            uint8_t *d_px = to_host ? reinterpret_cast<uint8_t *>(dev + px_off) : d_pixels_out + (size_t)base * pixel_stride;
            JA_TRY(jpeg_amd_decode_batch(ctx, &L, m, d_coef, plane, reinterpret_cast<const uint16_t *>(dev + quanta_off), kQSlotElems,
                                         JPEG_AMD_MAX_PLANES, cosited, color, d_px, to_host ? npx : pixel_stride));
            JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
            if (!to_host) {                                  // the pixels stay where they are: done when the kernels are
                JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->stream));
                return JPEG_AMD_OK;
            }
            JA_HIP(ctx, hipStreamWaitEvent(ctx->file_d2h, ctx->file_decoded[slot], 0));
            if (!direct_out) JA_HIP(ctx, hipMemcpyAsync(host + px_off, dev + px_off, npx * m, hipMemcpyDeviceToHost, ctx->file_d2h));
            else if (pixel_stride == npx) JA_HIP(ctx, hipMemcpyAsync(h_pixels + (size_t)base * npx, dev + px_off, npx * m, hipMemcpyDeviceToHost, ctx->file_d2h));
            else
                for (int i = 0; i < m; ++i)
                    JA_HIP(ctx, hipMemcpyAsync(h_pixels + (size_t)(base + i) * pixel_stride, dev + px_off + npx * i, npx, hipMemcpyDeviceToHost, ctx->file_d2h));
            JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->file_d2h));
            return JPEG_AMD_OK;
        };
        result = submit();
        if (result != JPEG_AMD_OK) break;
        // chunk k - 1 is copied out by the copy threads WHILE the others decode chunk k + 1; it has
        // to be finished before chunk k + 1 is submitted (its download lands in the same pinned slot)
        if (k >= 1 && copies_out) begin_drain(k - 1);
    }
    { const int ds = end_drain(); if (result == JPEG_AMD_OK) result = ds; }
    if (result != JPEG_AMD_OK) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->file_d2h); return result; }
    // the last chunk: wait for it (and for everything before it on the download stream), copy it out
    JA_HIP(ctx, wait_event(ctx->file_done[(nchunks - 1) & 1]));
    if (copies_out) { begin_drain(nchunks - 1); JA_TRY(end_drain()); }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_decompress_batch(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                              int n_images, int nthreads, int cosited, jpeg_amd_color color,
                              uint8_t *h_pixels, size_t pixel_stride, jpeg_amd_frame_info *info_out)
try {
    if (!h_pixels) return JPEG_AMD_EINVAL;
    return decompress_batch_impl(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_pixels, nullptr, pixel_stride, info_out);
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_batch_device(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                     int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                     uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *info_out)
try {
    if (!d_pixels) return JPEG_AMD_EINVAL;
    return decompress_batch_impl(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr, d_pixels, pixel_stride, info_out);
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
    // JPEG.Common: 8-bit, arity 1 or 3 (jpeg.swift:357-424)
    if (frame->precision != 8 || (nc != 1 && nc != 3)) return JPEG_AMD_ENOSUP;
    jpeg_amd_layout L;
    JA_TRY(layout_of_frame(frame, quanta_key, h_quanta_keys, ntables, &L));
    std::vector<std::vector<int16_t>> planes((size_t)nc);
    int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) {
        planes[c].resize(plane_samples(&L, c));
        coef[c] = planes[c].data();
    }
    JA_TRY(jpeg_amd_host_encode(ctx, &L, h_pixels, color, h_quanta, ntables, coef));
    return jpeg_amd_jpeg_encode_spectral(frame, quanta_key, coef, h_quanta, h_quanta_keys, ntables, scans, nscans,
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
    std::vector<std::vector<int16_t>> planes((size_t)nc);
    int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) {
        planes[c].resize(plane_samples(&L, c));
        coef[c] = planes[c].data();
    }
    JA_TRY(jpeg_amd_host_rectangular_spectral(ctx, &L, h_rect, h_quanta, ntables, coef));
    return jpeg_amd_jpeg_encode_spectral(frame, quanta_key, coef, h_quanta, h_quanta_keys, ntables, scans, nscans,
                                         metadata, nmetadata, h_out, capacity, nbytes);
}
JA_NOTHROW_TAIL

// ---- many pictures of one geometry -> JPEG files: one fused encode launch per chunk, the host
//      threads entropy-code the planes of a chunk as soon as they are back ------------------------
namespace {

// Pixels -> files; the pixels in host memory (h_pixels) or already on the device (d_pixels_in): jpeg_amd_compress_batch[_device].
int compress_batch_impl(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels, const uint8_t *d_pixels_in,
                        size_t pixel_stride, int n_images, jpeg_amd_color color,
                        const int32_t *quanta_key, const uint16_t *h_quanta, const int32_t *h_quanta_keys,
                        int ntables, const jpeg_amd_scan *scans, int nscans,
                        const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                        uint8_t *h_out, size_t out_stride, size_t nbytes[])
{
    JA_TRY(bind(ctx));
    const bool on_device = d_pixels_in != nullptr;
    if (!frame || (!h_pixels && !on_device) || !quanta_key || !h_quanta || !h_quanta_keys || !scans || !h_out || !nbytes || n_images < 0)
        return JPEG_AMD_EINVAL;
    if (n_images == 0) return JPEG_AMD_OK;
    const int nc = frame->ncomponents;
    if (frame->precision != 8 || (nc != 1 && nc != 3)) return JPEG_AMD_ENOSUP;
    const size_t npx = (size_t)frame->width * frame->height * 3;
    if (pixel_stride == 0) pixel_stride = npx;
    if (pixel_stride < npx) return JPEG_AMD_EINVAL;
    jpeg_amd_layout L;
    JA_TRY(layout_of_frame(frame, quanta_key, h_quanta_keys, ntables, &L));
    size_t plane[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) plane[c] = plane_samples(&L, c);
    const int chunk = std::min(n_images, 32);
    if (nthreads <= 0) nthreads = default_host_threads();
    nthreads = std::max(1, nthreads);

    const uint16_t *d_q = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    // Sequential scans: the coefficients come down as SPARSE entries (k_sparsify: a descriptor per block + an entry per
    // nonzero coefficient, an eighth of the planes for a typical picture) and go to the writer in that form
    // (jpeg_amd_jpeg_encode_sparse); a picture whose entries do not fit its arena comes down as planes, like every picture of a
    // progressive frame, or of a frame too large for 32-bit descriptors (sparse_budget).
    const SparseBudget sb = sparse_budget(L);
    const size_t blocks = sb.blocks, arena = sb.arena, sparse_elems = sb.elems;
    const bool sparse_down = frame->process != 2 && sb.ok;
    // slot layout (pinned and device alike): [pixels x chunk][coef plane 0 x chunk][plane 1 x chunk][plane 2 x chunk][sparse x chunk][counts]
    size_t coef_off[JPEG_AMD_MAX_PLANES] = {};
    size_t off = align256(npx * chunk);
    for (int c = 0; c < nc; ++c) { coef_off[c] = off; off += align256(plane[c] * 2 * chunk); }
    const size_t sparse_off = off;  off += sparse_down ? align256(sparse_elems * 4 * chunk) : 0;
    const size_t count_off = off;   off += align256((size_t)chunk * 4);
    const size_t slot_bytes = off;
    JA_TRY(ensure_file_staging(ctx, slot_bytes));

    const int nchunks = (n_images + chunk - 1) / chunk;
    // a caller whose pixels are page-locked gets them uploaded from where they are: nothing to stage
    const bool direct_in = on_device || is_pinned_host(h_pixels, (size_t)(n_images - 1) * pixel_stride + npx);
    const size_t piece = (size_t)4 << 20, per_image = (npx + piece - 1) / piece;   // pixels are staged in pieces of <= 4 MiB
    // The device side of chunk k, asynchronous: pixels up and kernels on the context's stream; on the second stream, behind
    // them, the first stage of the download -- the entry counts (or, for a progressive frame, the planes).  Device slot and
    // pinned slot k & 1 were last used by chunk k - 2, whose download was waited for before its files were written.
    auto submit = [&](int k) -> int {
        const int slot = k & 1, m = std::min(chunk, n_images - k * chunk);
        char *host = static_cast<char *>(ctx->file_pinned[slot]);
        char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * slot_bytes;
        int16_t *d_coef[JPEG_AMD_MAX_PLANES] = {};
        for (int c = 0; c < nc; ++c) d_coef[c] = reinterpret_cast<int16_t *>(dev + coef_off[c]);
        const uint8_t *d_px = reinterpret_cast<const uint8_t *>(dev);
        size_t d_px_stride = npx;
        if (on_device) { d_px = d_pixels_in + (size_t)k * chunk * pixel_stride; d_px_stride = pixel_stride; }   // encoded where they are
        else if (!direct_in) JA_HIP(ctx, hipMemcpyAsync(dev, host, npx * m, hipMemcpyHostToDevice, ctx->stream));
        else if (pixel_stride == npx) JA_HIP(ctx, hipMemcpyAsync(dev, h_pixels + (size_t)k * chunk * npx, npx * m, hipMemcpyHostToDevice, ctx->stream));
        else
            for (int i = 0; i < m; ++i)
                JA_HIP(ctx, hipMemcpyAsync(dev + npx * i, h_pixels + ((size_t)k * chunk + i) * pixel_stride, npx, hipMemcpyHostToDevice, ctx->stream));
        JA_TRY(jpeg_amd_encode_batch(ctx, &L, m, d_px, d_px_stride, color, d_q, 0, ntables, d_coef, plane));
        if (sparse_down) {
            PlaneSet cs{};
            for (int c = 0; c < nc; ++c) { cs.ptr[c] = d_coef[c]; cs.stride[c] = plane[c]; }
            uint32_t *sp = reinterpret_cast<uint32_t *>(dev + sparse_off);
            JA_HIP(ctx, launch_sparsify(ctx->stream, m, L, cs, sp, sparse_elems, sp + blocks, sparse_elems, (uint32_t)arena,
                                        reinterpret_cast<uint32_t *>(dev + count_off)));
        }
        JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
        JA_HIP(ctx, hipStreamWaitEvent(ctx->file_d2h, ctx->file_decoded[slot], 0));
        if (sparse_down) JA_HIP(ctx, hipMemcpyAsync(host + count_off, dev + count_off, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->file_d2h));
        else
            for (int c = 0; c < nc; ++c)
                JA_HIP(ctx, hipMemcpyAsync(host + coef_off[c], dev + coef_off[c], plane[c] * 2 * m, hipMemcpyDeviceToHost, ctx->file_d2h));
        JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->file_d2h));
        return JPEG_AMD_OK;
    };
    // The second stage of chunk k's download, once its counts are in: per picture the descriptors and the entries in use --
    // or its planes, where the entries did not fit.  Issued BEFORE chunk k + 1 is submitted, so that it does not queue up
    // behind that chunk's kernels on the download stream.
    auto fetch = [&](int k) -> int {
        const int slot = k & 1, m = std::min(chunk, n_images - k * chunk);
        char *host = static_cast<char *>(ctx->file_pinned[slot]);
        char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * slot_bytes;
        if (sparse_down) {
            JA_HIP(ctx, wait_event(ctx->file_done[slot]));
            const uint32_t *count = reinterpret_cast<const uint32_t *>(host + count_off);
            for (int i = 0; i < m; ++i) {
                if (count[i] <= arena) {
                    const size_t at = sparse_off + sparse_elems * 4 * (size_t)i;
                    JA_HIP(ctx, hipMemcpyAsync(host + at, dev + at, (blocks + count[i]) * 4, hipMemcpyDeviceToHost, ctx->file_d2h));
                } else {
                    for (int c = 0; c < nc; ++c)
                        JA_HIP(ctx, hipMemcpyAsync(host + coef_off[c] + plane[c] * 2 * i, dev + coef_off[c] + plane[c] * 2 * i, plane[c] * 2,
                                                   hipMemcpyDeviceToHost, ctx->file_d2h));
                }
            }
        }
        JA_HIP(ctx, hipEventRecord(ctx->file_fetched[slot], ctx->file_d2h));
        return JPEG_AMD_OK;
    };
    // One parallel region of the host threads: the files of chunk `code` are written from what came down into its pinned slot
    // (code >= 0) and the pixels of chunk `stage` are copied into its pinned slot (stage < nchunks).  The caller's pixels
    // are pageable memory: copying them to pinned memory on all threads and uploading from there is what keeps the upload
    // asynchronous and at the speed of the link.
    WorkerPool &pool = pool_with(ctx->workers, std::min(nthreads, 2 * chunk));   // (kept in the context between calls)
    struct Finish { WorkerPool &p; ~Finish() { p.finish(); } } finish_on_exit{pool};
    auto host_region = [&](int code, int stage, int fetch_chunk) -> int {
        int m_code = 0, m_stage = 0;
        const char *down = nullptr;
        char *stage_host = nullptr;
        if (code >= 0) {
            m_code = std::min(chunk, n_images - code * chunk);
            JA_HIP(ctx, wait_event(ctx->file_fetched[code & 1]));
            down = static_cast<const char *>(ctx->file_pinned[code & 1]);
        }
        if (stage < nchunks && !direct_in) {
            m_stage = std::min(chunk, n_images - stage * chunk);
            stage_host = static_cast<char *>(ctx->file_pinned[stage & 1]);   // (its last upload, chunk stage - 2, is long complete)
        }
        std::vector<int> status((size_t)std::max(m_code, 1), JPEG_AMD_OK);
        const int copies = (int)(per_image * (size_t)m_stage);
        pool.begin(m_code + copies, [&](int j) {
            if (j < m_code) {
                const size_t image = (size_t)code * chunk + (size_t)j;
                const uint32_t count = sparse_down ? reinterpret_cast<const uint32_t *>(down + count_off)[j] : 0;
                if (sparse_down && count <= arena) {
                    const uint32_t *sp = reinterpret_cast<const uint32_t *>(down + sparse_off) + sparse_elems * (size_t)j;
                    status[(size_t)j] = jpeg_amd_jpeg_encode_sparse(frame, quanta_key, sp, sp + blocks, count, h_quanta, h_quanta_keys, ntables, scans,
                                                                    nscans, metadata, nmetadata, h_out + image * out_stride, out_stride, &nbytes[image]);
                } else {
                    const int16_t *planes[JPEG_AMD_MAX_PLANES] = {};
                    for (int c = 0; c < nc; ++c) planes[c] = reinterpret_cast<const int16_t *>(down + coef_off[c]) + plane[c] * j;
                    status[(size_t)j] = jpeg_amd_jpeg_encode_spectral(frame, quanta_key, planes, h_quanta, h_quanta_keys, ntables, scans, nscans,
                                                                      metadata, nmetadata, h_out + image * out_stride, out_stride, &nbytes[image]);
                }
            } else {
                const size_t q = (size_t)(j - m_code), i = q / per_image, lo = (q % per_image) * piece, len = std::min(piece, npx - lo);
                std::memcpy(stage_host + npx * i + lo, h_pixels + ((size_t)stage * chunk + i) * pixel_stride + lo, len);
            }
        }, nthreads);
        // while the other threads are at it, this one waits for the kernels of the chunk on the device and starts the second
        // stage of its download, which then runs beside the rest of the region
        const int fetched_status = fetch_chunk >= 0 ? fetch(fetch_chunk) : JPEG_AMD_OK;
        pool.finish();
        if (fetched_status != JPEG_AMD_OK) return fetched_status;
        for (int st : status) if (st != JPEG_AMD_OK) return st;   // EINVAL with nbytes[i] > out_stride: buffer too small
        return JPEG_AMD_OK;
    };
    int result = host_region(-1, 0, -1);
    if (result == JPEG_AMD_OK) result = submit(0);
    for (int k = 0; k < nchunks && result == JPEG_AMD_OK; ++k) {
        result = host_region(k - 1, k + 1, k);                    // ... while the device works on chunk k
        if (result == JPEG_AMD_OK && k + 1 < nchunks) result = submit(k + 1);
    }
    if (result == JPEG_AMD_OK) result = host_region(nchunks - 1, nchunks, -1);
    if (result != JPEG_AMD_OK) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->file_d2h); }
    return result;
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
    return compress_batch_impl(ctx, frame, h_pixels, nullptr, pixel_stride, n_images, color, quanta_key, h_quanta, h_quanta_keys, ntables,
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
    return compress_batch_impl(ctx, frame, nullptr, d_pixels, pixel_stride, n_images, color, quanta_key, h_quanta, h_quanta_keys, ntables,
                               scans, nscans, metadata, nmetadata, nthreads, h_out, out_stride, nbytes);
}
JA_NOTHROW_TAIL

// ---- lossless spectral transforms: rotate, flip, crop, requantise (examples/rotate, examples/recompress) ------------------
namespace {

// whether the op mirrors the SOURCE's x / y axis (FLIP_H / FLIP_V act in the output frame, after the transpose)
bool mirrors_source_x(int op) { return (op & JPEG_AMD_XFORM_TRANSPOSE) ? (op & JPEG_AMD_XFORM_FLIP_V) : (op & JPEG_AMD_XFORM_FLIP_H); }
bool mirrors_source_y(int op) { return (op & JPEG_AMD_XFORM_TRANSPOSE) ? (op & JPEG_AMD_XFORM_FLIP_H) : (op & JPEG_AMD_XFORM_FLIP_V); }

// The output layout and, per plane, the region's origin in that plane's blocks.
struct TransformPlan {
    jpeg_amd_layout out;
    int ox[JPEG_AMD_MAX_PLANES], oy[JPEG_AMD_MAX_PLANES];
};

int plan_transform(const jpeg_amd_layout *in, int op, const jpeg_amd_region *region, TransformPlan *tp)
{
    JA_TRY(check_layout(in, -1));
    if (op < 0 || op > 7) return JPEG_AMD_EINVAL;
    const jpeg_amd_region r = region ? *region : jpeg_amd_region{0, 0, in->width, in->height};
    const int mx = 8 * in->scale_x, my = 8 * in->scale_y;
    if (r.x < 0 || r.y < 0 || r.x >= in->width || r.y >= in->height || r.x % mx || r.y % my) return JPEG_AMD_EINVAL;
    if (r.width <= 0 || r.height <= 0) return JPEG_AMD_EINVAL;
    // Spectral.set(width:) / set(height:) from the region's origin, then the example's trim of the edges that the op moves
    // to the top or left (examples/rotate/main.swift: set(width: size.x - size.x % (8 * scale.x)))
    jpeg_amd_layout c = *in;
    c.width = r.width;
    c.height = r.height;
    if (mirrors_source_x(op)) c.width -= c.width % mx;
    if (mirrors_source_y(op)) c.height -= c.height % my;
    if (c.width <= 0 || c.height <= 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout o = c;
    if (op & JPEG_AMD_XFORM_TRANSPOSE) {
        o.width = c.height; o.height = c.width;
        o.scale_x = c.scale_y; o.scale_y = c.scale_x;
        for (int p = 0; p < c.nplanes; ++p) { o.factor_x[p] = c.factor_y[p]; o.factor_y[p] = c.factor_x[p]; }
    }
    JA_TRY(jpeg_amd_layout_units(&o));
    for (int p = 0; p < c.nplanes; ++p) {
        if ((long long)o.units_x[p] * o.units_y[p] > (1LL << 30)) return JPEG_AMD_EINVAL;
        tp->ox[p] = r.x / mx * in->factor_x[p];
        tp->oy[p] = r.y / my * in->factor_y[p];
    }
    tp->out = o;
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd_transform_layout(const jpeg_amd_layout *in, int op, const jpeg_amd_region *region, jpeg_amd_layout *out)
{
    if (!in || !out) return JPEG_AMD_EINVAL;
    TransformPlan tp;
    JA_TRY(plan_transform(in, op, region, &tp));
    *out = tp.out;
    return JPEG_AMD_OK;
}

int jpeg_amd_transform_quanta(int op, const uint16_t in[64], uint16_t out[64])
{
    if (!in || !out || op < 0 || op > 7) return JPEG_AMD_EINVAL;
    uint16_t t[64];
    for (int z = 0; z < 64; ++z) t[z] = in[xform_source(op, z)];
    std::memcpy(out, t, sizeof t);
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_transform_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, int op,
                                      const jpeg_amd_region *region, const int16_t *const d_coef_in[], const size_t in_stride[],
                                      const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                      const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[],
                                      int32_t *d_overflow)
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, d_quanta_out ? ntables : -1));
    if (d_quanta_out && (ntables < 1 || ntables > JPEG_AMD_MAX_PLANES)) return JPEG_AMD_EINVAL;
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    TransformPlan tp;
    JA_TRY(plan_transform(L, op, region, &tp));
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef_in || !in_stride || !d_coef_out || !out_stride || (d_quanta_out && !d_quanta)) return JPEG_AMD_EINVAL;
    PlaneSet cin;
    PlaneSetMut cout;
    JA_TRY(plane_set(L, d_coef_in, in_stride, false, &cin));
    JA_TRY(plane_set(L, d_coef_out, out_stride, true, &cout));
    JA_HIP(ctx, launch_transform(ctx->stream, n_images, op, *L, tp.out, tp.ox, tp.oy, cin, QuantaRef{d_quanta, quanta_stride},
                                 d_quanta_out, cout, d_overflow));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_transform(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int op, const jpeg_amd_region *region,
                                const int16_t *const d_coef_in[], const uint16_t *h_quanta, int ntables,
                                const uint16_t *h_quanta_out, int16_t *const d_coef_out[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    const uint16_t *d_q = nullptr, *d_qo = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    if (h_quanta_out) JA_TRY(stage_quanta(ctx, h_quanta_out, ntables, &d_qo));
    if (!ctx->d_flag) JA_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_flag), 256));
    JA_HIP(ctx, hipMemsetAsync(ctx->d_flag, 0, sizeof(int32_t), ctx->stream));
    JA_TRY(jpeg_amd_spectral_transform_batch(ctx, L, 1, op, region, d_coef_in, kOneImage, d_q, 0, ntables, d_qo, d_coef_out, kOneImage,
                                             ctx->d_flag));
    int32_t flag = 0;
    JA_HIP(ctx, hipMemcpyAsync(&flag, ctx->d_flag, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return flag ? JPEG_AMD_EINVAL : JPEG_AMD_OK;
}

// ---- file to file in the coefficient domain: what jpeg_amd_transform and jpeg_amd_reduce share ---------------------------
namespace {
extern "C++" {

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
    std::vector<std::vector<int16_t>> planes((size_t)nc);
    int16_t *coef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) {
        planes[c].resize((size_t)64 * fi.units_x[c] * fi.units_y[c]);
        coef[c] = planes[c].data();
    }
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64];
    JA_TRY(jpeg_amd_jpeg_decode_spectral_mt(h_jpeg, nbytes, coef, quanta, &fi, nthreads));
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
    std::vector<std::vector<int16_t>> outp((size_t)nc);
    int16_t *ocoef[JPEG_AMD_MAX_PLANES] = {};
    for (int c = 0; c < nc; ++c) {
        outp[c].resize(plane_samples(&O, c));
        ocoef[c] = outp[c].data();
    }
    {
        DeviceBag bag(ctx);
        const int16_t *d_in[JPEG_AMD_MAX_PLANES] = {};
        int16_t *d_out[JPEG_AMD_MAX_PLANES] = {};
        JA_TRY(bag.upload_planes<int16_t>(&L, coef, d_in));
        JA_TRY(bag.alloc_planes(&O, d_out));
        JA_TRY(device(L, d_in, &quanta[0][0], nc, d_out));
        JA_TRY(bag.download_planes(&O, ocoef, d_out));
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
    return jpeg_amd_jpeg_encode_spectral(&of, keys, ocoef, tables.data(), tkeys.data(), (int)tkeys.size(), scans.data(), nscans,
                                         meta.data(), nmeta, h_out, capacity, nbytes_out);
}

}  // extern "C++"
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

// ---- spectral reduce: 1/2, 1/4, 1/8 size, coefficients in and out (include/jpeg_amd.h, "spectral reduce") ---------------
namespace {

// N = 8 / denom for a denom of the reduce contract, else 0.
int reduce_n(int denom) { return denom == 2 || denom == 4 || denom == 8 ? 8 / denom : 0; }

// A zero divisor among the tables the planes of L use.
bool has_zero_quantum(const jpeg_amd_layout *L, const uint16_t *h_tables)
{
    for (int p = 0; p < L->nplanes; ++p)
        for (int z = 0; z < 64; ++z)
            if (h_tables[64 * L->qi[p] + z] == 0) return true;
    return false;
}

}  // namespace

int jpeg_amd_reduce_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out)
{
    if (!out) return JPEG_AMD_EINVAL;
    JA_TRY(check_layout(in, -1));
    const int n = reduce_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout r = *in;
    r.width = (int32_t)(((long long)in->width * n + 7) / 8);
    r.height = (int32_t)(((long long)in->height * n + 7) / 8);
    JA_TRY(jpeg_amd_layout_units(&r));
    *out = r;
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_reduce_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, int denom,
                                   const int16_t *const d_coef_in[], const size_t in_stride[],
                                   const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                   const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    const int n = reduce_n(denom);
    if (n == 0) return JPEG_AMD_EINVAL;
    jpeg_amd_layout O;
    JA_TRY(jpeg_amd_reduce_layout(L, denom, &O));
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) == 0) return JPEG_AMD_EINVAL;      // no block whose edge could be replicated
    if (n_images == 0) return JPEG_AMD_OK;
    if (!d_coef_in || !in_stride || !d_coef_out || !out_stride || !d_quanta) return JPEG_AMD_EINVAL;
    PlaneSet cin;
    PlaneSetMut cout;
    JA_TRY(plane_set(L, d_coef_in, in_stride, true, &cin));
    JA_TRY(plane_set(L, d_coef_out, out_stride, true, &cout));
    for (int p = 0; p < L->nplanes; ++p) {
        if (n_images > 1 && out_stride[p] < plane_samples(&O, p)) return JPEG_AMD_EINVAL;      // the images' outputs would overlap
        // the kernel loads and stores 16-byte pieces: every block of every image starts on a 16-byte boundary
        if (reinterpret_cast<uintptr_t>(d_coef_in[p]) % 16 || reinterpret_cast<uintptr_t>(d_coef_out[p]) % 16) return JPEG_AMD_EINVAL;
        if (n_images > 1 && (in_stride[p] % 8 || out_stride[p] % 8)) return JPEG_AMD_EINVAL;
    }
    JA_HIP(ctx, launch_spectral_reduce(ctx->stream, n_images, n, *L, O, cin, QuantaRef{d_quanta, quanta_stride}, d_quanta_out, cout));
    return JPEG_AMD_OK;
}

int jpeg_amd_spectral_reduce(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int denom, const int16_t *const d_coef_in[],
                             const uint16_t *h_quanta, int ntables, const uint16_t *h_quanta_out, int16_t *const d_coef_out[])
{
    JA_TRY(bind(ctx));
    JA_TRY(check_layout(L, ntables));
    if (reduce_n(denom) == 0 || !h_quanta || ntables < 1 || ntables > JPEG_AMD_MAX_PLANES) return JPEG_AMD_EINVAL;
    if (has_zero_quantum(L, h_quanta_out ? h_quanta_out : h_quanta)) return JPEG_AMD_EINVAL;
    if (!d_coef_in || !d_coef_out) return JPEG_AMD_EINVAL;
    for (int p = 0; p < L->nplanes; ++p)
        if (plane_samples(L, p) == 0 || !d_coef_in[p] || !d_coef_out[p]) return JPEG_AMD_EINVAL;
    const uint16_t *d_q = nullptr, *d_qo = nullptr;
    JA_TRY(stage_quanta(ctx, h_quanta, ntables, &d_q));
    if (h_quanta_out) JA_TRY(stage_quanta(ctx, h_quanta_out, ntables, &d_qo));
    JA_TRY(jpeg_amd_spectral_reduce_batch(ctx, L, 1, denom, d_coef_in, kOneImage, d_q, 0, ntables, d_qo, d_coef_out, kOneImage));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JPEG_AMD_OK;
}

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

}  // extern "C"
