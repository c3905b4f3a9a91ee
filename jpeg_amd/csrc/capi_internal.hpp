// capi_internal.hpp -- what the units of the C layer (capi*.hip) share: the context, the status macros, the layout checks,
// the argument record of the batch decodes and the buffer and staging helpers.  The helpers are defined in capi.hip.  The
// request record of the resample calls, and the two internal routes that take it, are in resample_request.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <chrono>
#include <system_error>
#include <thread>
#include <vector>

#include "interleave.hpp"
#include "interval_plan.hpp"
#include "kernels.hpp"
#include "resample_request.hpp"
#include "sparse_format.hpp"
#include "transform.hpp"
#include "worker_pool.hpp"

// Device memory a context keeps between calls and grows on demand (ensure_buffer).
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
};

struct jpeg_amd_ctx {
    int device = 0;
    int flags = 0;                 // jpeg_amd_ctx_create's
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
    // jpeg_amd_encode_tensor_batch: the bytes of a chunk, between the front launch and the encoder.  A buffer of its own: the
    // staged encode behind it regrows `scratch`.
    DeviceBuffer tensor_px;
    // jpeg_amd_spectral_expand_mixed: the item records and workgroup prefix of its launch.  A buffer of its own: the mixed
    // call that follows an expand rewrites `mixed`.
    DeviceBuffer expand;
    // the file calls to tensors (capi_files.hip): the coefficient planes of a chunk's files.  Only the heads of the blocks of
    // the views' windows are ever written: nothing else of it may be read.
    DeviceBuffer file_planes;
    // jpeg_amd_jpeg_decode_spectral_device and the batch file paths under JPEG_AMD_CTX_DEVICE_ENTROPY: the files' records and
    // blocks of a launch of k_huffman_intervals, and its statuses.
    DeviceBuffer entropy;
    int64_t device_entropy_files = 0;   // files whose entropy decoding ran on the device, since the context was made
    hipEvent_t entropy_ev[2] = {nullptr, nullptr};   // around every launch of k_huffman_intervals (made on first use)
    double device_entropy_kernel_ms = 0;              // their sum
    int qslot = 0;
    int last_hip = 0;
    // staging of the batch file paths (jpeg_amd_decompress_batch, jpeg_amd_decompress_tensor_mixed, jpeg_amd_compress_batch), kept
    // between calls: two pinned host slots (the host threads work in one while the device works from / into the other) and two
    // device slots.  The decodes run worker_pool.hpp's ChunkLoop over it (below, "the batch file paths"); the encode has its own loop.
    void *file_pinned[2] = {nullptr, nullptr};
    void *file_device = nullptr;                      // both device slots
    size_t file_pinned_bytes = 0, file_device_bytes = 0;
    hipEvent_t file_done[2] = {nullptr, nullptr};     // chunk's pixels are where the call leaves them (decode) / first stage of its download is back (encode)
    hipEvent_t file_decoded[2] = {nullptr, nullptr};  // chunk's kernels are done (device -> host copy may start)
    hipEvent_t file_fetched[2] = {nullptr, nullptr};  // encode: the second stage of the chunk's download is back
    hipStream_t file_d2h = nullptr;                   // downloads overlap the next chunk's uploads (full-duplex PCIe)
    std::unique_ptr<jpeg_amd::WorkerPool> workers, copiers;   // host threads of the batch file paths: entropy coding; copies out of the pinned slots
    std::vector<std::vector<uint32_t>> records;       // a sparse record per entropy-decoding thread
};

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

namespace jpeg_amd {
namespace capi {

constexpr int kQSlots = 32;                                   // staged table sets in flight
constexpr size_t kQSlotElems = JPEG_AMD_MAX_PLANES * 64;      // uint16 per slot

// The single-image forms are their batch forms with one image, staged tables and these strides.
constexpr size_t kOneImage[JPEG_AMD_MAX_PLANES] = {0, 0, 0, 0};

int bind(jpeg_amd_ctx *ctx);
int check_layout(const jpeg_amd_layout *L, int ntables);
int check_planes_cover_image(const jpeg_amd_layout *L);
int check_batch8(const jpeg_amd_layout *L, int n_images, jpeg_amd_color color);
size_t plane_samples(const jpeg_amd_layout *L, int p);
int ensure_buffer(jpeg_amd_ctx *ctx, DeviceBuffer &buf, size_t bytes);
int stage_quanta(jpeg_amd_ctx *ctx, const uint16_t *h_quanta, int ntables, const uint16_t **d_out);
size_t align256(size_t n);
size_t scratch_planes_bytes(const jpeg_amd_layout *L, int n_images, size_t sample_bytes);
int scratch_planes(jpeg_amd_ctx *ctx, const jpeg_amd_layout *L, int n_images, size_t sample_bytes, PlaneSetMut *ps);
jpeg_amd_layout layout_of_info(const jpeg_amd_frame_info &fi, int nplanes);
int layout_of_frame(jpeg_amd_frame_info *frame, const int32_t *quanta_key, const int32_t *h_quanta_keys, int ntables,
                    jpeg_amd_layout *L);
int reduce_n(int denom);   // (capi_spectral.hip)
// What the calls that take a tensor source require of it, beyond jpeg_amd_tensor_source_extent (capi_tensor.hip).
int check_tensor_source(int n_images, const void *d_src, size_t src_stride, int32_t w, int32_t h,
                        const jpeg_amd_tensor_source *src, size_t *elem_bytes);

// What the calls that take or write a sparse record require of a frame's block count, summed in 64 bits: descriptors are
// 32-bit indices, and one value means no block.
inline int check_sparse_blocks(const jpeg_amd_layout &L)
{
    return sparse_budget(L).blocks >= sparse::kAbsent ? JPEG_AMD_EINVAL : JPEG_AMD_OK;
}
// k_sparsify's per-image cursor is a uint32 that takes up to 64 entries per block, fitting or not: only below 2^26 blocks is
// the count it leaves the image's entry count.
inline bool sparsify_count_fits(size_t blocks) { return 64 * (uint64_t)blocks < ((uint64_t)1 << 32); }

// What jpeg_amd_spectral_expand_mixed requires of one item; *groups: the workgroups it takes (capi.hip).
int check_expand_item(const jpeg_amd_expand_item &item, uint64_t *groups);
// (check_resampled_mixed and decode_views_mixed, what the file calls use of the mixed resample calls: resample_request.hpp)
// "colour stage": what the contract requires of a call's colour, judged with the target.
inline int check_colour(const jpeg_amd_colour &c, int n_images)
{
    if (std::isnan(c.lo) || std::isnan(c.hi) || c.lo > c.hi) return JPEG_AMD_EINVAL;
    if (n_images > 0 && !c.h_matrices) return JPEG_AMD_EINVAL;
    for (size_t k = 0; n_images > 0 && k < 12 * (size_t)n_images; ++k)
        if (!std::isfinite(c.h_matrices[k]) || std::fabs(c.h_matrices[k]) > kColourMaxEntry) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}
// "warped resample": what the contract requires of one matrix.
inline int check_warp_matrix(const float *m)
{
    if (!m) return JPEG_AMD_EINVAL;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(m[k]) || std::fabs(m[k]) > kWarpMaxEntry) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}
// "projective resample": what the contract requires of one matrix m[9] on a canvas of out_w x out_h (both in 1 .. 2^30, judged
// before): the entries as check_warp_matrix's, and the denominator W(cx, cy) = m20 cx + m21 cy + m22 at least S / 16 at the
// four corners of the canvas, S = |m20| out_w + |m21| out_h + |m22| at least 2^-30.  In double: every product and sum is
// rounded by at most 2^-53 of itself, so S and W are within 2^-50 S of their exact values, far inside the margin that the
// header's derivation leaves (it counts 3 * 2^-24 S for the kernel's own rounding).
inline int check_project_matrix(const float *m, int32_t out_w, int32_t out_h)
{
    if (!m) return JPEG_AMD_EINVAL;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(m[k]) || std::fabs(m[k]) > kWarpMaxEntry) return JPEG_AMD_EINVAL;
    const double w = out_w, h = out_h, m20 = m[6], m21 = m[7], m22 = m[8];
    const double S = (std::fabs(m20) * w + std::fabs(m21) * h) + std::fabs(m22);
    if (S < kProjectMinScale) return JPEG_AMD_EINVAL;
    const double low = std::min(std::min(m22, m20 * w + m22), std::min(m21 * h + m22, (m20 * w + m21 * h) + m22));
    return low < S / kProjectMaxForeshortening ? JPEG_AMD_EINVAL : JPEG_AMD_OK;
}
// "placed resample": what a placed call refuses of its placement as a whole, and of one image's window on its canvas.
inline int check_placement(const jpeg_amd_placement &p, int n_images)
{
    if (p.mode != JPEG_AMD_PLACE_WINDOWS && p.mode != JPEG_AMD_PLACE_FIT && p.mode != JPEG_AMD_PLACE_FIT_DOWN) return JPEG_AMD_EINVAL;
    if (p.anchor != JPEG_AMD_ANCHOR_CENTRE && p.anchor != JPEG_AMD_ANCHOR_TOP_LEFT) return JPEG_AMD_EINVAL;
    if (p.mode == JPEG_AMD_PLACE_WINDOWS && !p.h_windows && n_images > 0) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}
inline int check_window(const jpeg_amd_region &w, int32_t out_w, int32_t out_h)
{
    if (w.width < 1 || w.height < 1 || w.x < 0 || w.y < 0) return JPEG_AMD_EINVAL;
    if (w.x > out_w - w.width || w.y > out_h - w.height) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}
// Image i's window under a checked placement, for a source of src_w x src_h as the user sees it (oriented), checked.
inline int placed_window(const jpeg_amd_placement &p, int i, int32_t src_w, int32_t src_h, int32_t out_w, int32_t out_h,
                         jpeg_amd_region *w)
{
    if (p.mode == JPEG_AMD_PLACE_WINDOWS) *w = p.h_windows[i];
    else if (const int st = jpeg_amd_place_window(p.mode, p.anchor, src_w, src_h, out_w, out_h, w)) return st;
    return check_window(*w, out_w, out_h);
}

// ---- the batch file paths: the staging, and what the two decode pipelines share (capi_file.hip) ---------------------------------
// Both decode pipelines (files of one geometry to pixels, capi_file.hip; files of mixed sizes to one tensor, capi_files.hip) are
// the chunk loop of worker_pool.hpp (ChunkLoop) over the staging below, with FileBatch::device() as its device side and
// FileBatch::decode_to_slot() as the work of its threads; what differs is where a chunk's parts lie in its slot and what submit(k)
// enqueues.  The encode pipeline has another shape (a two-stage download, one parallel region per step) and its own loop.

// Where the parts of a staging slot of the batch pipelines begin (pinned and device slots alike): take(n) gives the next n
// bytes, aligned to 256, and a part of no bytes takes none.  Each pipeline uses the parts it has.
struct SlotLayout {
    size_t coef_off[JPEG_AMD_MAX_PLANES] = {};
    size_t quanta_off = 0, skip_off = 0, where_off = 0, sparse_off = 0, count_off = 0, px_off = 0, slot_bytes = 0;
    size_t take(size_t n)
    {
        const size_t at = slot_bytes;
        slot_bytes += align256(n);
        return at;
    }
};
// A file of a chunk whose planes k_huffman_intervals produces (JPEG_AMD_CTX_DEVICE_ENTROPY): its block (interval_plan.hpp) lies
// in the pinned slot where its first plane would lie, `bytes` long; `record` counts from the block's first byte and names no
// planes yet.  Written by the thread that decodes the file, read by the directing thread once the chunk is complete.
struct DeviceEntropyFile {
    bool on = false;
    interval::IntervalFile record{};
    size_t bytes = 0;
};
// ... and what submit(k) hands to decode_blocks_on_device for it: where the block lies (pinned) and the planes to write.
struct DeviceEntropyJob {
    const DeviceEntropyFile *file;
    const char *h_block;
    int16_t *d_planes[JPEG_AMD_MAX_PLANES];
};
// The blocks up (a copy each, on the context's stream), one launch of k_huffman_intervals, the statuses back; waits for them and
// returns the first that is not OK, in job and interval order.  (capi_entropy.hip)
int decode_blocks_on_device(jpeg_amd_ctx *ctx, const DeviceEntropyJob *jobs, int n);

// One call of a batch decode of files behind its checks: what the two pipelines share of it.
struct FileBatch {
    jpeg_amd_ctx *ctx;
    const uint8_t *const *h_jpeg;
    const size_t *nbytes;
    int n_images, nthreads, cosited;
    bool auto_threads;
    jpeg_amd_color color;
    ChunkLoop loop;

    // Where a file, one of the m of its chunk, goes in the chunk's pinned slot: the slot's packed records, the file's tables
    // and, should it travel dense, its planes.
    struct Into {
        int slot, m;
        uint32_t *packed;
        uint16_t (*quanta)[64];
        int16_t *planes[JPEG_AMD_MAX_PLANES];
        size_t room = 0;                       // bytes of planes[0]: what a device file's block may take
        DeviceEntropyFile *device = nullptr;   // where to note that the file took the device route (nullptr: it may not)
    };
    // One file, on a thread of the file queue: sparse into the thread's own record, then packed behind the records already in
    // the slot (one fetch_add on loop.packed_end[slot]; *where: its offset in `packed`, elements); where the sparse decoder says
    // ENOSUP, or sb.ok is false, into the planes on nthreads / m threads (*dense).  `frame`: what the file must be;
    // inspect_dense: look at the headers of a file that goes into planes, because nobody has yet.
    // Under JPEG_AMD_CTX_DEVICE_ENTROPY, and with to.device, the planner is asked first: a file it takes, whose block fits
    // to.room, is a dense file (*dense) whose planes the device produces -- only its block and its tables are written.
    int decode_to_slot(int file, const Into &to, const jpeg_amd_frame_info &frame, const SparseBudget &sb, bool inspect_dense,
                       std::vector<uint32_t> &record, uint64_t *where, bool *dense);
    // The loop's device side on the context's stream and events, around the pipeline's submit(k).
    ChunkDevice device(std::function<int(int)> submit);
    // The chunk loop over chunks `first` on the context's threads; every way out is through after_both_streams.
    int run_chunks(const std::vector<int> &first, const FileQueue::Decode &decode, const ChunkDevice &dev);
};
int host_threads(int nthreads, bool *auto_threads);   // the `nthreads` argument: <= 0 = default_host_threads(); at least 1
// JPEG.Common recognises 8-bit images of arity 1 or 3 (jpeg.swift:357-424): what the pixel calls take
inline bool jpeg_common(int precision, int ncomponents) { return precision == 8 && (ncomponents == 1 || ncomponents == 3); }
// Two pinned host slots of slot_bytes and two device slots of device_slot_bytes, two events per slot and the second stream.
int ensure_file_staging(jpeg_amd_ctx *ctx, size_t slot_bytes, size_t device_slot_bytes);
int default_host_threads();                   // how many host threads "all cores" means
hipError_t wait_event(hipEvent_t ev);         // by polling
WorkerPool &pool_with(std::unique_ptr<WorkerPool> &pool, int threads);   // the context's pool, with at least `threads` threads
int after_both_streams(jpeg_amd_ctx *ctx, int result);   // the way out of the pipelines: a failure waits for both streams

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

// Small RAII bag of device buffers for the host wrappers: single buffers, or every plane of a layout (T: the 16-bit sample;
// a plane without samples gets the 16 bytes of an empty buffer and no copy).
struct DeviceBag {
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

}  // namespace capi
}  // namespace jpeg_amd
