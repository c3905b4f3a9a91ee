// capi_files.hip -- the C ABI, files of mixed sizes and layouts to one tensor (jpeg_amd_decompress_tensor_mixed) or to
// resized bytes (jpeg_amd_decompress_resized_mixed): the file front end of the mixed calls of capi_view.hip.  The contract,
// the route and the cost are stated in include/jpeg_amd.h ("files to tensors"); the host threads are worker_pool.hpp's, the
// staging is capi_file.hip's.
#pragma clang fp contract(off)

#include "capi_internal.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace {

constexpr int kChunkFiles = 32;                        // files per chunk, at most
constexpr size_t kChunkPlaneBytes = (size_t)1 << 30;   // device planes per chunk, at most (one larger file is a chunk)

// What pass 0 knows of one file.
struct FileSpec {
    jpeg_amd_frame_info info;
    jpeg_amd_layout layout;
    jpeg_amd_view view;
    jpeg_amd_region window[JPEG_AMD_MAX_PLANES];   // blocks the expand writes: the view's, or the whole planes (head 8)
    int32_t head;
    SparseBudget sb;
    size_t plane_off[JPEG_AMD_MAX_PLANES];          // of its planes in the chunk's device planes, bytes
    size_t dense_off;                               // of its planes in the pinned slot's dense part, bytes
    // written by the thread that decodes the file, read by the directing thread once the file's chunk is complete
    uint64_t where;                                 // its record [descriptors][entries] in the slot's packed records, elements
    bool dense;                                     // decoded into planes: uploaded whole, not expanded
};

// A chunk: files [i0, i0 + m), and where the parts of its staging slot begin.  [quanta .. packed records] goes up in one copy.
struct FileChunk {
    int i0, m;
    size_t quanta_off, items_off, groups_off, sparse_off, dense_off, device_bytes, slot_bytes;
};

// One call behind its checks.
struct FilesDecode {
    jpeg_amd_ctx *ctx;
    const uint8_t *const *h_jpeg;
    const size_t *nbytes;
    int n_images, nthreads, cosited;
    bool auto_threads;
    jpeg_amd_color color;
    int32_t out_w, out_h;
    int filter;
    bool tensor;
    const jpeg_amd_tensor_spec *spec;
    const uint8_t *h_flip;
    void *d_dst;
    size_t dst_stride, elem_bytes;
    std::vector<FileSpec> files;               // (declared before run()'s queue: the threads write into it until they are stopped)
    std::vector<FileChunk> chunks;
    std::vector<int> chunk_of;                 // per file
    std::atomic<size_t> packed_end[2];         // per slot: elements of the records packed so far

    int decode_file(int file, std::vector<uint32_t> &record);
    int submit(int k);
    int run();
};

bool same_frame(const jpeg_amd_frame_info &a, const jpeg_amd_frame_info &b)
{
    bool same = a.width == b.width && a.height == b.height && a.precision == b.precision && a.ncomponents == b.ncomponents;
    for (int c = 0; same && c < a.ncomponents; ++c)
        same = a.factor_x[c] == b.factor_x[c] && a.factor_y[c] == b.factor_y[c] && a.units_x[c] == b.units_x[c] && a.units_y[c] == b.units_y[c];
    return same;
}

// The entropy decoding of one file, on a thread of the file queue, into pinned slot k & 1 of its chunk k: sparse first, packed
// behind the records already in the slot as BatchDecode::decode_file packs them; planes where the sparse decoder says ENOSUP.
int FilesDecode::decode_file(int file, std::vector<uint32_t> &record)
{
    const int k = chunk_of[(size_t)file], slot = k & 1;
    const FileChunk &ch = chunks[(size_t)k];
    FileSpec &f = files[(size_t)file];
    char *host = static_cast<char *>(ctx->file_pinned[slot]);
    uint16_t(*quanta)[64] = reinterpret_cast<uint16_t(*)[64]>(host + ch.quanta_off + (size_t)(file - ch.i0) * kQSlotElems * 2);
    f.dense = true;
    if (f.sb.ok) {
        if (record.size() < f.sb.elems) record.resize(f.sb.elems);      // (this thread's; kept in the context between calls)
        size_t n = 0;
        jpeg_amd_frame_info seen{};
        const int ss = jpeg_amd_jpeg_decode_sparse(h_jpeg[file], nbytes[file], record.data(), f.sb.blocks, record.data() + f.sb.blocks,
                                                   f.sb.arena, &n, quanta, &seen);
        if (ss == JPEG_AMD_OK) {
            if (!same_frame(seen, f.info)) return JPEG_AMD_EINVAL;      // (the bytes changed under the call)
            f.where = packed_end[slot].fetch_add(f.sb.blocks + n);
            std::memcpy(reinterpret_cast<uint32_t *>(host + ch.sparse_off) + f.where, record.data(), (f.sb.blocks + n) * 4);
            f.dense = false;
            return JPEG_AMD_OK;
        }
        if (ss != JPEG_AMD_ENOSUP) return ss;
    }
    // progressive, a missing restart marker, too dense: planes (fewer files than threads: the spare threads go to its restart
    // intervals)
    const int inner = std::max(1, nthreads / ch.m);
    int16_t *planes[JPEG_AMD_MAX_PLANES] = {};
    size_t at = f.dense_off;
    for (int c = 0; c < f.layout.nplanes; ++c) {
        planes[c] = reinterpret_cast<int16_t *>(host + ch.dense_off + at);
        at += align256(plane_samples(&f.layout, c) * 2);
    }
    return jpeg_amd_jpeg_decode_spectral_mt(h_jpeg[file], nbytes[file], planes, quanta, nullptr, inner > 1 && auto_threads ? 0 : inner);
}

// The device side of chunk k, asynchronous on the context's stream: the planes of its dense files, ONE copy of the tables, the
// item records and the packed records, ONE windowed expand, then the mixed call on the chunk's images, as it stands.  The
// plane buffer is one for all chunks: chunk k's copies and expand come behind chunk k - 1's kernels on the stream.
// (a failure in here leaves copies and kernels in flight: run()'s tail waits for both streams)
int FilesDecode::submit(int k)
{
    const int slot = k & 1;
    const FileChunk &ch = chunks[(size_t)k];
    char *host = static_cast<char *>(ctx->file_pinned[slot]);
    char *dev = static_cast<char *>(ctx->file_device) + (size_t)slot * chunks[0].device_bytes;   // (device_bytes: the call's largest, in every chunk)
    char *d_planes = static_cast<char *>(ctx->file_planes.ptr);
    const size_t rec_bytes = expand_mixed_record_bytes();
    std::vector<jpeg_amd_image> images((size_t)ch.m);
    uint32_t *groups = reinterpret_cast<uint32_t *>(host + ch.groups_off);
    int n_items = 0;
    uint64_t acc = 0;
    for (int i = 0; i < ch.m; ++i) {
        const FileSpec &f = files[(size_t)(ch.i0 + i)];
        jpeg_amd_image &im = images[(size_t)i];
        im = jpeg_amd_image{};
        im.layout = f.layout;
        im.d_quanta = reinterpret_cast<const uint16_t *>(dev + ch.quanta_off + (size_t)i * kQSlotElems * 2);
        im.ntables = f.layout.nplanes;
        jpeg_amd_expand_item item{};
        item.layout = f.layout;
        size_t at = f.dense_off;
        for (int c = 0; c < f.layout.nplanes; ++c) {
            item.d_coef[c] = reinterpret_cast<int16_t *>(d_planes + f.plane_off[c]);
            im.d_coef[c] = item.d_coef[c];
            item.window[c] = f.window[c];
            if (f.dense) {
                const size_t bytes = plane_samples(&f.layout, c) * 2;
                JA_HIP(ctx, hipMemcpyAsync(item.d_coef[c], host + ch.dense_off + at, bytes, hipMemcpyHostToDevice, ctx->stream));
                at += align256(bytes);
            }
        }
        if (f.dense) continue;
        item.head = f.head;
        item.desc_at = f.where;
        item.entries_at = f.where + f.sb.blocks;
        expand_mixed_record(host + ch.items_off + rec_bytes * (size_t)n_items, item);
        groups[n_items++] = (uint32_t)acc;
        acc += expand_mixed_groups(item);            // (the chunk's sum fits a grid: judged in pass 0)
    }
    groups[n_items] = (uint32_t)acc;
    JA_HIP(ctx, hipMemcpyAsync(dev + ch.quanta_off, host + ch.quanta_off, ch.sparse_off - ch.quanta_off + packed_end[slot].load() * 4,
                               hipMemcpyHostToDevice, ctx->stream));
    JA_HIP(ctx, launch_expand_mixed(ctx->stream, n_items, dev + ch.items_off, reinterpret_cast<const uint32_t *>(dev + ch.groups_off),
                                    (uint32_t)acc, reinterpret_cast<const uint32_t *>(dev + ch.sparse_off)));
    std::vector<jpeg_amd_view> views((size_t)ch.m);
    for (int i = 0; i < ch.m; ++i) views[(size_t)i] = files[(size_t)(ch.i0 + i)].view;
    void *d_out = static_cast<char *>(d_dst) + (size_t)ch.i0 * dst_stride * elem_bytes;
    if (tensor)
        JA_TRY(jpeg_amd_decode_tensor_filter_mixed(ctx, ch.m, images.data(), cosited, color, views.data(), out_w, out_h, filter, spec,
                                                   h_flip ? h_flip + ch.i0 : nullptr, d_out, dst_stride));
    else
        JA_TRY(jpeg_amd_decode_resized_filter_mixed(ctx, ch.m, images.data(), cosited, color, views.data(), out_w, out_h, filter,
                                                    static_cast<uint8_t *>(d_out), dst_stride));
    JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
    return JPEG_AMD_OK;
}

// The chunk loop, as BatchDecode::run has it: ONE queue of files for the whole call, decoded on t_n host threads beside this
// one, which directs; this thread submits a chunk as soon as its last file is in.  Chunk j is decoded into pinned slot j & 1,
// which is free once chunk j - 2's copies have read it (file_decoded[slot] is recorded behind them).
int FilesDecode::run()
{
    int result = JPEG_AMD_OK;
    packed_end[0].store(0); packed_end[1].store(0);
    const int nchunks = (int)chunks.size(), t_n = std::min(nthreads, n_images);
    std::vector<int> first;
    for (const FileChunk &ch : chunks) first.push_back(ch.i0);
    first.push_back(n_images);
    {
        // (the queue stops and joins the threads on every way out, a failed chunk included, BEFORE `files`, which they write
        // into, goes away with this call -- and before it trims their records)
        FileQueue queue(pool_with(ctx->workers, t_n + 1), ctx->records, first, t_n, [this](int file, std::vector<uint32_t> &record) {
            try { return decode_file(file, record); } catch (...) { return (int)JPEG_AMD_ENOMEM; }
        }, (size_t)16 << 20);
        for (int k = 0; k < nchunks && result == JPEG_AMD_OK; ++k) {
            // With threads, chunk k + 1 is opened while they are in chunk k; without, this thread decodes chunk k itself (in wait(k)).
            const int j = queue.threaded() ? k + 1 : k;
            if (j >= 2 && j < nchunks) {
                const hipError_t w = wait_event(ctx->file_decoded[j & 1]);
                if (w != hipSuccess) { ctx->last_hip = (int)w; result = JPEG_AMD_EHIP; break; }
                packed_end[j & 1].store(0);                       // (chunks 0 and 1 start from the initial zeros)
            }
            queue.open(std::min(j + 1, nchunks));
            result = queue.wait(k);
            if (result == JPEG_AMD_OK) result = submit(k);
        }
    }
    if (result != JPEG_AMD_OK) return after_both_streams(ctx, result);
    JA_HIP(ctx, wait_event(ctx->file_decoded[(nchunks - 1) & 1]));
    return JPEG_AMD_OK;
}

int decompress_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads, int cosited,
                     jpeg_amd_color color, const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h, int filter, bool tensor,
                     const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride,
                     jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views)
{
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_jpeg || !nbytes)) return JPEG_AMD_EINVAL;
    FilesDecode d;
    d.ctx = ctx; d.h_jpeg = h_jpeg; d.nbytes = nbytes; d.n_images = n_images; d.cosited = cosited; d.color = color;
    d.out_w = out_w; d.out_h = out_h; d.filter = filter; d.tensor = tensor; d.spec = spec; d.h_flip = h_flip; d.d_dst = d_dst;
    d.dst_stride = dst_stride;
    d.files.resize((size_t)n_images);
    // ---- pass 0: the headers, file by file; the first file that is refused ends it
    int bad = n_images, bad_status = JPEG_AMD_OK;
    std::vector<jpeg_amd_image> images((size_t)n_images);
    std::vector<jpeg_amd_view> views((size_t)n_images);
    for (int i = 0; i < n_images && bad == n_images; ++i) {
        FileSpec &f = d.files[(size_t)i];
        int st = h_jpeg[i] ? jpeg_amd_jpeg_inspect(h_jpeg[i], nbytes[i], &f.info) : JPEG_AMD_EINVAL;
        // JPEG.Common recognises 8-bit images of arity 1 or 3 (jpeg.swift:357-424)
        if (st == JPEG_AMD_OK && (f.info.precision != 8 || (f.info.ncomponents != 1 && f.info.ncomponents != 3))) st = JPEG_AMD_ENOSUP;
        if (st == JPEG_AMD_OK) {
            if (h_info) h_info[i] = f.info;
            f.layout = layout_of_info(f.info, f.info.ncomponents);
            const jpeg_amd_region source = h_source_regions ? h_source_regions[i] : jpeg_amd_region{0, 0, f.info.width, f.info.height};
            // the data-loader call's view (decode_crops_tensor_mixed): the cheapest denominator, then the rectangle at it
            f.view.denom = jpeg_amd_view_denom(source.width, source.height, out_w, out_h);
            st = jpeg_amd_view_of_source(&f.layout, f.view.denom, &source, &f.view.region);
        }
        if (st != JPEG_AMD_OK) { bad = i; bad_status = st; break; }
        if (h_views) h_views[i] = f.view;
        views[(size_t)i] = f.view;
        // (the planes do not exist yet: what the mixed call judges of a pointer is that it is there)
        jpeg_amd_image &im = images[(size_t)i];
        im = jpeg_amd_image{};
        im.layout = f.layout;
        for (int c = 0; c < f.layout.nplanes; ++c) im.d_coef[c] = reinterpret_cast<const int16_t *>(&f);
        im.d_quanta = reinterpret_cast<const uint16_t *>(&f);
        im.ntables = f.layout.nplanes;
    }
    // ... then what the mixed call refuses of the files in front of that one, the target included; the tap limit last
    int taps = JPEG_AMD_OK;
    JA_TRY(check_resampled_mixed(n_images, bad, images.data(), cosited, color, views.data(), out_w, out_h, filter, spec, tensor, d_dst,
                                 dst_stride, &taps));
    JA_TRY(bad_status);
    JA_TRY(taps);
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it
    d.elem_bytes = 1;
    if (tensor) JA_TRY(jpeg_amd_tensor_extent(spec, out_w, out_h, &d.elem_bytes, nullptr));

    // ---- the windows, and the chunks: consecutive files, at most kChunkFiles and kChunkPlaneBytes of planes
    const size_t rec_bytes = expand_mixed_record_bytes();
    d.chunk_of.resize((size_t)n_images);
    size_t slot_bytes = 0, device_bytes = 0, plane_bytes = 0;
    for (int i0 = 0; i0 < n_images;) {
        FileChunk ch{};
        ch.i0 = i0;
        size_t planes = 0, dense = 0, sparse = 0;
        uint64_t groups = 0;
        for (; i0 + ch.m < n_images && ch.m < kChunkFiles; ++ch.m) {
            FileSpec &f = d.files[(size_t)(i0 + ch.m)];
            size_t mine = 0;
            for (int c = 0; c < f.layout.nplanes; ++c) mine += align256(plane_samples(&f.layout, c) * 2);
            if (ch.m > 0 && planes + mine > kChunkPlaneBytes) break;
            // an image the tile kernel takes is read inside its view's windows, at the denominator's head; the one-image
            // fallback of any other reads whole planes (the predicate is plan_mixed's)
            f.head = 8;
            if (fused_decode_supported(f.layout, cosited != 0)) {
                JA_TRY(jpeg_amd_view_window(&f.layout, cosited, f.view.denom, &f.view.region, f.window));
                f.head = f.view.denom >= 4 ? 1 : f.view.denom == 2 ? 4 : 8;
            } else {
                for (int c = 0; c < f.layout.nplanes; ++c) f.window[c] = jpeg_amd_region{0, 0, f.layout.units_x[c], f.layout.units_y[c]};
            }
            // (the decoder wants room for a whole block -- 72 entries -- in front of every block: without it a file of a
            // few blocks would never travel sparse)
            f.sb = sparse_budget(f.layout);
            f.sb.arena += 72; f.sb.elems += 72;
            f.dense_off = dense;
            for (int c = 0; c < f.layout.nplanes; ++c) {
                f.plane_off[c] = planes;
                planes += align256(plane_samples(&f.layout, c) * 2);
            }
            dense += mine;
            if (f.sb.ok) sparse += f.sb.elems * 4;
            jpeg_amd_expand_item item{};
            item.layout = f.layout; item.head = f.head;
            for (int c = 0; c < f.layout.nplanes; ++c) item.window[c] = f.window[c];
            groups += expand_mixed_groups(item);
            d.chunk_of[(size_t)(i0 + ch.m)] = (int)d.chunks.size();
        }
        if (groups > 0x7fffffffu) return JPEG_AMD_EINVAL;          // more workgroups than a grid holds
        // slot layout: [quanta x m][item records x m][workgroup prefix m + 1][packed records ...] | [planes of the dense files]
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t was = at; at += align256(n); return was; };
        ch.quanta_off = take((size_t)ch.m * kQSlotElems * 2);
        ch.items_off = take((size_t)ch.m * rec_bytes);
        ch.groups_off = take(((size_t)ch.m + 1) * 4);
        ch.sparse_off = take(sparse);
        ch.device_bytes = at;                                      // the dense files' planes go straight into the plane buffer
        ch.dense_off = take(dense);
        ch.slot_bytes = at;
        slot_bytes = std::max(slot_bytes, ch.slot_bytes);
        device_bytes = std::max(device_bytes, ch.device_bytes);
        plane_bytes = std::max(plane_bytes, planes);
        d.chunks.push_back(ch);
        i0 += ch.m;
    }
    for (FileChunk &ch : d.chunks) ch.device_bytes = device_bytes;   // the device slots lie this far apart

    JA_TRY(bind(ctx));
    JA_TRY(ensure_file_staging(ctx, slot_bytes, device_bytes));
    JA_TRY(ensure_buffer(ctx, ctx->file_planes, std::max<size_t>(plane_bytes, 256)));
    d.auto_threads = nthreads <= 0;
    if (d.auto_threads) nthreads = default_host_threads();
    d.nthreads = std::max(1, nthreads);
    return d.run();
}

}  // namespace

int jpeg_amd_decompress_tensor_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                                     int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions, int32_t out_w,
                                     int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                     size_t dst_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions, out_w, out_h, filter, true, spec,
                            h_flip, d_dst, dst_stride, h_info, h_views);
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_resized_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                                      int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions, int32_t out_w,
                                      int32_t out_h, int filter, uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                      jpeg_amd_view *h_views)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions, out_w, out_h, filter, false,
                            nullptr, nullptr, d_pixels, pixel_stride, h_info, h_views);
}
JA_NOTHROW_TAIL
