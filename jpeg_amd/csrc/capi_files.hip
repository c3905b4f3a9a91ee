// capi_files.hip -- the C ABI, files of mixed sizes and layouts to one tensor (jpeg_amd_decompress_tensor_mixed) or to
// resized bytes (jpeg_amd_decompress_resized_mixed): the file front end of the mixed calls of capi_view.hip.  The contract,
// the route and the cost are stated in include/jpeg_amd.h ("files to tensors").  The pipeline is the one of the uniform batch
// decode -- worker_pool.hpp's chunk loop over capi_file.hip's staging, the threads' work and the loop's device side (see
// capi_internal.hpp) -- with chunks of the call's own cutting, no pixels to bring back, and this file's submit(k).
#pragma clang fp contract(off)

#include "capi_internal.hpp"
#include "orient.hpp"

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
    DeviceEntropyFile device;                       // ... or produced on the device from its block (JPEG_AMD_CTX_DEVICE_ENTROPY)
};

// A chunk: files [i0, i0 + m), and where the parts of its staging slot begin.  [quanta .. packed records] goes up in one copy.
struct FileChunk {
    int i0, m;
    size_t quanta_off, items_off, groups_off, sparse_off, dense_off, device_bytes, slot_bytes;
};

// The optional outputs of a file call, per file, each nullptr or the caller's array (four types: none can take another's place).
struct FileOutputs {
    jpeg_amd_frame_info *h_info = nullptr;
    jpeg_amd_view *h_views = nullptr;
    int32_t *h_orient_out = nullptr;
    float *h_matrices_out = nullptr;
};

// One call behind its checks.
struct FilesDecode : FileBatch {
    // what goes to the mixed call: the caller's request, with pass 0's per-file vectors in the place of the caller's arrays
    ResampleRequest mixed;
    std::vector<uint8_t> orient;               // per file, what the call applies; empty: no orientations reach the mixed call
    std::vector<jpeg_amd_region> windows;      // "placed resample": per file, pass 0's, go to the mixed call as they are ...
    jpeg_amd_placement in_windows;             // ... under this placement
    std::vector<float> matrices;               // with a map: pass 0's m_view per file
    std::vector<FileSpec> files;               // (the threads write into it until the loop has stopped them)
    std::vector<FileChunk> chunks;
    std::vector<int> chunk_of;                 // per file

    int decode_file(int file, std::vector<uint32_t> &record);
    int submit(int k);
    int run();
};

// The entropy decoding of one file, on a thread of the file queue, into pinned slot k & 1 of its chunk k.
int FilesDecode::decode_file(int file, std::vector<uint32_t> &record)
{
    const int k = chunk_of[(size_t)file];
    const FileChunk &ch = chunks[(size_t)k];
    FileSpec &f = files[(size_t)file];
    char *host = static_cast<char *>(ctx->file_pinned[k & 1]);
    Into to{k & 1, ch.m, reinterpret_cast<uint32_t *>(host + ch.sparse_off),
            reinterpret_cast<uint16_t(*)[64]>(host + ch.quanta_off + (size_t)(file - ch.i0) * kQSlotElems * 2), {}};
    size_t at = f.dense_off;
    for (int c = 0; c < f.layout.nplanes; ++c) {
        to.planes[c] = reinterpret_cast<int16_t *>(host + ch.dense_off + at);
        at += align256(plane_samples(&f.layout, c) * 2);
    }
    to.room = at - f.dense_off;                      // (a file's planes lie in a row here: a block may take them all)
    to.device = &f.device;
    return decode_to_slot(file, to, f.info, f.sb, false, record, &f.where, &f.dense);   // (what pass 0 saw, headers included)
}

// The device side of chunk k, asynchronous on the context's stream: the planes of its dense files, ONE copy of the tables, the
// item records and the packed records, ONE windowed expand, then the mixed call on the chunk's images, as it stands.  The
// plane buffer is one for all chunks: chunk k's copies and expand come behind chunk k - 1's kernels on the stream.
// (a failure in here leaves copies and kernels in flight: run_chunks() waits for both streams on the way out)
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
    std::vector<DeviceEntropyJob> jobs;
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
            if (f.dense && !f.device.on) {
                const size_t bytes = plane_samples(&f.layout, c) * 2;
                JA_HIP(ctx, hipMemcpyAsync(item.d_coef[c], host + ch.dense_off + at, bytes, hipMemcpyHostToDevice, ctx->stream));
                at += align256(bytes);
            }
        }
        if (f.device.on) {                           // its planes are produced on the device, from its block
            DeviceEntropyJob job{&f.device, host + ch.dense_off + f.dense_off, {}};
            for (int c = 0; c < f.layout.nplanes; ++c) job.d_planes[c] = item.d_coef[c];
            jobs.push_back(job);
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
    JA_HIP(ctx, hipMemcpyAsync(dev + ch.quanta_off, host + ch.quanta_off, ch.sparse_off - ch.quanta_off + loop.packed_end[slot].load() * 4,
                               hipMemcpyHostToDevice, ctx->stream));
    JA_TRY(decode_blocks_on_device(ctx, jobs.data(), (int)jobs.size()));
    JA_HIP(ctx, launch_expand_mixed(ctx->stream, n_items, dev + ch.items_off, reinterpret_cast<const uint32_t *>(dev + ch.groups_off),
                                    (uint32_t)acc, reinterpret_cast<const uint32_t *>(dev + ch.sparse_off)));
    std::vector<jpeg_amd_view> views((size_t)ch.m);
    for (int i = 0; i < ch.m; ++i) views[(size_t)i] = files[(size_t)(ch.i0 + i)].view;
    ResampleRequest::Room room;
    JA_TRY(decode_views_mixed(ctx, ch.m, images.data(), cosited, color, views.data(), mixed.images(ch.i0, ch.m, &room)));
    JA_HIP(ctx, hipEventRecord(ctx->file_decoded[slot], ctx->stream));
    JA_HIP(ctx, hipEventRecord(ctx->file_done[slot], ctx->stream));     // the tensor stays where it is: done when the kernels are
    return JPEG_AMD_OK;
}

// The chunk loop (ChunkLoop, worker_pool.hpp) without a drain.  (`files`, which the threads write into, is declared before it.)
int FilesDecode::run()
{
    std::vector<int> first;
    for (const FileChunk &ch : chunks) first.push_back(ch.i0);
    first.push_back(n_images);
    return run_chunks(first, [this](int file, std::vector<uint32_t> &record) { return decode_file(file, record); },
                      device([this](int k) { return submit(k); }));
}

// Every file call: the file arguments, what the caller asked of the resample (rq; with a map, rq.h_matrices against the upright
// images) and where the per-file results go.
int decompress_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads, int cosited,
                     jpeg_amd_color color, const jpeg_amd_region *h_source_regions, const ResampleRequest &rq, const FileOutputs &out)
{
    // every argument first, the context last: nothing is enqueued, and the device is not touched, for a call that is refused
    if (n_images < 0 || n_images > 65535) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_jpeg || !nbytes)) return JPEG_AMD_EINVAL;
    const bool mapped = rq.has_map();
    if (mapped && n_images > 0 && !rq.h_matrices) return JPEG_AMD_EINVAL;
    const int32_t out_w = rq.out_w, out_h = rq.out_h;
    const uint8_t *const h_orient = rq.h_orient;
    const jpeg_amd_placement *const place = rq.place;
    const size_t k = rq.matrix_floats();
    FilesDecode d;
    d.ctx = ctx; d.h_jpeg = h_jpeg; d.nbytes = nbytes; d.n_images = n_images; d.cosited = cosited; d.color = color;
    d.files.resize((size_t)n_images);
    // (1 behind a refused file: the mixed call's judgement stops in front of it; mapped: the orientation goes into the matrix)
    if (h_orient && !mapped) d.orient.assign((size_t)n_images, 1);
    if (mapped) d.matrices.assign(k * (size_t)n_images, 0.0f);
    if (place) d.windows.assign((size_t)n_images, jpeg_amd_region{0, 0, 0, 0});
    d.in_windows = jpeg_amd_placement{JPEG_AMD_PLACE_WINDOWS, JPEG_AMD_ANCHOR_CENTRE, d.windows.data(), {0, 0, 0}, 0};
    for (int c = 0; place && c < 3; ++c) d.in_windows.fill[c] = place->fill[c];
    d.mixed = rq;
    d.mixed.oriented(d.orient.empty() ? nullptr : d.orient.data()).placed(place ? &d.in_windows : nullptr, nullptr);
    if (mapped) d.mixed.mapped(rq.map, d.matrices.data(), rq.warp);
    // ---- pass 0: the headers, file by file; the first file that is refused ends it
    int bad = n_images, bad_status = JPEG_AMD_OK;
    std::vector<jpeg_amd_image> images((size_t)n_images);
    std::vector<jpeg_amd_view> views((size_t)n_images);
    for (int i = 0; i < n_images && bad == n_images; ++i) {
        FileSpec &f = d.files[(size_t)i];
        int st = h_jpeg[i] ? jpeg_amd_jpeg_inspect(h_jpeg[i], nbytes[i], &f.info) : JPEG_AMD_EINVAL;
        if (st == JPEG_AMD_OK && !jpeg_common(f.info.precision, f.info.ncomponents)) st = JPEG_AMD_ENOSUP;
        if (st == JPEG_AMD_OK) {
            if (out.h_info) out.h_info[i] = f.info;
            f.layout = layout_of_info(f.info, f.info.ncomponents);
            // the orientation the call applies: the file's tag, or the caller's value; the source rectangle is one of the
            // ORIENTED image then, and `source` the stored rectangle that holds its pixels
            int32_t o = 1;
            if (h_orient && h_orient[i] == JPEG_AMD_ORIENT_EXIF) st = jpeg_amd_jpeg_orientation(h_jpeg[i], nbytes[i], &o);
            else if (h_orient) o = h_orient[i];
            // `seen`: the rectangle of the oriented image the caller named, or the whole of it, w' x h' -- which is what the
            // denominator is chosen for; `source`: the stored rectangle that holds its pixels
            jpeg_amd_region source{0, 0, f.info.width, f.info.height}, seen = source;
            if (st == JPEG_AMD_OK && !orientation_valid(o)) st = JPEG_AMD_EINVAL;
            if (st == JPEG_AMD_OK) {
                const OrientedSource whole = oriented_source(o, 0, f.info.width, f.info.height);
                seen = h_source_regions ? h_source_regions[i] : jpeg_amd_region{0, 0, whole.w, whole.h};
                st = jpeg_amd_orient_region(o, f.info.width, f.info.height, &seen, &source);
            }
            if (st == JPEG_AMD_OK && mapped) {
                // the matrix says what is read -- the view and the matrix against it are jpeg_amd_warp_view's, or
                // ("projective resample", "bicubic warp") jpeg_amd_project_filter_view's at the request's filter, nine numbers each
                if (out.h_orient_out) out.h_orient_out[i] = o;
                st = map_view(rq, &f.layout, o, rq.h_matrices + k * (size_t)i, &f.view, &d.matrices[k * (size_t)i]);
                if (st == JPEG_AMD_OK && out.h_matrices_out)
                    std::memcpy(out.h_matrices_out + k * (size_t)i, &d.matrices[k * (size_t)i], k * sizeof(float));
            } else if (st == JPEG_AMD_OK) {
                if (h_orient) d.orient[(size_t)i] = (uint8_t)o;
                if (out.h_orient_out) out.h_orient_out[i] = o;
                // the data-loader call's view (decode_crops_tensor_mixed): the cheapest denominator, then the rectangle at it
                // placed: the file's window, of the oriented rectangle's size; the denominator is chosen against it
                jpeg_amd_region want{0, 0, out_w, out_h};
                if (place) {
                    st = check_placement(*place, n_images);
                    if (st == JPEG_AMD_OK) st = placed_window(*place, i, seen.width, seen.height, out_w, out_h, &want);
                }
                if (st == JPEG_AMD_OK) {
                    if (place) d.windows[(size_t)i] = want;
                    f.view.denom = jpeg_amd_view_denom(seen.width, seen.height, want.width, want.height);
                    st = jpeg_amd_view_of_source(&f.layout, f.view.denom, &source, &f.view.region);
                }
            }
        }
        if (st != JPEG_AMD_OK) { bad = i; bad_status = st; break; }
        if (out.h_views) out.h_views[i] = f.view;
        if (place && rq.h_windows_out) rq.h_windows_out[i] = d.windows[(size_t)i];
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
    JA_TRY(check_resampled_mixed(n_images, bad, images.data(), cosited, color, views.data(), d.mixed, &taps));
    JA_TRY(bad_status);
    JA_TRY(taps);
    if (n_images == 0) return JPEG_AMD_OK;   // nothing to do, and no context needed for it

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
            f.sb = sparse_budget(f.layout, kSparseDecoderHeadroom);    // (or a file of a few blocks would never travel sparse)
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
        SlotLayout at;
        ch.quanta_off = at.take((size_t)ch.m * kQSlotElems * 2);
        ch.items_off = at.take((size_t)ch.m * rec_bytes);
        ch.groups_off = at.take(((size_t)ch.m + 1) * 4);
        ch.sparse_off = at.take(sparse);
        ch.device_bytes = at.slot_bytes;                           // the dense files' planes go straight into the plane buffer
        ch.dense_off = at.take(dense);
        ch.slot_bytes = at.slot_bytes;
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
    d.nthreads = host_threads(nthreads, &d.auto_threads);
    return d.run();
}

}  // namespace

int jpeg_amd_decompress_tensor_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                                     int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions, int32_t out_w,
                                     int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                     size_t dst_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride).through(filter),
                            FileOutputs{h_info, h_views});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_resized_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images, int nthreads,
                                      int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions, int32_t out_w,
                                      int32_t out_h, int filter, uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                      jpeg_amd_view *h_views)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride).through(filter),
                            FileOutputs{h_info, h_views});
}
JA_NOTHROW_TAIL

// The two file calls with an orientation per file ("oriented resample"): 0 = the file's EXIF tag, 1 .. 8 = that value.
int jpeg_amd_decompress_tensor_oriented_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                              int nthreads, int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions,
                                              int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                              const uint8_t *h_flip, const uint8_t *h_orient, void *d_dst, size_t dst_stride,
                                              jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride).through(filter).oriented(h_orient),
                            FileOutputs{h_info, h_views, h_orient_out});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_resized_oriented_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                               int nthreads, int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions,
                                               int32_t out_w, int32_t out_h, int filter, const uint8_t *h_orient, uint8_t *d_pixels,
                                               size_t pixel_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                               int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride).through(filter).oriented(h_orient),
                            FileOutputs{h_info, h_views, h_orient_out});
}
JA_NOTHROW_TAIL

// The two file calls with a placement ("placed resample"): the oriented calls above are these with place == nullptr.
int jpeg_amd_decompress_tensor_placed_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                            int nthreads, int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions,
                                            int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                            const uint8_t *h_flip, const uint8_t *h_orient, const jpeg_amd_placement *place,
                                            jpeg_amd_region *h_windows_out, void *d_dst, size_t dst_stride, jpeg_amd_frame_info *h_info,
                                            jpeg_amd_view *h_views, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                .through(filter).oriented(h_orient).placed(place, h_windows_out),
                            FileOutputs{h_info, h_views, h_orient_out});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_resized_placed_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                             int nthreads, int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions,
                                             int32_t out_w, int32_t out_h, int filter, const uint8_t *h_orient,
                                             const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out, uint8_t *d_pixels,
                                             size_t pixel_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                             int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                                .through(filter).oriented(h_orient).placed(place, h_windows_out),
                            FileOutputs{h_info, h_views, h_orient_out});
}
JA_NOTHROW_TAIL

// The two file calls through an affine map ("warped resample"): each file's view and matrix from jpeg_amd_warp_view in pass 0.
int jpeg_amd_decompress_resized_warped_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                             int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                             const float *h_matrices, const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                             uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                             float *h_matrices_out, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr,
                            ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                                .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp),
                            FileOutputs{h_info, h_views, h_orient_out, h_matrices_out});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_tensor_warped_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                            int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                            const float *h_matrices, const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                            const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride,
                                            jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, float *h_matrices_out,
                                            int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp),
                            FileOutputs{h_info, h_views, h_orient_out, h_matrices_out});
}
JA_NOTHROW_TAIL

// The two file calls to a tensor with the "colour stage": with colour == nullptr each is the call it is named after, whose
// request it then builds.
int jpeg_amd_decompress_tensor_colour_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                            int nthreads, int cosited, jpeg_amd_color color, const jpeg_amd_region *h_source_regions,
                                            int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                            const uint8_t *h_flip, const uint8_t *h_orient, const jpeg_amd_placement *place,
                                            jpeg_amd_region *h_windows_out, const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride,
                                            jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_source_regions,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                .through(filter).oriented(h_orient).placed(place, h_windows_out).coloured(colour),
                            FileOutputs{h_info, h_views, h_orient_out});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_tensor_warped_colour_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                                   int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                                   const float *h_matrices, const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                                   const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const jpeg_amd_colour *colour,
                                                   void *d_dst, size_t dst_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                                   float *h_matrices_out, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                .oriented(h_orient).mapped(ResampleMap::Affine, h_matrices, warp).coloured(colour),
                            FileOutputs{h_info, h_views, h_orient_out, h_matrices_out});
}
JA_NOTHROW_TAIL

// The two file calls through a homography ("projective resample", "bicubic warp"): each file's view and matrix from
// jpeg_amd_project_filter_view in pass 0; the tensor form with the "colour stage", or colour == nullptr for none.  The forms
// without a filter argument are these with JPEG_AMD_FILTER_BILINEAR.
int jpeg_amd_decompress_resized_projected_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                                int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                                const float *h_matrices, const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                                uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                                jpeg_amd_view *h_views, float *h_matrices_out, int32_t *h_orient_out)
{
    return jpeg_amd_decompress_resized_projected_filter_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_orient, h_matrices, warp,
                                                              JPEG_AMD_FILTER_BILINEAR, out_w, out_h, d_pixels, pixel_stride, h_info, h_views,
                                                              h_matrices_out, h_orient_out);
}

int jpeg_amd_decompress_resized_projected_filter_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                                       int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                                       const float *h_matrices, const jpeg_amd_warp *warp, int filter, int32_t out_w,
                                                       int32_t out_h, uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                                       jpeg_amd_view *h_views, float *h_matrices_out, int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr,
                            ResampleRequest::bytes(out_w, out_h, d_pixels, pixel_stride)
                                .through(filter).oriented(h_orient).mapped(ResampleMap::Projective, h_matrices, warp),
                            FileOutputs{h_info, h_views, h_orient_out, h_matrices_out});
}
JA_NOTHROW_TAIL

int jpeg_amd_decompress_tensor_projected_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                               int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                               const float *h_matrices, const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                               const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const jpeg_amd_colour *colour,
                                               void *d_dst, size_t dst_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                               float *h_matrices_out, int32_t *h_orient_out)
{
    return jpeg_amd_decompress_tensor_projected_filter_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, h_orient, h_matrices, warp,
                                                             JPEG_AMD_FILTER_BILINEAR, out_w, out_h, spec, h_flip, colour, d_dst, dst_stride,
                                                             h_info, h_views, h_matrices_out, h_orient_out);
}

int jpeg_amd_decompress_tensor_projected_filter_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                                      int nthreads, int cosited, jpeg_amd_color color, const uint8_t *h_orient,
                                                      const float *h_matrices, const jpeg_amd_warp *warp, int filter, int32_t out_w,
                                                      int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                                      const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride,
                                                      jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, float *h_matrices_out,
                                                      int32_t *h_orient_out)
try {
    return decompress_mixed(ctx, h_jpeg, nbytes, n_images, nthreads, cosited, color, nullptr,
                            ResampleRequest::elements(out_w, out_h, spec, h_flip, d_dst, dst_stride)
                                .through(filter).oriented(h_orient).mapped(ResampleMap::Projective, h_matrices, warp).coloured(colour),
                            FileOutputs{h_info, h_views, h_orient_out, h_matrices_out});
}
JA_NOTHROW_TAIL
